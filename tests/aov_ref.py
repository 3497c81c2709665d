"""The averaged feature planes (rt_aov_* of include/rt_hip.h) restated in numpy, for tests/test_aov_cpu.py and
tests/test_aov_gpu.py: the sample pattern, the rays of the definition in float32 one operation at a time, their
casts through rt.cast_host (which tests/test_guide_cpu.py pins against the oracle) and the sums in sample order."""
from __future__ import annotations

import functools

import numpy as np

import raytracing_gpu_amd as rt

F32 = np.float32
PLANES = ("normal", "albedo", "depth", "prim", "coverage")


def _reversed(k: int, base: int, digits: int) -> int:
    r = 0
    for _ in range(digits):
        r, k = r * base + k % base, k // base
    return r


def pattern(S: int, lens: int = 1, footprint: int = 1, shutter: int = 1) -> np.ndarray:
    """[S][5] float32: du, dv, lx, ly, f."""
    P, bits = 1, 0
    while P < S:
        P, bits = 2 * P, bits + 1
    out = np.zeros((S, 5), F32)
    k = 0
    for s in range(S):
        out[s, 0] = F32(2 * s + 1) / F32(2 * S) if footprint else F32(0.5)
        out[s, 1] = F32(2 * _reversed(s, 2, bits) + 1) / F32(2 * P) if footprint else F32(0.5)
        if lens:
            while True:
                k += 1
                x = 2.0 * (_reversed(k, 3, 10) / 59049.0) - 1.0  # Python floats: double
                y = 2.0 * (_reversed(k, 5, 7) / 78125.0) - 1.0
                if x * x + y * y <= 1.0:
                    break
            out[s, 2], out[s, 3] = F32(x), F32(y)
        out[s, 4] = F32(_reversed(s, 7, 5) / 16807.0) if shutter else F32(0.5)
    return out


def rays(cam, W: int, H: int, entry, lens: int) -> np.ndarray:
    """[H * W][8] float32: the rays of one table entry for every pixel, row 0 the bottom row."""
    v = lambda a: np.array(list(a), F32)
    du, dv, lx, ly, f = (F32(x) for x in entry)
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    su = ((i.astype(F32) + du) / F32(W))[..., None]
    sv = ((j.astype(F32) + dv) / F32(H))[..., None]
    o = np.broadcast_to(v(cam.origin), (H, W, 3))
    d = v(cam.lower_left) + su * v(cam.horizontal) + sv * v(cam.vertical) - v(cam.origin)
    if lens:
        rx, ry = F32(cam.lens_radius) * lx, F32(cam.lens_radius) * ly
        offset = rx * v(cam.u) + ry * v(cam.v)
        o = o + offset
        d = d - offset
    out = np.zeros((H, W, 8), F32)
    out[..., :3], out[..., 3:6] = o, d
    out[..., 6] = F32(cam.time0) + f * (F32(cam.time1) - F32(cam.time0))
    assert su.dtype == F32 and d.dtype == F32 and o.dtype == F32
    return out.reshape(-1, 8)


def planes(soa, W: int, H: int, S: int, lens: int = 1, footprint: int = 1, shutter: int = 1) -> dict:
    """The five planes of the definition, and "hits" (int) beside them."""
    tab = pattern(S, lens, footprint, shutter)
    sn = sa = None
    st, hits, first = np.zeros(H * W, F32), np.zeros(H * W, np.int32), np.full(H * W, -1, np.int32)
    for s in range(S):
        h = rt.cast_host(soa, rays(soa.camera, W, H, tab[s], lens))
        sn = h["n"].copy() if s == 0 else sn + h["n"]
        sa = h["albedo"].copy() if s == 0 else sa + h["albedo"]
        hit = h["prim"] >= 0
        st = np.where(hit, np.where(hits > 0, st + h["t"], h["t"]), st)
        first = np.where(hit & (hits == 0), h["prim"], first)
        hits = hits + hit
    with np.errstate(all="ignore"):
        depth = np.where(hits > 0, st / hits.astype(F32), F32(0.0)).astype(F32)
    out = {"normal": (sn / F32(S)).reshape(H, W, 3), "albedo": (sa / F32(S)).reshape(H, W, 3), "depth": depth.reshape(H, W),
           "prim": first.reshape(H, W), "coverage": (hits.astype(F32) / F32(S)).reshape(H, W), "hits": hits.reshape(H, W)}
    assert all(out[k].dtype == F32 for k in ("normal", "albedo", "depth", "coverage"))
    return out


@functools.lru_cache(maxsize=None)
def host_planes(name: str, W: int, H: int, S: int, lens: bool = True, footprint: bool = True, shutter: bool = True) -> dict:
    """rt.guide_host(..., samples=S) of a scene of tests/guide_cases.py, computed once and shared (read only)."""
    import guide_cases as gc

    d = rt.guide_host(gc.soa(name), W, H, samples=S, lens=lens, footprint=footprint, shutter=shutter)
    for a in d.values():
        a.setflags(write=False)
    return d


def same_planes(got: dict, want: dict) -> list:
    """The planes of PLANES that differ in any byte."""
    return [k for k in PLANES if np.ascontiguousarray(got[k]).tobytes() != np.ascontiguousarray(want[k]).tobytes()]
