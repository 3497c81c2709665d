"""The camera-ray culling rule of rt_kernels.hip (TileFrustum, bin_tiles_kernel, bin_masks_kernel) restated in
numpy float64, and the inputs its guarantee is tested with.

The rule: per tile of 2^kTileShift pixels squared, a bounding sphere is kept unless it lies farther than a margin
outside one of the four side planes of the tile's pinhole frustum.  The guarantee: every camera ray of the tile
(any jitter in [0, 1], any lens offset up to the lens radius, any time of the shutter) that hits something
inside a sphere finds that sphere kept, at a distance of at least `nearest`.  tests/test_ctile_cpu.py checks
the restatement on hand-made cameras and spheres, tests/test_ctile_gpu.py holds the device's tables to it.

Nothing is taken from the code under test but kTileShift and kTileCap (source_constants).
"""
from __future__ import annotations

import os
import re

import numpy as np

import raytracing_gpu_amd as rt

F32, F64 = np.float32, np.float64
NEAR_REL = 1e-9  # a plane distance this close to its threshold may fall either way on the device


def source_constants() -> dict:
    """kTileShift and kTileCap as rt_kernels.hip defines them."""
    src = open(os.path.join(os.path.dirname(rt.__file__), "csrc", "rt_kernels.hip")).read()
    return {k: int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("kTileShift", "kTileCap")}


def camera_of(scene) -> dict:
    """The camera record of a scene (anything with .soa, or an rt_scene_soa) as float32 arrays and floats."""
    c = getattr(scene, "soa", scene).camera
    d = {k: np.array(list(getattr(c, k)), F32) for k in ("origin", "lower_left", "horizontal", "vertical", "u", "v", "w")}
    d.update(lens_radius=F32(c.lens_radius), time0=F32(c.time0), time1=F32(c.time1))
    return d


def make_camera(origin, lower_left, horizontal, vertical, lens_radius=0.0, time0=0.0, time1=1.0) -> dict:
    """A hand-made camera record; u and v (the lens plane) are the unit horizontal and vertical."""
    d = {"origin": np.asarray(origin, F32), "lower_left": np.asarray(lower_left, F32),
         "horizontal": np.asarray(horizontal, F32), "vertical": np.asarray(vertical, F32)}
    d["u"] = (d["horizontal"] / np.linalg.norm(d["horizontal"])).astype(F32)
    d["v"] = (d["vertical"] / np.linalg.norm(d["vertical"])).astype(F32)
    d["w"] = np.cross(d["u"], d["v"]).astype(F32)
    d.update(lens_radius=F32(lens_radius), time0=F32(time0), time1=F32(time1))
    return d


def tile_grid(W: int, H: int, shift: int) -> tuple[int, int]:
    ts = 1 << shift
    return (W + ts - 1) >> shift, (H + ts - 1) >> shift


def tile_rect(W: int, H: int, t: int, shift: int) -> tuple[int, int, int, int]:
    """(i0, j0, i1, j1) of tile t: pixels i0 <= i < i1, j0 <= j < j1 (the last column and row may be partial)."""
    tx, _ = tile_grid(W, H, shift)
    i0, j0 = (t % tx) << shift, (t // tx) << shift
    return i0, j0, min(i0 + (1 << shift), W), min(j0 + (1 << shift), H)


def float_rd(m) -> np.ndarray:
    """float64 -> float32 rounded towards -inf; NaN -> -inf."""
    m = np.asarray(m, F64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = m.astype(F32)
        f = np.where(f.astype(F64) > m, np.nextafter(f, F32(-np.inf)), f).astype(F32)
    return np.where(np.isnan(m), F32(-np.inf), f).astype(F32)


class Frustum:
    """TileFrustum::init for tile t of a W x H image, every operation in float64 in the kernel's order."""

    def __init__(self, cam: dict, W: int, H: int, t: int, shift: int):
        i0, j0, i1, j1 = tile_rect(W, H, t, shift)
        us = (F64(i0 - 0.01) / W, F64(i1 + 0.01) / W)
        vs = (F64(j0 - 0.01) / H, F64(j1 + 0.01) / H)
        O = cam["origin"].astype(F64)
        ll, h, v = (cam[k].astype(F64) for k in ("lower_left", "horizontal", "vertical"))
        D = np.zeros((4, 3), F64)
        Dc = np.zeros(3, F64)
        for c, (cu, cv) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):
            D[c] = ((ll + us[cu] * h) + vs[cv] * v) - O
            Dc = Dc + 0.25 * D[c]
        N = np.zeros((4, 3), F64)
        with np.errstate(all="ignore"):
            for c in range(4):
                a, b = D[c], D[(c + 1) & 3]
                m = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
                ln = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
                sg = -1.0 if ((m[0] * Dc[0] + m[1] * Dc[1]) + m[2] * Dc[2]) < 0 else 1.0
                N[c] = sg * m / ln
            nf = np.array([h[1] * v[2] - h[2] * v[1], h[2] * v[0] - h[0] * v[2], h[0] * v[1] - h[1] * v[0]])
            nl = np.sqrt((nf[0] * nf[0] + nf[1] * nf[1]) + nf[2] * nf[2])
            self.dmin = abs((D[0][0] * nf[0] + D[0][1] * nf[1]) + D[0][2] * nf[2]) / nl
        self.L = F64(abs(F32(cam["lens_radius"]))) * (1.0 + 1e-5) + 1e-7
        self.O, self.N, self.D = O, N, D
        self.ok = bool(self.dmin > 2.0 * self.L and self.dmin < 1e30 and not np.isnan(N).any())

    def _rel(self, sph):
        s = np.asarray(sph, F32).reshape(-1, 4).astype(F64)
        C = s[:, :3] - self.O
        with np.errstate(all="ignore"):
            dist = np.sqrt((C[:, 0] * C[:, 0] + C[:, 1] * C[:, 1]) + C[:, 2] * C[:, 2])
        return s, C, dist

    def nearest64(self, sph) -> np.ndarray:
        """Lower bound on the distance from any ray origin of the tile's family to any point of the sphere."""
        s, C, dist = self._rel(sph)
        with np.errstate(all="ignore"):
            return (((dist - s[:, 3]) - self.L) - 1e-5 * ((dist + s[:, 3]) + self.L)) - 1e-6

    def nearest(self, sph) -> np.ndarray:
        return float_rd(self.nearest64(sph))

    def sees(self, sph) -> tuple[np.ndarray, np.ndarray]:
        """(kept[n], near[n]): near marks a sphere with a plane distance within NEAR_REL of its threshold -m."""
        s, C, dist = self._rel(sph)
        with np.errstate(all="ignore"):
            reach = (dist + s[:, 3]) + self.L
            m = ((s[:, 3] + 4e-3 * reach) + self.L * np.maximum(1.0, reach / (self.dmin - self.L))) + 1e-6
            always = ~(m < 1e300)
            pd = (C[:, None, 0] * self.N[None, :, 0] + C[:, None, 1] * self.N[None, :, 1]) + C[:, None, 2] * self.N[None, :, 2]
            drop = (pd < -m[:, None]).any(axis=1)
            near = (np.abs(pd + m[:, None]) <= NEAR_REL * np.abs(m[:, None])).any(axis=1)
        return always | ~drop, near & ~always


class Tables:
    """The rule over every tile: kept[t, q], near[t, q], key[t, q] (float32 `nearest`), ok[t]."""

    def __init__(self, cam: dict, W: int, H: int, sph, shift: int, cap: int):
        self.W, self.H, self.shift, self.cap = W, H, shift, cap
        self.tx, self.ty = tile_grid(W, H, shift)
        nt = self.tx * self.ty
        sph = np.asarray(sph, F32).reshape(-1, 4)
        self.kept = np.ones((nt, len(sph)), bool)
        self.near = np.zeros((nt, len(sph)), bool)
        self.key = np.zeros((nt, len(sph)), F32)
        self.ok = np.zeros(nt, bool)
        for t in range(nt):
            fr = Frustum(cam, W, H, t, shift)
            self.ok[t] = fr.ok
            self.key[t] = fr.nearest(sph)
            if fr.ok:
                self.kept[t], self.near[t] = fr.sees(sph)

    def counts(self) -> np.ndarray:
        """bin_tiles_kernel's cnt: the kept spheres of a tile, -1 when they pass cap or the camera is degenerate."""
        c = self.kept.sum(axis=1)
        return np.where(self.ok & (c <= self.cap), c, -1).astype(np.int64)

    def masks(self) -> np.ndarray:
        """bin_masks_kernel's masks: bit w clear when entry w < min(n, 32) is dropped; every other bit set."""
        n = min(self.kept.shape[1], 32)
        m = np.full(len(self.kept), 0xFFFFFFFF, np.int64)
        for w in range(n):
            m &= ~np.where(self.ok & ~self.kept[:, w], 1 << w, 0)
        return m


def rays_of_tile(cam: dict, W: int, H: int, t: int, n: int, seed: int, shift: int | None = None) -> np.ndarray:
    """n camera rays of tile t's family as (n, 8) float32 rows o[3], d[3], time, 0, in the renderer's float
    arithmetic: s = (i + jitter) / W, o = origin + off, d = lower_left + s horizontal + v vertical - origin - off,
    off = lens_radius (x u + y v) with x^2 + y^2 <= 1.  The first 16 are the tile's four corners (jitter 0 and 1)
    with lens offsets on the rim and times at the shutter ends; of the rest, a quarter lie on the lens rim and a
    quarter at a shutter end.  Not the renderer's own samples: any ray of the family is covered by the rule."""
    shift = source_constants()["kTileShift"] if shift is None else shift
    g = np.random.default_rng([seed, t])
    i0, j0, i1, j1 = tile_rect(W, H, t, shift)
    k = np.arange(n)
    pi = g.integers(i0, i1, n).astype(F32)
    pj = g.integers(j0, j1, n).astype(F32)
    ju, jv = g.random(n, F32), g.random(n, F32)
    ang = g.uniform(0.0, 2.0 * np.pi, n)
    rad = np.sqrt(g.random(n))
    rad[k % 4 == 1] = 1.0  # the rim
    tm = g.random(n, F32)
    tm[k % 4 == 2] = F32(k[k % 4 == 2] % 8 == 2)  # the shutter's ends
    c = min(16, n)
    corner = [(i0, 0.0, j0, 0.0), (i1 - 1, 1.0, j0, 0.0), (i1 - 1, 1.0, j1 - 1, 1.0), (i0, 0.0, j1 - 1, 1.0)]
    for q in range(c):
        pi[q], ju[q], pj[q], jv[q] = corner[q % 4]
        ang[q], rad[q] = (q // 4) * 0.5 * np.pi + 0.25 * np.pi * (q % 2), 1.0
        tm[q] = F32((q // 2) % 2)
    lx = (rad * np.cos(ang)).astype(F32)
    ly = (rad * np.sin(ang)).astype(F32)
    s = ((pi + ju) / F32(W)).astype(F32)[:, None]
    v = ((pj + jv) / F32(H)).astype(F32)[:, None]
    Lr = F32(cam["lens_radius"])
    off = (cam["u"][None, :] * (Lr * lx)[:, None] + cam["v"][None, :] * (Lr * ly)[:, None]).astype(F32)
    o = (cam["origin"][None, :] + off).astype(F32)
    d = ((((cam["lower_left"][None, :] + s * cam["horizontal"][None, :]) + v * cam["vertical"][None, :])
          - cam["origin"][None, :]) - off).astype(F32)
    out = np.zeros((n, 8), F32)
    out[:, :3], out[:, 3:6] = o, d
    out[:, 6] = cam["time0"] + tm * (cam["time1"] - cam["time0"])
    return out


def entry_of_prim(scene) -> np.ndarray:
    """under[p, w]: primitive p lies under top-level entry w of the scene's world list (a primitive of an
    instanced BVH lies under every entry that instances it), found by walking the object table."""
    s = getattr(scene, "soa", scene)
    under = np.zeros((s.n_prims, s.n_world), bool)

    def walk(oi: int, w: int, depth: int = 0):
        o = s.objects[oi]
        assert depth <= 8
        if o.kind == rt.OBJ_PRIM:
            under[o.a, w] = True
        elif o.kind == rt.OBJ_LIST:
            under[o.a:o.a + o.b, w] = True
        elif o.kind == rt.OBJ_BVH:
            for k in range((1 << (o.b - 1)) - 1, (1 << o.b) - 1):  # the last row holds the leaves
                for p in (s.nodes[o.a + k].leaf_a, s.nodes[o.a + k].leaf_b):
                    if p >= 0:
                        under[p, w] = True
        else:  # OBJ_XFORM's child, OBJ_MEDIUM's boundary
            assert o.kind in (rt.OBJ_XFORM, rt.OBJ_MEDIUM)
            walk(o.a, w, depth + 1)

    for w in range(s.n_world):
        walk(s.world[w], w)
    return under


def spheres_of(scene):
    """(p[n, 10] float64, type[n]) of the scene's primitives when every one is a sphere or a moving sphere, else
    None."""
    s = getattr(scene, "soa", scene)
    ty = np.array([s.prims[k].type & 0xFF for k in range(s.n_prims)])
    if not np.isin(ty, (rt.PRIM_SPHERE, rt.PRIM_MOVING_SPHERE)).all():
        return None
    return np.array([list(s.prims[k].p) for k in range(s.n_prims)], F64), ty


def sphere_hits(spheres, rays, t_min: float = 0.001) -> np.ndarray:
    """t[r, p] in float64: the smallest root above t_min of ray r against sphere p (sphere.h's quadratic; a
    moving sphere's centre is c0 + (time - t0) / dt * dc), +inf where there is none."""
    p, ty = spheres
    r = np.asarray(rays, F32).astype(F64)
    o, d, tm = r[:, None, :3], r[:, None, 3:6], r[:, None, 6]
    with np.errstate(all="ignore"):
        mv = (ty == rt.PRIM_MOVING_SPHERE)[None, :]
        f = np.where(mv, (tm - p[None, :, 7]) / np.where(mv, p[None, :, 8], 1.0), 0.0)
        cen = p[None, :, :3] + f[:, :, None] * np.where(mv[:, :, None], p[None, :, 4:7], 0.0)
        oc = o - cen
        a = (d * d).sum(axis=2)
        hb = (oc * d).sum(axis=2)
        c = (oc * oc).sum(axis=2) - p[None, :, 3] ** 2
        disc = hb * hb - a * c
        sq = np.sqrt(np.where(disc > 0, disc, np.nan))
        t1, t2 = (-hb - sq) / a, (-hb + sq) / a
        t = np.where(t1 > t_min, t1, np.where(t2 > t_min, t2, np.inf))
    return np.where(np.isnan(t), np.inf, t)
