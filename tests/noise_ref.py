"""The noise monitor's reference in a few lines of numpy (include/rt_hip.h has the definitions),
shared by tests/test_noise_cpu.py and tests/test_noise_gpu.py: integer moments in uint64, the formula
in float64 in the documented order, tiles of 16 x 16 pixels."""
import ctypes

import numpy as np

TILE = 16
HEADER = 96
MAX_FBS = 32768


def random_fbs(nfb, n, seed, special=False):
    """nfb frame buffers of n values, U(-0.3, 1.3) with exact zeros; special: NaN and +-inf too."""
    rng = np.random.default_rng(seed)
    fbs = rng.uniform(-0.3, 1.3, (nfb, n)).astype(np.float32)
    fbs[rng.random(fbs.shape) < 0.05] = 0.0
    if special:
        for v in (np.nan, np.inf, -np.inf):
            fbs[rng.random(fbs.shape) < 0.03] = v
    return fbs


def quantise(oracle, fbs, W, H):
    """c = quant(fb) per frame buffer through the oracle, in the frame buffer's own order (bottom row
    first): [nfb][H*W*3] uint64."""
    out = []
    for f in fbs:
        q = oracle.quantize_fb(f, W, H)  # PPM order: top row first
        out.append(q.reshape(H, W * 3)[::-1].reshape(-1).astype(np.uint64))
    return np.stack(out)


def moments(c):
    """(S1, S2) of quantised frame buffers c [n][values], uint64."""
    c2 = c * c
    return c2.sum(0, dtype=np.uint64), (c2 * c2).sum(0, dtype=np.uint64)


def noise_map(S1, S2, n, rows, width):
    """[rows][width] float32 noise of n frame buffers with moments S1, S2 (uint64, [rows*width*3])."""
    S1 = np.asarray(S1, np.uint64).reshape(rows, width, 3)
    S2 = np.asarray(S2, np.uint64).reshape(rows, width, 3)
    D = (np.uint64(n) * S2 - S1 * S1).sum(-1, dtype=np.uint64)
    S = S1.sum(-1, dtype=np.uint64)
    a = D.astype(np.float64) / (3.0 * n * n * (n - 1) * 4228250625.0)
    m = S.astype(np.float64) / (3.0 * n * 65025.0)
    m = np.maximum(m, 2.0 ** -16)
    return (128.0 * np.sqrt(a / m)).astype(np.float32)


def tiles(nmap, threshold):
    """(tile_max float32 [ty][tx], tile_above int32 [ty][tx]) of a noise map."""
    rows, width = nmap.shape
    ty, tx = (rows + TILE - 1) // TILE, (width + TILE - 1) // TILE
    tmax, tabove = np.zeros((ty, tx), np.float32), np.zeros((ty, tx), np.int32)
    for y in range(ty):
        for x in range(tx):
            t = nmap[y * TILE:(y + 1) * TILE, x * TILE:(x + 1) * TILE]
            tmax[y, x] = t.max()
            tabove[y, x] = int((t > np.float32(threshold)).sum())
    return tmax, tabove


def ulps(x):
    """Non-negative float32 values as integers that count ulps."""
    return np.asarray(x, np.float32).view(np.uint32).astype(np.int64)


def pick_threshold(nmap):
    """A float32 threshold midway between two adjacent distinct values of the map (the pair nearest the
    middle of the distinct values that lies at least 8 ulp apart), with no value of the map within
    2 ulp of it: a count of values above it cannot depend on one ulp of any value.  Asserts that
    property."""
    v = np.unique(np.asarray(nmap, np.float32))
    assert len(v) >= 3, "the map needs distinct values"
    gaps = np.flatnonzero(np.diff(ulps(v)) >= 8) + 1
    assert len(gaps), "no two adjacent values 8 ulp apart"
    k = int(gaps[np.argmin(np.abs(gaps - len(v) // 2))])
    t = np.float32((np.float64(v[k - 1]) + np.float64(v[k])) / 2)
    assert v[k - 1] < t < v[k]
    assert np.abs(ulps(v) - ulps(t)).min() > 2, "a reference value lies within 2 ulp of the threshold"
    return float(t)


def pack(rtlib, info, S1, S2):
    """rt_noise_blob_pack of uint64 moments (S1 stored as u32)."""
    L = rtlib.lib()
    s1 = np.ascontiguousarray(S1, np.uint32)
    s2 = np.ascontiguousarray(S2, np.uint64)
    need = ctypes.c_size_t()
    assert L.rt_noise_blob_pack(ctypes.byref(info), None, None, None, 0, ctypes.byref(need)) == 0
    assert need.value == HEADER + 12 * s1.size
    buf = ctypes.create_string_buffer(need.value)
    assert L.rt_noise_blob_pack(ctypes.byref(info), s1.ctypes.data, s2.ctypes.data, buf, need.value, None) == 0
    return buf.raw


def blob_measure(rtlib, blob, threshold, rows, width):
    """(status, report dict, tile_max, tile_above, map) of rt_noise_blob_measure."""
    ty, tx = (rows + TILE - 1) // TILE, (width + TILE - 1) // TILE
    tmax, tabove = np.zeros((ty, tx), np.float32), np.zeros((ty, tx), np.int32)
    nmap = np.zeros((rows, width), np.float32)
    rep = rtlib.rt_noise_report()
    rc = rtlib.lib().rt_noise_blob_measure(bytes(blob), len(blob), threshold, ctypes.byref(rep), tmax.ctypes.data,
                                           tabove.ctypes.data, nmap.ctypes.data)
    return rc, rep.as_dict(), tmax, tabove, nmap


def split_blob(blob, n_values):
    """(S1, S2) as uint64 arrays from a monitor's blob."""
    S2 = np.frombuffer(blob, "<u8", n_values, HEADER)
    S1 = np.frombuffer(blob, "<u4", n_values, HEADER + 8 * n_values)
    return S1.astype(np.uint64), S2.copy()
