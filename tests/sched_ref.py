"""The item schedule of rt_kernels.hip restated in numpy: integers only.

Everything here is computed from arrays a context reads back (rt_schedule_read) or from the oracle's
per-pixel segment counts; nothing is taken from the code under test but the documented constants
(source_constants).  tests/test_sched_cpu.py checks these functions on hand-made arrays,
tests/test_sched_gpu.py holds the device to them.
"""
from __future__ import annotations

import math

import numpy as np

from flat_cases import source_constants  # kOrderTile, kProbeRadius (parsed from rt_kernels.hip)  # noqa: F401


def item_index(q, f, i, fb_count: int, W: int):
    """Item of (owned-row position q, fb f, pixel i): row-major, the fb inside the row."""
    return q * (fb_count * W) + f * W + i


def oracle_item_costs(segs, rows, W: int) -> np.ndarray:
    """segs[f]: the oracle's seg_per_pixel of fb f as [H, W]; rows: the owned image rows (rt_owned_rows),
    ascending.  The cost of every item in item order, clamped to 65535 as the kernels record it."""
    rows = np.asarray(rows, np.int64)
    nfb = len(segs)
    out = np.zeros((len(rows), nfb, W), np.int64)
    for f in range(nfb):
        out[:, f, :] = np.asarray(segs[f], np.int64).reshape(-1, W)[rows]
    return np.minimum(out.reshape(-1), 65535)


def keys_measured(cost, shift: int) -> np.ndarray:
    return np.minimum(255, np.asarray(cost, np.int64) >> shift)


def shift_measured(cmax: int, step: bool, cost_shift: int = -1) -> int:
    """Cost buckets of 2^shift segments: from 3 (stepwise kernel) or 0, wider while the largest cost would
    pass bucket 255 (stepwise) or 1023, at most 8.  options.cost_shift >= 0 replaces it (at most 12)."""
    if cost_shift >= 0:
        return min(12, cost_shift)
    shift, top = (3, 255) if step else (0, 1023)
    while shift < 8 and (cmax >> shift) > top:
        shift += 1
    return shift


def perm_ref(key) -> np.ndarray:
    """Descending by key, natural order inside a key."""
    return np.argsort(-np.asarray(key, np.int64), kind="stable").astype(np.int64)


def hist256(key) -> np.ndarray:
    return np.bincount(np.asarray(key, np.int64), minlength=256)[:256]


def n_long_floor(items: int, long_pct: float) -> int:
    return int(math.floor(items * float(long_pct) / 100.0))


def n_long_ref(key, long_pct: float) -> int:
    """Whole buckets from the top while they fit in floor(items * long_pct / 100)."""
    hist = hist256(key)
    want = n_long_floor(len(key), long_pct)
    nl = 0
    for v in range(255, -1, -1):
        if nl + int(hist[v]) > want:
            break
        nl += int(hist[v])
    return nl


def split_bucket(thr: float, shift: int) -> int:
    return int(math.ceil(thr / float(1 << shift)))


def n_split_ref(key, thr: float, shift: int) -> int:
    """Items in the buckets at or above ceil(thr / 2^shift); thr is options.split_min_segments."""
    bt = split_bucket(thr, shift)
    return int(hist256(key)[max(bt, 0):].sum()) if bt <= 255 else 0


def smooth_ref(raw, prow: int, pw: int, radius: int) -> np.ndarray:
    """Mean of the clipped (2 radius + 1)^2 window in 1/16 segment, rounded half up, clamped to 65535."""
    raw = np.asarray(raw, np.int64).reshape(prow, pw)
    s = np.zeros((prow + 1, pw + 1), np.int64)
    s[1:, 1:] = raw.cumsum(0).cumsum(1)
    q, i = np.arange(prow)[:, None], np.arange(pw)[None, :]
    q0, q1 = np.maximum(q - radius, 0), np.minimum(q + radius + 1, prow)
    i0, i1 = np.maximum(i - radius, 0), np.minimum(i + radius + 1, pw)
    total = s[q1, i1] - s[q0, i1] - s[q1, i0] + s[q0, i0]
    n = (q1 - q0) * (i1 - i0)
    return np.minimum(65535, (16 * total + n // 2) // n).reshape(-1)


def shift_probe(spp: int, step: bool, cost_shift: int = -1) -> int:
    if cost_shift >= 0:
        return cost_shift
    shift = 3 if step else 1
    while shift < 12 and ((32 * spp) >> shift) > 255:
        shift += 1
    return shift


def probe_keys_ref(smooth, rows: int, W: int, fb_count: int, spp: int, ps: int, pw: int, shift: int) -> np.ndarray:
    """Key of every item from the smoothed grid point of its (row position // ps, pixel // ps)."""
    sm = np.asarray(smooth, np.int64)
    q = np.arange(rows)[:, None, None]
    i = np.arange(W)[None, None, :]
    v = sm[(q // ps) * pw + i // ps] * spp
    v = np.broadcast_to(v, (rows, fb_count, W))
    return np.minimum(255, v >> (4 + shift)).reshape(-1)


def spread_ref(head, nw: int, top: int) -> np.ndarray:
    """Position k (chunk c = k // 64, lane l = k % 64) of the 64 nw first positions takes rank l nw + c of
    the head for l < top, else rank top nw + c (64 - top) + l - top."""
    head = np.asarray(head)
    k = np.arange(64 * nw)
    c, l = k // 64, k % 64
    src = np.where(l < top, l * nw + c, top * nw + c * (64 - top) + l - top)
    return head[src]


def rest_keys(key_sorted_rest, shift: int) -> np.ndarray:
    """Claim-order key of unsplit positions from their cost buckets: the bucket's midpoint, at most 256."""
    b = np.asarray(key_sorted_rest, np.int64)
    return np.minimum(256, (b << shift) + ((1 << shift) >> 1))


def order_ref(split_len, rest_key) -> np.ndarray:
    """One sequence descending by key over the split samples (keys split_len, entries 0 .. n-1) and the
    unsplit positions (keys rest_key, entries n + r): samples before unsplit positions of the same key,
    each group in its own order."""
    sl = np.asarray(split_len, np.int64)
    rk = np.asarray(rest_key, np.int64)
    n = len(sl)
    keys = np.concatenate([sl, rk])
    group = np.concatenate([np.zeros(n, np.int64), np.ones(len(rk), np.int64)])
    entry = np.arange(n + len(rk), dtype=np.int64)
    # lexsort: last key is the primary one
    return entry[np.lexsort((entry, group, -keys))]
