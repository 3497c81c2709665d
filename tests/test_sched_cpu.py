"""tests/sched_ref.py (the item schedule restated in numpy) on hand-made arrays: the reference that
tests/test_sched_gpu.py holds the device to must itself be what DESIGN.md 3.1d / 3.1e says."""
import numpy as np
import pytest

import sched_ref as sr


def test_source_constants():
    k = sr.source_constants()
    assert k["kOrderTile"] == 4096 and k["kProbeRadius"] == 5, k


def test_item_index_is_row_major_with_the_fb_inside_the_row():
    W, nfb = 7, 2
    seen = [sr.item_index(q, f, i, nfb, W) for q in range(3) for f in range(nfb) for i in range(W)]
    assert seen == list(range(3 * nfb * W))
    segs = [np.arange(5 * W).reshape(5, W), 1000 + np.arange(5 * W).reshape(5, W)]
    cost = sr.oracle_item_costs(segs, [1, 4], W)
    assert cost[sr.item_index(1, 1, 3, nfb, W)] == 1000 + 4 * W + 3
    assert cost[sr.item_index(0, 0, 6, nfb, W)] == 1 * W + 6
    assert sr.oracle_item_costs([np.full((1, 2), 70000)], [0], 2).tolist() == [65535, 65535]


def test_keys_clamp_at_255():
    assert sr.keys_measured([0, 7, 8, 2039, 2040, 65535], 3).tolist() == [0, 0, 1, 254, 255, 255]
    assert sr.keys_measured([254, 255, 256, 4000], 0).tolist() == [254, 255, 255, 255]


def test_shift_measured():
    assert sr.shift_measured(0, True) == 3 and sr.shift_measured(2047, True) == 3  # 2047 >> 3 = 255
    assert sr.shift_measured(2048, True) == 4 and sr.shift_measured(65535, True) == 8
    assert sr.shift_measured(1023, False) == 0 and sr.shift_measured(1024, False) == 1
    assert sr.shift_measured(65535, False) == 6  # 65535 >> 6 = 1023
    assert sr.shift_measured(10**6, False) == 8  # the cap
    assert sr.shift_measured(49, True, cost_shift=0) == 0 and sr.shift_measured(49, True, cost_shift=13) == 12


def test_perm_is_descending_and_stable():
    key = [3, 9, 3, 0, 9, 3]
    assert sr.perm_ref(key).tolist() == [1, 4, 0, 2, 5, 3]


def test_n_long_takes_whole_buckets():
    key = np.array([5] * 3 + [4] * 4 + [1] * 93)
    assert sr.n_long_ref(key, 0.0) == 0
    assert sr.n_long_ref(key, 2.0) == 0   # floor 2 < the top bucket's 3
    assert sr.n_long_ref(key, 3.0) == 3
    assert sr.n_long_ref(key, 6.9) == 3   # floor 6 < 3 + 4
    assert sr.n_long_ref(key, 7.0) == 7
    assert sr.n_long_ref(key, 100.0) == 100
    assert sr.n_long_floor(4608, 2.0) == 92


def test_n_split_counts_the_buckets_from_the_threshold():
    key = np.array([0, 1, 2, 3, 3, 255])
    assert sr.split_bucket(24.0, 3) == 3 and sr.split_bucket(25.0, 3) == 4 and sr.split_bucket(1.0, 3) == 1
    assert sr.n_split_ref(key, 24.0, 3) == 3
    assert sr.n_split_ref(key, 25.0, 3) == 1
    assert sr.n_split_ref(key, 1.0, 3) == 5     # bucket 0 (fewer than 8 segments) stays unsplit
    assert sr.n_split_ref(key, 1.0, 0) == 5
    assert sr.n_split_ref(key, 256.0, 0) == 0   # bucket 256 does not exist: nothing split


def test_smooth_window_rounding_and_clamp():
    r = 5
    raw = np.arange(1, 13 * 14 + 1).reshape(13, 14)
    got = sr.smooth_ref(raw, 13, 14, r).reshape(13, 14)
    for q, i in ((0, 0), (6, 7), (12, 13), (3, 12)):
        win = raw[max(q - r, 0):q + r + 1, max(i - r, 0):i + r + 1]
        assert got[q, i] == (16 * int(win.sum()) + win.size // 2) // win.size
    assert sr.smooth_ref([3], 1, 1, r).tolist() == [48]
    assert sr.smooth_ref([1, 2], 1, 2, r).tolist() == [24, 24]            # 16 * 3 / 2
    assert sr.smooth_ref([1, 1, 2], 1, 3, r).tolist() == [21, 21, 21]     # (64 + 1) // 3
    # clamp: a mean of 4095 segments is 65520, 4096 would be 65536
    assert sr.smooth_ref([4095] * 4, 2, 2, r).tolist() == [65520] * 4
    assert sr.smooth_ref([4096] * 4, 2, 2, r).tolist() == [65535] * 4
    assert sr.smooth_ref([5000, 60000], 1, 2, r).tolist() == [65535] * 2


def test_probe_keys():
    # 3 row positions x 5 pixels, 2 fbs, grid step 2: grid 2 x 3
    smooth = np.array([16 * 8, 16 * 16, 16 * 24, 16 * 800, 0, 16 * 7])
    key = sr.probe_keys_ref(smooth, 3, 5, 2, 4, 2, 3, 3).reshape(3, 2, 5)
    assert key[0, 0].tolist() == [4, 4, 8, 8, 12] and key[1, 1].tolist() == [4, 4, 8, 8, 12]
    assert key[2, 0].tolist() == [255, 255, 0, 0, 3]  # 800 * 4 >> 3 = 400 clamps; 7 * 4 >> 3 = 3
    assert sr.shift_probe(2, True) == 3 and sr.shift_probe(2, False) == 1
    assert sr.shift_probe(63, True) == 3 and sr.shift_probe(64, True) == 4  # 32 * 64 >> 3 = 256
    assert sr.shift_probe(16, False) == 2 and sr.shift_probe(100, True, cost_shift=5) == 5


@pytest.mark.parametrize("top", [0, 1, 7, 64])
@pytest.mark.parametrize("nw", [1, 3, 16])
def test_spread_is_a_permutation(nw, top):
    head = np.arange(64 * nw) + 1000
    got = sr.spread_ref(head, nw, top)
    assert sorted(got.tolist()) == head.tolist()
    if top == 0:
        assert got.tolist() == head.tolist()
    if top == 64:  # position k takes rank (k % 64) * nw + k // 64: a transpose
        assert got.reshape(nw, 64).T.reshape(-1).tolist() == head.tolist()


def test_spread_by_hand():
    """nw = 3, top = 2: every chunk of 64 starts with two strided ranks (c, 3 + c), then 62 neighbours."""
    got = sr.spread_ref(np.arange(192), 3, 2)
    want = [0, 3] + list(range(6, 68)) + [1, 4] + list(range(68, 130)) + [2, 5] + list(range(130, 192))
    assert got.tolist() == want


def test_order_by_hand():
    """2 items, spp 3: item 0 split into samples of 5, 12 and 4 segments, item 1 unsplit in bucket 1 of 8
    segments (midpoint 12): the tie goes to the sample."""
    rk = sr.rest_keys([1], 3)
    assert rk.tolist() == [12]
    assert sr.order_ref([5, 12, 4], rk).tolist() == [1, 3, 0, 2]
    # ties inside each group keep their order; an unsplit key of 256 (clamped midpoint) precedes every sample
    assert sr.rest_keys([255, 40, 31, 0], 3).tolist() == [256, 256, 252, 4]
    assert sr.order_ref([255, 4, 255, 4], [256, 255, 4, 4]).tolist() == [4, 0, 2, 5, 1, 3, 6, 7]
    assert sr.order_ref([], [9, 9, 1]).tolist() == [0, 1, 2]
    assert sr.order_ref([1, 2, 3], []).tolist() == [2, 1, 0]
    assert sr.rest_keys([3, 0], 0).tolist() == [3, 0]  # buckets of one segment: the count itself


def test_order_is_a_permutation():
    g = np.random.default_rng(7)
    sl = g.integers(0, 256, 5000)
    rk = np.sort(sr.rest_keys(g.integers(0, 40, 3000), 3))[::-1]
    got = sr.order_ref(sl, rk)
    assert sorted(got.tolist()) == list(range(8000))
    keys = np.concatenate([sl, rk])[got]
    assert (np.diff(keys) <= 0).all()
    for v in np.unique(keys):  # samples first, each group ascending
        e = got[keys == v]
        s, r = e[e < 5000], e[e >= 5000]
        assert e.tolist() == sorted(s.tolist()) + sorted(r.tolist())
