"""The item schedule read back (rt_schedule_get_info / rt_schedule_read) and held to tests/sched_ref.py.

A pixel does not depend on the order in which items are claimed, so a schedule bug that still yields a
permutation renders the oracle's frames: nothing in the parity tests sees a sort that is not descending or
not stable, a key that wraps, a spread that does not run or a split threshold that selects nothing.  Here
the recorded item costs are compared with the oracle's per-pixel segment counts, and every later stage
(keys, order, long prefix, split items, probe grid, spread head, claim order) with its restatement in numpy
from the arrays read back.  Every launch is also compared with the oracle's frame buffers bit for bit, so a
getter that disturbed the state would show.  Groups as DESIGN.md 4.2 lists them.
"""
import functools

import numpy as np
import pytest

import flat_cases
import sched_ref as sr
from flat_scenes import FlatScene

pytestmark = pytest.mark.gpu

REF, PIX = 0, 1
CAMS = pytest.mark.parametrize("cam", [REF, PIX], ids=["ref", "per_pixel"])
STEP = "render_step_kernel<"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def mirror_box() -> FlatScene:
    """Two nested closed boxes of fuzz-0 metal of albedo 1 around the camera, as one world BVH: a path
    ends only at the depth limit.  (One box leaks: a reflection that starts within hit()'s t_min of the
    next wall passes through it.  The outer box returns such a ray.)"""
    s = FlatScene(aspect=2.0)
    m = s.metal((1.0, 1.0, 1.0), 0.0)
    ids = []
    for a in (2.0, 2.5):
        b = a + 1.0  # the sides overlap at the edges
        ids += [s.rect("xy", -b, b, -b, b, a, m), s.rect("xy", -b, b, -b, b, -a, m), s.rect("xz", -b, b, -b, b, a, m),
                s.rect("xz", -b, b, -b, b, -a, m), s.rect("yz", -b, b, -b, b, a, m), s.rect("yz", -b, b, -b, b, -a, m)]
    s.world = [s.bvh(ids)]
    s.camera((0.3, 0.2, -0.5), (0.1, 0.0, 1.0), 60.0)
    return s


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(what Context.upload takes, the oracle's scene)."""
    import raytracing_gpu_amd as rt
    from oracle import ref_cpu

    if name == "mirror_box":
        s = mirror_box()
        return s, ref_cpu.RefScene.from_flat(s.soa)
    if ":" in name:
        s = flat_cases.get(name).scene
        return s, ref_cpu.RefScene.from_flat(s.soa)
    return rt.Scene.builtin(name), ref_cpu.RefScene(name)


@functools.lru_cache(maxsize=None)
def _oracle(name, W, H, spp, first, nfb, depth, cam):
    """Per fb: the oracle's frame [H, W, 3] and its segments per pixel [H, W]."""
    ref = _scene(name)[1]
    frames, segs = [], []
    for f in range(nfb):
        fb, _, sp = ref.render(W, H, spp, first + f, depth, cam, seg_per_pixel=True)
        frames.append(fb.reshape(H, W, 3))
        segs.append(sp.reshape(H, W).astype(np.int64))
    return frames, segs


class Cfg:
    def __init__(self, name, W, H, spp, nfb, first=0, depth=50, band=None):
        self.name, self.W, self.H, self.spp, self.nfb, self.first, self.depth, self.band = name, W, H, spp, nfb, first, depth, band

    def args(self, rtlib, cam, **kw):
        b = self.band or (0, 0, 1)
        return rtlib.make_args(self.W, self.H, self.spp, self.first, self.nfb, self.depth, cam, band_rows=b[0], band_first=b[1],
                               band_stride=b[2], **kw)

    def __repr__(self):
        return f"{self.name} {self.W}x{self.H} {self.spp}spp x {self.nfb}fb first {self.first} band {self.band}"


def _launch(rtlib, ctx, cfg, cam, **kw):
    """One launch compared with the oracle's frames; returns (owned rows, the oracle's item costs)."""
    import torch

    args = cfg.args(rtlib, cam, **kw)
    rows = rtlib.owned_rows(args)
    ctx.render_init(cfg.W, cfg.H, 1984)
    fb = torch.full((cfg.nfb * len(rows) * cfg.W * 3,), float("nan"), dtype=torch.float32, device="cuda")
    try:
        cnt = ctx.render(args, fb.data_ptr())
    except rtlib.RtError as e:
        if e.status == rtlib.RT_ERR_HIP:  # a device error: nothing more starts on this GPU
            pytest.exit(f"{cfg}: {e}", returncode=3)
        raise
    got = fb.cpu().numpy().reshape(cfg.nfb, len(rows), cfg.W, 3)
    frames, segs = _oracle(cfg.name, cfg.W, cfg.H, cfg.spp, cfg.first, cfg.nfb, cfg.depth, cam)
    for f in range(cfg.nfb):
        diff = (_bits(got[f]) != _bits(frames[f][rows])).any(axis=2)
        assert not diff.any(), f"{cfg} fb {f}: {int(diff.sum())} pixels differ from the oracle"
    assert cnt["samples"] == cfg.nfb * len(rows) * cfg.W * cfg.spp
    return rows, sr.oracle_item_costs(segs, rows, cfg.W)


def _read(rtlib, ctx, which):
    return ctx.schedule_read(which).astype(np.int64)


def _absent(rtlib, ctx, which):
    with pytest.raises(rtlib.RtError) as e:
        ctx.schedule_read(which)
    return e.value.status == rtlib.RT_ERR_STATE


def _is_step(ctx):
    return ctx.last_render_kernel().startswith(STEP)


def _mask(ctx):
    k = ctx.last_render_kernel()
    return int(k[k.index("<") + 1:k.index(">")])


# ------------------------------------------------------------------ a. recorded item costs
COST_CASES = {
    "big1_lds": (Cfg("big1", 64, 36, 2, 2), {}, STEP, flat_cases.F_LDS | flat_cases.F_STEP, 0),
    "big1_7x3_fb37": (Cfg("big1", 7, 3, 5, 2, first=37), {}, STEP, 0, 0),
    "big1_share": (Cfg("big1", 80, 45, 2, 2, band=(4, 1, 3)), {}, STEP, 0, 0),
    "cornell_smoke": (Cfg("cornell_smoke", 48, 48, 4, 2), {}, "render_kernel<", 0, flat_cases.F_STEP),
    "flat_merged": (Cfg("world:two_bvhs", flat_cases.W, flat_cases.H, flat_cases.SPP, flat_cases.NFB), dict(lds=False),
                    "render_kernel<", flat_cases.F_MERGE, flat_cases.F_STEP),
    "flat_step_list": (Cfg("world:bvh_7_prims", flat_cases.W, flat_cases.H, flat_cases.SPP, flat_cases.NFB), {}, STEP,
                       flat_cases.F_STEP, 0),
    "big1_widest": (Cfg("big1", 64, 36, 2, 2), dict(widest=True), "render_kernel<", 0, flat_cases.F_STEP),
    "big1_no_step": (Cfg("big1", 64, 36, 2, 2), dict(step=False), "render_kernel<", 0, flat_cases.F_STEP),
}


@CAMS
@pytest.mark.parametrize("case", list(COST_CASES))
def test_item_costs_equal_the_oracle(rtlib, gpu_ctx, oracle, case, cam):
    """a. The first launch of a configuration (RT_FLAG_FRESH) records every item's segment count: item
    q (fb_count W) + f W + i holds the oracle's count of pixel (owned row q, i) of fb f."""
    cfg, kw, family, has, lacks = COST_CASES[case]
    gpu_ctx.upload(_scene(cfg.name)[0])
    rows, want = _launch(rtlib, gpu_ctx, cfg, cam, fresh=True, **kw)
    assert gpu_ctx.last_render_kernel().startswith(family), gpu_ctx.last_render_kernel()
    assert _mask(gpu_ctx) & has == has and _mask(gpu_ctx) & lacks == 0, gpu_ctx.last_render_kernel()
    info = gpu_ctx.schedule_info()
    assert info["items"] == len(want) == cfg.nfb * len(rows) * cfg.W
    assert info["pending_key_valid"] == 1 and info["perm_key_valid"] == 0
    got = _read(rtlib, gpu_ctx, rtlib.RT_SCHED_ITEM_COST)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{cfg}: {bad.size} item costs differ, first item {bad[:1]}: {got[bad[:1]]} != {want[bad[:1]]}"
    assert len(np.unique(want)) >= 8, "degenerate input"


# ------------------------------------------------------------------ b. the measured schedule
def _check_measured(rtlib, ctx, cfg, cam, opts, want_cost, thr):
    """After the launch that built the schedule: perm, shift, n_long, n_split from the recorded costs."""
    info = ctx.schedule_info()
    cost = _read(rtlib, ctx, rtlib.RT_SCHED_ITEM_COST)
    assert np.array_equal(cost, want_cost)
    assert info["perm_kind"] == 1 and info["perm_key_valid"] == 1 and info["items"] == len(cost) and info["spp"] == cfg.spp
    shift = sr.shift_measured(int(cost.max()), _is_step(ctx), opts["cost_shift"])
    assert info["shift"] == shift, (info, int(cost.max()))
    key = sr.keys_measured(cost, shift)
    perm = _read(rtlib, ctx, rtlib.RT_SCHED_PERM)
    want = sr.perm_ref(key)
    bad = np.flatnonzero(perm != want)
    assert bad.size == 0, f"{cfg} shift {shift}: perm differs at {bad.size} positions, first {bad[:1]}: {perm[bad[:1]]} != {want[bad[:1]]}"
    assert info["n_long"] == sr.n_long_ref(key, opts["long_pct"]), info
    if thr is not None:
        assert info["n_split"] == sr.n_split_ref(key, thr, shift), info
        assert info["rest_n"] == len(cost) - info["n_split"]
    return info, cost, key, perm


MEASURED = {
    "42": Cfg("big1", 7, 3, 2, 2),          # less than one wave: the ballot loop runs with idle lanes
    "4096": Cfg("big1", 64, 32, 2, 2),      # exactly one sort tile
    "4097": Cfg("big1", 241, 17, 4, 1),     # a second tile of one item
    "4608": Cfg("big1", 64, 36, 2, 2),
    "smoke": Cfg("cornell_smoke", 48, 48, 4, 2),  # render_kernel's rule: shift from 0, limit 1023
}


@CAMS
@pytest.mark.parametrize("cost_shift", [-1, 0], ids=["auto", "shift0"])
@pytest.mark.parametrize("case", list(MEASURED))
def test_measured_schedule(rtlib, gpu_ctx, ctx_opts, oracle, case, cost_shift, cam):
    """b. The second launch of a configuration sorts the items by the first one's counts: descending cost
    buckets, natural order inside a bucket (at shift 0 the keys are the exact counts: many distinct keys
    among one wave's 64)."""
    cfg = MEASURED[case]
    assert cfg.nfb * cfg.H * cfg.W == (4608 if case == "smoke" else int(case))
    assert sr.source_constants()["kOrderTile"] == 4096
    ctx_opts(cost_shift=cost_shift, split_min_segments=24.0)
    gpu_ctx.upload(_scene(cfg.name)[0])
    _, want = _launch(rtlib, gpu_ctx, cfg, cam, fresh=True)
    _launch(rtlib, gpu_ctx, cfg, cam)
    assert gpu_ctx.last_render_schedule() & rtlib.RT_SCHED_PREVIOUS
    assert _is_step(gpu_ctx) == (case != "smoke")
    info, cost, key, _ = _check_measured(rtlib, gpu_ctx, cfg, cam, gpu_ctx.options(), want, 24.0)
    if cost_shift == 0 and case != "42":
        assert max(len(np.unique(key[k:k + 64])) for k in range(0, len(key), 64)) >= 12, "one wave's keys are not varied"


@pytest.mark.parametrize("long_pct", [0.0, None, 100.0], ids=["0", "default", "100"])
def test_long_prefix(rtlib, gpu_ctx, ctx_opts, oracle, long_pct):
    cfg = MEASURED["4608"]
    if long_pct is not None:
        ctx_opts(long_pct=long_pct)
    opts = gpu_ctx.options()
    gpu_ctx.upload(_scene(cfg.name)[0])
    _, want = _launch(rtlib, gpu_ctx, cfg, REF, fresh=True)
    _launch(rtlib, gpu_ctx, cfg, REF)
    info, cost, key, _ = _check_measured(rtlib, gpu_ctx, cfg, REF, opts, want, None)
    if long_pct == 0.0:
        assert info["n_long"] == 0
    elif long_pct == 100.0:
        assert info["n_long"] == 4608
    else:
        assert 0 < opts["long_pct"] < 100 and info["n_long"] <= sr.n_long_floor(4608, opts["long_pct"])


@CAMS
def test_top_bucket_saturates_in_natural_order(rtlib, gpu_ctx, ctx_opts, oracle, cam):
    """b. cost_shift 0 with items of 256 segments and more: they share key 255, and perm keeps them in
    natural order in front of everything else."""
    cfg = Cfg("big1", 32, 18, 64, 1)
    ctx_opts(cost_shift=0, split_min_segments=24.0)
    gpu_ctx.upload(_scene(cfg.name)[0])
    _, want = _launch(rtlib, gpu_ctx, cfg, cam, fresh=True)
    top = np.flatnonzero(want >= 255)
    over = np.flatnonzero(want >= 256)
    assert over.size >= 8, over.size
    assert (np.diff(top) > 1).sum() >= 4, "the saturating items are not interleaved with lower ones"
    assert len(np.unique(want[top])) >= 4, "the saturating items all cost the same"
    _launch(rtlib, gpu_ctx, cfg, cam)
    info, cost, key, perm = _check_measured(rtlib, gpu_ctx, cfg, cam, gpu_ctx.options(), want, 24.0)
    assert info["shift"] == 0
    assert np.array_equal(perm[:top.size], top)


# ------------------------------------------------------------------ c. the probe schedule
def _check_probe(rtlib, ctx, cfg, cam, rows, want_cost, opts, raw_oracle=None):
    info = ctx.schedule_info()
    nrows = len(rows)
    ps = info["ps"]
    want_ps = opts["probe_schedule"]
    if want_ps < 0:  # automatic: the smallest step with step^2 spp fb_count >= 200
        want_ps = next(p for p in range(1, 65) if p * p * cfg.spp * cfg.nfb >= 200 or p == 64)
    assert ps == want_ps
    assert info["prow"] == -(-nrows // ps) and info["pw"] == -(-cfg.W // ps) and info["pitems"] == info["prow"] * info["pw"]
    raw = _read(rtlib, ctx, rtlib.RT_SCHED_PROBE_RAW)
    pd = opts["probe_depth"] if opts["probe_depth"] >= 0 else (10 if _is_step(ctx) else 20)
    cap = min(cfg.depth, pd) if pd > 0 else cfg.depth
    assert raw.size == info["pitems"] and raw.min() >= 1 and raw.max() <= cap, (raw.min(), raw.max(), cap)
    if raw_oracle is not None:
        grid = raw_oracle[rows][::ps, ::ps].reshape(-1)
        assert np.array_equal(raw, np.minimum(grid, 65535)), "probe counts differ from the oracle's one-sample counts"
    radius = sr.source_constants()["kProbeRadius"]
    smooth = _read(rtlib, ctx, rtlib.RT_SCHED_PROBE_SMOOTH)
    want_smooth = sr.smooth_ref(raw, info["prow"], info["pw"], radius)
    bad = np.flatnonzero(smooth != want_smooth)
    assert bad.size == 0, f"{bad.size} smoothed grid points differ, first {bad[:1]}: {smooth[bad[:1]]} != {want_smooth[bad[:1]]}"
    shift = sr.shift_probe(cfg.spp, _is_step(ctx), opts["cost_shift"])
    assert info["shift"] == shift and info["perm_kind"] == 2 and info["spp"] == cfg.spp
    key = sr.probe_keys_ref(smooth, nrows, cfg.W, cfg.nfb, cfg.spp, ps, info["pw"], shift)
    want = sr.perm_ref(key)
    if info["spread_ran"]:
        n = 64 * info["spread_waves"]
        want[:n] = sr.spread_ref(want[:n].copy(), info["spread_waves"], info["spread_top"])
    perm = _read(rtlib, ctx, rtlib.RT_SCHED_PERM)
    bad = np.flatnonzero(perm != want)
    assert bad.size == 0, f"{cfg} ps {ps}: perm differs at {bad.size} positions, first {bad[:1]}: {perm[bad[:1]]} != {want[bad[:1]]}"
    assert info["n_long"] == sr.n_long_floor(len(key), opts["long_pct"])
    assert info["n_split"] == 0 and info["split_state"] == -1 and info["perm_key_valid"] == 0 and info["pending_key_valid"] == 1
    # the probe-scheduled launch is the measuring one
    assert np.array_equal(_read(rtlib, ctx, rtlib.RT_SCHED_ITEM_COST), want_cost)
    return info, raw, smooth, key, perm


@CAMS
@pytest.mark.parametrize("band", [None, (3, 1, 2)], ids=["full", "band"])
@pytest.mark.parametrize("ps", [1, 3, 7, -1], ids=["ps1", "ps3", "ps7", "auto"])
@pytest.mark.parametrize("scene", ["big1", "world:two_bvhs"])
def test_probe_schedule(rtlib, gpu_ctx, ctx_opts, oracle, scene, ps, band, cam):
    """c. A first launch orders its items by a probe: one sample at every ps-th row position and pixel
    (last grid row and column partial), smoothed over 11 x 11 grid points, times spp, in cost buckets."""
    cfg = Cfg(scene, 80, 45, 8, 2, band=band)
    kw = {} if scene == "big1" else dict(lds=False)  # the list world: render_kernel's F_BVH variants probe
    # buckets of one segment at the explicit steps (the oracle's one-sample counts give 19 to 29 distinct keys at
    # step 1, 8 to 13 at 3, 3 to 6 at 7, where the 11 x 11 window covers most of the 12 x 7 grid); the automatic
    # buckets of 8 segments, which hold two or three keys at this size, with the automatic step
    ctx_opts(probe_schedule=ps, probe_depth=0 if ps in (1, 7) else -1, spread_first=0, cost_shift=0 if ps > 0 else -1)
    opts = gpu_ctx.options()
    gpu_ctx.upload(_scene(cfg.name)[0])
    rows, want = _launch(rtlib, gpu_ctx, cfg, cam, fresh=True, **kw)
    assert gpu_ctx.last_render_schedule() == rtlib.RT_SCHED_PROBE
    assert _is_step(gpu_ctx) == (scene == "big1")
    raw_oracle = None
    if opts["probe_depth"] == 0:  # sample 0 of the first fb: a one-sample render of the oracle makes the same draws
        raw_oracle = _oracle(cfg.name, cfg.W, cfg.H, 1, cfg.first, 1, cfg.depth, cam)[1][0]
    info, raw, smooth, key, _ = _check_probe(rtlib, gpu_ctx, cfg, cam, rows, want, opts, raw_oracle)
    if opts["probe_depth"] == 0:
        assert len(np.unique(key)) >= (16 if ps == 1 else 3), "degenerate input"


def test_probe_means_above_4095_segments_clamp(rtlib, gpu_ctx, ctx_opts, oracle):
    """c / advisor finding 3.  Camera inside closed mirror boxes at max_depth 5000: every probed path has
    thousands of segments, the 11 x 11 means exceed 4095 segments = 65535 sixteenths, and the smoothed
    grid must saturate there.  Before the clamp in probe_smooth_kernel the stored mean wrapped modulo 2^16
    (a mean of 5000 segments became 14464 sixteenths = 904 segments), which sorts the costliest region
    behind cheaper ones.  On a library without the clamp this test fails with all 128 smoothed grid points
    differing, the first holding 2155 where 65535 is due."""
    cfg = Cfg("mirror_box", 16, 8, 2, 2, depth=5000)
    # cost_shift is set: no stepwise variant is compiled for this world's features, so the launch runs
    # render_kernel, while the automatic buckets follow the world's shape and stay the stepwise kernel's
    # (DESIGN.md 7); the rule for the automatic shift is checked on big1 and two_bvhs above
    ctx_opts(probe_schedule=1, probe_depth=0, spread_first=0, cost_shift=3)
    opts = gpu_ctx.options()
    one = _oracle(cfg.name, cfg.W, cfg.H, 1, 0, 1, cfg.depth, REF)[1][0]
    radius = sr.source_constants()["kProbeRadius"]
    exact = [(16 * int(one[max(q - radius, 0):q + radius + 1, max(i - radius, 0):i + radius + 1].sum())) /
             one[max(q - radius, 0):q + radius + 1, max(i - radius, 0):i + radius + 1].size for q in range(cfg.H) for i in range(cfg.W)]
    assert max(exact) > 16 * 4095, max(exact)
    gpu_ctx.upload(_scene(cfg.name)[0])
    rows, want = _launch(rtlib, gpu_ctx, cfg, REF, fresh=True)
    assert gpu_ctx.last_render_schedule() == rtlib.RT_SCHED_PROBE
    info, raw, smooth, key, perm = _check_probe(rtlib, gpu_ctx, cfg, REF, rows, want, opts, one)
    assert smooth.max() == 65535 and (smooth[np.array(exact) > 16 * 4095] == 65535).all()


# ------------------------------------------------------------------ d. the spread head
@pytest.mark.parametrize("top", [1, 7, 64])
def test_spread_head(rtlib, gpu_ctx, ctx_opts, oracle, top):
    """d. options.spread_first on a launch of at least 64 x waves items (waves from the info of a small
    launch of the same kernel on this device): the info says the spread ran and the head is spread_ref's."""
    ctx_opts(spread_first=top, probe_schedule=3)
    opts = gpu_ctx.options()
    gpu_ctx.upload(_scene("big1")[0])
    small = Cfg("big1", 64, 36, 2, 2)
    rows, want = _launch(rtlib, gpu_ctx, small, REF, fresh=True)
    info = gpu_ctx.schedule_info()
    waves = info["spread_waves"]
    assert waves > 0 and info["spread_top"] == top
    assert 4608 < 64 * waves and info["spread_ran"] == 0  # too few items: the plain sort (checked in _check_probe)
    _check_probe(rtlib, gpu_ctx, small, REF, rows, want, opts)
    W = 640
    H = -(-64 * waves // (2 * W))
    cfg = Cfg("big1", W, H, 2, 2)
    rows, want = _launch(rtlib, gpu_ctx, cfg, REF, fresh=True)
    info = gpu_ctx.schedule_info()
    assert info["spread_waves"] == waves and info["items"] >= 64 * waves
    assert info["spread_ran"] == 1 and info["spread_top"] == top, info
    _, _, _, key, perm = _check_probe(rtlib, gpu_ctx, cfg, REF, rows, want, opts)
    plain = sr.perm_ref(key)
    assert not np.array_equal(perm[:64 * waves], plain[:64 * waves]), "the spread changed nothing: degenerate input"


# ------------------------------------------------------------------ e. the split claim order
def _split_run(rtlib, ctx, cfg, cam, **kw):
    """measure, record, replay"""
    seen = []
    for k in range(3):
        rows, want = _launch(rtlib, ctx, cfg, cam, fresh=k == 0, **kw)
        seen.append(ctx.last_render_schedule())
    return want, seen


def _check_split(rtlib, ctx, cfg, cam, want, thr, ordered=True):
    info, cost, key, perm = _check_measured(rtlib, ctx, cfg, cam, ctx.options(), want, thr)
    ns, shift = info["n_split"], info["shift"]
    bt = sr.split_bucket(thr, shift)
    assert ns > 0 and info["split_state"] == 1
    assert np.array_equal(np.sort(perm[:ns]), np.flatnonzero(key >= bt))
    sl = _read(rtlib, ctx, rtlib.RT_SCHED_SPLIT_LEN)
    assert sl.size == ns * cfg.spp
    per = sl.reshape(ns, cfg.spp)
    exact = (per < 255).all(axis=1)
    assert exact.any()
    assert np.array_equal(per.sum(axis=1)[exact], cost[perm[:ns]][exact]), "split sample lengths do not add up to their item's cost"
    if not ordered:
        assert info["order_ok"] == 0 and _absent(rtlib, ctx, rtlib.RT_SCHED_ORDER)
        return info
    assert info["order_ok"] == 1
    order = _read(rtlib, ctx, rtlib.RT_SCHED_ORDER)
    want_order = sr.order_ref(sl, sr.rest_keys(key[perm[ns:]], shift))
    assert order.size == ns * cfg.spp + info["rest_n"]
    bad = np.flatnonzero(order != want_order)
    assert bad.size == 0, f"{cfg} thr {thr}: claim order differs at {bad.size} positions, first {bad[:1]}: {order[bad[:1]]} != {want_order[bad[:1]]}"
    return info


@CAMS
@pytest.mark.parametrize("thr", [1.0, 24.0], ids=["every_item", "thr24"])
@pytest.mark.parametrize("shape", [(4, 2), (8, 1)], ids=["4spp_2fb", "8spp_1fb"])
def test_split_claim_order(rtlib, gpu_ctx, ctx_opts, oracle, shape, thr, cam):
    """e. Measure, record, replay: the split items are perm's first n_split positions, their recorded
    sample lengths add up to the item's measured cost, and the replay claims samples and unsplit items in
    one sequence, longest first, samples before unsplit items of the same key."""
    cfg = Cfg("big1", 64, 36, shape[0], shape[1])
    ctx_opts(split_min_segments=thr)
    gpu_ctx.upload(_scene("big1")[0])
    want, seen = _split_run(rtlib, gpu_ctx, cfg, cam)
    assert seen[1] & rtlib.RT_SCHED_PREVIOUS and seen[2] == rtlib.RT_SCHED_PREVIOUS | rtlib.RT_SCHED_SPLIT_REPLAY, seen
    info = _check_split(rtlib, gpu_ctx, cfg, cam, want, thr)
    if thr == 24.0:
        assert 0 < info["n_split"] < info["items"] and info["rest_n"] > 0


def test_split_threshold_above_every_cost(rtlib, gpu_ctx, ctx_opts, oracle):
    cfg = Cfg("big1", 64, 36, 4, 2)
    gpu_ctx.upload(_scene("big1")[0])
    segs = _oracle(cfg.name, cfg.W, cfg.H, cfg.spp, 0, cfg.nfb, cfg.depth, REF)[1]
    thr = float(8 * (max(int(s.max()) for s in segs) // 8 + 2))  # above the largest cost's bucket
    ctx_opts(split_min_segments=thr)
    want, seen = _split_run(rtlib, gpu_ctx, cfg, REF)
    assert seen[2] == rtlib.RT_SCHED_PREVIOUS, seen
    info, *_ = _check_measured(rtlib, gpu_ctx, cfg, REF, gpu_ctx.options(), want, thr)
    assert info["n_split"] == 0 and info["split_state"] == -1 and info["order_ok"] == 0
    assert _absent(rtlib, gpu_ctx, rtlib.RT_SCHED_ORDER) and _absent(rtlib, gpu_ctx, rtlib.RT_SCHED_SPLIT_LEN)


def test_split_without_claim_order(rtlib, gpu_ctx, ctx_opts, oracle):
    cfg = Cfg("big1", 64, 36, 4, 2)
    ctx_opts(split_min_segments=24.0, split_order=0)
    gpu_ctx.upload(_scene("big1")[0])
    want, seen = _split_run(rtlib, gpu_ctx, cfg, REF)
    assert seen[2] == rtlib.RT_SCHED_PREVIOUS | rtlib.RT_SCHED_SPLIT_REPLAY, seen
    _check_split(rtlib, gpu_ctx, cfg, REF, want, 24.0, ordered=False)


def test_split_render_kernel_parking_variant(rtlib, gpu_ctx, ctx_opts, oracle):
    """e. render_kernel's parking variants split too (cornell_smoke, a list of rects, boxes and media, on the
    widest variant from global memory); split_min_segments keeps the threshold bucket within the 256 keys."""
    cfg = Cfg("cornell_smoke", 48, 48, 4, 2)
    ctx_opts(split_min_segments=24.0)
    gpu_ctx.upload(_scene(cfg.name)[0])
    want, seen = _split_run(rtlib, gpu_ctx, cfg, REF, widest=True, lds=False)
    assert not _is_step(gpu_ctx) and _mask(gpu_ctx) & flat_cases.F_LDS == 0
    assert seen[2] == rtlib.RT_SCHED_PREVIOUS | rtlib.RT_SCHED_SPLIT_REPLAY, seen
    _check_split(rtlib, gpu_ctx, cfg, REF, want, 24.0)


# ------------------------------------------------------------------ the getter changes nothing
def test_tile_launch_and_reads_leave_the_schedule_alone(rtlib, gpu_ctx, ctx_opts, oracle):
    """rt_render_tiles between two launches, and the read-backs themselves, leave every array and the info
    as they were; the launch after them replays as if nothing had happened."""
    import torch

    cfg = Cfg("big1", 64, 36, 4, 2)
    ctx_opts(split_min_segments=24.0)
    gpu_ctx.upload(_scene("big1")[0])
    want, seen = _split_run(rtlib, gpu_ctx, cfg, REF)
    _check_split(rtlib, gpu_ctx, cfg, REF, want, 24.0)
    kinds = (rtlib.RT_SCHED_ITEM_COST, rtlib.RT_SCHED_PERM, rtlib.RT_SCHED_PROBE_RAW, rtlib.RT_SCHED_PROBE_SMOOTH,
             rtlib.RT_SCHED_SPLIT_LEN, rtlib.RT_SCHED_ORDER)
    before = (gpu_ctx.schedule_info(), [_read(rtlib, gpu_ctx, k) for k in kinds])
    fb = torch.zeros(cfg.nfb * cfg.H * cfg.W * 3, dtype=torch.float32, device="cuda")
    gpu_ctx.render_init(cfg.W, cfg.H, 1984)
    gpu_ctx.render_tiles(cfg.args(rtlib, REF), [0, 5], fb.data_ptr())
    after = (gpu_ctx.schedule_info(), [_read(rtlib, gpu_ctx, k) for k in kinds])
    assert before[0] == after[0]
    for k, a, b in zip(kinds, before[1], after[1]):
        assert np.array_equal(a, b), k
    _launch(rtlib, gpu_ctx, cfg, REF)
    assert gpu_ctx.last_render_schedule() == rtlib.RT_SCHED_PREVIOUS | rtlib.RT_SCHED_SPLIT_REPLAY
    assert gpu_ctx.schedule_info() == before[0]


def test_read_conventions(rtlib, gpu_ctx, oracle):
    """RT_ERR_STATE for an array the context does not hold, RT_ERR_ARG for an unknown one and for a short
    buffer (with the size reported)."""
    import ctypes

    ctx = rtlib.Context(0)
    try:
        for k in range(6):
            assert _absent(rtlib, ctx, k)
        with pytest.raises(rtlib.RtError) as e:
            ctx.schedule_read(6)
        assert e.value.status == rtlib.RT_ERR_ARG
        assert ctx.schedule_info()["items"] == 0 and ctx.schedule_info()["perm_kind"] == 0
    finally:
        ctx.close()
    cfg = Cfg("big1", 7, 3, 2, 2)
    gpu_ctx.upload(_scene("big1")[0])
    _launch(rtlib, gpu_ctx, cfg, REF, fresh=True)
    need = ctypes.c_size_t(0)
    buf = np.full(42 * 2, 0xAB, np.uint8)
    rc = rtlib.lib().rt_schedule_read(gpu_ctx._c, rtlib.RT_SCHED_ITEM_COST, buf.ctypes.data, 10, ctypes.byref(need))
    assert rc == rtlib.RT_ERR_ARG and need.value == 84 and (buf == 0xAB).all()
