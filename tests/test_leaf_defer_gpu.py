"""GPU parity of the stepwise kernel's deferred leaf pass (rt_kernels.hip: trav_node, leaf_vote).

A lane of render_step_kernel carries the hit leaf child of a node pair along (`pend`) instead of testing
it in the step that found it; the wave tests the leaves of all its lanes in one pass when a lane holds
more than the one it has room for, when leaf_pass_min lanes hold one (above 64, as shipped: never by
count), and in a flush pass before every shading phase.  Every launch here equals the oracle bit for bit,
segment count included, on the smallest shapes at which each of those triggers is the only one that can
run, or runs together with another.

The triangle-mesh variants keep the immediate pass (two more spilled VGPRs with the deferral), so there
is no door case here; tests/test_schedule_gpu.py and tests/test_flat_gpu.py cover them as before.
"""
import functools

import numpy as np
import pytest

import flat_cases
import test_flat_gpu
from flat_scenes import FlatScene

pytestmark = pytest.mark.gpu

REF, PIX = 0, 1
CAMS = pytest.mark.parametrize("cam", [REF, PIX], ids=["ref", "per_pixel"])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _big1(W, H, spp, nfb, cam):
    """The oracle's frames and segment count of big1 (computed once per shape and camera mode)."""
    from oracle import ref_cpu

    ref = ref_cpu.RefScene("big1")
    out = [ref.render(W, H, spp, f, 50, cam) for f in range(nfb)]
    return [o[0].reshape(H, W, 3) for o in out], sum(int(o[1]["segments"]) for o in out)


def _flat(oracle, scene, W, H, spp, nfb, cam, depth=50):
    ref = oracle.RefScene.from_flat(scene.soa)
    out = [ref.render(W, H, spp, f, depth, cam) for f in range(nfb)]
    return [o[0].reshape(H, W, 3) for o in out], sum(int(o[1]["segments"]) for o in out), \
        {k: sum(int(o[1][k]) for o in out) for k in out[0][1]}


def _launch(rtlib, ctx, W, H, spp, nfb, cam, depth=50, **kw):
    import torch

    args = rtlib.make_args(W, H, spp, 0, nfb, depth, cam, **kw)
    ctx.render_init(W, H, 1984)
    fb = torch.full((nfb * H * W * 3,), float("nan"), dtype=torch.float32, device="cuda")
    try:
        cnt = ctx.render(args, fb.data_ptr())
    except rtlib.RtError as e:
        if e.status == rtlib.RT_ERR_HIP:  # a device error: nothing more starts on this GPU
            pytest.exit(f"{W}x{H} {kw}: {e}", returncode=3)
        raise
    return fb.cpu().numpy().reshape(nfb, H, W, 3), cnt


def _same(got, want, label):
    for f in range(len(want)):
        diff = (_bits(got[f]) != _bits(want[f])).any(axis=2)
        assert not diff.any(), f"{label} fb {f}: {int(diff.sum())} px differ, first at {np.argwhere(diff)[0]}"


@CAMS
@pytest.mark.parametrize("bins", [True, False], ids=["bins", "no_bins"])
@pytest.mark.parametrize("shape", [(1, 1, 64), (8, 1, 8)], ids=["1x1x64", "8x1x8"])
def test_few_lanes_only_the_flush_and_overfull_lanes_test_leaves(rtlib, gpu_ctx, ctx_opts, oracle, shape, bins, cam):
    """One and eight busy lanes in the launch's only busy wave: no count of holding lanes is ever
    reached, so a lane's leaves are tested by the flush before its shading phase (or at once where its
    pair yields two).  With the tile lists (forced on) the camera rays skip the tree and only scattered
    rays traverse; without them every ray does."""
    W, H, spp = shape
    want, segs = _big1(W, H, spp, 1, cam)
    ctx_opts(bins_min_items_per_lane=0.0)
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    got, cnt = _launch(rtlib, gpu_ctx, W, H, spp, 1, cam, bins=bins)
    assert gpu_ctx.last_render_kernel() == "render_step_kernel<25730>", gpu_ctx.last_render_kernel()
    _same(got, want, f"{shape} bins {bins}")
    assert cnt["segments"] == segs


@CAMS
@pytest.mark.parametrize("shape", [(64, 1), (96, 54)], ids=["64x1", "96x54"])
def test_full_and_ragged_waves(rtlib, gpu_ctx, oracle, shape, cam):
    """One exactly full wave, and 81 waves the last of which is ragged (96 x 54 x 2 = 162 x 64 items,
    claimed 64 at a time by waves whose lanes end at different times): the product launch, the exact
    visit set and the oracle agree, and the F_STATS twin returns the product's frames and segments."""
    W, H = shape
    spp = nfb = 2
    want, segs = _big1(W, H, spp, nfb, cam)
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    prod, cnt = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam)
    assert gpu_ctx.last_render_kernel() == "render_step_kernel<25730>", gpu_ctx.last_render_kernel()
    _same(prod, want, "product")
    assert cnt["segments"] == segs
    exact, ecnt = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam, exact=True)
    assert np.array_equal(_bits(exact), _bits(prod)) and ecnt["segments"] == segs
    stats, scnt = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam, stats=True)
    assert gpu_ctx.last_render_kernel() == "render_step_kernel<25731>", gpu_ctx.last_render_kernel()
    assert np.array_equal(_bits(stats), _bits(prod)) and scnt["segments"] == segs


@CAMS
@pytest.mark.parametrize("n", [3, 4, 5])
def test_root_pair_of_leaves(rtlib, gpu_ctx, oracle, n, cam):
    """flat_cases.garden(n) as a BVH world at 48x27: with 3 primitives the traversal tree is a root pair of
    a leaf and a pair of leaves, so a lane's first step can leave it over-full (two hit leaf children),
    and the second finds two more while one is pending; 4 and 5 add one level.  (FlatScene.bvh writes
    reference BVHs of 3 primitives and more, so 3 is the smallest world this writer can state.)"""
    W, H, spp, nfb = 48, 27, 4, 2
    scene = flat_cases.garden(n, n)
    want, segs, _ = _flat(oracle, scene, W, H, spp, nfb, cam)
    gpu_ctx.upload(scene)
    for kw in ({}, dict(lds=False), dict(bins=False), dict(stats=True)):
        got, cnt = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam, **kw)
        assert gpu_ctx.last_render_kernel().split("<")[1] in ("25730>", "25731>", "17538>"), gpu_ctx.last_render_kernel()
        _same(got, want, f"garden({n}) {kw}")
        assert cnt["segments"] == segs, kw


@CAMS
def test_leaf_pending_when_the_stack_overflows(rtlib, gpu_ctx, oracle, cam):
    """deep:chain piles more far children on a lane's stack than it holds while the lane carries a leaf:
    the overflow's fallback to the exact visit set still gives the oracle's pixels (every launch of
    tests/test_flat_gpu.py's harness, the stats twin's fallbacks > 0 included)."""
    kernel = test_flat_gpu._run_case(rtlib, gpu_ctx, oracle, "deep:chain", cam)
    assert kernel.startswith("render_step_kernel<"), kernel


def _duplicates(swap: bool = False) -> FlatScene:
    """Coincident duplicate spheres and moving spheres under one world BVH (the primitives of the
    deferring variants), in both orders of reference rank against position.  Their candidate ranges
    coincide, so the search cannot order them and the query goes to the exact visit set, whose rule
    (the first visited wins) picks the copy of lower rank.  The copies of one sphere sit far apart in
    the primitive order, so the traversal tree meets them in different steps -- one as a carried leaf,
    one in the pass its pair triggers.  swap: the two materials exchanged (the evidence's twin)."""
    s = flat_cases.look(FlatScene())
    red, blue = s.lambertian((0.9, 0.1, 0.1)), s.lambertian((0.1, 0.1, 0.9))
    if swap:
        red, blue = blue, red
    grey = s.metal((0.8, 0.8, 0.8), 0.1)
    spots = [(-1.6, 0.3, 0.4), (0.0, 0.4, 1.0), (1.5, 0.2, 0.6), (-0.7, 0.9, 2.0), (0.9, 1.0, 2.2)]

    def copies(m):
        return [s.sphere(c, 0.45, m) for c in spots[:3]] + \
               [s.moving(c, (c[0] + 0.2, c[1] + 0.3, c[2]), 0.0, 1.0, 0.4, m) for c in spots[3:]]

    first = copies(red)
    fill = [s.sphere((x, 0.15, 3.2), 0.3, grey) for x in (-2.0, -1.0, 0.0, 1.0, 2.0)]
    again = copies(blue)
    s.world.append(s.bvh(first[:2] + again[2:4] + fill + again[:2] + first[2:4] + [first[4], again[4], flat_cases.ground(s)]))
    return s


@CAMS
def test_ties_across_deferred_and_immediate_leaves(rtlib, gpu_ctx, oracle, cam):
    """Coincident duplicate primitives: the copy of lower reference rank still wins, whichever of the
    two the lane tested first.  Evidence on the oracle alone: with the copies' materials exchanged the
    picture changes, so the winners are visible."""
    W, H, spp, nfb = 48, 27, 4, 2
    scene = _duplicates()
    want, segs, _ = _flat(oracle, scene, W, H, spp, nfb, cam)
    twin, _, _ = _flat(oracle, _duplicates(swap=True), W, H, spp, nfb, cam)
    assert not all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(want, twin)), "the ties are not seen"
    gpu_ctx.upload(scene)
    for kw in ({}, dict(lds=False), dict(bins=False), dict(exact=True), dict(step=False)):
        got, cnt = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam, **kw)
        if not kw.get("exact") and kw.get("step", True):  # the sphere variants: the ones that defer
            assert gpu_ctx.last_render_kernel() in ("render_step_kernel<25730>", "render_step_kernel<17538>"), \
                gpu_ctx.last_render_kernel()
        _same(got, want, f"duplicates {kw}")
        assert cnt["segments"] == segs, kw


@CAMS
def test_probe_scheduled_first_launch(rtlib, gpu_ctx, oracle, cam):
    """A one-shot draw (RT_FLAG_FRESH, spp x nfb = 4: probe launch under the F_PROBE twin, which gets the
    same traversal, then the render in the probe's order) at 160x90 equals the natural-order launch bit
    for bit, with its segment count."""
    W, H, spp, nfb = 160, 90, 2, 2
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    base, bcnt = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam, schedule=False)
    assert gpu_ctx.last_render_schedule() == 0
    got, cnt = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam, fresh=True)
    assert gpu_ctx.last_render_schedule() == rtlib.RT_SCHED_PROBE
    assert gpu_ctx.last_render_kernel() == "render_step_kernel<25730>", gpu_ctx.last_render_kernel()
    assert np.array_equal(_bits(got), _bits(base))
    assert cnt["segments"] == bcnt["segments"]
    want, segs = _big1(W, H, spp, nfb, cam)
    _same(got, want, "fresh")
    assert cnt["segments"] == segs
