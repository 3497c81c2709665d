"""GPU parity of the miss-first pass order of render_step_kernel's sphere variants (<25730>, <25731>, <17538>,
the probe <287874>), both bodies.

A shading pass of these variants first ends the searches that certainly missed (block A), refills, sets up
the camera rays (Q) and then runs the heavy block once (C: settle, hit record, scatter) for bounce hits and
listed camera hits together.  Per lane nothing may change, so every case compares every float of every frame
buffer with the CPU oracle bit for bit, together with the segment and sample counts.  The scenes are written
ones (flat_scenes.py, flat_cases.py) built around what each block does: nothing but misses, nothing but hits,
a horizon that crosses tiles, paths that end inside C (the depth limit, fuzzed metal that absorbs), a world
with a primitive entry after its BVH (A must decline), camera rays that traverse, both camera modes, the
twins, split launches and a probe-scheduled launch.
"""
import functools

import numpy as np
import pytest

import flat_cases
from flat_cases import PIX, REF
from flat_scenes import FlatScene

pytestmark = pytest.mark.gpu

PLAIN, GENERAL = 1, 0
SPHERE = ("render_step_kernel<25730>", "render_step_kernel<25731>", "render_step_kernel<17538>")
W0, H0 = 64, 40


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _garden():
    return flat_cases.garden(17, 3)  # a BVH of 16 spheres and the ground as the whole world


def _sky():
    s = _garden()
    s.camera((0.0, 1.6, -5.0), (0.0, 60.0, -4.0), 30.0)  # straight up: no ray meets anything
    return s


def _floor():
    s = _garden()
    s.camera((0.0, 3.0, 1.0), (0.0, 0.0, 1.1), 40.0, vup=(0, 0, 1))  # straight down: every camera ray hits
    return s


def _metal():
    s = flat_cases.look(FlatScene())
    m = s.metal((0.8, 0.8, 0.8), 1.0)  # fuzz 1: many scattered rays point into the surface and are absorbed
    s.world.append(s.bvh(flat_cases.grid_spheres(s, 12, [m], 5) + [flat_cases.ground(s, m)]))
    return s


def _trailing():
    return flat_cases.world_shape("bvh_7_prims")  # a BVH, then six primitive entries and the ground


SCENES = {"garden": _garden, "sky": _sky, "floor": _floor, "metal": _metal, "trailing": _trailing}


@functools.lru_cache(maxsize=None)
def _scene(key):
    return SCENES[key]()


@functools.lru_cache(maxsize=None)
def _want(key, W, H, spp, nfb, depth, cam):
    """The oracle's frame buffers [H, W, 3], one per fb, and its counters summed over the fbs."""
    from oracle import ref_cpu

    ref = ref_cpu.RefScene.from_flat(_scene(key).soa)
    fbs, tot = [], None
    for f in range(nfb):
        fb, c, _ = ref.render(W, H, spp, f, depth, cam)
        fbs.append(fb.reshape(H, W, 3))
        tot = dict(c) if tot is None else {k: tot[k] + c[k] for k in tot}
    return fbs, tot


def _sees_sky(key):
    """[H0, W0] bool from the oracle at depth 1, where a path that hits anything ends black at the depth limit
    (no scene here has a light) and a miss adds the background: a pixel some sample of which misses."""
    return np.stack(_want(key, W0, H0, 4, 2, 1, REF)[0]).any(axis=(0, 3))


def _launch(rtlib, ctx, W, H, spp, nfb, depth, cam, **kw):
    import torch

    args = rtlib.make_args(W, H, spp, 0, nfb, depth, cam, **kw)
    ctx.render_init(W, H, 1984)
    fb = torch.full((nfb * H * W * 3,), float("nan"), dtype=torch.float32, device="cuda")
    cnt = ctx.render(args, fb.data_ptr())
    return fb.cpu().numpy().reshape(nfb, H, W, 3), cnt


def _check(got, cnt, key, W, H, spp, nfb, depth, cam, what=""):
    fbs, tot = _want(key, W, H, spp, nfb, depth, cam)
    for f in range(nfb):
        diff = (_bits(got[f]) != _bits(fbs[f])).any(axis=2)
        assert not diff.any(), f"{what} fb {f}: {int(diff.sum())} pixels differ, first at {np.argwhere(diff)[0]}"
    assert cnt["segments"] == tot["segments"], what
    assert cnt["samples"] == nfb * H * W * spp, what
    return tot


def _run(rtlib, ctx, key, W=W0, H=H0, spp=4, nfb=2, depth=50, cam=REF, body=PLAIN, kernel=SPHERE[0], **kw):
    ctx.upload(_scene(key))
    got, cnt = _launch(rtlib, ctx, W, H, spp, nfb, depth, cam, **kw)
    assert ctx.last_render_kernel() == kernel, ctx.last_render_kernel()
    assert ctx.last_render_body() == body
    return cnt, _check(got, cnt, key, W, H, spp, nfb, depth, cam)


# ---------------------------------------------------------------- 1. what the camera sees
@pytest.mark.parametrize("spp", [1, 4])
def test_sky_only(rtlib, gpu_ctx, oracle, spp):
    """Every sample is one miss: block A ends it, the refill and Q follow, C never has a lane."""
    cnt, tot = _run(rtlib, gpu_ctx, "sky", spp=spp)
    assert tot["segments"] == 2 * W0 * H0 * spp, "the camera sees something"


def test_every_camera_ray_hits(rtlib, gpu_ctx, oracle):
    """No camera ray misses, so A sees bounce misses only and every listed camera ray goes through C."""
    _run(rtlib, gpu_ctx, "floor")
    assert not _sees_sky("floor").any(), "a camera ray misses"


def test_horizon_crosses_tiles(rtlib, gpu_ctx, oracle):
    """Sky above, spheres and ground below: waves hold camera misses, camera hits and bounces together."""
    _run(rtlib, gpu_ctx, "garden")
    sky = _sees_sky("garden")
    t = sky.reshape(H0 // 8, 8, W0 // 8, 8)  # the camera tiles are 8 x 8 pixels (kTileShift 3)
    mixed = t.any(axis=(1, 3)) & (~t).any(axis=(1, 3))
    assert mixed.any(), "no 8 x 8 camera tile holds both sky and surface"


# ---------------------------------------------------------------- 2. item counts around one wave
@pytest.mark.parametrize("W,H", [(35, 1), (32, 2), (13, 5)], ids=["35", "64", "65"])
def test_item_counts(rtlib, gpu_ctx, oracle, W, H):
    """35, 64 and 65 items: less than a wave, exactly one chunk, one chunk and one lane of the next."""
    _run(rtlib, gpu_ctx, "garden", W=W, H=H, nfb=1)


# ---------------------------------------------------------------- 3. paths that end inside C
@pytest.mark.parametrize("depth", [1, 2])
def test_depth_limit(rtlib, gpu_ctx, oracle, depth):
    """max_depth 1 and 2: every hit path ends at the depth limit, inside C, and starts its next sample in a
    later pass with its table entry read at that camera setup."""
    cnt, tot = _run(rtlib, gpu_ctx, "garden", depth=depth)
    assert tot["segments"] <= depth * 2 * W0 * H0 * 4


@pytest.mark.parametrize("cam", [REF, PIX], ids=["ref", "per_pixel"])
def test_fuzzed_metal_absorbs(rtlib, gpu_ctx, oracle, cam):
    """Nothing but metal of fuzz 1: paths end by no-scatter inside C.  Evidence: with a bright sky and depth 50
    a path ends black only when it is absorbed, and some pixel below the horizon is black in the oracle."""
    _run(rtlib, gpu_ctx, "metal", cam=cam)
    img = np.stack(_want("metal", W0, H0, 4, 2, 50, cam)[0])
    assert (~img.any(axis=3)).any(), "no pixel whose every sample was absorbed"


def test_primitive_entry_after_the_bvh(rtlib, gpu_ctx, oracle):
    """n_world > 1: a search without a candidate may still hit a trailing entry, so A declines every lane."""
    cnt, tot = _run(rtlib, gpu_ctx, "trailing", W=40, H=24)


# ---------------------------------------------------------------- 4. launch kinds
def test_camera_rays_traverse(rtlib, gpu_ctx, oracle):
    """bins=False: no tile lists, camera rays go to mode 1 and only traversals reach A and C."""
    _run(rtlib, gpu_ctx, "garden", bins=False)
    assert gpu_ctx.camera_tiles_info()["last_used"] == 0


def test_per_pixel_camera(rtlib, gpu_ctx, oracle):
    _run(rtlib, gpu_ctx, "garden", cam=PIX)


def test_counting_twin(rtlib, gpu_ctx, oracle):
    """<25731>, the stepwise kernel with the node / primitive / fallback counters, in both bodies: the oracle's
    pixels, segments and samples, and counters that count.

    What its counters can be held to: block A skips a settle that tests and counts nothing, so per search the
    reorder adds and removes no test.  But the culled search's node and primitive totals are not a function
    of the scene in either order: a lane's leaf test waits for the wave's vote (the deferred leaf pass) and
    is culled against the `bhi` it has by then, and which lanes share a wave follows the work counter's
    timing.  Measured (profiles/r16/stats_repeat.txt): at 600 x 400 four launches of ONE library give four
    different node totals (137 926 975 .. 137 939 435, the parent's library too), so the totals vary from run
    to run; at 64 x 36 each library repeats its own total and the two orders differ by 60 in 994 317.  So
    there is no reference for the culled totals to equal; the exact visit set, which has one, runs render_kernel<3203> (no step variant
    carries F_EXACT) and is tests/test_parity_gpu.py's.  Here: the order-invariant figures exactly, and the
    culled totals only as counters that run: positive, node tests below the reference visit set's."""
    gpu_ctx.upload(_scene("garden"))
    tot = _want("garden", W0, H0, 4, 2, 50, REF)[1]
    body = []
    for k in range(2):  # cold: the plain body; the repeat is scheduled and records split items: the general body
        got, fast = _launch(rtlib, gpu_ctx, W0, H0, 4, 2, 50, REF, stats=True)
        assert gpu_ctx.last_render_kernel() == SPHERE[1]
        body.append(gpu_ctx.last_render_body())
        _check(got, fast, "garden", W0, H0, 4, 2, 50, REF, what=f"launch {k}")
        assert 0 < fast["node_tests"] < tot["node_tests"] and fast["prim_tests"] > 0, fast
    assert body[0] == PLAIN, body


def test_global_memory_twin(rtlib, gpu_ctx, oracle):
    _run(rtlib, gpu_ctx, "garden", kernel=SPHERE[2], lds=False)


def test_probe_scheduled_first_launch(rtlib, gpu_ctx, oracle):
    """RT_FLAG_FRESH with 8 samples per pixel over the frame buffers: the probe <287874> runs first."""
    _run(rtlib, gpu_ctx, "garden", fresh=True)
    assert gpu_ctx.last_render_schedule() == rtlib.RT_SCHED_PROBE


@pytest.mark.parametrize("cam", [REF, PIX], ids=["ref", "per_pixel"])
def test_warm_sequence_through_both_split_modes(rtlib, gpu_ctx, ctx_opts, oracle, cam):
    """Plain, recording (split_mode 1: ckpt written at a sample's start and at the item's end) and replay
    (split_mode 2: every sample an item of its own), the last two in the general body."""
    ctx_opts(split_min_segments=1.0)
    spp, nfb = 3, 2
    gpu_ctx.upload(_scene("garden"))
    sched, body = [], []
    for k in range(3):
        got, cnt = _launch(rtlib, gpu_ctx, W0, H0, spp, nfb, 50, cam)
        sched.append(gpu_ctx.last_render_schedule())
        body.append(gpu_ctx.last_render_body())
        assert gpu_ctx.last_render_kernel() == SPHERE[0]
        _check(got, cnt, "garden", W0, H0, spp, nfb, 50, cam, what=f"launch {k}")
    assert sched[1] & rtlib.RT_SCHED_PREVIOUS and sched[2] & rtlib.RT_SCHED_PREVIOUS, sched
    assert sched[2] & rtlib.RT_SCHED_SPLIT_REPLAY and not sched[1] & rtlib.RT_SCHED_SPLIT_REPLAY, sched
    assert body == [PLAIN, GENERAL, GENERAL], body
