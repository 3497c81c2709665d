"""GPU parity of the shading passes of render_step_kernel's sphere variants (<25730>, <25731>, <17538>, the
probe <287874>), both bodies.

In the REF camera mode these variants take the lens offset and time of sample s from the camera table
(cam_tab[s], read from global memory where s is set: there is no LDS copy, so no cap on spp), and their
shading passes re-read the arguments that only they use from the argument segment.  Neither may show: every
case is big1 at depth 50, seed 1984, and compares every float of every frame buffer with the CPU oracle bit
for bit, with the oracle's segment count over the rendered pixels and the sample count.

The oracle knows one seed, 1984.  The launch with another seed in test_stale_table is compared with
render_kernel (step=False, code this file does not cover) on a context of its own that never held another
table.
"""
import functools

import numpy as np
import pytest

import adapt_ref as ar

pytestmark = pytest.mark.gpu

REF, PIX = 0, 1
CAMS = pytest.mark.parametrize("cam", [REF, PIX], ids=["ref", "per_pixel"])
PLAIN, GENERAL = 1, 0
STEP = "render_step_kernel<25730>"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _want(W, H, spp, nfb, cam):
    """Per fb: the oracle's frame buffer [H, W, 3] and its segments per pixel [H, W]."""
    from oracle import ref_cpu

    ref = ref_cpu.RefScene("big1")
    out = []
    for f in range(nfb):
        fb, _, segs = ref.render(W, H, spp, f, 50, cam, seg_per_pixel=True)
        out.append((fb.reshape(H, W, 3), segs.reshape(H, W)))
    return out


def _launch(rtlib, ctx, W, H, spp, nfb, cam, init=True, seed=1984, **kw):
    import torch

    args = rtlib.make_args(W, H, spp, 0, nfb, 50, cam, seed=seed, **kw)
    rows = rtlib.owned_rows(args)
    if init:
        ctx.render_init(W, H, seed)
    fb = torch.full((nfb * len(rows) * W * 3,), float("nan"), dtype=torch.float32, device="cuda")
    cnt = ctx.render(args, fb.data_ptr())
    return fb.cpu().numpy().reshape(nfb, len(rows), W, 3), rows, cnt


def _check(got, rows, cnt, W, H, spp, nfb, cam, what=""):
    want = _want(W, H, spp, nfb, cam)
    for f in range(nfb):
        diff = (_bits(got[f]) != _bits(want[f][0][rows])).any(axis=2)
        assert not diff.any(), f"{what} fb {f}: {int(diff.sum())} pixels differ"
    assert cnt["segments"] == sum(int(want[f][1][rows].sum()) for f in range(nfb)), what
    assert cnt["samples"] == nfb * len(rows) * W * spp, what


# ---------------------------------------------------------------- 1. plain launches, spp 1, 2 and 3
W0, H0, NFB0 = 64, 36, 2  # 4608 items, 72 chunks
SPPS = pytest.mark.parametrize("spp", [1, 2, 3])


@SPPS
@CAMS
def test_natural_order(rtlib, gpu_ctx, oracle, cam, spp):
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    got, rows, cnt = _launch(rtlib, gpu_ctx, W0, H0, spp, NFB0, cam, schedule=False)
    assert gpu_ctx.last_render_kernel() == STEP
    assert gpu_ctx.last_render_schedule() == 0
    assert gpu_ctx.last_render_body() == PLAIN
    _check(got, rows, cnt, W0, H0, spp, NFB0, cam)


@SPPS
@CAMS
def test_probe_scheduled_one_shot(rtlib, gpu_ctx, oracle, cam, spp):
    """RT_FLAG_FRESH: with 4 or more samples per pixel over the frame buffers the probe kernel (<287874>, one
    sample per lane: table entry 0) runs first and its order is the launch's; below that the order is natural."""
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    got, rows, cnt = _launch(rtlib, gpu_ctx, W0, H0, spp, NFB0, cam, fresh=True)
    assert gpu_ctx.last_render_schedule() == (rtlib.RT_SCHED_PROBE if spp * NFB0 >= 4 else 0)
    assert gpu_ctx.last_render_body() == PLAIN
    _check(got, rows, cnt, W0, H0, spp, NFB0, cam)


@SPPS
@CAMS
def test_band_share(rtlib, gpu_ctx, oracle, cam, spp):
    """Every second row from the second: a row table that is not the identity."""
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    got, rows, cnt = _launch(rtlib, gpu_ctx, W0, H0, spp, NFB0, cam, band_rows=1, band_first=1, band_stride=2)
    assert len(rows) == H0 // 2 and rows[0] == 1
    assert gpu_ctx.last_render_body() == PLAIN
    _check(got, rows, cnt, W0, H0, spp, NFB0, cam)


# ---------------------------------------------------------------- 2. the table follows spp and seed
def test_stale_table(rtlib, gpu_ctx, oracle):
    """One context: REF at spp 2, 3, 2, then another seed, then seed 1984 again.  The table is keyed by
    (scene, seed, spp); a launch that read the one before it would differ from the oracle at every pixel."""
    W, H, nfb = W0, H0, NFB0
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    for k, spp in enumerate([2, 3, 2]):
        got, rows, cnt = _launch(rtlib, gpu_ctx, W, H, spp, nfb, REF, schedule=False)
        assert gpu_ctx.last_render_body() == PLAIN
        _check(got, rows, cnt, W, H, spp, nfb, REF, what=f"launch {k} (spp {spp})")
    got7, rows, cnt7 = _launch(rtlib, gpu_ctx, W, H, 2, nfb, REF, seed=7, schedule=False)
    assert gpu_ctx.last_render_kernel() == STEP and gpu_ctx.last_render_body() == PLAIN
    other = rtlib.Context(0)
    try:
        other.upload(rtlib.Scene.builtin("big1"))
        exp7, _, ecnt7 = _launch(rtlib, other, W, H, 2, nfb, REF, seed=7, schedule=False, step=False)
        assert other.last_render_kernel().startswith("render_kernel<")
    finally:
        other.close()
    assert np.array_equal(_bits(got7), _bits(exp7)), "seed 7 differs from render_kernel on a fresh context"
    assert cnt7["segments"] == ecnt7["segments"] and cnt7["samples"] == nfb * H * W * 2
    assert not np.array_equal(_bits(got7), _bits(got)), "seed 7 drew seed 1984's image"
    got, rows, cnt = _launch(rtlib, gpu_ctx, W, H, 2, nfb, REF, schedule=False)
    _check(got, rows, cnt, W, H, 2, nfb, REF, what="seed 1984 after seed 7")


# ---------------------------------------------------------------- 3. the general body
@CAMS
def test_warm_sequence_with_every_item_split(rtlib, gpu_ctx, ctx_opts, oracle, cam):
    """The measuring launch is plain; the recording launch (split_mode 1: sample-start states written at
    every camera setup with s > 0) and the replay (split_mode 2: every sample an item of its own, whose
    camera ray needs table entry s and nothing else) are general.  Every launch is the oracle's."""
    ctx_opts(split_min_segments=1.0)
    W, H, spp, nfb = 96, 54, 3, 2
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    sched, body = [], []
    for k in range(3):
        got, rows, cnt = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam)
        sched.append(gpu_ctx.last_render_schedule())
        body.append(gpu_ctx.last_render_body())
        _check(got, rows, cnt, W, H, spp, nfb, cam, what=f"launch {k}")
    assert sched[1] & rtlib.RT_SCHED_PREVIOUS and sched[2] & rtlib.RT_SCHED_PREVIOUS, sched
    assert sched[2] & rtlib.RT_SCHED_SPLIT_REPLAY and not sched[1] & rtlib.RT_SCHED_SPLIT_REPLAY, sched
    assert body == [PLAIN, GENERAL, GENERAL], body


# ---------------------------------------------------------------- 4. the twins
@pytest.mark.parametrize("kw, kernel", [(dict(stats=True), "render_step_kernel<25731>"),
                                        (dict(lds=False), "render_step_kernel<17538>")], ids=["stats", "no_lds"])
def test_twins(rtlib, gpu_ctx, oracle, kw, kernel):
    spp = 3
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    got, rows, cnt = _launch(rtlib, gpu_ctx, W0, H0, spp, NFB0, REF, **kw)
    assert gpu_ctx.last_render_kernel() == kernel
    assert gpu_ctx.last_render_body() == PLAIN
    if "stats" in kw:
        assert cnt["node_tests"] > 0 and cnt["prim_tests"] > 0
    _check(got, rows, cnt, W0, H0, spp, NFB0, REF)


# ---------------------------------------------------------------- 5. with and without camera tile lists
@pytest.mark.parametrize("bins", [False, True], ids=["no_bins", "bins"])
@CAMS
def test_camera_tile_lists_on_and_off(rtlib, gpu_ctx, oracle, cam, bins):
    """bins=False: camera rays traverse the tree, so a phase's second shading pass is rare and the tile
    pointers are null; bins=True: camera rays are answered from their tile's list and shaded in the second
    pass of the phase that set them up."""
    spp = 2
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    got, rows, cnt = _launch(rtlib, gpu_ctx, W0, H0, spp, NFB0, cam, bins=bins)
    assert gpu_ctx.camera_tiles_info()["last_used"] == (1 if bins else 0)
    assert gpu_ctx.last_render_kernel() == STEP
    assert gpu_ctx.last_render_body() == PLAIN
    _check(got, rows, cnt, W0, H0, spp, NFB0, cam)


# ---------------------------------------------------------------- 6. rt_render_tiles
@CAMS
def test_tile_launch(rtlib, gpu_ctx, oracle, cam):
    """rt_render_tiles for every other 16 x 16 tile (the last tile row is 4 rows high): the listed pixels
    are the oracle's, every other float stays as it was."""
    import torch

    W, H, spp, nfb = W0, H0, 3, NFB0
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    gpu_ctx.render_init(W, H, 1984)
    args = rtlib.make_args(W, H, spp, 0, nfb, 50, cam)
    ty, tx = ar.tile_grid(H, W)
    tiles = list(range(0, ty * tx, 2))
    m = np.isin(ar.pixel_tiles(H, W), tiles)
    fb = torch.full((nfb * H * W * 3,), float("nan"), dtype=torch.float32, device="cuda")
    cnt = gpu_ctx.render_tiles(args, tiles, fb.data_ptr())
    assert gpu_ctx.last_render_kernel() == STEP
    assert gpu_ctx.last_render_body() == PLAIN
    got = fb.cpu().numpy().reshape(nfb, H, W, 3)
    want = _want(W, H, spp, nfb, cam)
    for f in range(nfb):
        assert np.array_equal(_bits(got[f][m]), _bits(want[f][0][m])), f"fb {f}: listed pixels differ"
        assert np.isnan(got[f][~m]).all(), f"fb {f}: floats outside the listed tiles were written"
    assert cnt["segments"] == sum(int(want[f][1][m].sum()) for f in range(nfb))
    assert cnt["samples"] == nfb * int(m.sum()) * spp
