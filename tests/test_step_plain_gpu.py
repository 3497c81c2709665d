"""GPU parity of render_step_kernel's two bodies (the sphere variants: <25730>, <25731>, <17538>).

A launch that splits no samples and fits the item pool's packed words (at most 2^32 items; width, height
and fb_count at most 65536) runs the plain body, every other launch the general one;
Context.last_render_body() says which (1 plain, 0 general).  Which body runs must not show: every case is
big1 at depth 50, seed 1984, and compares every float of every frame buffer with the CPU oracle bit for
bit, with the oracle's segment count over the rendered pixels and the sample count.

Not tested: more than 2^32 items.  Such a launch is hours long.
"""
import functools

import numpy as np
import pytest

import adapt_ref as ar

pytestmark = pytest.mark.gpu

REF, PIX = 0, 1
CAMS = pytest.mark.parametrize("cam", [REF, PIX], ids=["ref", "per_pixel"])
PLAIN, GENERAL = 1, 0


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


def _launch(rtlib, ctx, W, H, spp, nfb, cam, init=True, **kw):
    import torch

    args = rtlib.make_args(W, H, spp, 0, nfb, 50, cam, **kw)
    rows = rtlib.owned_rows(args)
    if init:
        ctx.render_init(W, H, 1984)
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


# ---------------------------------------------------------------- 1. plain launches of every kind
SMALL = (64, 36, 2, 2)  # W, H, spp, nfb: 4608 items, 72 chunks


@CAMS
def test_natural_order_is_plain(rtlib, gpu_ctx, oracle, cam):
    W, H, spp, nfb = SMALL
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    got, rows, cnt = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam, schedule=False)
    assert gpu_ctx.last_render_kernel() == "render_step_kernel<25730>"
    assert gpu_ctx.last_render_schedule() == 0
    assert gpu_ctx.last_render_body() == PLAIN
    _check(got, rows, cnt, W, H, spp, nfb, cam)


@CAMS
def test_measuring_launch_and_the_unsplit_launch_after_it_are_plain(rtlib, gpu_ctx, ctx_opts, oracle, cam):
    """The first scheduled launch of a configuration records its items' costs; the launch after it, with
    RT_FLAG_NO_SPLIT, claims its items through the order built from them (perm) and splits nothing, though
    the threshold would split every item."""
    ctx_opts(split_min_segments=1.0)
    W, H, spp, nfb = SMALL
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    got, rows, cnt = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam)
    assert gpu_ctx.last_render_schedule() & rtlib.RT_SCHED_PREVIOUS == 0
    assert gpu_ctx.last_render_body() == PLAIN
    _check(got, rows, cnt, W, H, spp, nfb, cam, "measuring launch")
    got, rows, cnt = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam, split=False)
    assert gpu_ctx.last_render_schedule() == rtlib.RT_SCHED_PREVIOUS
    assert gpu_ctx.last_render_body() == PLAIN
    _check(got, rows, cnt, W, H, spp, nfb, cam, "launch in measured order")


@CAMS
def test_probe_scheduled_one_shot_is_plain(rtlib, gpu_ctx, oracle, cam):
    W, H, spp, nfb = SMALL
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    got, rows, cnt = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam, fresh=True)
    assert gpu_ctx.last_render_schedule() == rtlib.RT_SCHED_PROBE
    assert gpu_ctx.last_render_body() == PLAIN
    _check(got, rows, cnt, W, H, spp, nfb, cam)


@CAMS
def test_band_share_is_plain(rtlib, gpu_ctx, oracle, cam):
    """Every second row from the second: a row table that is not the identity."""
    W, H, spp, nfb = SMALL
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    got, rows, cnt = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam, band_rows=1, band_first=1, band_stride=2)
    assert len(rows) == H // 2 and rows[0] == 1
    assert gpu_ctx.last_render_body() == PLAIN
    _check(got, rows, cnt, W, H, spp, nfb, cam)


@CAMS
def test_tile_launch_is_plain(rtlib, gpu_ctx, oracle, cam):
    """rt_render_tiles for every other 16 x 16 tile (the last tile row is 4 rows high): the listed pixels
    are the oracle's, every other float stays as it was."""
    import torch

    W, H, spp, nfb = SMALL
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    gpu_ctx.render_init(W, H, 1984)
    args = rtlib.make_args(W, H, spp, 0, nfb, 50, cam)
    ty, tx = ar.tile_grid(H, W)
    tiles = list(range(0, ty * tx, 2))
    m = np.isin(ar.pixel_tiles(H, W), tiles)
    fb = torch.full((nfb * H * W * 3,), float("nan"), dtype=torch.float32, device="cuda")
    cnt = gpu_ctx.render_tiles(args, tiles, fb.data_ptr())
    assert gpu_ctx.last_render_kernel() == "render_step_kernel<25730>"
    assert gpu_ctx.last_render_body() == PLAIN
    got = fb.cpu().numpy().reshape(nfb, H, W, 3)
    want = _want(W, H, spp, nfb, cam)
    for f in range(nfb):
        assert np.array_equal(_bits(got[f][m]), _bits(want[f][0][m])), f"fb {f}: listed pixels differ"
        assert np.isnan(got[f][~m]).all(), f"fb {f}: floats outside the listed tiles were written"
    assert cnt["segments"] == sum(int(want[f][1][m].sum()) for f in range(nfb))
    assert cnt["samples"] == nfb * int(m.sum()) * spp


# ---------------------------------------------------------------- 2. the boundary of the packed words
@pytest.mark.parametrize("shape, body", [((65536, 1), PLAIN), ((1, 65536), PLAIN), ((65537, 1), GENERAL),
                                         ((1, 65537), GENERAL)], ids=["65536x1", "1x65536", "65537x1", "1x65537"])
def test_the_pool_words_hold_16_bits(rtlib, gpu_ctx, oracle, shape, body):
    """A column or a row index of 65535 is the last one a half of a packed word holds: width and height
    65536 are plain, 65537 general.  spp 1, 1 fb (not probe-eligible: natural order).  rt_render and the
    oracle accept all four shapes."""
    W, H = shape
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    got, rows, cnt = _launch(rtlib, gpu_ctx, W, H, 1, 1, REF)
    assert gpu_ctx.last_render_kernel() == "render_step_kernel<25730>"
    assert gpu_ctx.last_render_body() == body
    _check(got, rows, cnt, W, H, 1, 1, REF)


@functools.lru_cache(maxsize=None)
def _want_2x1(nfb):
    """The oracle's 2 x 1 frame buffers 0 .. nfb - 1 at spp 1 ([nfb][1][2][3]) and their segments ([nfb])."""
    from oracle import ref_cpu

    ref = ref_cpu.RefScene("big1")
    fbs, segs = np.empty((nfb, 1, 2, 3), np.float32), np.empty(nfb, np.int64)
    for f in range(nfb):
        fb, c, _ = ref.render(2, 1, 1, f, 50, REF)
        fbs[f], segs[f] = fb.reshape(1, 2, 3), c["segments"]
    return fbs, segs


def test_the_pool_words_hold_16_bits_of_the_frame_buffer(rtlib, gpu_ctx, oracle):
    """The other half of the word that holds the column: a frame-buffer index of 65535 is the last one it
    holds, so fb_count 65536 is plain and 65537 general.  A 2 x 1 image at spp 1 in natural order keeps such a
    launch at 131 074 items.  The launches agree bit for bit on the 65536 buffers they share; buffers 0, 1,
    4099 k, 65534, 65535 and 65536 (and, the oracle being quick at this size, every other one) are the
    oracle's, with its segment count."""
    W, H, N = 2, 1, 65536
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    plain, rows, cnt_p = _launch(rtlib, gpu_ctx, W, H, 1, N, REF, schedule=False)
    assert gpu_ctx.last_render_kernel() == "render_step_kernel<25730>"
    assert gpu_ctx.last_render_body() == PLAIN
    general, rows_g, cnt_g = _launch(rtlib, gpu_ctx, W, H, 1, N + 1, REF, schedule=False)
    assert gpu_ctx.last_render_kernel() == "render_step_kernel<25730>"
    assert gpu_ctx.last_render_body() == GENERAL
    assert list(rows) == [0] and list(rows_g) == [0]
    assert np.array_equal(_bits(plain), _bits(general[:N])), "the bodies differ on the buffers they share"
    want, segs = _want_2x1(N + 1)
    listed = [0, 1] + list(range(4099, N, 4099)) + [N - 2, N - 1, N]
    for f in listed:
        assert np.array_equal(_bits(general[f]), _bits(want[f])), f"fb {f} differs from the oracle"
    assert np.array_equal(_bits(general), _bits(want))
    assert cnt_p["segments"] == int(segs[:N].sum()) and cnt_g["segments"] == int(segs.sum())
    assert cnt_p["samples"] == N * W * H and cnt_g["samples"] == (N + 1) * W * H


# ---------------------------------------------------------------- 3. general launches stay general
@CAMS
def test_split_launches_take_the_general_body(rtlib, gpu_ctx, ctx_opts, oracle, cam):
    """The warm sequence of tests/test_refill_gpu.py with every item split: the measuring launch is plain,
    the recording launch (split_mode 1) and the replay (split_mode 2) are general."""
    ctx_opts(split_min_segments=1.0)
    W, H, spp, nfb = 96, 54, 2, 2
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
def test_twins_are_plain(rtlib, gpu_ctx, oracle, kw, kernel):
    W, H, spp, nfb = SMALL
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    got, rows, cnt = _launch(rtlib, gpu_ctx, W, H, spp, nfb, REF, **kw)
    assert gpu_ctx.last_render_kernel() == kernel
    assert gpu_ctx.last_render_body() == PLAIN
    if "stats" in kw:
        assert cnt["node_tests"] > 0 and cnt["prim_tests"] > 0
    _check(got, rows, cnt, W, H, spp, nfb, REF)
