"""GPU parity of render_step_kernel's refill: items handed to idle lanes from the wave's decoded chunk.

The sphere variants decode a claimed chunk of 64 positions at once (perm, row_q, the RNG slot and its
state, one position per lane) and hand the entries to the lanes without an item; split launches decode
per lane as before.  Which lane runs an item must not show: every frame buffer is compared with the
oracle bit for bit, with the oracle's segment count over the owned rows and the sample count.  All cases
are big1 at depth 50, seed 1984.  The shapes are the borders of the hand-out: fewer items than a chunk,
exactly one, one more; spp 1, where every sample end ends an item and refills of many lanes straddle
chunk borders, with and without a schedule (perm); a band share's row table; a warm sequence through
both split modes; the global-memory, counting and natural-order launches.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REF, PIX = 0, 1
CAMS = pytest.mark.parametrize("cam", [REF, PIX], ids=["ref", "per_pixel"])


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


def _launch(rtlib, ctx, W, H, spp, nfb, cam, **kw):
    import torch

    args = rtlib.make_args(W, H, spp, 0, nfb, 50, cam, **kw)
    rows = rtlib.owned_rows(args)
    ctx.render_init(W, H, 1984)
    fb = torch.full((nfb * len(rows) * W * 3,), float("nan"), dtype=torch.float32, device="cuda")
    cnt = ctx.render(args, fb.data_ptr())
    return fb.cpu().numpy().reshape(nfb, len(rows), W, 3), rows, cnt, ctx.last_render_schedule()


def _check(got, rows, cnt, W, H, spp, nfb, cam, what=""):
    want = _want(W, H, spp, nfb, cam)
    for f in range(nfb):
        diff = (_bits(got[f]) != _bits(want[f][0][rows])).any(axis=2)
        assert not diff.any(), f"{what} fb {f}: {int(diff.sum())} pixels differ"
    assert cnt["segments"] == sum(int(want[f][1][rows].sum()) for f in range(nfb)), what
    assert cnt["samples"] == nfb * len(rows) * W * spp, what


@CAMS
@pytest.mark.parametrize("shape", [(7, 5), (16, 4), (13, 5)], ids=["35_items", "64_items", "65_items"])
def test_items_around_one_chunk(rtlib, gpu_ctx, oracle, shape, cam):
    """Fewer items than one chunk, exactly one chunk, one item over: every other wave's whole claim lies
    past the end, and so does the rest of the last chunk."""
    W, H = shape
    spp, nfb = 2, 1
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    got, rows, cnt, _ = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam)
    assert gpu_ctx.last_render_kernel() == "render_step_kernel<25730>"
    _check(got, rows, cnt, W, H, spp, nfb, cam)


@CAMS
@pytest.mark.parametrize("nfb", [2, 4], ids=["2fb_no_perm", "4fb_probe_perm"])
def test_one_sample_items(rtlib, gpu_ctx, oracle, nfb, cam):
    """spp 1: every sample end ends an item, so a refill serves many lanes and straddles chunk borders.
    2 fb is not probe-eligible (spp * fb_count < 4): positions are items; 4 fb is: claimed through perm."""
    W, H, spp = 96, 54, 1
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    got, rows, cnt, sched = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam)
    if nfb == 4:
        assert sched == rtlib.RT_SCHED_PROBE, sched
    else:
        assert sched == 0, sched
    _check(got, rows, cnt, W, H, spp, nfb, cam)


@CAMS
def test_band_share(rtlib, gpu_ctx, oracle, cam):
    """Bands of 4 rows, every third from the second: a row table that is not the identity, and an image
    height that is no multiple of the band."""
    W, H, spp, nfb = 96, 54, 2, 2
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    got, rows, cnt, _ = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam, band_rows=4, band_first=1, band_stride=3)
    assert 0 < len(rows) < H and rows[0] == 4
    _check(got, rows, cnt, W, H, spp, nfb, cam)


@CAMS
def test_warm_sequence_through_the_split_modes(rtlib, gpu_ctx, ctx_opts, oracle, cam):
    """The same configuration three times with every item split: a probe-scheduled launch, the recording
    launch (split_mode 1), the replay of the split samples (split_mode 2)."""
    ctx_opts(split_min_segments=1.0)
    W, H, spp, nfb = 96, 54, 2, 2
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    seen = []
    for k in range(3):
        got, rows, cnt, sched = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam)
        seen.append(sched)
        _check(got, rows, cnt, W, H, spp, nfb, cam, what=f"launch {k}")
    assert seen[0] == rtlib.RT_SCHED_PROBE and seen[1] & rtlib.RT_SCHED_PREVIOUS, seen
    assert seen[2] == rtlib.RT_SCHED_PREVIOUS | rtlib.RT_SCHED_SPLIT_REPLAY, seen


@pytest.mark.parametrize("kw, kernel", [
    (dict(bins=False), "render_step_kernel<25730>"),      # camera rays traverse the tree
    (dict(lds=False), "render_step_kernel<17538>"),       # the global-memory twin
    (dict(stats=True), "render_step_kernel<25731>"),      # the counting twin
    (dict(schedule=False), "render_step_kernel<25730>"),  # natural order: no probe, no perm
], ids=["no_bins", "no_lds", "stats", "no_schedule"])
def test_twins_and_natural_order(rtlib, gpu_ctx, oracle, kw, kernel):
    W, H, spp, nfb = 64, 36, 2, 2
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    got, rows, cnt, sched = _launch(rtlib, gpu_ctx, W, H, spp, nfb, REF, **kw)
    assert gpu_ctx.last_render_kernel() == kernel
    if "schedule" in kw:
        assert sched == 0, sched
    _check(got, rows, cnt, W, H, spp, nfb, REF)
