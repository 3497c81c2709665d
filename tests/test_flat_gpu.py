"""GPU parity on written scenes: whatever tests/flat_cases.py writes down as an rt_scene_soa goes to
rt_scene_upload and to the oracle's ref_scene_from_flat, and the kernels must give the oracle's float
bits and segment count -- on the data-dependent branches the built-in scenes never take (stored boxes
that do not nest, traversal stack overflow, shutters and sphere time ranges, medium / world-shape /
image-shape conditions, the LDS fit limits).  tests/test_flat_cpu.py checks the same cases as inputs
(finite, not sky, the branch reached) without a GPU.

Every case: 40x24, 4 spp (probe-eligible), 2 fbs, the launches of _run_case below.  A device error
ends the session (exit status 3): nothing more is started on a GPU that has faulted.
"""
import numpy as np
import pytest

import flat_cases
from flat_cases import NFB, PIX, REF, SPP, H, W

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _mask(kernel: str) -> int:
    return int(kernel[kernel.index("<") + 1:kernel.index(">")])


def _launch(rtlib, ctx, want, depth, cam, label, **kw):
    import torch

    args = rtlib.make_args(W, H, SPP, 0, NFB, depth, cam, **kw)
    ctx.render_init(W, H, 1984)
    fb = torch.full((NFB * H * W * 3,), float("nan"), dtype=torch.float32, device="cuda")
    try:
        cnt = ctx.render(args, fb.data_ptr())
    except rtlib.RtError as e:
        if e.status == rtlib.RT_ERR_HIP:  # a device error: nothing more starts on this GPU
            pytest.exit(f"{label}: {e}", returncode=3)
        raise
    if not kw.get("stats"):  # the stats twin is checked on segments only
        got = fb.cpu().numpy().reshape(NFB, H, W, 3)
        for f in range(NFB):
            diff = (_bits(got[f]) != _bits(want.fbs[f])).any(axis=2)
            assert not diff.any(), f"{label} fb {f}: {int(diff.sum())} px differ, first at {np.argwhere(diff)[0]}"
    assert cnt["segments"] == want.counters["segments"], label
    return cnt


def _run_case(rtlib, ctx, oracle, name, cam):
    """The launches of one scene (all bit-exact, all with the oracle's segment count): the default launch
    cold; three more with split_min_segments = 1 (scheduled, split-recording, split-replay); the exact
    visit set; the widest variant from global memory; the segment loop where the world is one BVH (or a
    BVH and primitives); the stats twin."""
    c = flat_cases.get(name)
    want = flat_cases.oracle_render(oracle, name, cam)
    before = ctx.options()
    try:
        if c.options:
            ctx.set_options(**c.options)
        ctx.set_options(split_min_segments=1.0)  # per launch: a cold launch is what it is without it
        ctx.upload(c.scene)
        _launch(rtlib, ctx, want, c.depth, cam, f"{name} cold")
        kernel = ctx.last_render_kernel()
        assert ctx.last_render_schedule() & rtlib.RT_SCHED_PREVIOUS == 0
        if c.family is not None:
            assert kernel.startswith(c.family), kernel
        assert _mask(kernel) & c.mask_has == c.mask_has and _mask(kernel) & c.mask_lacks == 0, kernel
        sched = []
        for k in ("scheduled", "split-recording", "split-replay"):
            _launch(rtlib, ctx, want, c.depth, cam, f"{name} {k}")
            sched.append(ctx.last_render_schedule())
        assert all(x & rtlib.RT_SCHED_PREVIOUS for x in sched), sched
        if kernel.startswith(flat_cases.STEP):  # the stepwise kernel splits samples: the third repeat replays them
            assert sched[2] & rtlib.RT_SCHED_SPLIT_REPLAY, sched
        ctx.set_options(split_min_segments=before["split_min_segments"])
        _launch(rtlib, ctx, want, c.depth, cam, f"{name} exact", exact=True)
        _launch(rtlib, ctx, want, c.depth, cam, f"{name} widest global", widest=True, lds=False)
        if c.family == flat_cases.STEP:
            _launch(rtlib, ctx, want, c.depth, cam, f"{name} no step", step=False)
            assert ctx.last_render_kernel().startswith(flat_cases.RENDER)
        cnt = _launch(rtlib, ctx, want, c.depth, cam, f"{name} stats", stats=True)
        if c.fallbacks:
            assert cnt["fallbacks"] > 0, "the traversal stack never overflowed"
        if c.family == flat_cases.RENDER:  # list worlds: the merged search where it applies, else the entry loop
            _launch(rtlib, ctx, want, c.depth, cam, f"{name} global", lds=False)
            assert bool(_mask(ctx.last_render_kernel()) & flat_cases.F_MERGE) == c.merged, ctx.last_render_kernel()
        if c.merged:  # ... and then the entry loop of hittable_list.h:23-39 too
            ctx.set_options(merged_search=rtlib.RT_MERGE_OFF)
            ctx.upload(c.scene)
            _launch(rtlib, ctx, want, c.depth, cam, f"{name} entry loop", lds=False)
            assert _mask(ctx.last_render_kernel()) & flat_cases.F_MERGE == 0
    finally:
        ctx.set_options(**before)
    return kernel


def _params(group):
    out = []
    for name in flat_cases.group(group):
        out.append(pytest.param(name, REF, id=f"{name.split(':')[1]}-ref"))
        if flat_cases.CASES[name].per_pixel:
            out.append(pytest.param(name, PIX, id=f"{name.split(':')[1]}-per_pixel"))
    assert any(p.values[1] == PIX for p in out), group
    return out


@pytest.mark.parametrize("name,cam", _params("bvh"))
def test_bvh_sizes(rtlib, gpu_ctx, oracle, name, cam):
    """Reference-layout BVHs of 3..33 primitives (rows 2..6, last rows with and without leaf_b) as the
    whole world (stepwise kernel) and as a list entry (merged search and entry loop)."""
    _run_case(rtlib, gpu_ctx, oracle, name, cam)


@pytest.mark.parametrize("name,cam", _params("boxes"))
def test_stored_boxes(rtlib, gpu_ctx, oracle, name, cam):
    """Stored boxes that are not the union of their children: loosened, a mid-level box its children
    poke out of (build_traversal_tree's non-nesting guard), a last-row box that cuts its primitive, a
    root box that hides part of the scene.  The oracle honours what is stored; so must the culled search."""
    _run_case(rtlib, gpu_ctx, oracle, name, cam)


@pytest.mark.parametrize("name,cam", _params("deep"))
def test_deep_traversal_tree(rtlib, gpu_ctx, oracle, name, cam):
    """A chain of spheres that piles more than 16 far children on the traversal stack; the ones that no
    longer fit hold the first hits of the rays between two of the spheres' cones, so the overflow must
    fall back to the exact visit set.  The stats twin's `fallbacks > 0` is asserted; the proof that the
    overflow path ran is the pixels: a build with `overflow = true` removed differs from the oracle in
    about 500 of the 960 pixels of this case (MI355X)."""
    _run_case(rtlib, gpu_ctx, oracle, name, cam)


@pytest.mark.parametrize("name,cam", _params("time"))
def test_time_ranges(rtlib, gpu_ctx, oracle, name, cam):
    """Camera shutters other than [0, 1], moving spheres with (t0, dt) = (2, 0.5) beside (0, 1) ones, and
    sphere-bounded media beyond each of medium_inert's limits."""
    _run_case(rtlib, gpu_ctx, oracle, name, cam)


@pytest.mark.parametrize("name,cam", _params("world"))
def test_world_shapes(rtlib, gpu_ctx, oracle, name, cam):
    """Each side of the kernel selection rules, with the family and variant bits asserted."""
    _run_case(rtlib, gpu_ctx, oracle, name, cam)


@pytest.mark.parametrize("name,cam", _params("lds"))
def test_lds_fit(rtlib, gpu_ctx, oracle, name, cam):
    """Scenes just under and just over the LDS fit tests (sizes from kLdsBudget in the source)."""
    _run_case(rtlib, gpu_ctx, oracle, name, cam)


def test_lds_fit_pairs_differ(rtlib, gpu_ctx, oracle):
    for kind, bit in (("spheres", flat_cases.F_LDS), ("triangles", flat_cases.F_QLDS)):
        masks = []
        for side in ("under", "over"):
            c = flat_cases.get(f"lds:{kind}_{side}")
            gpu_ctx.upload(c.scene)
            _launch(rtlib, gpu_ctx, flat_cases.oracle_render(oracle, f"lds:{kind}_{side}", REF), c.depth, REF, f"{kind} {side}")
            masks.append(_mask(gpu_ctx.last_render_kernel()))
        assert masks[0] & bit and not masks[1] & bit, (kind, masks)


@pytest.mark.parametrize("name,cam", _params("camera"))
def test_cameras(rtlib, gpu_ctx, oracle, name, cam):
    """Cameras inside a dielectric and inside a medium, a lens wider than the focus distance, fields of
    view of 1 and 170 degrees, a camera 1e4 from a unit scene, the scene scaled by 1e-3 and 1e3.

    The camera 1e4 away sees the spheres from 22 000 radii, where sphere.h's float test no longer resolves
    them: rt_scene_validate refuses it (tests/test_flat_cpu.py; 1 216 of 1 920 pixels differed where camera
    rays took the culled search).  far_400r is the same scene from 400 radii, below the limit of 512, as a
    world BVH and under an instance."""
    _run_case(rtlib, gpu_ctx, oracle, name, cam)


@pytest.mark.parametrize("name,cam", _params("shade"))
def test_shading_matrix(rtlib, gpu_ctx, oracle, name, cam):
    """Every primitive type under one material over one texture, including images whose sizes are no
    multiple of the 8x8 texel tile, at 1 and 3 bytes per pixel, and the no-data image."""
    _run_case(rtlib, gpu_ctx, oracle, name, cam)


@pytest.mark.parametrize("name,cam", _params("ties"))
def test_ties(rtlib, gpu_ctx, oracle, name, cam):
    _run_case(rtlib, gpu_ctx, oracle, name, cam)


@pytest.mark.parametrize("name,cam", _params("random"))
def test_random_scenes(rtlib, gpu_ctx, oracle, name, cam):
    _run_case(rtlib, gpu_ctx, oracle, name, cam)
