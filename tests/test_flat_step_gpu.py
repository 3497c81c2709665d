"""GPU parity of the straight-line traversal step of the deferring variants (rt_kernels.hip: trav_node):
the sphere variants and, since their deferred leaf pass is on, the triangle-mesh variants.

The step's decision (descend / push / pop / end) is a chain of selects: the stack top is read in every
step, at entry 0 when the stack is empty, and the far child is written by a store that is masked off
when the stack is full (the stacks fill their LDS exactly: there is no entry 16).  tests/test_flat_gpu.py
and tests/test_leaf_defer_gpu.py pin the step's ordinary paths; here are the shapes at which exactly
those two accesses sit on either side of their limits.  Every launch equals the oracle bit for bit,
segment count included.
"""
import pytest

import flat_cases
import test_flat_gpu
from test_leaf_defer_gpu import CAMS, REF, _flat, _launch, _same

pytestmark = pytest.mark.gpu

F_TRI, F_STEP, F_WORLD, F_QLDS = 1 << 3, 1 << 14, 1 << 15, 1 << 16


def _defers(kernel: str) -> bool:
    """A sphere variant of the stepwise kernel (the deferring family of C2: no mesh, no world tree)."""
    m = test_flat_gpu._mask(kernel)
    return kernel.startswith("render_step_kernel<") and m & F_STEP != 0 and m & (F_TRI | F_WORLD | F_QLDS) == 0


@CAMS
@pytest.mark.parametrize("n", [8, 16, 24, 40, 72])
def test_stack_boundary(rtlib, gpu_ctx, oracle, n, cam):
    """flat_cases.chain(n): a ray along the axis enters both children of every level, so the far ones pile
    up on the 16-entry stack.  With 8 and 16 spheres the tree is too shallow to fill it; 24 and 40 reach
    sp == 16 (the masked store) and unwind to sp == 0 (the read of entry 0) from both sides of the limit;
    72 overflows, and the stats twin reports the fallbacks to the exact visit set."""
    W, H, spp, nfb = 48, 27, 4, 2
    scene = flat_cases.chain(n)
    want, segs, _ = _flat(oracle, scene, W, H, spp, nfb, cam)
    gpu_ctx.upload(scene)
    for kw in ({}, dict(lds=False), dict(bins=False), dict(stats=True)):
        got, cnt = _launch(rtlib, gpu_ctx, W, H, spp, nfb, cam, **kw)
        assert _defers(gpu_ctx.last_render_kernel()), gpu_ctx.last_render_kernel()
        _same(got, want, f"chain({n}) {kw}")
        assert cnt["segments"] == segs, kw
        if n == 72 and kw.get("stats"):
            assert cnt["fallbacks"] > 0, "the traversal stack never overflowed"


@CAMS
@pytest.mark.parametrize("shape", [(1, 1, 64), (8, 1, 8)], ids=["1x1x64", "8x1x8"])
@pytest.mark.parametrize("n", [3, 4, 5])
def test_pop_into_the_end(rtlib, gpu_ctx, oracle, n, shape, cam):
    """flat_cases.garden(n) with one and eight busy lanes: the trees are one to three levels deep, so a
    search ends (no hit inner child at sp == 0) within a step or two of its start, and the idle lanes of
    the wave sit at sp == 0 through all of them."""
    W, H, spp = shape
    scene = flat_cases.garden(n, n)
    want, segs, _ = _flat(oracle, scene, W, H, spp, 1, cam)
    gpu_ctx.upload(scene)
    for kw in ({}, dict(bins=False)):
        got, cnt = _launch(rtlib, gpu_ctx, W, H, spp, 1, cam, **kw)
        assert _defers(gpu_ctx.last_render_kernel()), gpu_ctx.last_render_kernel()
        _same(got, want, f"garden({n}) {shape} {kw}")
        assert cnt["segments"] == segs, kw


def test_quantized_mesh_variant(rtlib, gpu_ctx, oracle):
    """The quantized-tree mesh variant (16-bit stack entries after the quantized pairs; it defers its
    leaves and takes the straight-line step too): tests/test_flat_gpu.py's launches of lds:triangles_under."""
    kernel = test_flat_gpu._run_case(rtlib, gpu_ctx, oracle, "lds:triangles_under", REF)
    assert test_flat_gpu._mask(kernel) & (F_STEP | F_QLDS) == F_STEP | F_QLDS, kernel


def test_world_tree_variant_untouched(rtlib, gpu_ctx, ctx_opts, oracle):
    """The world-tree variants keep trav_step: one launch of world:two_bvhs with options.world_tree = 1.
    (test_flat_gpu._run_case expects that case's default kernel family, so the launch goes through its
    _launch directly, against the same cached oracle result.)"""
    name = "world:two_bvhs"
    c = flat_cases.get(name)
    want = flat_cases.oracle_render(oracle, name, REF)
    ctx_opts(world_tree=1)
    gpu_ctx.upload(c.scene)
    test_flat_gpu._launch(rtlib, gpu_ctx, want, c.depth, REF, f"{name} world tree")
    kernel = gpu_ctx.last_render_kernel()
    assert kernel.startswith("render_step_kernel<") and test_flat_gpu._mask(kernel) & F_WORLD, kernel
