"""The kernels against what the reference's own class headers wrote down, with no oracle in between.

tests/golden/refhdr_renders.npz holds the frame buffers and segment counts that the reference's headers,
compiled for the host (oracle/refhdr/), gave for one written scene of every group of flat_cases.py and for
big1 and cornell_smoke (tests/golden/make_refhdr_golden.py).  Every other GPU test compares with the
oracle, a restatement by reading; here a misreading that the oracle and the kernels share would show.
Each scene: the default launch and the exact visit set, 40x24, 4 spp, 2 fbs, REF camera mode.  A device
error ends the session (exit status 3): nothing more is started on a GPU that has faulted.
"""
import numpy as np
import pytest

import refhdr_cases
from flat_cases import NFB, REF, SPP, H, W
from refhdr_cases import first_difference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def record():
    return np.load(refhdr_cases.GOLDEN)


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("key", refhdr_cases.RECORDED)
def test_kernel_matches_the_record(rtlib, gpu_ctx, record, key, exact):
    import torch

    e = refhdr_cases.recorded_entry(key)
    gpu_ctx.upload(e.scene)
    gpu_ctx.render_init(W, H, 1984)
    fb = torch.full((NFB * H * W * 3,), float("nan"), dtype=torch.float32, device="cuda")
    try:
        cnt = gpu_ctx.render(rtlib.make_args(W, H, SPP, 0, NFB, e.depth, REF, exact=exact), fb.data_ptr())
    except rtlib.RtError as err:
        if err.status == rtlib.RT_ERR_HIP:  # a device error: nothing more starts on this GPU
            pytest.exit(f"{key}: {err}", returncode=3)
        raise
    got = fb.cpu().numpy().reshape(NFB, H, W, 3)
    name = refhdr_cases.key_name(key)
    for f in range(NFB):
        d = first_difference(got[f], record[f"{name}_fb{f}"].view(np.float32))
        assert d is None, f"{key} fb {f}: {d[0]} px differ, first at {d[1]}"
    assert cnt["segments"] == int(record[f"{name}_segments"].sum()), key
