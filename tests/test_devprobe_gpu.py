"""GPU checks of the arithmetic that host and device code share, one value at a time (oracle/devprobe.py):
hipcc's device pass == hipcc's host pass as uint32, on the input sets of tests/devprobe_cases.py and on every
1021st bit pattern of both signs, one test per family.  tests/test_devprobe_cpu.py ties the host pass to g++
and to exact references, so what is equal here is right.  Two NaNs count as equal; how many differ in payload
or sign is printed.  A HIP error from a probe entry ends the session: nothing more starts on that GPU.

Also here: rt_render_init with seeds whose high half is not zero, against the oracle.
"""
import numpy as np
import pytest

import devprobe_cases as dc
from test_devprobe_cpu import CASES, DET_FNS, SEEDS_INIT, assert_same, init_slots

from oracle import devprobe as dp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_ctx):
    """The probe opens the device itself; gpu_ctx only says that there is one."""


def both(entry, *args, **kw):
    """(device, host pass) results of one probe entry."""
    try:
        dev = entry("dev", *args, **kw)
    except dp.ProbeError as e:  # a device error: nothing more starts on this GPU
        pytest.exit(str(e), returncode=3)
    return dev, entry("host", *args, **kw)


@pytest.mark.parametrize("fn", DET_FNS + ["quant"])
def test_device_equals_host_pass_unary(fn):
    cases = dc.quant() if fn == "quant" else CASES[fn]()
    for name, xs in (("cases", cases), ("every 1021st", dc.strided(1021))):
        d, h = both(dp.unary, fn, xs)
        assert_same(d, h, (xs,), f"{fn} device / host pass, {name}")


def test_device_equals_host_pass_atan2():
    y, x = dc.atan2()
    d, h = both(dp.atan2, y, x)
    assert_same(d, h, (y, x), "det_atan2f device / host pass")


def test_device_equals_host_pass_checker():
    a, b, c = dc.checker()
    d, h = both(dp.checker, a, b, c)
    assert_same(d, h, (a, b, c), "checker_odd device / host pass")
    x = dc.checker_args()
    (dn, dk), (hn, hk) = both(dp.sin_neg, x)
    assert np.array_equal(dn, hn) and np.array_equal(dk, hk)


def test_device_equals_host_pass_xorwow():
    st, _ = dc.xorwow_states()
    d, h = both(dp.xorwow, st)
    for got, want, what in zip(d, h, ("word", "uniform", "state after")):
        assert np.array_equal(got, want), what
    d, h = both(dp.seed_state, dc.seeds())
    assert np.array_equal(d, h)


def test_device_equals_host_pass_denoise_math():
    s1, s2, n = dc.dn_moments()
    (dM, dV), (hM, hV) = both(dp.dn_prepare, s1, s2, n)
    assert np.array_equal(dM, hM) and np.array_equal(dV, hV)
    d, h = both(dp.dn_q_of, hM)
    assert np.array_equal(d, h)
    d, h = both(dp.dn_term, dc.dn_term_ops())
    assert np.array_equal(d, h)
    P, cnt, xf = dc.dn_weight_ops()
    d, h = both(dp.dn_weight, P, cnt)
    assert np.array_equal(d, h)
    d, h = both(dp.dn_weight, P, cnt, xf)
    assert np.array_equal(d, h)
    d, h = both(dp.dn_feature_x, *dc.dn_features())
    assert_same(d, h, dc.dn_features()[:1], "feature_x device / host pass")
    d, h = both(dp.dn_patch_span, dc.dn_spans())
    assert np.array_equal(d, h)
    (dl, dg), (hl, hg) = both(dp.dn_linear_gain, *dc.dn_linear_ops())
    assert np.array_equal(dl, hl) and np.array_equal(dg, hg)


@pytest.mark.parametrize("seed", SEEDS_INIT, ids=[hex(s) for s in SEEDS_INIT])
def test_render_init_with_64_bit_seeds(rtlib, gpu_ctx, oracle, seed):
    """rt_render_init == curand_init(seed, slot, 0) where the seed's high half counts (every other test seeds
    with 1984 or 7); tests/test_devprobe_cpu.py ties oracle.xorwow_init to the pure-Python generator there."""
    W, H = 64, 36
    gpu_ctx.render_init(W, H, seed)
    got = gpu_ctx.read_states(0, W * H)
    for s in init_slots(W, H):
        assert np.array_equal(got[s], oracle.xorwow_init(seed, s, 0)), s
