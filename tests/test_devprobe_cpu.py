"""CPU checks of the arithmetic that host and device code share, one value at a time (oracle/devprobe.py).

1. hipcc's host pass == g++ as uint32, for every function of csrc/rt_detmath.h, on the input sets of
   tests/devprobe_cases.py and on every 1021st bit pattern of both signs.  Two NaNs count as equal; how many
   differ in payload or sign is printed (DESIGN.md section 4 records where).
2. Accuracy against mpmath at 120 bits on the input sets and on every 65 521st bit pattern.  Wherever the
   header's reduction is exact (everything but sin / cos / tan above 2^20) the error is at most 0.5 ulp + MARGIN.
   MARGIN[fn] is four times the worst relative error of the double that det_*f casts to float, in float ulps
   (times 2^24), measured over the same inputs by `python tests/test_devprobe_cpu.py`:

       fn     inputs    worst float error (ulp)   at x           double before the cast   4 * that * 2^24   MARGIN
       sin     40 874   0.4999052                 0x39e89b2c     2^-51.74                 2^-25.74 ulp      2^-25
       cos     40 874   0.4999549                 0x44c90fc5     2^-51.84                 2^-25.84 ulp      2^-25
       tan     40 874   0.4999738                 0x3f9645fa     2^-51.05                 2^-25.05 ulp      2^-25
       log     33 209   0.5 - 2^-26 (a)           0x3f7ffffe     2^-51.56                 2^-25.56 ulp      2^-25
       pow5   198 052   0.5 exactly (b)           0x30800000     2^-52.02                 2^-26.02 ulp      2^-26
       acos    32 660   0.4999791                 0xbab08f74     2^-48.40 (c)             2^-22.40 ulp      2^-22
       atan2   69 314   0.4999999                 y 0xaef38bdb   2^-51.24                 2^-25.24 ulp      2^-25
                                                  x 0x58088ba5

   (a) log(1 - 2^-23) = -2^-23 (1 + 2^-24 + ...) lies just past the midpoint of two floats.  (b) (2^-30)^5 = 2^-150
   is the midpoint of 0 and the least denormal: a tie, rounded to even.  (c) the root of 1 - x^2 is one Newton
   step from a float seed, good to 2^-49, not to 2^-53.
   (each MARGIN is the measured figure rounded up to a power of two; all are far below the 2^-10 ulp at which
   the double evaluation itself would be the finding).  Every sampled result is in fact the correctly rounded
   float.  For 2^20 < |x| <= 1e9 the products of the three-part reduction are no longer exact: sin and cos are
   held to an absolute error of 2^-22 (one rounding of fn * 1.5707963267341256 at magnitude 2^30 gives 2^-23,
   the float rounding 2^-25; measured 2^-23.56), tan to the bit-identity tests only.
   The linear sweep of the test that this file replaces (|x| <= 74, sin, cos and log) is held to the same 0.5 ulp.
3. rtx::next / uniform / seed_state, quant and the scalar functions of rt_denoise_math.h in hipcc's host pass
   against references that are none of the code under test.
"""
import functools
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

import devprobe_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import devprobe as dp  # noqa: E402

U32 = np.uint32
DET_FNS = ["sin", "cos", "tan", "log", "pow5", "acos"]
CASES = {"sin": dc.trig, "cos": dc.trig, "tan": dc.trig, "log": dc.log, "pow5": dc.pow5, "acos": dc.acos}
QNAN = 0x7FC00000
MARGIN = {"sin": 2.0 ** -25, "cos": 2.0 ** -25, "tan": 2.0 ** -25, "log": 2.0 ** -25, "pow5": 2.0 ** -26,
          "acos": 2.0 ** -22, "atan2": 2.0 ** -25}
ONE_E9 = dc.bits(1e9)
TWO20 = dc.bits(2.0 ** 20)


def isnan(b):
    return (np.asarray(b, U32) & U32(0x7FFFFFFF)) > U32(0x7F800000)


def same(a, b):
    """Equal as uint32, or both NaN."""
    return (a == b) | (isnan(a) & isnan(b))


def assert_same(a, b, inputs, what):
    bad = np.nonzero(~same(a, b))[0]
    payload = int((isnan(a) & isnan(b) & (a != b)).sum())
    print(f"{what}: {a.size} values, {bad.size} differ, {payload} NaN pairs with another payload or sign")
    assert bad.size == 0, f"{what}: {bad.size} differ, first " + ", ".join(
        f"{[hex(int(np.atleast_1d(x)[i])) for x in inputs]} -> {int(a[i]):#x} / {int(b[i]):#x}" for i in bad[:5])


# ------------------------------------------------------------------ 1. hipcc's host pass == g++
@pytest.mark.parametrize("fn", DET_FNS)
def test_host_pass_equals_gxx_unary(fn):
    for name, xs in (("cases", CASES[fn]()), ("every 1021st", dc.strided(1021))):
        assert_same(dp.unary("host", fn, xs), dp.unary("gxx", fn, xs), (xs,), f"det_{fn}f host pass / g++, {name}")


def test_host_pass_equals_gxx_atan2():
    y, x = dc.atan2()
    assert_same(dp.atan2("host", y, x), dp.atan2("gxx", y, x), (y, x), "det_atan2f host pass / g++")


def test_host_pass_equals_gxx_checker():
    a, b, c = dc.checker()
    h, g = dp.checker("host", a, b, c), dp.checker("gxx", a, b, c)
    assert_same(h, g, (a, b, c), "checker_odd host pass / g++")
    assert 0.2 < h.mean() < 0.8  # both answers occur
    x = dc.checker_args()
    (hn, hk), (gn, gk) = dp.sin_neg("host", x), dp.sin_neg("gxx", x)
    assert np.array_equal(hn, gn) and np.array_equal(hk, gk)
    assert hk.any() and not hk.all()  # both paths of checker_odd


def test_checker_is_the_sign_of_the_product():
    """checker_odd against its definition, det_sinf(a) * det_sinf(b) * det_sinf(c) < 0 in float32."""
    a, b, c = dc.checker()
    s = [dp.unary("gxx", "sin", v).view(np.float32) for v in (a, b, c)]
    with np.errstate(all="ignore"):
        want = ((s[0] * s[1]) * s[2] < 0).astype(U32)
    assert np.array_equal(dp.checker("host", a, b, c), want)


# ------------------------------------------------------------------ 2. accuracy against mpmath
def _mp():
    import mpmath

    mpmath.mp.prec = 120
    return mpmath


def _ulp_of(mpm, exact):
    """The float32 ulp at the magnitude of exact (an mpf): 2^(e - 23), e clamped to [-126, 127]."""
    if exact == 0:
        return mpm.ldexp(1, -149)
    e = mpm.frexp(exact)[1] - 1
    return mpm.ldexp(1, min(max(e, -126), 127) - 23)


OVERFLOW = Fraction(2 ** 128 - 2 ** 103)  # from here a correctly rounded float is inf


def _error(mpm, got_bits, exact, margin):
    """|float(got) - exact| in float ulps; an inf is right (0) where exact rounds to it, wrong (inf) elsewhere."""
    got = np.array([got_bits], U32).view(np.float32)[0]
    if np.isinf(got):
        lim = mpm.mpf(OVERFLOW.numerator) * (1 - margin * 2.0 ** -24)
        return 0.0 if (exact >= lim if got > 0 else exact <= -lim) else float("inf")
    return float(abs(mpm.mpf(float(got)) - exact) / _ulp_of(mpm, exact))


def _exact_unary(mpm, fn, x):
    x = mpm.mpf(float(x))
    return {"sin": mpm.sin, "cos": mpm.cos, "tan": mpm.tan, "log": mpm.log, "acos": mpm.acos, "pow5": lambda v: v ** 5}[fn](x)


def _domain(fn, xs):
    """The inputs at which det_fn has a finite argument in its domain (sin / cos / tan: |x| <= 2^20)."""
    a = xs & U32(0x7FFFFFFF)
    if fn in ("sin", "cos", "tan"):
        return a <= TWO20
    if fn == "log":
        return (xs > 0) & (xs < dc.INF)
    if fn == "acos":
        return a <= dc.bits(1.0)
    return a < dc.INF


@functools.lru_cache(maxsize=None)
def _accuracy(fn):
    """(inputs, worst float error in ulps, its x, worst relative error of the double before the cast)."""
    mpm = _mp()
    xs = np.unique(np.concatenate([CASES[fn](), dc.strided(65521)]))
    xs = xs[_domain(fn, xs)]
    got = dp.unary("gxx", fn, xs)
    dbl = dp.unary_double_gxx(fn, xs)
    with np.errstate(all="ignore"):  # the cast of that double is det_fn's result
        assert np.array_equal(dbl.astype(np.float32).view(U32), got)
    worst, worst_x, rel = 0.0, 0, 0.0
    for xb, xf, g, d in zip(xs.tolist(), xs.view(np.float32).tolist(), got.tolist(), dbl.tolist()):
        exact = _exact_unary(mpm, fn, xf)
        e = _error(mpm, g, exact, MARGIN[fn])
        if e > worst:
            worst, worst_x = e, xb
        if exact != 0:
            rel = max(rel, float(abs((mpm.mpf(d) - exact) / exact)))
    return xs.size, worst, worst_x, rel


@pytest.mark.parametrize("fn", DET_FNS)
def test_accuracy_unary(fn):
    n, worst, worst_x, rel = _accuracy(fn)
    print(f"det_{fn}f: {n} inputs, worst {worst:.7f} ulp at {worst_x:#010x}, double before the cast 2^{np.log2(rel):.2f}")
    assert MARGIN[fn] <= 2.0 ** -10
    assert worst <= 0.5 + MARGIN[fn], f"det_{fn}f({worst_x:#010x}): {worst} ulp"


@pytest.mark.parametrize("fn", ["sin", "cos"])
def test_accuracy_above_the_exact_reduction(fn):
    """2^20 < |x| <= 1e9: absolute error at most 2^-22."""
    mpm = _mp()
    xs = np.unique(np.concatenate([dc.trig(), dc.strided(65521)]))
    a = xs & U32(0x7FFFFFFF)
    xs = xs[(a > TWO20) & (a <= ONE_E9)]
    assert xs.size > 3000
    got = dp.unary("gxx", fn, xs).view(np.float32)
    f = {"sin": mpm.sin, "cos": mpm.cos}[fn]
    worst, worst_x = 0.0, 0
    for xb, xf, g in zip(xs.tolist(), xs.view(np.float32).tolist(), got.tolist()):
        e = float(abs(mpm.mpf(g) - f(mpm.mpf(xf))))
        if e > worst:
            worst, worst_x = e, xb
    print(f"det_{fn}f above 2^20: {xs.size} inputs, worst absolute error 2^{np.log2(worst):.2f} at {worst_x:#010x}")
    assert worst <= 2.0 ** -22, f"det_{fn}f({worst_x:#010x}): 2^{np.log2(worst):.2f}"


@pytest.mark.parametrize("fn", DET_FNS)
def test_outside_the_domain(fn):
    """What the header defines there: the default NaN for |x| > 1e9 (sin / cos / tan), x < 0 (log), |x| > 1
    (acos) and every NaN but log's, which returns its argument; log(+-0) = -inf, log(inf) = inf, (+-inf)^5."""
    xs = np.unique(np.concatenate([CASES[fn](), dc.strided(65521)]))
    got = dp.unary("gxx", fn, xs)
    a = xs & U32(0x7FFFFFFF)
    nan = isnan(xs)
    if fn in ("sin", "cos", "tan"):
        out = nan | (a > ONE_E9)
        assert (got[out] == QNAN).all() and not isnan(got[~out]).any()
    elif fn == "acos":
        out = nan | (a > dc.bits(1.0))
        assert (got[out] == QNAN).all() and not isnan(got[~out]).any()
    elif fn == "log":
        assert np.array_equal(got[nan], xs[nan])
        assert (got[a == 0] == 0xFF800000).all()
        neg = ~nan & (a != 0) & (xs >= dc.SIGN)
        assert (got[neg] == QNAN).all()
        assert (got[xs == dc.INF] == dc.INF).all()
    else:
        assert isnan(got[nan]).all() and np.array_equal(got[a == dc.INF], xs[a == dc.INF])


ATAN2_MPMATH = 1 << 16  # of the random pairs; every pair is screened in long double below


def _atan2_exact(mpm, y, x):
    import math

    if y == 0 or x == 0 or math.isinf(y) or math.isinf(x):  # C's table: a multiple of pi / 4
        k = round(math.atan2(y, x) / (math.pi / 4))
        return mpm.pi * k / 4
    return mpm.atan2(mpm.mpf(y), mpm.mpf(x))


@functools.lru_cache(maxsize=None)
def _accuracy_atan2():
    mpm = _mp()
    y, x = dc.atan2()
    got = dp.atan2("gxx", y, x)
    dbl = dp.atan2_double_gxx(y, x)
    ok = ~(isnan(y) | isnan(x))
    assert isnan(got[~ok]).all() and not isnan(got[ok]).any()
    # every pair in x87 long double (64-bit significand, so its own error is far below 2^-20 float ulp): a pair
    # within 2^-20 ulp of the bound, or over it, goes to mpmath with the first ATAN2_MPMATH random pairs
    assert np.finfo(np.longdouble).nmant >= 63
    with np.errstate(all="ignore"):
        yl, xl = y.view(np.float32).astype(np.longdouble), x.view(np.float32).astype(np.longdouble)
        want = np.arctan2(yl, xl)
        e = np.floor(np.log2(np.abs(want)))
        ulp = np.exp2(np.clip(np.where(np.isfinite(e), e, -149), -126, 127) - 23)
        err = np.abs(got.view(np.float32).astype(np.longdouble) - want) / ulp
    close = ok & ~(err <= 0.5 - 2.0 ** -20)
    first_random = y.size - dc.ATAN2_RANDOM
    pick = np.nonzero(ok & ((np.arange(y.size) < first_random + ATAN2_MPMATH) | close))[0]
    worst, worst_i, rel = 0.0, 0, 0.0
    yf, xf = y.view(np.float32), x.view(np.float32)
    for i in pick.tolist():
        exact = _atan2_exact(mpm, float(yf[i]), float(xf[i]))
        er = _error(mpm, int(got[i]), exact, MARGIN["atan2"])
        if er > worst:
            worst, worst_i = er, i
        if exact != 0:
            rel = max(rel, float(abs((mpm.mpf(float(dbl[i])) - exact) / exact)))
    return pick.size, int(close.sum()), worst, (int(y[worst_i]), int(x[worst_i])), rel


def test_accuracy_atan2():
    n, close, worst, at, rel = _accuracy_atan2()
    print(f"det_atan2f: {n} pairs in mpmath ({close} sent by the long double screen of all {dc.atan2()[0].size}), "
          f"worst {worst:.7f} ulp at y {at[0]:#010x} x {at[1]:#010x}, double before the cast 2^{np.log2(rel):.2f}")
    assert MARGIN["atan2"] <= 2.0 ** -10
    assert worst <= 0.5 + MARGIN["atan2"], f"det_atan2f{at}: {worst} ulp"


def test_detmath_on_the_linear_sweep():
    """The sweep of the test this file replaces (test_detmath_against_libm: x = i * 0.00037f for |i| <= 200 000,
    sin and cos of x and log of |x| + 1e-7f, then held to 2e-7 relative against double libm), held to
    0.5 ulp + MARGIN like every other input.  All 400 001 arguments are screened in x87 long double, whose own
    error is far below 2^-20 float ulp; a result within 2^-20 ulp of the bound, or over it, goes to mpmath."""
    mpm = _mp()
    assert np.finfo(np.longdouble).nmant >= 63
    x = np.arange(-200000, 200001).astype(np.float32) * np.float32(0.00037)
    args = {"sin": x, "cos": x, "log": np.abs(x) + np.float32(1e-7)}
    for fn, ref in (("sin", np.sin), ("cos", np.cos), ("log", np.log)):
        xs = np.ascontiguousarray(args[fn]).view(U32)
        got = dp.unary("gxx", fn, xs)
        assert np.array_equal(got, dp.unary("host", fn, xs))
        with np.errstate(all="ignore"):
            want = ref(args[fn].astype(np.longdouble))
            e = np.floor(np.log2(np.abs(want)))
            ulp = np.exp2(np.clip(np.where(np.isfinite(e), e, -149), -126, 127) - 23)
            gl = got.view(np.float32).astype(np.longdouble)
            err = np.abs(gl - want) / ulp
            old = np.abs(gl - want) <= (2e-7 if fn != "log" else 4e-7) * np.maximum(1, np.abs(want))
        assert old.all(), f"det_{fn}f: the replaced test's own bound"
        close = np.nonzero(~(err <= 0.5 - 2.0 ** -20))[0]
        worst = 0.0
        for i in close.tolist():
            worst = max(worst, _error(mpm, int(got[i]), _exact_unary(mpm, fn, float(args[fn][i])), MARGIN[fn]))
        print(f"det_{fn}f on the linear sweep: worst {float(err.max()):.7f} ulp in long double, {close.size} sent to mpmath, worst of them {worst:.7f}")
        assert worst <= 0.5 + MARGIN[fn]


# ------------------------------------------------------------------ 3. exact references for the other families
def rne_f32_of_u32(w):
    """float32 nearest to each uint32, ties to even, in integer arithmetic; returned as float64 (exact)."""
    w = np.asarray(w, np.uint64)
    length = np.frexp(w.astype(np.float64))[1].astype(np.uint64)  # bit length: a uint32 is exact in float64
    sh = np.where(length > 24, length - np.uint64(24), np.uint64(0))
    q, r = w >> sh, w & ((np.uint64(1) << sh) - np.uint64(1))
    half = np.where(sh > 0, np.uint64(1) << (np.maximum(sh, np.uint64(1)) - np.uint64(1)), np.uint64(0))
    up = (sh > 0) & ((r > half) | ((r == half) & ((q & np.uint64(1)) == 1)))
    return ((q + up.astype(np.uint64)) << sh).astype(np.float64)


def uniform_ref(word):
    """curand_uniform: float32(float32_RNE(w) * 2^-32 + 2^-33).  The sum has at most 34 significant bits, so
    float64 holds it exactly and the one rounding is the cast."""
    return (rne_f32_of_u32(word) * 2.0 ** -32 + 2.0 ** -33).astype(np.float32).view(U32)


def xorwow_ref(st):
    st = np.asarray(st, U32)
    v4 = dc.xorwow_v4_after(st[:, 1:])
    d = st[:, 0] + U32(362437)
    after = np.concatenate([d[:, None], st[:, 2:6], v4[:, None]], axis=1)
    return v4 + d, after


def test_rne_reference_itself():
    assert rne_f32_of_u32([0, 1, (1 << 24) + 1, (1 << 24) + 3, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF]).tolist() == [
        0.0, 1.0, float(1 << 24), float((1 << 24) + 4), float(0xFFFFFF00), float(1 << 32), float(1 << 32)]


def check_xorwow(side):
    from test_oracle_cpu import _py_next

    st, chosen = dc.xorwow_states()
    word, ubits, after = dp.xorwow(side, st)
    want_word, want_after = xorwow_ref(st)
    assert np.array_equal(word[chosen >= 0].astype(np.int64), chosen[chosen >= 0])  # the words the set was built for
    assert np.array_equal(word, want_word) and np.array_equal(after, want_after)
    assert np.array_equal(ubits, uniform_ref(word))
    u = ubits.view(np.float32)
    assert u.min() == np.float32(2.0 ** -33) and u.max() == np.float32(1.0)  # words 0 and 2^32 - 1: (0, 1]
    for i in list(range(int((chosen >= 0).sum()))) + list(range(st.shape[0] - 256, st.shape[0])):  # pure Python
        w, d, v = _py_next(int(st[i, 0]), [int(x) for x in st[i, 1:]])
        assert (w, [d] + v) == (int(word[i]), after[i].tolist()), i


def check_seed_state(side):
    from test_oracle_cpu import _py_state

    seeds = dc.seeds()
    got = dp.seed_state(side, seeds)
    for s, row in zip(seeds.tolist(), got.tolist()):
        d, v = _py_state(s, 0, None)
        assert row == [d] + v, hex(s)


def test_xorwow_host_pass():
    check_xorwow("host")
    check_seed_state("host")


SEEDS_INIT = [(1 << 32) - 1, 1 << 32, 0x9E3779B97F4A7C15, (1 << 64) - 1]


def init_slots(W, H):
    """The slot classes of test_render_init_states_match_curand_init (tests/test_parity_gpu.py) on a W x H image."""
    rng = np.random.default_rng(7)
    return sorted(set(s for s in [0, 1, 2, 15, 16, 17, 1023, W * H - 1] if s < W * H) | set(int(s) for s in rng.integers(0, W * H, 200)))


def test_oracle_xorwow_init_with_64_bit_seeds(oracle):
    """oracle.xorwow_init == the pure-Python generator where the high half of the seed is not zero."""
    from test_oracle_cpu import ROCRAND_PRECOMP, _py_state, _rocrand_table

    assert os.path.exists(ROCRAND_PRECOMP), "rocRAND's jump tables are the pure-Python generator's"
    seq = _rocrand_table("h_xorwow_sequence_jump_matrices")
    slots = init_slots(64, 36)
    for seed in SEEDS_INIT:
        for s in slots[:8] + slots[8::6] + slots[-1:]:
            d, v = _py_state(seed, s, seq)
            assert [int(x) for x in oracle.xorwow_init(seed, s, 0)] == [d] + v, (hex(seed), s)


def quant_ref(xb):
    """trunc(256 * clamp(float32(sqrt_f64(x)), 0, 0.999f)), a NaN giving 0.  Rounding the double root to float
    gives the correctly rounded float root (double rounding is innocuous for sqrt at p = 24, 2p + 2 <= 53)."""
    x = np.asarray(xb, U32).view(np.float32)
    with np.errstate(all="ignore"):
        r = np.sqrt(x.astype(np.float64)).astype(np.float32)
    c = np.where(r < 0, np.float32(0), np.where(r > np.float32(0.999), np.float32(0.999), r)).astype(np.float32)
    q = (c.astype(np.float64) * 256.0)  # exact
    return np.where(np.isnan(r), 0, np.trunc(np.nan_to_num(q))).astype(U32)


def check_quant(side):
    xs = dc.quant()
    got = dp.unary(side, "quant", xs)
    assert np.array_equal(got, quant_ref(xs))
    assert set(got.tolist()) == set(range(256))  # every level, so both sides of every threshold
    sw = dc.strided(1021)
    assert np.array_equal(dp.unary(side, "quant", sw), quant_ref(sw))


def test_quant_host_pass():
    check_quant("host")


def rne(fr, p, emin):
    """The Fraction fr >= 0 rounded to nearest even at precision p with the least exponent emin (IEEE binary
    with denormals; no overflow handling)."""
    if fr == 0:
        return fr
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    assert Fraction(2) ** e <= fr < Fraction(2) ** (e + 1)
    q = Fraction(2) ** (max(e, emin) - (p - 1))
    n = fr / q
    k, rem = divmod(n.numerator, n.denominator)
    if 2 * rem > n.denominator or (2 * rem == n.denominator and k & 1):
        k += 1
    return k * q


def f64(fr):
    return rne(fr, 53, -1022)


def f32_bits(fr):
    return int(np.float32(float(rne(fr, 24, -126))).view(U32))  # the float() and float32() of it are exact


def check_denoise_math(side):
    import denoise_ref as dr
    import guide_ref as gr

    # prepare: the numpy definition, and Fractions rounded once per operation
    s1, s2, n = dc.dn_moments()
    M, V = dp.dn_prepare(side, s1, s2, n)
    Q, Mr, Vr = dr.prepare(s1.reshape(-1, 1, 1), s2.reshape(-1, 1, 1), n.reshape(-1, 1))
    assert np.array_equal(M, Mr.ravel().view(U32)) and np.array_equal(V, Vr.ravel().view(U32))
    for a, b, c, m, v in zip(s1.tolist(), s2.tolist(), n.tolist(), M.tolist(), V.tolist()):
        q = (256 * a + c // 2) // c
        assert m == f32_bits(Fraction(q, 256))
        assert v == f32_bits(f64(Fraction(c * b - a * a) / f64(f64(Fraction(c * c)) * (c - 1))))
    assert (V[(s1 == 0)] == 0).all() and (M.view(np.float32).max() == 255.0)
    assert np.array_equal(dp.dn_q_of(side, M), Q.ravel().astype(U32))
    # term
    ops = dc.dn_term_ops()
    o = ops.view(np.float32)
    got = dp.dn_term(side, ops)
    want = dr.term(*(o[:, k] for k in range(7)))
    assert np.array_equal(got.astype(np.int64), want)
    assert got.min() == -64 * 256 and got.max() == 64 * 256 and len(set(got.tolist())) > 200
    # weight, both overloads
    P, cnt, xf = dc.dn_weight_ops()
    w = dp.dn_weight(side, P, cnt)
    assert np.array_equal(w.astype(np.uint64), dr.weight(P, cnt))
    assert w.max() == 65536 and w.min() == 0 and np.unique(w[cnt == 49]).size > 10000
    wf = dp.dn_weight(side, P, cnt, xf)
    assert np.array_equal(wf.astype(np.uint64), gr.weight(P, cnt, xf.view(np.float32)))
    # feature_x
    p, q, g = dc.dn_features()
    pf, qf, gf = p.view(np.float32), q.view(np.float32), g.view(np.float32)
    x = dp.dn_feature_x(side, p, q, g)
    want = gr.feature_x(pf[:, 0:3], pf[:, 3:6], pf[:, 6], qf[:, 0:3], qf[:, 3:6], qf[:, 6], (gf[:, 0], gf[:, 1], gf[:, 2]))
    assert np.array_equal(x, np.ascontiguousarray(want).view(U32))
    assert not isnan(x).any() and (x == dc.bits(64.0)).sum() > 1000 and (x == dc.INF).any() and (x == 0).any()
    # patch_span
    a = dc.dn_spans()
    want = [int(((np.arange(-f, f + 1) + pp >= 0) & (np.arange(-f, f + 1) + pp < size) & (np.arange(-f, f + 1) + pp + oo >= 0)
                 & (np.arange(-f, f + 1) + pp + oo < size)).sum()) for pp, oo, f, size in a.tolist()]
    assert dp.dn_patch_span(side, a).tolist() == want
    # linear and gain
    Num, Den = dc.dn_linear_ops()
    lin, gain = dp.dn_linear_gain(side, Num, Den)
    for nu, de, l, gn in zip(Num.tolist(), Den.tolist(), lin.tolist(), gain.tolist()):
        den = f64(f64(f64(Fraction(de)) * 256) * 65025)
        assert l == f32_bits(f64(f64(Fraction(nu)) / den)), (nu, de)
        assert gn == f32_bits(f64(Fraction(de)) / 65536), de


def test_denoise_math_host_pass():
    check_denoise_math("host")


if __name__ == "__main__":  # the table of the header comment
    for fn_ in DET_FNS:
        n_, worst_, x_, rel_ = _accuracy(fn_)
        print(f"{fn_:6s} {n_:8d}  {worst_:.7f}  {x_:#010x}  2^{np.log2(rel_):.2f}  margin 2^{np.log2(4 * rel_ * 2 ** 24):.2f}")
    n_, close_, worst_, at_, rel_ = _accuracy_atan2()
    print(f"atan2  {n_:8d}  {worst_:.7f}  {at_}  2^{np.log2(rel_):.2f}  margin 2^{np.log2(4 * rel_ * 2 ** 24):.2f}  ({close_} from the screen)")
