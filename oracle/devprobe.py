"""ctypes wrapper of the device probe (oracle/_build/librt_devprobe.so, oracle/devprobe/rt_devprobe.hip) and of
its g++ twin (oracle/_build/librt_devprobe_gxx.so).

TEST INFRASTRUCTURE ONLY.  The probe runs the arithmetic that host and device code share (csrc/rt_detmath.h,
rt_xorwow.h, rt_quant.h, rt_denoise_math.h) one value at a time, compiled by each compiler that reads it:

    side "dev"   hipcc's device pass, in a kernel on the GPU
    side "host"  hipcc's host pass, no GPU needed
    side "gxx"   g++ with the oracle's flags (rt_detmath.h's functions only)

Floats go in and come out as uint32 bit patterns.  A HIP error from a "dev" entry raises ProbeError.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_int, c_size_t, c_uint32, c_void_p

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_build", "librt_devprobe.so")
GXX_LIB_PATH = os.path.join(HERE, "_build", "librt_devprobe_gxx.so")

UNARY = {"sin": 0, "cos": 1, "tan": 2, "log": 3, "pow5": 4, "acos": 5, "quant": 6}
SIDES = ("dev", "host", "gxx")


class ProbeError(RuntimeError):
    def __init__(self, entry: str, status: int):
        super().__init__(f"{entry}: HIP error {status}")
        self.entry, self.status = entry, status


_libs: dict = {}


def _lib(side: str) -> ctypes.CDLL:
    path = GXX_LIB_PATH if side == "gxx" else LIB_PATH
    if path not in _libs:
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: run `python -m raytracing_gpu_amd._build`")
        _libs[path] = ctypes.CDLL(path)
    return _libs[path]


def _u32(a) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype == np.float32:
        a = a.view(np.uint32)
    return np.ascontiguousarray(a, np.uint32)


def _call(side: str, name: str, *args):
    assert side in SIDES, side
    fn = getattr(_lib(side), f"devprobe_{name}_{side}")
    fn.restype = c_int
    conv = []
    for a in args:
        if isinstance(a, np.ndarray):
            conv.append(c_void_p(a.ctypes.data))
        elif a is None:
            conv.append(c_void_p(None))
        else:
            conv.append(a)
    st = fn(*conv)
    if st != 0:
        raise ProbeError(f"devprobe_{name}_{side}", st)


def unary(side: str, fn: str, x) -> np.ndarray:
    """det_sinf .. det_acosf or quant of each x (float32 or its bits): uint32 bits, quant's int as uint32."""
    x = _u32(x).ravel()
    y = np.empty(x.size, np.uint32)
    _call(side, "unary", c_int(UNARY[fn]), x, y, c_size_t(x.size))
    return y


def unary_range(side: str, fn: str, first: int, count: int, out: np.ndarray | None = None) -> np.ndarray:
    """unary() over the bit patterns first .. first + count - 1 (no operand array; sides "dev" and "host")."""
    y = np.empty(count, np.uint32) if out is None else out
    assert y.dtype == np.uint32 and y.size == count and y.flags.c_contiguous
    _call(side, "unary_range", c_int(UNARY[fn]), c_uint32(first), y, c_size_t(count))
    return y


def atan2(side: str, y, x) -> np.ndarray:
    y, x = _u32(y).ravel(), _u32(x).ravel()
    assert y.size == x.size
    out = np.empty(x.size, np.uint32)
    _call(side, "binary", y, x, out, c_size_t(x.size))
    return out


def checker(side: str, a, b, c) -> np.ndarray:
    a, b, c = _u32(a).ravel(), _u32(b).ravel(), _u32(c).ravel()
    assert a.size == b.size == c.size
    out = np.empty(a.size, np.uint32)
    _call(side, "checker", a, b, c, out, c_size_t(a.size))
    return out


def sin_neg(side: str, x):
    """sin_neg_fast: (neg, ok) as bool arrays."""
    x = _u32(x).ravel()
    out = np.empty(x.size, np.uint32)
    _call(side, "sin_neg", x, out, c_size_t(x.size))
    return (out & 1) != 0, (out & 2) != 0


def xorwow(side: str, states):
    """One rtx::next and one rtx::uniform from each state [n][6] (d, v0..v4): (word [n], uniform bits [n],
    state after next [n][6])."""
    st = np.ascontiguousarray(states, np.uint32).reshape(-1, 6)
    n = st.shape[0]
    word, ubits, after = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty((n, 6), np.uint32)
    _call(side, "xorwow", st, word, ubits, after, c_size_t(n))
    return word, ubits, after


def seed_state(side: str, seeds) -> np.ndarray:
    seeds = np.ascontiguousarray(seeds, np.uint64).ravel()
    out = np.empty((seeds.size, 6), np.uint32)
    _call(side, "seed_state", seeds, out, c_size_t(seeds.size))
    return out


def dn_prepare(side: str, s1, s2, n):
    s1 = np.ascontiguousarray(s1, np.uint32).ravel()
    s2 = np.ascontiguousarray(s2, np.uint64).ravel()
    n = np.ascontiguousarray(n, np.int32).ravel()
    assert s1.size == s2.size == n.size
    M, V = np.empty(s1.size, np.uint32), np.empty(s1.size, np.uint32)
    _call(side, "dn_prepare", s1, s2, n, M, V, c_size_t(s1.size))
    return M, V


def dn_q_of(side: str, M) -> np.ndarray:
    M = _u32(M).ravel()
    q = np.empty(M.size, np.uint32)
    _call(side, "dn_q_of", M, q, c_size_t(M.size))
    return q


def dn_term(side: str, ops) -> np.ndarray:
    """ops [n][7] float32: Ma Va Mb Vb alpha kk eps."""
    ops = _u32(ops).reshape(-1, 7)
    t = np.empty(ops.shape[0], np.int32)
    _call(side, "dn_term", ops, t, c_size_t(ops.shape[0]))
    return t


def dn_weight(side: str, P, cnt, xf=None) -> np.ndarray:
    P = np.ascontiguousarray(P, np.int32).ravel()
    cnt = np.ascontiguousarray(cnt, np.int32).ravel()
    xf = None if xf is None else _u32(xf).ravel()
    assert P.size == cnt.size and (xf is None or xf.size == P.size)
    w = np.empty(P.size, np.uint32)
    _call(side, "dn_weight", P, cnt, xf, w, c_size_t(P.size))
    return w


def dn_feature_x(side: str, p, q, gains) -> np.ndarray:
    """p, q [n][7] float32 (normal, albedo, depth), gains [n][3] (normal, albedo, depth)."""
    p, q, g = _u32(p).reshape(-1, 7), _u32(q).reshape(-1, 7), _u32(gains).reshape(-1, 3)
    assert p.shape == q.shape and g.shape[0] == p.shape[0]
    xf = np.empty(p.shape[0], np.uint32)
    _call(side, "dn_feature_x", p, q, g, xf, c_size_t(p.shape[0]))
    return xf


def dn_patch_span(side: str, a) -> np.ndarray:
    """a [n][4] int32: p o f size."""
    a = np.ascontiguousarray(a, np.int32).reshape(-1, 4)
    out = np.empty(a.shape[0], np.int32)
    _call(side, "dn_patch_span", a, out, c_size_t(a.shape[0]))
    return out


def dn_linear_gain(side: str, Num, Den):
    Num = np.ascontiguousarray(Num, np.uint64).ravel()
    Den = np.ascontiguousarray(Den, np.uint64).ravel()
    assert Num.size == Den.size
    lin, gain = np.empty(Num.size, np.uint32), np.empty(Num.size, np.uint32)
    _call(side, "dn_linear_gain", Num, Den, lin, gain, c_size_t(Num.size))
    return lin, gain


def unary_double_gxx(fn: str, x) -> np.ndarray:
    """The double that det_*f casts to float (g++ build; log for positive finite x, acos for |x| <= 1)."""
    x = _u32(x).ravel()
    y = np.empty(x.size, np.float64)
    f = _lib("gxx").devprobe_unary_double_gxx
    f.restype = c_int
    assert f(c_int(UNARY[fn]), c_void_p(x.ctypes.data), c_void_p(y.ctypes.data), c_size_t(x.size)) == 0
    return y


def atan2_double_gxx(y, x) -> np.ndarray:
    y, x = _u32(y).ravel(), _u32(x).ravel()
    out = np.empty(x.size, np.float64)
    f = _lib("gxx").devprobe_atan2_double_gxx
    f.restype = c_int
    assert f(c_void_p(y.ctypes.data), c_void_p(x.ctypes.data), c_void_p(out.ctypes.data), c_size_t(x.size)) == 0
    return out
