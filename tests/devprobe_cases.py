"""The input sets of the device probe's tests (tests/test_devprobe_cpu.py, tests/test_devprobe_gpu.py): for each
family of shared arithmetic the arguments at which it can go wrong, as deterministic arrays.  Floats are uint32
bit patterns throughout.  Nothing here calls the code under test."""
import functools
import math

import numpy as np

U32 = np.uint32
SIGN = 0x80000000
INF = 0x7F800000
MAXF = 0x7F7FFFFF
MIN_NORMAL = 0x00800000  # 2^-126
MAX_DENORMAL = 0x007FFFFF
NANS = [0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7FC12345, 0x7FA00000, 0xFFC00000, 0xFF800001, 0xFFFFFFFF, 0xFFD54321]


def bits(v) -> int:
    """The bit pattern of float32(v), v a Python float rounded once."""
    return int(np.float32(v).view(U32))


def around(v, k=64):
    """The 2k + 1 floats within k ulps of float32(v) (v > 0, away from 0 and inf)."""
    b = bits(v)
    return np.arange(b - k, b + k + 1, dtype=np.int64)


def both_signs(a):
    a = np.asarray(a, np.int64) & 0x7FFFFFFF
    return np.concatenate([a, a | SIGN])


def _finish(parts):
    return np.unique(np.concatenate([np.asarray(p, np.int64).ravel() for p in parts])).astype(U32)


def strided(step):
    """Every step-th bit pattern, both signs."""
    return both_signs(np.arange(0, 1 << 31, step, dtype=np.int64)).astype(U32)


@functools.lru_cache(maxsize=None)
def lcg64(count, seed=0x2545F4914F6CDD1D):
    """count words of Knuth's MMIX LCG x <- 6364136223846793005 x + 1442695040888963407 (mod 2^64), in order;
    the high 32 bits of each state.  4096 states stepped in Python, the rest by the 4096-step jump."""
    A, C, M = 6364136223846793005, 1442695040888963407, (1 << 64) - 1
    L = 4096
    first, x, aL, cL = [], seed, 1, 0
    for _ in range(L):
        x = (A * x + C) & M
        first.append(x)
        aL, cL = (aL * A) & M, (cL * A + C) & M
    rows = -(-count // L)
    out = np.empty((rows, L), np.uint64)
    cur = np.array(first, np.uint64)
    with np.errstate(over="ignore"):
        for r in range(rows):
            out[r] = cur
            cur = cur * np.uint64(aL) + np.uint64(cL)
    return (out.ravel()[:count] >> np.uint64(32)).astype(U32)


# ------------------------------------------------------------------ rt_detmath.h
TRIG_K = [1, 2, 3, 4, 5, 6, 7, 8, 2 ** 10, 2 ** 17, 2 ** 20, 2 ** 29]
TWO20 = float(2 ** 20)


@functools.lru_cache(maxsize=None)
def trig():
    """sin / cos / tan."""
    parts = [[0, 1, MAX_DENORMAL, MIN_NORMAL]]
    parts += [around(k * math.pi / 2) for k in TRIG_K]  # k pi / 2 rounded to double, then to float
    parts += [around(2.0 ** -20), around(2.0 ** 17), around(TWO20), around(1e9)]
    parts += [[INF]]
    return _finish([both_signs(np.concatenate([np.asarray(p, np.int64) for p in parts])), NANS])


@functools.lru_cache(maxsize=None)
def log():
    den = [1 << j for j in range(23)] + [(1 << j) | ((1 << j) >> 1) | 1 for j in range(23)] + [MAX_DENORMAL]
    parts = [den, around(1.0), around(2.0), around(math.sqrt(2.0)), np.arange(MIN_NORMAL - 64, MIN_NORMAL + 65),
             [0, SIGN, INF, INF | SIGN, MAXF, bits(-1.0), bits(-1e-40), bits(-3e38), 1 | SIGN], NANS]
    return _finish(parts)


@functools.lru_cache(maxsize=None)
def pow5():
    """x^5 is denormal for 2^-29.8 <= |x| < 2^-25.2, 0 below, inf from 2^25.6."""
    parts = [np.arange(bits(2.0 ** -31), bits(2.0 ** -24), 1021), np.arange(bits(2.0 ** 25), bits(2.0 ** 26), 1021),
             around(2.0 ** (-149 / 5)), around(2.0 ** (-150 / 5)), around(2.0 ** (-126 / 5)), around(2.0 ** (128 / 5)),
             around(1.0), [0, 1, MAX_DENORMAL, MIN_NORMAL, MAXF, INF]]
    return _finish([both_signs(np.concatenate([np.asarray(p, np.int64) for p in parts])), NANS])


@functools.lru_cache(maxsize=None)
def acos():
    one = bits(1.0)
    parts = [np.arange(one - 64, one + 3), [0, 1, 2, MAX_DENORMAL, MIN_NORMAL, bits(0.5), bits(2.0), MAXF, INF]]
    return _finish([both_signs(np.concatenate([np.asarray(p, np.int64) for p in parts])), NANS])


ATAN2_SPECIAL = [0, SIGN, 1, 1 | SIGN, MIN_NORMAL, MIN_NORMAL | SIGN, 0x3F800000, 0x3F800000 | SIGN, MAXF, MAXF | SIGN,
                 INF, INF | SIGN, 0x7FC00000]
ATAN2_RANDOM = 1 << 22


@functools.lru_cache(maxsize=None)
def atan2():
    """(y bits, x bits)."""
    sp = np.array(ATAN2_SPECIAL, np.int64)
    ys, xs = [np.repeat(sp, sp.size)], [np.tile(sp, sp.size)]
    for ratio in (math.tan(math.pi / 8), 1.0):  # atan_pos's two switches
        for x in (1.0, 3.0, 2.0 ** -100, 2.0 ** 100):
            for sy in (0, SIGN):
                for sx in (0, SIGN):
                    y = around(ratio * x)
                    ys.append(y | sy)
                    xs.append(np.full(y.size, bits(x) | sx, np.int64))
    r = lcg64(2 * ATAN2_RANDOM)
    ys.append(r[0::2].astype(np.int64))
    xs.append(r[1::2].astype(np.int64))
    return np.concatenate(ys).astype(U32), np.concatenate(xs).astype(U32)


@functools.lru_cache(maxsize=None)
def checker_args():
    """Arguments of sin_neg_fast: the limits of its range, k pi, and values on both sides."""
    inside = [2.0 ** -20, 1e-3, 0.5, 3.0, 3.5, 31.4, 1000.0, 2.0 ** 17]
    outside = [0.0, 1e-45, 2.0 ** -21, np.nextafter(np.float32(2.0 ** -20), np.float32(0)), np.nextafter(np.float32(2.0 ** 17), np.float32(1e9)),
               2.0 ** 18, 1e9, 2e9]
    parts = [[bits(v) for v in inside + outside], [INF]]
    parts += [around(k * math.pi, 8) for k in list(range(1, 65)) + [2 ** 10, 41721, 41722, 2 ** 20]]
    return _finish([both_signs(np.concatenate([np.asarray(p, np.int64) for p in parts])), NANS[:2]])


@functools.lru_cache(maxsize=None)
def checker():
    """(a, b, c): the cross product of a small set on both sides of [2^-20, 2^17] (both paths of checker_odd),
    every argument of checker_args() in each position beside two fixed ones, and random triples of moderate size."""
    small = np.array([bits(v) for v in (2.0 ** -20, 0.5, -3.5, 31.4, -1000.0, 2.0 ** 17, 0.0, -0.0, 2.0 ** -21, -(2.0 ** 18), 1e9, 2e9)]
                     + [INF, 0x7FC00000, 1], np.int64)
    n = small.size
    A = [np.repeat(small, n * n)]
    B = [np.tile(np.repeat(small, n), n)]
    C = [np.tile(small, n * n)]
    args = checker_args().astype(np.int64)
    for other in ((bits(1.0), bits(-2.0)), (bits(4.0), bits(2.0 ** -22))):
        o0, o1 = np.full(args.size, other[0], np.int64), np.full(args.size, other[1], np.int64)
        for tri in ((args, o0, o1), (o0, args, o1), (o1, o0, args)):
            A.append(tri[0]), B.append(tri[1]), C.append(tri[2])
    # random floats with exponents 2^-24 .. 2^20: sign, 8 exponent values cycled, random mantissa
    r = lcg64(3 << 16).astype(np.int64)
    e = 127 - 24 + (r >> 23) % 45
    f = (r & (SIGN | 0x7FFFFF)) | (e << 23)
    A.append(f[0::3]), B.append(f[1::3]), C.append(f[2::3])
    return tuple(np.concatenate(p).astype(U32) for p in (A, B, C))


# ------------------------------------------------------------------ rt_xorwow.h
XORWOW_WORDS = sorted(set([0, 1, (1 << 24) + 1, (1 << 24) + 3, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFF81, 0xFFFFFFFF]
                          + [w for k in range(1, 32) for w in ((1 << k) - 1, 1 << k, (1 << k) + 1)]))
XORWOW_RANDOM = 1 << 20


def xorwow_v4_after(v):
    """v[4] after one step of the recurrence, v [n][5] uint32 (numpy, not the code under test)."""
    v = np.asarray(v, U32)
    t = v[:, 0] ^ (v[:, 0] >> U32(2))
    return (v[:, 4] ^ (v[:, 4] << U32(4))) ^ (t ^ (t << U32(1)))


@functools.lru_cache(maxsize=None)
def xorwow_states():
    """[n][6] (d, v0..v4) and the word each must give (-1: not chosen).  For a chosen word w, d is solved from
    w = v4' + d + 362437 with four different v."""
    words = np.repeat(np.array(XORWOW_WORDS, np.int64), 4)
    r = lcg64(6 * XORWOW_RANDOM + 5 * words.size, seed=12345)
    v = r[:5 * words.size].reshape(-1, 5)
    d = (words - xorwow_v4_after(v).astype(np.int64) - 362437) % (1 << 32)
    chosen = np.concatenate([d[:, None].astype(U32), v], axis=1)
    rand = r[5 * words.size:].reshape(-1, 6)
    want = np.concatenate([words, np.full(rand.shape[0], -1, np.int64)])
    return np.concatenate([chosen, rand]).astype(U32), want


SEEDS64 = [0, 1, 7, 1984, 0xFFFFFFFF, 1 << 32, (1 << 32) + 1, 0x9E3779B97F4A7C15, (1 << 63), (1 << 64) - 1]


@functools.lru_cache(maxsize=None)
def seeds():
    r = lcg64(2 * 4096, seed=99).astype(np.uint64)
    return np.concatenate([np.array(SEEDS64, np.uint64), (r[0::2] << np.uint64(32)) | r[1::2]])


# ------------------------------------------------------------------ rt_quant.h
@functools.lru_cache(maxsize=None)
def quant():
    parts = [around((k / 256.0) ** 2, 8) for k in range(1, 256)]
    parts += [around(float(np.float32(0.999)) ** 2, 8), around(1.0, 8), around(4.0, 8)]
    parts += [[0, SIGN, 1, 1 | SIGN, MAX_DENORMAL, MIN_NORMAL, bits(-1.0), bits(-1e-30), MAXF, MAXF | SIGN, INF, INF | SIGN], NANS]
    return _finish(parts)


# ------------------------------------------------------------------ rt_denoise_math.h
DN_N = [2, 3, 255, 256, 32767, 32768]


@functools.lru_cache(maxsize=None)
def dn_moments():
    """(s1, s2, n) of n samples c <= 255: m samples of a and n - m of b.  Holds s1 = s2 = 0, both maxima (all 255),
    D = 0 (all samples equal) and the largest D (half 0, half 255)."""
    rows = []
    r = lcg64(3 * 64, seed=5).astype(np.int64)
    for n in DN_N:
        combos = [(m, 255, 0) for m in (0, 1, n // 2, n - 1, n)] + [(n, c, 0) for c in (1, 127, 128, 254)]
        combos += [(1, 1, 0), (n - 1, 254, 255), (n // 3, 17, 200)]
        combos += [(int(r[3 * i] % (n + 1)), int(r[3 * i + 1] % 256), int(r[3 * i + 2] % 256)) for i in range(64)]
        for m, a, b in combos:
            rows.append((m * a + (n - m) * b, m * a * a + (n - m) * b * b, n))
    a = np.array(rows, np.int64)
    return a[:, 0].astype(U32), a[:, 1].astype(np.uint64), a[:, 2].astype(np.int32)


@functools.lru_cache(maxsize=None)
def dn_term_ops():
    """[n][7] float32 bits: Ma Va Mb Vb alpha kk eps.  The cross product holds den -> 0 (eps denormal, V = 0),
    kk = inf against V = 0 (NaN), d * d overflowing (M = 3e19); the constructed rows put t at and around +-64."""
    f = np.float32
    M = [0.0, 1 / 256, 100.25, 255.0, 65025.0, 3e19]
    V = [0.0, 1e-30, 0.5, 1e4, 3e38]
    grid = np.array(np.meshgrid(M, V, M, V, [0.0, 1.0, 1e30], [0.25, 1.0, np.inf], [1e-45, 1e-10, 1.0], indexing="ij"), np.float64)
    ops = [grid.reshape(7, -1).T.astype(f)]
    one = around(1.0, 8).astype(U32).view(f)
    z = np.zeros(one.size, f)
    ops.append(np.stack([z + f(8), z, z, z, z, z + f(1), one], axis=1))  # t = 64 / eps
    ops.append(np.stack([z, z + f(0.5), z, z + f(0.5), z + f(64), z + f(1e-30), one], axis=1))  # t = -64 / eps
    ops.append(np.stack([around(8.0, 8).astype(U32).view(f), z, z, z, z, z + f(1), z + f(1)], axis=1))  # t = Ma^2 / 64 * ...
    # moderate operands, where t is neither clamped nor 0: M = Q / 256, V up to 16, k up to 2
    u = (lcg64(7 << 14, seed=3).astype(np.float64) / 2.0 ** 32).reshape(-1, 7)
    k = (0.05 + 2 * u[:, 5]).astype(f)
    ops.append(np.stack([(np.floor(u[:, 0] * 65281) / 256).astype(f), (16 * u[:, 1] ** 4).astype(f), (np.floor(u[:, 2] * 65281) / 256).astype(f),
                         (16 * u[:, 3] ** 4).astype(f), np.floor(3 * u[:, 4]).astype(f), k * k, (10.0 ** (-10 * u[:, 6])).astype(f)], axis=1))
    return np.ascontiguousarray(np.concatenate(ops)).view(U32)


@functools.lru_cache(maxsize=None)
def dn_weight_ops():
    """(P, cnt, xf): for cnt = 1 .. 49 every P from -8 to 2048 cnt + 8, so both sides of every value at which
    s8 * 65536 crosses an integer, P = 2048 cnt (x = 8, s = 0) and beyond; then the far ends."""
    P, cnt = [], []
    for c in range(1, 50):
        p = np.concatenate([np.arange(-8, 2048 * c + 9), [-(1 << 31), -2048 * c, 4096 * c, (1 << 31) - 1]])
        P.append(p)
        cnt.append(np.full(p.size, c))
    P, cnt = np.concatenate(P).astype(np.int32), np.concatenate(cnt).astype(np.int32)
    xfs = np.array([0.0, 1e-3, 0.5, 3.999, 7.9999995, 8.0, 64.0, np.inf], np.float32)
    xf = xfs[(np.arange(P.size) // 3) % xfs.size]
    return P, cnt, np.ascontiguousarray(xf).view(U32)


@functools.lru_cache(maxsize=None)
def dn_features():
    """(p [n][7], q [n][7], gains [n][3]) float32 bits: hit / miss pairs (z = 0 is a miss), z_p + z_q = 0,
    a gain of inf against a zero and a non-zero distance, and random hits."""
    f = np.float32
    r = lcg64(17 * 4096, seed=77).astype(np.float64) / 2.0 ** 32
    u = r.reshape(-1, 17)
    p = np.concatenate([u[:, 0:3] * 2 - 1, u[:, 3:6], 0.1 + 100 * u[:, 6:7]], axis=1).astype(f)
    q = np.concatenate([u[:, 7:10] * 2 - 1, u[:, 10:13], 0.1 + 100 * u[:, 13:14]], axis=1).astype(f)
    g = (u[:, 14:17] * 8).astype(f)
    k = np.arange(p.shape[0])
    p[k % 8 == 1, 6] = 0  # p a miss
    q[k % 8 == 2, 6] = 0  # q a miss
    p[k % 8 == 3, 6] = 0
    q[k % 8 == 3, 6] = 0  # both
    q[k % 8 == 4, 6] = -p[k % 8 == 4, 6]  # z_p + z_q = 0
    g[k % 16 == 4, 2] = 0  # ... against a depth gain of 0: inf * 0
    g[k % 8 == 5, 0] = np.inf
    q[k % 16 == 5, 0:3] = p[k % 16 == 5, 0:3]  # inf * 0
    g[k % 8 == 6, :] = 0
    q[k % 8 == 7] = p[k % 8 == 7]  # the same pixel
    g[k % 16 == 7, 1] = np.inf
    return tuple(np.ascontiguousarray(a).view(U32) for a in (p, q, g))


@functools.lru_cache(maxsize=None)
def dn_spans():
    """[n][4] int32: p o f size with p and p + o inside [0, size)."""
    rows = [(p, o, f, size) for size in (1, 2, 7, 64) for p in range(size) for o in range(-10, 11) for f in range(4)
            if 0 <= p + o < size]
    return np.array(rows, np.int32)


@functools.lru_cache(maxsize=None)
def dn_linear_ops():
    """(Num, Den) uint64, Den > 0: small and large, exact and inexact in double."""
    den = [1, 2, 3, 65535, 65536, 65537, (1 << 24) + 1, (1 << 40) + 1, (1 << 53) + 1, (1 << 62) + 12345]
    rows = []
    for d in den:
        for num in (0, 1, d, 255 * d, 65025 * 256 * min(d, 1 << 38), d // 3, (1 << 53) + 1, (1 << 63) + 1025):
            rows.append((num % (1 << 64), d))
    r = lcg64(4 * 2048, seed=31).astype(np.uint64)
    num = ((r[0::4] << np.uint64(32)) | r[1::4]) >> (r[2::4] % np.uint64(40))
    dd = (((r[2::4] << np.uint64(32)) | r[3::4]) >> (r[1::4] % np.uint64(48))) | np.uint64(1)
    return (np.concatenate([np.array([n for n, _ in rows], np.uint64), num]),
            np.concatenate([np.array([d for _, d in rows], np.uint64), dd]))
