"""The denoiser's definition (include/rt_hip.h, "denoiser") in numpy, written from the header's text and
shared by tests/test_denoise_cpu.py and tests/test_denoise_gpu.py.  It does not call the library: float32
array operations for a term and a weight (numpy rounds each once, as the header asks), uint64 / int64 for every
sum, one search offset at a time with the patch sums as 49 shifted adds."""
import numpy as np

F32 = np.float32


def prepare(S1, S2, n):
    """(Q uint64, M float32, V float32) of moments [rows][width][3] (uint64); n: an int, or [rows][width]."""
    S1 = np.asarray(S1, np.uint64)
    S2 = np.asarray(S2, np.uint64)
    n = np.asarray(n, np.uint64)
    if n.ndim == 0:
        n = np.full(S1.shape[:2], n, np.uint64)
    assert int(n.min()) >= 2
    n = n[:, :, None]
    Q = (np.uint64(256) * S1 + n // np.uint64(2)) // n
    assert int(Q.max()) < 2 ** 24
    M = Q.astype(F32) / F32(256.0)
    D = n * S2 - S1 * S1
    nd = n.astype(np.float64)
    V = (D.astype(np.float64) / (nd * nd * (nd - 1.0))).astype(F32)
    return Q, M, V


def term(Ma, Va, Mb, Vb, alpha, kk, eps):
    """T of pairs of values, int64 arrays; every operand float32."""
    with np.errstate(all="ignore"):
        d = Ma - Mb
        num = d * d - alpha * (Va + np.minimum(Va, Vb))
        den = eps + kk * (Va + Vb)
        t = num / den
        t = np.where(t > F32(-64.0), t, F32(-64.0))  # a NaN counts as -64
        t = np.where(t > F32(64.0), F32(64.0), t)
        return (t * F32(256.0)).astype(np.int32).astype(np.int64)  # truncating cast


def weight(P, cnt):
    x = P.astype(F32) / (256 * cnt).astype(F32)
    x = np.where(x < 0, F32(0), x)
    s = F32(1.0) - x * F32(0.125)
    s = np.where(s < 0, F32(0), s)
    s2 = s * s
    s4 = s2 * s2
    s8 = s4 * s4
    return (s8 * F32(65536.0)).astype(np.uint32).astype(np.uint64)


def quant(lin):
    """write_frame_buffer's quantisation of float32 values (never NaN here)."""
    r = np.sqrt(np.asarray(lin, F32))
    c = np.minimum(np.maximum(r, F32(0.0)), F32(0.999))
    return (F32(256.0) * c).astype(np.int32).astype(np.uint8)


def _span(size, o, f):
    """[size] int64: the patch offsets u, |u| <= f, with p + u and p + o + u inside [0, size)."""
    p = np.arange(size)[:, None]
    u = np.arange(-f, f + 1)[None, :]
    return (((p + u >= 0) & (p + u < size) & (p + o + u >= 0) & (p + o + u < size)).sum(1)).astype(np.int64)


def denoise(S1, S2, n, rows, width, R, f, k, alpha, eps):
    """(image uint8 [rows][width][3], gain float32 [rows][width]) of moments (uint64, rows*width*3 values, rows
    ascending) after n frame buffers (an int, or [rows][width] ints)."""
    S1 = np.asarray(S1, np.uint64).reshape(rows, width, 3)
    S2 = np.asarray(S2, np.uint64).reshape(rows, width, 3)
    Q, M, V = prepare(S1, S2, n)
    k, alpha, eps = F32(k), F32(alpha), F32(eps)
    with np.errstate(all="ignore"):
        kk = k * k
    Num = np.zeros((rows, width, 3), np.uint64)
    Den = np.zeros((rows, width), np.uint64)
    for oy in range(-R, R + 1):
        for ox in range(-R, R + 1):
            if abs(oy) >= rows or abs(ox) >= width:
                continue
            ya, yb = max(0, -oy), rows - max(0, oy)  # the pixels a with a + o inside
            xa, xb = max(0, -ox), width - max(0, ox)
            T = np.zeros((rows + 2 * f, width + 2 * f), np.int64)  # zero border: patch pixels outside the image
            T[f + ya:f + yb, f + xa:f + xb] = term(M[ya:yb, xa:xb], V[ya:yb, xa:xb], M[ya + oy:yb + oy, xa + ox:xb + ox],
                                                   V[ya + oy:yb + oy, xa + ox:xb + ox], alpha, kk, eps).sum(-1)
            P = np.zeros((rows, width), np.int64)
            for uy in range(2 * f + 1):
                for ux in range(2 * f + 1):
                    P += T[uy:uy + rows, ux:ux + width]
            cnt = 3 * _span(rows, oy, f)[:, None] * _span(width, ox, f)[None, :]
            assert int(np.abs(P).max()) <= 147 * 16384
            W = weight(P[ya:yb, xa:xb], cnt[ya:yb, xa:xb])  # the pixels p with q = p + o inside
            if oy == 0 and ox == 0:
                assert (W == 65536).all()
            Num[ya:yb, xa:xb] += W[:, :, None] * Q[ya + oy:yb + oy, xa + ox:xb + ox]
            Den[ya:yb, xa:xb] += W
    assert int(Num.max()) < 2 ** 49 and int(Den.min()) >= 65536
    lin = (Num.astype(np.float64) / (Den.astype(np.float64)[:, :, None] * 256.0 * 65025.0)).astype(F32)
    gain = (Den.astype(np.float64) / 65536.0).astype(F32)
    return quant(lin), gain


def window_pixels(rows, width, R):
    """[rows][width] float32: the pixels of the search window of every pixel that lie inside the image."""
    cy = np.array([min(rows - 1, y + R) - max(0, y - R) + 1 for y in range(rows)])
    cx = np.array([min(width - 1, x + R) - max(0, x - R) + 1 for x in range(width)])
    return (cy[:, None] * cx[None, :]).astype(F32)
