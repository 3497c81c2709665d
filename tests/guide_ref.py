"""The guided denoise's definition (include/rt_hip.h, "guided denoise") in numpy, written from the header's text
on top of tests/denoise_ref.py (prepare, term, the patch spans and the quantisation are imported from there), and
shared by tests/test_guide_cpu.py and tests/test_guide_gpu.py.  It does not call the library."""
import numpy as np

import denoise_ref as dr

F32 = np.float32


def feature_x(Np, Ap, Zp, Nq, Aq, Zq, gains):
    """xf of pairs of pixels: N, A [..., 3] float32, Z [...] float32; gains = (normal, albedo, depth)."""
    gn, ga, gz = (F32(g) for g in gains)
    with np.errstate(all="ignore"):
        dn, da = Np - Nq, Ap - Aq
        fn = dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1] + dn[..., 2] * dn[..., 2]
        fa = da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1] + da[..., 2] * da[..., 2]
        r = (Zp - Zq) / (Zp + Zq)
        fz = r * r
        xf = fn * gn + fa * ga + fz * gz
    xf = np.where(np.isnan(xf), F32(64.0), xf).astype(F32)
    mp, mq = Zp == 0, Zq == 0
    xf = np.where(mp & mq, F32(0.0), xf)
    return np.where(mp != mq, F32(64.0), xf).astype(F32)


def weight(P, cnt, xf):
    x = P.astype(F32) / (256 * cnt).astype(F32)
    x = np.where(x < 0, F32(0), x)
    x = np.where(xf > x, xf, x).astype(F32)  # fmaxf(x, xf): xf is never a NaN
    s = F32(1.0) - x * F32(0.125)
    s = np.where(s < 0, F32(0), s)
    s2 = s * s
    s4 = s2 * s2
    s8 = s4 * s4
    return (s8 * F32(65536.0)).astype(np.uint32).astype(np.uint64)


def denoise(S1, S2, n, rows, width, R, f, k, alpha, eps, normal, albedo, depth, gains):
    """denoise_ref.denoise with the feature planes normal, albedo [rows][width][3] and depth [rows][width]."""
    S1 = np.asarray(S1, np.uint64).reshape(rows, width, 3)
    S2 = np.asarray(S2, np.uint64).reshape(rows, width, 3)
    N, A = np.asarray(normal, F32).reshape(rows, width, 3), np.asarray(albedo, F32).reshape(rows, width, 3)
    Z = np.asarray(depth, F32).reshape(rows, width)
    Q, M, V = dr.prepare(S1, S2, n)
    k, alpha, eps = F32(k), F32(alpha), F32(eps)
    with np.errstate(all="ignore"):
        kk = k * k
    Num = np.zeros((rows, width, 3), np.uint64)
    Den = np.zeros((rows, width), np.uint64)
    for oy in range(-R, R + 1):
        for ox in range(-R, R + 1):
            if abs(oy) >= rows or abs(ox) >= width:
                continue
            ya, yb = max(0, -oy), rows - max(0, oy)
            xa, xb = max(0, -ox), width - max(0, ox)
            a, b = (slice(ya, yb), slice(xa, xb)), (slice(ya + oy, yb + oy), slice(xa + ox, xb + ox))
            T = np.zeros((rows + 2 * f, width + 2 * f), np.int64)
            T[f + ya:f + yb, f + xa:f + xb] = dr.term(M[a], V[a], M[b], V[b], alpha, kk, eps).sum(-1)
            P = np.zeros((rows, width), np.int64)
            for uy in range(2 * f + 1):
                for ux in range(2 * f + 1):
                    P += T[uy:uy + rows, ux:ux + width]
            cnt = 3 * dr._span(rows, oy, f)[:, None] * dr._span(width, ox, f)[None, :]
            if oy == 0 and ox == 0:
                W = dr.weight(P[a], cnt[a])
                assert (W == 65536).all()
            else:
                W = weight(P[a], cnt[a], feature_x(N[a], A[a], Z[a], N[b], A[b], Z[b], gains))
            Num[a] += W[:, :, None] * Q[b]
            Den[a] += W
    lin = (Num.astype(np.float64) / (Den.astype(np.float64)[:, :, None] * 256.0 * 65025.0)).astype(F32)
    gain = (Den.astype(np.float64) / 65536.0).astype(F32)
    return dr.quant(lin), gain
