"""A plain numpy float64 restatement of rmd_denoise_atrous_dual (include/raymond_hip.h states the definition), in two readings.

atrous_dual / filtered_halves: vectorised over the pixels, looping over the levels and over the 25 taps in raster order (j ascending, then i
ascending).  Per tap the two colour weights — w_B from (c_B, v_B), w_A from (c_A, v_A) — and ONE feature weight, which cuts both; half A's sums
take w_B, half B's take w_A.  Every sum is made in the order the definition gives, so it differs from the kernel only by the device's exp.
atrous_dual_by_pixel: the same definition read pixel by pixel with Python floats, sharing only u, v, f, g and the masks with the first; the two
agree bit for bit (tests/test_denoise_atrous_dual_host.py).
"""
import numpy as np

from denoise_atrous_ref import H5, _exp, _fmin
from denoise_dual_guided_ref import feature_planes
from denoise_dual_ref import combine
from denoise_guided_ref import CHANNELS
from denoise_ref import EPS, mean_and_variance


def _inputs(S_a, Q_a, S_b, Q_b, n_a, n_b, F, G, n_f, k_f, tau):
    S_a, Q_a, S_b, Q_b = (np.asarray(x, dtype=np.float64) for x in (S_a, Q_a, S_b, Q_b))
    n_a, n_b = np.asarray(n_a), np.asarray(n_b)
    u_a, v_a, ok_a = mean_and_variance(S_a, Q_a, n_a)
    u_b, v_b, ok_b = mean_and_variance(S_b, Q_b, n_b)
    dual = ok_a & ok_b
    guide = feature_planes(F, G, n_f, dual, k_f, tau) if F is not None else None
    return S_a, S_b, n_a, n_b, u_a, v_a, u_b, v_b, dual, guide


def _colour_weight(c, var, cq, vq, k2, alpha):
    D = None
    for ch in range(3):
        du = c[..., ch] - cq[..., ch]
        term = (du * du - alpha * (var[..., ch] + np.minimum(var[..., ch], vq[..., ch]))) / (EPS + k2 * (var[..., ch] + vq[..., ch]))
        D = term if D is None else D + term
    D = D / 3.0
    return np.exp(-np.where(D > 0.0, D, 0.0))


def filtered_halves_all(S_a, Q_a, S_b, Q_b, n_a, n_b, levels, k=3.0, alpha=1.0, F=None, G=None, n_f=None, k_f=1.0, tau=1e-2):
    """{count: (f_A, f_B)} after each of the level counts in `levels`, from one run to the largest of them (values at pixels that are not dual-valid
    are unspecified), and the dual-validity mask."""
    S_a, S_b, n_a, n_b, u_a, v_a, u_b, v_b, dual, guide = _inputs(S_a, Q_a, S_b, Q_b, n_a, n_b, F, G, n_f, k_f, tau)
    wanted = {int(l) for l in levels}
    halves = {0: (u_a, u_b)} if 0 in wanted else {}
    H, W = dual.shape
    k2, alpha = float(k) * float(k), float(alpha)
    state = [u_a.copy(), v_a.copy(), u_b.copy(), v_b.copy()]
    py, px = np.arange(H)[:, None], np.arange(W)[None, :]
    with np.errstate(all="ignore"):
        for level in range(max(wanted)):
            s = 1 << level
            ca, va, cb, vb = state
            acc = [np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W))]
            for j in range(-2, 3):
                for i in range(-2, 3):
                    qy, qx = py + s * j, px + s * i
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    take = dual & inside & dual[qyc, qxc]
                    if not take.any():
                        continue
                    caq, vaq, cbq, vbq = ca[qyc, qxc], va[qyc, qxc], cb[qyc, qxc], vb[qyc, qxc]
                    w_a = _colour_weight(ca, va, caq, vaq, k2, alpha)
                    w_b = _colour_weight(cb, vb, cbq, vbq, k2, alpha)
                    if guide is not None:
                        ff, gg, den, fvalid = guide
                        fq, gq = ff[qyc, qxc], gg[qyc, qxc]
                        Df = np.zeros((H, W))
                        for ch in range(CHANNELS):
                            df = ff[..., ch] - fq[..., ch]
                            phi = (df * df - (gg[..., ch] + np.minimum(gg[..., ch], gq[..., ch]))) / den[..., ch]
                            Df = np.where(phi > Df, phi, Df)  # a NaN phi is skipped by the comparison
                        wf = np.exp(-Df)  # once, for both passes
                        both = fvalid & fvalid[qyc, qxc]
                        w_a = np.where(both & (wf < w_a), wf, w_a)
                        w_b = np.where(both & (wf < w_b), wf, w_b)
                    h = H5[i + 2] * H5[j + 2]
                    for w, cq, vq, o in ((w_b, caq, vaq, 0), (w_a, cbq, vbq, 3)):  # half A under w_B, half B under w_A
                        hw = h * w
                        acc[o] = np.where(take[..., None], acc[o] + hw[..., None] * cq, acc[o])
                        acc[o + 1] = np.where(take[..., None], acc[o + 1] + (hw * hw)[..., None] * vq, acc[o + 1])
                        acc[o + 2] = np.where(take, acc[o + 2] + hw, acc[o + 2])
            state = [acc[0] / acc[2][..., None], acc[1] / (acc[2] * acc[2])[..., None], acc[3] / acc[5][..., None], acc[4] / (acc[5] * acc[5])[..., None]]
            if level + 1 in wanted:
                halves[level + 1] = (state[0], state[2])
    return halves, dual


def filtered_halves(S_a, Q_a, S_b, Q_b, n_a, n_b, levels=5, k=3.0, alpha=1.0, F=None, G=None, n_f=None, k_f=1.0, tau=1e-2):
    """f_A, f_B and the dual-validity mask."""
    halves, dual = filtered_halves_all(S_a, Q_a, S_b, Q_b, n_a, n_b, [levels], k, alpha, F, G, n_f, k_f, tau)
    return (*halves[int(levels)], dual)


def atrous_dual(S_a, Q_a, S_b, Q_b, n_a, n_b, levels=5, k=3.0, alpha=1.0, F=None, G=None, n_f=None, k_f=1.0, tau=1e-2):
    """The two halves' (H, W, 3) sums and sums of squares and (H, W) counts; F, G: (H, W, 7) feature sums and sums of squares at the (H, W) counts
    n_f, or all None -> (out (H, W, 3), err (H, W))."""
    f_a, f_b, dual = filtered_halves(S_a, Q_a, S_b, Q_b, n_a, n_b, levels, k, alpha, F, G, n_f, k_f, tau)
    return combine(f_a, f_b, np.asarray(S_a, dtype=np.float64), np.asarray(S_b, dtype=np.float64), np.asarray(n_a), np.asarray(n_b), dual)


def atrous_dual_by_pixel(S_a, Q_a, S_b, Q_b, n_a, n_b, levels=5, k=3.0, alpha=1.0, F=None, G=None, n_f=None, k_f=1.0, tau=1e-2):
    """The second reading: every dual-valid pixel's taps one after another, in Python floats."""
    S_a, S_b, n_a, n_b, u_a, v_a, u_b, v_b, dual, guide = _inputs(S_a, Q_a, S_b, Q_b, n_a, n_b, F, G, n_f, k_f, tau)
    H, W = dual.shape
    k2, alpha = float(k) * float(k), float(alpha)
    c, var = [u_a.copy(), u_b.copy()], [v_a.copy(), v_b.copy()]  # index 0: half A, 1: half B
    old = np.seterr(all="ignore")
    try:
        for level in range(int(levels)):
            s = 1 << level
            nc, nv = [c[0].copy(), c[1].copy()], [var[0].copy(), var[1].copy()]
            for y in range(H):
                for x in range(W):
                    if not dual[y, x]:
                        continue
                    A, B, Ws = [[0.0] * 3, [0.0] * 3], [[0.0] * 3, [0.0] * 3], [0.0, 0.0]
                    for j in range(-2, 3):
                        for i in range(-2, 3):
                            qy, qx = y + s * j, x + s * i
                            if not (0 <= qy < H and 0 <= qx < W) or not dual[qy, qx]:
                                continue
                            w = [0.0, 0.0]  # the colour weight made from half 0 (w_A) and from half 1 (w_B)
                            for h in range(2):
                                D = None
                                for ch in range(3):
                                    a, b = np.float64(c[h][y, x, ch]), np.float64(c[h][qy, qx, ch])
                                    va, vb = np.float64(var[h][y, x, ch]), np.float64(var[h][qy, qx, ch])
                                    du = a - b
                                    term = (du * du - alpha * (va + _fmin(va, vb))) / (EPS + k2 * (va + vb))
                                    D = term if D is None else D + term
                                D = D / 3.0
                                w[h] = _exp(-(float(D) if D > 0.0 else 0.0))
                            if guide is not None and guide[3][y, x] and guide[3][qy, qx]:
                                ff, gg, den, _ = guide
                                Df = 0.0
                                for ch in range(CHANNELS):
                                    df = ff[y, x, ch] - ff[qy, qx, ch]
                                    phi = (df * df - (gg[y, x, ch] + _fmin(gg[y, x, ch], gg[qy, qx, ch]))) / den[y, x, ch]
                                    if phi > Df:
                                        Df = float(phi)
                                wf = _exp(-Df)
                                w = [wf if wf < w[0] else w[0], wf if wf < w[1] else w[1]]
                            for h in range(2):  # half h takes the OTHER half's weight
                                hw = (H5[i + 2] * H5[j + 2]) * w[1 - h]
                                for ch in range(3):
                                    A[h][ch] = A[h][ch] + hw * float(c[h][qy, qx, ch])
                                    B[h][ch] = B[h][ch] + (hw * hw) * float(var[h][qy, qx, ch])
                                Ws[h] = Ws[h] + hw
                    for h in range(2):
                        for ch in range(3):
                            nc[h][y, x, ch] = np.float64(A[h][ch]) / np.float64(Ws[h])
                            nv[h][y, x, ch] = np.float64(B[h][ch]) / np.float64(Ws[h] * Ws[h])
            c, var = nc, nv
    finally:
        np.seterr(**old)
    return combine(c[0], c[1], S_a, S_b, n_a, n_b, dual)
