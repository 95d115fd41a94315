"""A plain numpy float64 restatement of rmd_denoise_atrous (include/raymond_hip.h states the definition), in two readings.

atrous / atrous_all: vectorised over the pixels, looping over the levels and over the 25 taps in raster order (j ascending, then i ascending);
every sum is made in the order the definition gives, so it differs from the kernel only by the device's exp.
atrous_by_pixel: the same definition read pixel by pixel with Python floats, sharing only u, v, f, g and the validity masks with the first; the
two agree bit for bit (tests/test_denoise_atrous_host.py).
"""
import numpy as np

from denoise_guided_ref import CHANNELS, feature_mean_and_variance
from denoise_ref import EPS, mean_and_variance

H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
MAX_LEVELS = 8


def _inputs(S, Q, F, G, n, k_f, tau):
    S = np.asarray(S, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    n = np.asarray(n)
    u, v, valid = mean_and_variance(S, Q, n)
    ff = gg = fvalid = den = None
    if F is not None:
        F = np.asarray(F, dtype=np.float64)
        G = np.asarray(G, dtype=np.float64)
        kf2 = float(k_f) * float(k_f)
        ff, gg, fvalid = feature_mean_and_variance(F, G, n, valid)
        with np.errstate(all="ignore"):
            s = np.ones_like(ff)
            s[..., CHANNELS - 1] = ff[..., CHANNELS - 1] * ff[..., CHANNELS - 1]
            a = float(tau) * s
            den = EPS + kf2 * np.where(a > gg, a, gg)
    with np.errstate(all="ignore"):
        raw = S / n.astype(np.float64)[..., None]
    return u, v, valid, ff, gg, fvalid, den, raw


def atrous_all(S, Q, n, levels, k=3.0, alpha=1.0, F=None, G=None, k_f=1.0, tau=1e-2):
    """The frames after each of the level counts in `levels`, from one run to the largest of them: {count: (H, W, 3) filtered means}."""
    u, v, valid, ff, gg, fvalid, den, raw = _inputs(S, Q, F, G, n, k_f, tau)
    H, W = valid.shape
    k2, alpha = float(k) * float(k), float(alpha)
    c, var = u.copy(), v.copy()
    py, px = np.arange(H)[:, None], np.arange(W)[None, :]
    wanted = {int(l) for l in levels}
    out = {}
    if 0 in wanted:
        out[0] = np.where(valid[..., None], c, raw)
    with np.errstate(all="ignore"):
        for level in range(max(wanted)):
            s = 1 << level
            A, B, Ws = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W))
            for j in range(-2, 3):
                for i in range(-2, 3):
                    qy, qx = py + s * j, px + s * i
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    take = valid & inside & valid[qyc, qxc]
                    if not take.any():
                        continue
                    cq, vq = c[qyc, qxc], var[qyc, qxc]
                    D = None
                    for ch in range(3):
                        du = c[..., ch] - cq[..., ch]
                        term = (du * du - alpha * (var[..., ch] + np.minimum(var[..., ch], vq[..., ch]))) / (EPS + k2 * (var[..., ch] + vq[..., ch]))
                        D = term if D is None else D + term
                    D = D / 3.0
                    w = np.exp(-np.where(D > 0.0, D, 0.0))
                    if ff is not None:
                        fq, gq = ff[qyc, qxc], gg[qyc, qxc]
                        Df = np.zeros((H, W))
                        for ch in range(CHANNELS):
                            df = ff[..., ch] - fq[..., ch]
                            phi = (df * df - (gg[..., ch] + np.minimum(gg[..., ch], gq[..., ch]))) / den[..., ch]
                            Df = np.where(phi > Df, phi, Df)  # a NaN phi is skipped by the comparison
                        wf = np.exp(-Df)
                        w = np.where(fvalid & fvalid[qyc, qxc] & (wf < w), wf, w)
                    hw = (H5[i + 2] * H5[j + 2]) * w
                    A = np.where(take[..., None], A + hw[..., None] * cq, A)
                    B = np.where(take[..., None], B + (hw * hw)[..., None] * vq, B)
                    Ws = np.where(take, Ws + hw, Ws)
            c, var = A / Ws[..., None], B / (Ws * Ws)[..., None]
            if level + 1 in wanted:
                out[level + 1] = np.where(valid[..., None], c, raw)
    return out


def atrous(S, Q, n, levels=5, k=3.0, alpha=1.0, F=None, G=None, k_f=1.0, tau=1e-2):
    """S, Q: (H, W, 3) sums and sums of squares; n: (H, W) sample counts; F, G: (H, W, 7) feature sums and sums of squares, or both None (the
    colour weight alone).  Returns the (H, W, 3) filtered means."""
    return atrous_all(S, Q, n, [levels], k=k, alpha=alpha, F=F, G=G, k_f=k_f, tau=tau)[int(levels)]


def _fmin(a, b):
    """fmin as the kernel's and numpy's minimum agree on wherever the result is used: a NaN operand gives a NaN term either way."""
    return float(np.minimum(a, b))


def _exp(x):
    """numpy's exp of one value, through the array loop the first reading's values take (a scalar may take another routine)."""
    return float(np.exp(np.array([x, x, x, x, x, x, x, x], dtype=np.float64))[0])


def atrous_by_pixel(S, Q, n, levels=5, k=3.0, alpha=1.0, F=None, G=None, k_f=1.0, tau=1e-2):
    """The second reading: every valid pixel's taps one after another, in Python floats."""
    u, v, valid, ff, gg, fvalid, den, raw = _inputs(S, Q, F, G, n, k_f, tau)
    H, W = valid.shape
    k2, alpha = float(k) * float(k), float(alpha)
    c, var = u.copy(), v.copy()
    old = np.seterr(all="ignore")
    try:
        for level in range(int(levels)):
            s = 1 << level
            nc, nv = c.copy(), var.copy()
            for y in range(H):
                for x in range(W):
                    if not valid[y, x]:
                        continue
                    A, B, Ws = [0.0] * 3, [0.0] * 3, 0.0
                    for j in range(-2, 3):
                        for i in range(-2, 3):
                            qy, qx = y + s * j, x + s * i
                            if not (0 <= qy < H and 0 <= qx < W) or not valid[qy, qx]:
                                continue
                            D = None
                            for ch in range(3):
                                a, b, va, vb = np.float64(c[y, x, ch]), np.float64(c[qy, qx, ch]), np.float64(var[y, x, ch]), np.float64(var[qy, qx, ch])
                                du = a - b
                                term = (du * du - alpha * (va + _fmin(va, vb))) / (EPS + k2 * (va + vb))
                                D = term if D is None else D + term
                            D = D / 3.0
                            w = _exp(-(float(D) if D > 0.0 else 0.0))
                            if ff is not None and fvalid[y, x] and fvalid[qy, qx]:
                                Df = 0.0
                                for ch in range(CHANNELS):
                                    df = ff[y, x, ch] - ff[qy, qx, ch]
                                    phi = (df * df - (gg[y, x, ch] + _fmin(gg[y, x, ch], gg[qy, qx, ch]))) / den[y, x, ch]
                                    if phi > Df:
                                        Df = float(phi)
                                wf = _exp(-Df)
                                if wf < w:
                                    w = wf
                            hw = (H5[i + 2] * H5[j + 2]) * w
                            for ch in range(3):
                                A[ch] = A[ch] + hw * float(c[qy, qx, ch])
                                B[ch] = B[ch] + (hw * hw) * float(var[qy, qx, ch])
                            Ws = Ws + hw
                    for ch in range(3):
                        nc[y, x, ch] = np.float64(A[ch]) / np.float64(Ws)
                        nv[y, x, ch] = np.float64(B[ch]) / np.float64(Ws * Ws)
            c, var = nc, nv
    finally:
        np.seterr(**old)
    return np.where(valid[..., None], c, raw)
