"""A plain numpy float64 restatement of rmd_denoise_dual_guided (include/raymond_hip.h states the definition).

`cross_filter` is denoise_dual_ref.cross_filter — the same patch sums in the same order — with denoise_guided_ref's feature weight applied where the
neighbour's weight is made: for a pair of feature-valid pixels D_f = max(0, max_j Phi_j) over j = 0..6 in order, w_f = exp(-D_f), and w = w_f where
w_f < w.  `denoise_dual_guided` runs it both ways with the same w_f and combines with denoise_dual_ref.combine.  The features carry their own
per-pixel count n_f.  `denoise_dual_guided_naive` reads the definition pixel by pixel with Python loops, for small frames: the vectorised form is
held to it.  The two differ from the kernel only by the device's exp.
"""
import numpy as np

import denoise_dual_ref
from denoise_guided_ref import CHANNELS
from denoise_ref import EPS, mean_and_variance


def feature_planes(F, G, n_f, dual, k_f, tau):
    """f, g, the denominators of Phi_j(p, .) and the feature-validity mask (dual-valid, n_f >= 2, all fourteen sums finite)."""
    F, G = np.asarray(F, dtype=np.float64), np.asarray(G, dtype=np.float64)
    nd = np.asarray(n_f).astype(np.float64)[..., None]
    kf2 = float(k_f) * float(k_f)
    with np.errstate(all="ignore"):
        ff = F / nd
        t = (G - F * ff) / (nd - 1.0)
        t = np.where(t < 0.0, 0.0, t)
        gg = t / nd
        s = np.ones_like(ff)
        s[..., CHANNELS - 1] = ff[..., CHANNELS - 1] * ff[..., CHANNELS - 1]
        a = float(tau) * s
        den = EPS + kf2 * np.where(a > gg, a, gg)
    fvalid = dual & (np.asarray(n_f) >= 2) & np.isfinite(F).all(axis=-1) & np.isfinite(G).all(axis=-1)
    return ff, gg, den, fvalid


def cross_filter(u_w, v_w, u_v, valid, radius, patch_radius, k, alpha, guide=None):
    """denoise_dual_ref.cross_filter; guide = (ff, gg, den, fvalid) adds the feature weight, None leaves it out (then the same operations as there)."""
    H, W = valid.shape
    r, f = int(radius), int(patch_radius)
    k2 = float(k) * float(k)
    alpha = float(alpha)
    ys, xs = np.arange(-f, H + f), np.arange(-f, W + f)
    ya, xa = np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)
    ua, va, oka = u_w[ya][:, xa], v_w[ya][:, xa], valid[ya][:, xa]
    acc = np.full((H, W, 3), -0.0)
    wsum = np.full((H, W), -0.0)
    py, px = np.arange(H)[:, None], np.arange(W)[None, :]
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            yb = np.clip(ys + dy, 0, H - 1)
            for dx in range(-r, r + 1):
                xb = np.clip(xs + dx, 0, W - 1)
                ub, vb, okb = u_w[yb][:, xb], v_w[yb][:, xb], valid[yb][:, xb]
                t = None
                for c in range(3):
                    du = ua[..., c] - ub[..., c]
                    term = (du * du - alpha * (va[..., c] + np.minimum(va[..., c], vb[..., c]))) / (EPS + k2 * (va[..., c] + vb[..., c]))
                    t = term if t is None else t + term
                taken = oka & okb
                T = np.where(taken, t, 0.0)
                Tc = taken.astype(np.int64)
                rows, crows = T[:, 0:W].copy(), Tc[:, 0:W].copy()
                for o in range(1, 2 * f + 1):
                    rows = rows + T[:, o : o + W]
                    crows = crows + Tc[:, o : o + W]
                ds, cnt = rows[0:H].copy(), crows[0:H].copy()
                for o in range(1, 2 * f + 1):
                    ds = ds + rows[o : o + H]
                    cnt = cnt + crows[o : o + H]
                D = ds / (3.0 * cnt.astype(np.float64))
                w = np.exp(-np.where(D > 0.0, D, 0.0))
                qy, qx = py + dy, px + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                use = valid & inside & valid[qyc, qxc]
                if guide is not None:
                    ff, gg, den, fvalid = guide
                    fq, gq = ff[qyc, qxc], gg[qyc, qxc]
                    Df = np.zeros((H, W))
                    for j in range(CHANNELS):
                        df = ff[..., j] - fq[..., j]
                        phi = (df * df - (gg[..., j] + np.minimum(gg[..., j], gq[..., j]))) / den[..., j]
                        Df = np.where(phi > Df, phi, Df)  # a NaN phi is skipped by the comparison
                    wf = np.exp(-Df)
                    both = fvalid & fvalid[qyc, qxc]
                    w = np.where(both & (wf < w), wf, w)
                acc = np.where(use[..., None], acc + w[..., None] * u_v[qyc, qxc], acc)
                wsum = np.where(use, wsum + w, wsum)
        return acc / wsum[..., None]


def filtered_halves(S_a, Q_a, S_b, Q_b, n_a, n_b, F=None, G=None, n_f=None, radius=10, patch_radius=3, k=0.45, alpha=1.0, k_f=1.0, tau=1e-2):
    """-> f_A, f_B, dual: the two cross-filtered halves before they are combined."""
    S_a, Q_a, S_b, Q_b = (np.asarray(x, dtype=np.float64) for x in (S_a, Q_a, S_b, Q_b))
    n_a, n_b = np.asarray(n_a), np.asarray(n_b)
    u_a, v_a, ok_a = mean_and_variance(S_a, Q_a, n_a)
    u_b, v_b, ok_b = mean_and_variance(S_b, Q_b, n_b)
    dual = ok_a & ok_b
    guide = None if F is None else feature_planes(F, G, n_f, dual, k_f, tau)
    f_a = cross_filter(u_b, v_b, u_a, dual, radius, patch_radius, k, alpha, guide)
    f_b = cross_filter(u_a, v_a, u_b, dual, radius, patch_radius, k, alpha, guide)
    return f_a, f_b, dual


def denoise_dual_guided(S_a, Q_a, S_b, Q_b, n_a, n_b, F=None, G=None, n_f=None, **params):
    """The two halves' (H, W, 3) sums and sums of squares and (H, W) counts, the (H, W, 7) feature sums and sums of squares with their own (H, W)
    counts n_f (F = G = None: exactly denoise_dual_ref.denoise_dual) -> (out (H, W, 3), err (H, W))."""
    f_a, f_b, dual = filtered_halves(S_a, Q_a, S_b, Q_b, n_a, n_b, F, G, n_f, **params)
    return denoise_dual_ref.combine(f_a, f_b, np.asarray(S_a, dtype=np.float64), np.asarray(S_b, dtype=np.float64), np.asarray(n_a), np.asarray(n_b), dual)


def denoise_dual_guided_naive(S_a, Q_a, S_b, Q_b, n_a, n_b, F, G, n_f, radius, patch_radius, k, alpha, k_f, tau):
    """The definition read pixel by pixel (slow: small frames only)."""
    u_a, v_a, ok_a = mean_and_variance(S_a, Q_a, n_a)
    u_b, v_b, ok_b = mean_and_variance(S_b, Q_b, n_b)
    dual = ok_a & ok_b
    H, W = dual.shape
    k2, kf2 = float(k) * float(k), float(k_f) * float(k_f)
    f_a, f_b = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    with np.errstate(all="ignore"):
        nf = np.asarray(n_f).astype(np.float64)

        def feat(y, x):
            n = nf[y, x]
            fs, gs = [], []
            for j in range(CHANNELS):
                fs.append(F[y, x, j] / n)
                t = (G[y, x, j] - F[y, x, j] * fs[j]) / (n - 1.0)
                if t < 0.0:
                    t = 0.0
                gs.append(t / n)
            ok = bool(dual[y, x]) and n_f[y, x] >= 2 and all(np.isfinite(F[y, x, j]) and np.isfinite(G[y, x, j]) for j in range(CHANNELS))
            return fs, gs, ok

        def w_f(p, q):
            fp, gp, okp = feat(*p)
            fq, gq, okq = feat(*q)
            if not (okp and okq):
                return None
            Df = 0.0
            for j in range(CHANNELS):
                s = 1.0 if j < CHANNELS - 1 else fp[j] * fp[j]
                a = float(tau) * s
                den = EPS + kf2 * (a if a > gp[j] else gp[j])
                df = fp[j] - fq[j]
                phi = (df * df - (gp[j] + min(gp[j], gq[j]))) / den
                if phi > Df:
                    Df = phi
            return np.exp(-Df)

        for y in range(H):
            for x in range(W):
                if not dual[y, x]:
                    continue
                for (uw, vw, uv, dst) in ((u_b, v_b, u_a, f_a), (u_a, v_a, u_b, f_b)):
                    acc, wsum = np.full(3, -0.0), -0.0
                    for dy in range(-radius, radius + 1):
                        for dx in range(-radius, radius + 1):
                            qy, qx = y + dy, x + dx
                            if 0 <= qy < H and 0 <= qx < W and dual[qy, qx]:
                                w = denoise_dual_ref._naive_weight(uw, vw, dual, (y, x), (qy, qx), patch_radius, k2, float(alpha))
                                wf = w_f((y, x), (qy, qx))
                                if wf is not None and wf < w:
                                    w = wf
                                acc = acc + w * uv[qy, qx]
                                wsum = wsum + w
                    dst[y, x] = acc / wsum
    return denoise_dual_ref.combine(f_a, f_b, S_a, S_b, n_a, n_b, dual)
