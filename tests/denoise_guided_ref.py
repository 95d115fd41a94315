"""A plain numpy float64 restatement of rmd_denoise_guided (include/raymond_hip.h states the definition).

denoise_ref.denoise with the feature weight added where the neighbour's weight is made: the colour distance D(p, q) is summed in the order
denoise_ref sums it (the kernel's), w_c = exp(-max(0, D)), then for a pair of feature-valid pixels D_f = max(0, max_j Phi_j) over j = 0..6 in
order, w_f = exp(-D_f), and w = w_f where w_f < w_c.  The two differ from the kernel only by the device's exp.
"""
import numpy as np

from denoise_ref import EPS, mean_and_variance

CHANNELS = 7


def feature_mean_and_variance(F, G, n, valid):
    """f = F / n, g = max(0, (G - F*f) / (n - 1)) / n, and the feature-validity mask (valid and all fourteen values finite)."""
    nd = n.astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        f = F / nd
        t = (G - F * f) / (nd - 1.0)
        t = np.where(t < 0.0, 0.0, t)
        g = t / nd
    fvalid = valid & np.isfinite(F).all(axis=-1) & np.isfinite(G).all(axis=-1)
    return f, g, fvalid


def denoise_guided(S, Q, F, G, n, radius=10, patch_radius=3, k=0.45, alpha=1.0, k_f=0.6, tau=1e-3):
    """S, Q: (H, W, 3) sums and sums of squares; F, G: (H, W, 7) feature sums and sums of squares, or both None (then exactly
    denoise_ref.denoise); n: (H, W) sample counts.  Returns the (H, W, 3) denoised means."""
    S = np.asarray(S, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    n = np.asarray(n)
    H, W = n.shape
    r, f = int(radius), int(patch_radius)
    k2 = float(k) * float(k)
    alpha = float(alpha)
    u, v, valid = mean_and_variance(S, Q, n)
    guided = F is not None
    if guided:
        F = np.asarray(F, dtype=np.float64)
        G = np.asarray(G, dtype=np.float64)
        kf2 = float(k_f) * float(k_f)
        ff, gg, fvalid = feature_mean_and_variance(F, G, n, valid)
        with np.errstate(all="ignore"):
            s = np.ones_like(ff)
            s[..., CHANNELS - 1] = ff[..., CHANNELS - 1] * ff[..., CHANNELS - 1]
            a = float(tau) * s
            den = EPS + kf2 * np.where(a > gg, a, gg)
    ys, xs = np.arange(-f, H + f), np.arange(-f, W + f)
    ya, xa = np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)
    ua, va, oka = u[ya][:, xa], v[ya][:, xa], valid[ya][:, xa]
    acc = np.full((H, W, 3), -0.0)
    wsum = np.full((H, W), -0.0)
    py, px = np.arange(H)[:, None], np.arange(W)[None, :]
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            yb = np.clip(ys + dy, 0, H - 1)
            for dx in range(-r, r + 1):
                xb = np.clip(xs + dx, 0, W - 1)
                ub, vb, okb = u[yb][:, xb], v[yb][:, xb], valid[yb][:, xb]
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
                if guided:
                    fq, gq = ff[qyc, qxc], gg[qyc, qxc]
                    Df = np.zeros((H, W))
                    for j in range(CHANNELS):
                        df = ff[..., j] - fq[..., j]
                        phi = (df * df - (gg[..., j] + np.minimum(gg[..., j], gq[..., j]))) / den[..., j]
                        Df = np.where(phi > Df, phi, Df)  # a NaN phi is skipped by the comparison
                    wf = np.exp(-Df)
                    both = fvalid & fvalid[qyc, qxc]
                    w = np.where(both & (wf < w), wf, w)
                uq = u[qyc, qxc]
                acc = np.where(use[..., None], acc + w[..., None] * uq, acc)
                wsum = np.where(use, wsum + w, wsum)
        out = acc / wsum[..., None]
        raw = S / n.astype(np.float64)[..., None]
    return np.where(valid[..., None], out, raw)


# ---------------------------------------------------------------- the frames the host and the device tests share
def step_edge_frame(seed):
    """48 x 32, 16 samples: colour 0.5 | 0.6 left and right of column 24 with per-sample noise sigma 0.4; noise-free features whose albedo changes
    at the edge.  -> S, Q, F, G, n, truth"""
    rng = np.random.default_rng(seed)
    W, H, n = 48, 32, 16
    truth = np.zeros((H, W, 3))
    truth[:, : W // 2] = 0.5
    truth[:, W // 2 :] = 0.6
    smp = truth[None] + rng.normal(0, 0.4, (n, H, W, 3))
    S, Q = smp.sum(0), (smp * smp).sum(0)
    f = np.zeros((H, W, CHANNELS))
    f[..., 2] = 1.0
    f[:, : W // 2, 3:6] = (0.8, 0.2, 0.2)
    f[:, W // 2 :, 3:6] = (0.2, 0.2, 0.8)
    f[..., 6] = 3.0
    F = f * n
    return S, Q, F, F * f, np.full((H, W), n), truth


def band_rmse(img, truth):
    """RMSE against truth over columns 20 .. 27 (the 8 columns around the edge at 24)."""
    return float(np.sqrt(np.mean((img[:, 20:28] - truth[:, 20:28]) ** 2)))


def hit_miss_frame():
    """40 x 24, 8 samples: mean 0.25 left of column 25, 0.75 from it on, a claimed per-sample variance of 0.5 (large colour weights across the
    step); first hits on the left (normal (0, 0, 1), albedo 0.5, depth 4), misses on the right.  -> S, Q, F, G, n, u"""
    W, H, n = 40, 24, 8
    u = np.full((H, W, 3), 0.25)
    u[:, 25:] = 0.75
    S = u * n
    Q = S * u + 0.5 * n * (n - 1)
    f = np.zeros((H, W, CHANNELS))
    f[:, :25, 2] = 1.0
    f[:, :25, 3:6] = 0.5
    f[:, :25, 6] = 4.0
    F = f * n
    return S, Q, F, F * f, np.full((H, W), n), u
