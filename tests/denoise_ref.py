"""A plain numpy float64 restatement of rmd_denoise (include/raymond_hip.h states the definition).

Vectorised over the pixels, looping over the neighbour offsets d in raster order; each offset's patch terms are summed row by row (o_x
ascending), then the row sums over o_y ascending; the neighbours are accumulated in raster order of d.  This is the order the kernel
sums in, so the two differ only by the device's exp.
"""
import numpy as np

EPS = 1e-10


def count_image(width, height, rects, counts):
    """The per-pixel sample counts: counts[i] inside rect i, 0 where no rect lies."""
    n = np.zeros((height, width), dtype=np.int64)
    for (l, t, w, h), c in zip(rects, counts):
        n[t : t + h, l : l + w] = c
    return n


def mean_and_variance(S, Q, n):
    """u = S / n, v = max(0, (Q - S*u) / (n - 1)) / n, and the validity mask (n >= 2 and all six values finite)."""
    nd = n.astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        u = S / nd
        t = (Q - S * u) / (nd - 1.0)
        t = np.where(t < 0.0, 0.0, t)
        v = t / nd
    valid = (n >= 2) & np.isfinite(S).all(axis=-1) & np.isfinite(Q).all(axis=-1)
    return u, v, valid


def denoise(S, Q, n, radius=10, patch_radius=3, k=0.45, alpha=1.0):
    """S, Q: (H, W, 3) float64 sums and sums of squares; n: (H, W) sample counts.  Returns the (H, W, 3) denoised means."""
    S = np.asarray(S, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    n = np.asarray(n)
    H, W = n.shape
    r, f = int(radius), int(patch_radius)
    k2 = float(k) * float(k)
    alpha = float(alpha)
    u, v, valid = mean_and_variance(S, Q, n)
    # positions a' = p + o of the term image: rows -f .. H+f-1, columns -f .. W+f-1 (clamped when read)
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
                rows, crows = T[:, 0:W].copy(), Tc[:, 0:W].copy()  # (H + 2f, W): the sums over o_x
                for o in range(1, 2 * f + 1):
                    rows = rows + T[:, o : o + W]
                    crows = crows + Tc[:, o : o + W]
                ds, cnt = rows[0:H].copy(), crows[0:H].copy()  # (H, W): then over o_y
                for o in range(1, 2 * f + 1):
                    ds = ds + rows[o : o + H]
                    cnt = cnt + crows[o : o + H]
                D = ds / (3.0 * cnt.astype(np.float64))
                w = np.exp(-np.where(D > 0.0, D, 0.0))
                qy, qx = py + dy, px + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                use = valid & inside & valid[qyc, qxc]
                uq = u[qyc, qxc]
                acc = np.where(use[..., None], acc + w[..., None] * uq, acc)
                wsum = np.where(use, wsum + w, wsum)
        out = acc / wsum[..., None]
        raw = S / n.astype(np.float64)[..., None]
    return np.where(valid[..., None], out, raw)
