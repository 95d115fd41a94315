"""A plain numpy float64 restatement of rmd_denoise_dual and rmd_tile_error_dual (include/raymond_hip.h states the definitions).

`cross_filter` is denoise_ref.denoise's loop — the same patch sums in the same order — with the weights taken from one half, the values from
the other and "valid" read as dual-valid; `denoise_dual` runs it both ways and combines.  `denoise_dual_naive` reads the definition pixel by
pixel with Python loops, for small frames: the vectorised form is held to it.
"""
import numpy as np

from denoise_ref import EPS, mean_and_variance


def cross_filter(u_w, v_w, u_v, valid, radius, patch_radius, k, alpha):
    """f(p) = sum_q w(p,q) u_v(q) / sum_q w(p,q), w = rmd_denoise's weight on (u_w, v_w) with `valid` as the validity.  (H, W, 3); rows of pixels
    that are not valid are meaningless (the caller replaces them)."""
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
                acc = np.where(use[..., None], acc + w[..., None] * u_v[qyc, qxc], acc)
                wsum = np.where(use, wsum + w, wsum)
        return acc / wsum[..., None]


def combine(f_a, f_b, S_a, S_b, n_a, n_b, dual):
    """out and err from the two filtered halves (the definition's last four lines)."""
    na, nb = n_a.astype(np.float64)[..., None], n_b.astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        out = (na * f_a + nb * f_b) / (na + nb)
        h = (f_a - f_b) / 2.0
        err = (h[..., 0] * h[..., 0] + h[..., 1] * h[..., 1] + h[..., 2] * h[..., 2]) / 3.0
        raw = (S_a + S_b) / (na + nb)
    return np.where(dual[..., None], out, raw), np.where(dual, err, np.nan)


def denoise_dual(S_a, Q_a, S_b, Q_b, n_a, n_b, radius=10, patch_radius=3, k=0.45, alpha=1.0):
    """The two halves' (H, W, 3) sums and sums of squares and (H, W) counts -> (out (H, W, 3), err (H, W))."""
    S_a, Q_a, S_b, Q_b = (np.asarray(x, dtype=np.float64) for x in (S_a, Q_a, S_b, Q_b))
    n_a, n_b = np.asarray(n_a), np.asarray(n_b)
    u_a, v_a, ok_a = mean_and_variance(S_a, Q_a, n_a)
    u_b, v_b, ok_b = mean_and_variance(S_b, Q_b, n_b)
    dual = ok_a & ok_b
    f_a = cross_filter(u_b, v_b, u_a, dual, radius, patch_radius, k, alpha)
    f_b = cross_filter(u_a, v_a, u_b, dual, radius, patch_radius, k, alpha)
    return combine(f_a, f_b, S_a, S_b, n_a, n_b, dual)


def tile_error_dual(err, rects):
    """sqrt(mean of err over the rect), +inf if the rect holds a NaN, 0 for a rect without pixels."""
    out = np.zeros(len(rects))
    for i, (l, t, w, h) in enumerate(rects):
        e = err[t : t + h, l : l + w]
        if e.size:
            out[i] = np.inf if np.isnan(e).any() else np.sqrt(e.sum() / e.size)
    return out


def _naive_weight(u, v, valid, p, q, f, k2, alpha):
    H, W = valid.shape
    total, taken = 0.0, 0
    for oy in range(-f, f + 1):
        row = 0.0
        for ox in range(-f, f + 1):
            a = (min(max(p[0] + oy, 0), H - 1), min(max(p[1] + ox, 0), W - 1))
            b = (min(max(q[0] + oy, 0), H - 1), min(max(q[1] + ox, 0), W - 1))
            t = 0.0
            if valid[a] and valid[b]:
                t = None
                for c in range(3):
                    du = u[a][c] - u[b][c]
                    term = (du * du - alpha * (v[a][c] + min(v[a][c], v[b][c]))) / (EPS + k2 * (v[a][c] + v[b][c]))
                    t = term if t is None else t + term
                taken += 1
            row = t if ox == -f else row + t  # the row's offsets summed with o_x ascending (an offset not taken adds 0.0)
        total = row if oy == -f else total + row
    D = total / (3.0 * float(taken))
    return np.exp(-(D if D > 0.0 else 0.0))


def denoise_dual_naive(S_a, Q_a, S_b, Q_b, n_a, n_b, radius, patch_radius, k, alpha):
    """The definition read pixel by pixel (slow: small frames only)."""
    u_a, v_a, ok_a = mean_and_variance(S_a, Q_a, n_a)
    u_b, v_b, ok_b = mean_and_variance(S_b, Q_b, n_b)
    dual = ok_a & ok_b
    H, W = dual.shape
    k2 = float(k) * float(k)
    f_a, f_b = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    with np.errstate(all="ignore"):
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
                                w = _naive_weight(uw, vw, dual, (y, x), (qy, qx), patch_radius, k2, float(alpha))
                                acc = acc + w * uv[qy, qx]
                                wsum = wsum + w
                    dst[y, x] = acc / wsum
    return combine(f_a, f_b, S_a, S_b, n_a, n_b, dual)
