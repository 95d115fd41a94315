"""A plain numpy float64 restatement of rmd_denoise_dual_select (include/raymond_hip.h states the definition).

`cross_filter_gain` is denoise_dual_guided_ref.cross_filter — the same operations in the same order — which also keeps the weight made at offset (0, 0)
and returns g = that weight / the sum of weights beside f.  `candidate` makes one candidate's f_A, f_B and per-pixel SURE, `winners` the windowed means
and the argmin, `blend` the weights m_i from the winners and the outputs.  `denoise_dual_select` runs them; `win=` replaces its own winners by given
ones (the device's: its exp may flip an argmin at a near tie, and everything after the winners is exact arithmetic on agreed inputs).
`denoise_dual_select_naive` reads the definition pixel by pixel with Python loops, for small frames: the vectorised form is held to it.
A candidate is a dict: k, alpha (1.0), guided (False), k_f (1.0), tau (1e-2).
"""
import numpy as np

import denoise_dual_ref
from denoise_dual_guided_ref import feature_planes
from denoise_guided_ref import CHANNELS
from denoise_ref import EPS, mean_and_variance

NO_WINNER = 0xFFFFFFFF


def _cand(c):
    return float(c["k"]), float(c.get("alpha", 1.0)), bool(c.get("guided", False)), float(c.get("k_f", 1.0)), float(c.get("tau", 1e-2))


def cross_filter_gain(u_w, v_w, u_v, valid, radius, patch_radius, k, alpha, guide=None):
    """-> f (H, W, 3), g (H, W): denoise_dual_guided_ref.cross_filter's f, and w(p, p) / sum_q w(p, q) of the same pass."""
    H, W = valid.shape
    r, f = int(radius), int(patch_radius)
    k2 = float(k) * float(k)
    alpha = float(alpha)
    ys, xs = np.arange(-f, H + f), np.arange(-f, W + f)
    ya, xa = np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)
    ua, va, oka = u_w[ya][:, xa], v_w[ya][:, xa], valid[ya][:, xa]
    acc = np.full((H, W, 3), -0.0)
    wsum = np.full((H, W), -0.0)
    wcentre = np.zeros((H, W))
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
                if dy == 0 and dx == 0:
                    wcentre = np.where(use, w, wcentre)
        return acc / wsum[..., None], wcentre / wsum


def half_sure(f, u, v, g):
    """((t_0 + t_1) + t_2) / 3 with t_c = ((d*d) - v_c) + ((2*v_c) * g), d = f_c - u_c."""
    with np.errstate(all="ignore"):
        t = None
        for c in range(3):
            d = f[..., c] - u[..., c]
            tc = (d * d - v[..., c]) + (2.0 * v[..., c]) * g
            t = tc if t is None else t + tc
        return t / 3.0


def _planes(S_a, Q_a, S_b, Q_b, n_a, n_b):
    u_a, v_a, ok_a = mean_and_variance(S_a, Q_a, n_a)
    u_b, v_b, ok_b = mean_and_variance(S_b, Q_b, n_b)
    return u_a, v_a, u_b, v_b, ok_a & ok_b


def candidate(planes, n_a, n_b, cand, F, G, n_f, radius, patch_radius):
    """-> f_A, f_B, sure of one candidate (sure is NaN where the pixel is not dual-valid)."""
    u_a, v_a, u_b, v_b, dual = planes
    k, alpha, guided, k_f, tau = _cand(cand)
    guide = feature_planes(F, G, n_f, dual, k_f, tau) if guided else None
    f_a, g_a = cross_filter_gain(u_b, v_b, u_a, dual, radius, patch_radius, k, alpha, guide)
    f_b, g_b = cross_filter_gain(u_a, v_a, u_b, dual, radius, patch_radius, k, alpha, guide)
    na, nb = n_a.astype(np.float64), n_b.astype(np.float64)
    with np.errstate(all="ignore"):
        sure = (na * half_sure(f_a, u_a, v_a, g_a) + nb * half_sure(f_b, u_b, v_b, g_b)) / (na + nb)
    return f_a, f_b, np.where(dual, sure, np.nan)


def window_means(sure, dual, window):
    """E (H, W): 0.0, then the dual-valid in-frame window pixels' values added in raster order, divided by their number."""
    H, W = dual.shape
    s, cnt = np.zeros((H, W)), np.zeros((H, W), dtype=np.int64)
    py, px = np.arange(H)[:, None], np.arange(W)[None, :]
    with np.errstate(all="ignore"):
        for dy in range(-window, window + 1):
            for dx in range(-window, window + 1):
                qy, qx = py + dy, px + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                use = inside & dual[qyc, qxc]
                s = np.where(use, s + sure[qyc, qxc], s)
                cnt = cnt + use
        return s / cnt.astype(np.float64)


def winners(sures, dual, window):
    """-> win (H, W) uint32 (NO_WINNER where not dual-valid), E: the list of window means."""
    E = [window_means(s, dual, window) for s in sures]
    best, eb = np.zeros(dual.shape, dtype=np.uint32), E[0]
    for i in range(1, len(E)):
        with np.errstate(all="ignore"):
            take = (E[i] < eb) | (np.isnan(eb) & ~np.isnan(E[i]))
        best, eb = np.where(take, np.uint32(i), best), np.where(take, E[i], eb)
    return np.where(dual, best, np.uint32(NO_WINNER)).astype(np.uint32), E


def blend_weights(win, n_cands, window):
    """m (n_cands, H, W): integer counts of the winners in the window over the count of dual-valid pixels there, one division."""
    H, W = win.shape
    cnt, total = np.zeros((n_cands, H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    py, px = np.arange(H)[:, None], np.arange(W)[None, :]
    for dy in range(-window, window + 1):
        for dx in range(-window, window + 1):
            qy, qx = py + dy, px + dx
            inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
            wq = win[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
            total += inside & (wq != NO_WINNER)
            for i in range(n_cands):
                cnt[i] += inside & (wq == i)
    with np.errstate(all="ignore"):
        return cnt.astype(np.float64) / total.astype(np.float64)[None]


def blend(m, fas, fbs, sures, S_a, S_b, n_a, n_b, dual, win):
    with np.errstate(all="ignore"):
        f_a, f_b, su = m[0][..., None] * fas[0], m[0][..., None] * fbs[0], m[0] * sures[0]
        for i in range(1, len(fas)):
            f_a, f_b, su = f_a + m[i][..., None] * fas[i], f_b + m[i][..., None] * fbs[i], su + m[i] * sures[i]
    out, err = denoise_dual_ref.combine(f_a, f_b, S_a, S_b, n_a, n_b, dual)
    return dict(out=out, err=err, sure=np.where(dual, su, np.nan), win=win)


def denoise_dual_select(S_a, Q_a, S_b, Q_b, n_a, n_b, cands, F=None, G=None, n_f=None, radius=10, patch_radius=3, sure_window=2, select_window=2, win=None,
                        parts=None):
    """-> dict(out (H, W, 3), err, sure (H, W), win (H, W) uint32, E: the window means, own_win: this restatement's winners).  `win`: winners to blend by
    instead of its own.  `parts`: a list of candidate() results computed before (the candidates' passes are the slow part)."""
    S_a, Q_a, S_b, Q_b = (np.asarray(x, dtype=np.float64) for x in (S_a, Q_a, S_b, Q_b))
    n_a, n_b = np.asarray(n_a), np.asarray(n_b)
    planes = _planes(S_a, Q_a, S_b, Q_b, n_a, n_b)
    dual = planes[4]
    if parts is None:
        parts = [candidate(planes, n_a, n_b, c, F, G, n_f, radius, patch_radius) for c in cands]
    fas, fbs, sures = ([p[j] for p in parts] for j in range(3))
    own, E = winners(sures, dual, sure_window)
    used = own if win is None else np.where(dual, np.asarray(win, dtype=np.uint32), np.uint32(NO_WINNER)).astype(np.uint32)
    res = blend(blend_weights(used, len(parts), select_window), fas, fbs, sures, S_a, S_b, n_a, n_b, dual, used)
    res.update(E=E, own_win=own, dual=dual, parts=parts)
    return res


def near_ties(E, dual, rel=1e-9):
    """The dual-valid pixels whose two smallest window means lie within rel * max|E| of each other without being equal (none with one candidate).  Equal
    ones are no tie to excuse: the lowest index wins them, and they are equal because two candidates went through the same operations (a candidate
    listed twice; radius 0, where every f is u) — on the device as well."""
    if len(E) < 2:
        return np.zeros(dual.shape, dtype=bool)
    A = np.stack(E)
    fin = np.isfinite(A)
    scale = np.max(np.abs(A[fin])) if fin.any() else 0.0
    srt = np.sort(np.where(np.isnan(A), np.inf, A), axis=0)
    with np.errstate(all="ignore"):
        close = ~(srt[1] - srt[0] > rel * scale) & ~(srt[1] == srt[0])
    return dual & close


# ---------------------------------------------------------------- the definition read pixel by pixel
def _naive_pass(uw, vw, uv, dual, guide, p, radius, patch_radius, k2, alpha):
    H, W = dual.shape
    y, x = p
    acc, wsum, wc = np.full(3, -0.0), -0.0, 0.0
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            qy, qx = y + dy, x + dx
            if 0 <= qy < H and 0 <= qx < W and dual[qy, qx]:
                w = denoise_dual_ref._naive_weight(uw, vw, dual, (y, x), (qy, qx), patch_radius, k2, alpha)
                if guide is not None:
                    ff, gg, den, fvalid = guide
                    if fvalid[y, x] and fvalid[qy, qx]:
                        Df = 0.0
                        for j in range(CHANNELS):
                            df = ff[y, x, j] - ff[qy, qx, j]
                            phi = (df * df - (gg[y, x, j] + min(gg[y, x, j], gg[qy, qx, j]))) / den[y, x, j]
                            if phi > Df:
                                Df = phi
                        wf = np.exp(-Df)
                        if wf < w:
                            w = wf
                acc = acc + w * uv[qy, qx]
                wsum = wsum + w
                if dy == 0 and dx == 0:
                    wc = w
    return acc / wsum, wc / wsum


def denoise_dual_select_naive(S_a, Q_a, S_b, Q_b, n_a, n_b, cands, F, G, n_f, radius, patch_radius, sure_window, select_window):
    """The definition read pixel by pixel (slow: small frames only) -> dict(out, err, sure, win)."""
    u_a, v_a, u_b, v_b, dual = _planes(S_a, Q_a, S_b, Q_b, n_a, n_b)
    H, W = dual.shape
    n = len(cands)
    fa, fb, sure = np.zeros((n, H, W, 3)), np.zeros((n, H, W, 3)), np.full((n, H, W), np.nan)
    with np.errstate(all="ignore"):
        for i, c in enumerate(cands):
            k, alpha, guided, k_f, tau = _cand(c)
            guide = feature_planes(F, G, n_f, dual, k_f, tau) if guided else None
            for y in range(H):
                for x in range(W):
                    if not dual[y, x]:
                        continue
                    sx = []
                    for (uw, vw, uv, vv, dst) in ((u_b, v_b, u_a, v_a, fa), (u_a, v_a, u_b, v_b, fb)):
                        f, g = _naive_pass(uw, vw, uv, dual, guide, (y, x), radius, patch_radius, k * k, alpha)
                        dst[i, y, x] = f
                        t = None
                        for ch in range(3):
                            d = f[ch] - uv[y, x, ch]
                            tc = (d * d - vv[y, x, ch]) + (2.0 * vv[y, x, ch]) * g
                            t = tc if t is None else t + tc
                        sx.append(t / 3.0)
                    na, nb = float(n_a[y, x]), float(n_b[y, x])
                    sure[i, y, x] = (na * sx[0] + nb * sx[1]) / (na + nb)

        def window(y, x, r):
            return [(qy, qx) for qy in range(y - r, y + r + 1) for qx in range(x - r, x + r + 1) if 0 <= qy < H and 0 <= qx < W and dual[qy, qx]]

        win = np.full((H, W), NO_WINNER, dtype=np.uint32)
        for y in range(H):
            for x in range(W):
                if not dual[y, x]:
                    continue
                best, eb = 0, None
                for i in range(n):
                    s = 0.0
                    qs = window(y, x, sure_window)
                    for q in qs:
                        s = s + sure[i][q]
                    e = s / float(len(qs))
                    if i == 0 or e < eb or (eb != eb and e == e):
                        best, eb = i, e
                win[y, x] = best
        f_a, f_b, su = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.full((H, W), np.nan)
        for y in range(H):
            for x in range(W):
                if not dual[y, x]:
                    continue
                qs = window(y, x, select_window)
                for i in range(n):
                    m = float(sum(1 for q in qs if win[q] == i)) / float(len(qs))
                    if i == 0:
                        f_a[y, x], f_b[y, x], su[y, x] = m * fa[0, y, x], m * fb[0, y, x], m * sure[0, y, x]
                    else:
                        f_a[y, x], f_b[y, x], su[y, x] = f_a[y, x] + m * fa[i, y, x], f_b[y, x] + m * fb[i, y, x], su[y, x] + m * sure[i, y, x]
    out, err = denoise_dual_ref.combine(f_a, f_b, np.asarray(S_a, dtype=np.float64), np.asarray(S_b, dtype=np.float64), np.asarray(n_a), np.asarray(n_b), dual)
    return dict(out=out, err=err, sure=su, win=win)
