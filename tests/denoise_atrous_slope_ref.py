"""A plain numpy float64 restatement of the three a-trous _slope calls (include/raymond_hip.h states the definition): rmd_denoise_atrous_slope,
rmd_denoise_atrous_dual_slope and rmd_denoise_atrous_dual_slope_region.

Only the denominator of Phi_j(p, .) changes, and it is the same at every level and for both halves: denoise_slope_ref.floored_den, made once from the
call's own feature means and feature-validity.  Every function here takes the denominator as an argument (`den`, inside the guide (f, g, den, fvalid)); the
operations are the existing restatements' own — denoise_atrous_ref.atrous_all's level, restated below as `single_level` because that module makes its
denominator inside its _inputs, and denoise_atrous_dual_region_ref._level, which already takes a guide.  The filtered frames differ from the kernels'
only by the device's exp.

atrous_slope / atrous_slope_all      — rmd_denoise_atrous_slope, vectorised over the pixels
atrous_slope_by_pixel                — the same definition read pixel by pixel with Python floats, the slope floor included (its own reading of m); the
                                       two agree bit for bit (tests/test_denoise_atrous_slope_host.py)
atrous_dual_slope                    — rmd_denoise_atrous_dual_slope -> (out, err)
atrous_dual_slope_region             — its region form on the needed sets of denoise_atrous_dual_region_ref: f and g exist on the prologue's set only, the
                                       floors on level 0's set only, and a floor that read a missing f is NaN — so "equal to the whole frame inside the
                                       region" proves the sets large enough for the slope too
"""
import numpy as np

import denoise_atrous_dual_ref as adref
import denoise_atrous_dual_region_ref as rref
from denoise_atrous_ref import H5, _exp, _fmin
from denoise_dual_guided_ref import feature_planes
from denoise_dual_ref import combine
from denoise_guided_ref import CHANNELS, feature_mean_and_variance
from denoise_ref import EPS, mean_and_variance
from denoise_slope_ref import floored_den, slope_planes


# ---------------------------------------------------------------- the single call
def single_inputs(S, Q, F, G, n, k_f, tau, slope):
    """u, v, valid, the guide (f, g, den, fvalid) with the floored denominator — None without features —, and S / n."""
    S, Q = np.asarray(S, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    n = np.asarray(n)
    u, v, valid = mean_and_variance(S, Q, n)
    guide = None
    if F is not None:
        ff, gg, fvalid = feature_mean_and_variance(np.asarray(F, dtype=np.float64), np.asarray(G, dtype=np.float64), n, valid)
        guide = (ff, gg, floored_den(ff, gg, fvalid, k_f, tau, slope), fvalid)
    with np.errstate(all="ignore"):
        raw = S / n.astype(np.float64)[..., None]
    return u, v, valid, guide, raw


def single_level(c, var, valid, guide, s, k2, alpha):
    """One level of denoise_atrous_ref.atrous_all at step s, operation for operation, with the caller's denominator -> (c, var) of the next level."""
    H, W = valid.shape
    py, px = np.arange(H)[:, None], np.arange(W)[None, :]
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
            if guide is not None:
                ff, gg, den, fvalid = guide
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
    return A / Ws[..., None], B / (Ws * Ws)[..., None]


def atrous_slope_all(S, Q, n, levels, k=3.0, alpha=1.0, F=None, G=None, k_f=1.0, tau=1e-2, slope=0.0):
    """{count: (H, W, 3) filtered means} after each of the level counts in `levels`, from one run to the largest of them."""
    u, v, valid, guide, raw = single_inputs(S, Q, F, G, n, k_f, tau, slope)
    k2, alpha = float(k) * float(k), float(alpha)
    c, var = u.copy(), v.copy()
    wanted = {int(l) for l in levels}
    out = {0: np.where(valid[..., None], c, raw)} if 0 in wanted else {}
    with np.errstate(all="ignore"):
        for level in range(max(wanted)):
            c, var = single_level(c, var, valid, guide, 1 << level, k2, alpha)
            if level + 1 in wanted:
                out[level + 1] = np.where(valid[..., None], c, raw)
    return out


def atrous_slope(S, Q, n, levels=5, k=3.0, alpha=1.0, F=None, G=None, k_f=1.0, tau=1e-2, slope=0.0):
    """rmd_denoise_atrous_slope -> the (H, W, 3) filtered means."""
    return atrous_slope_all(S, Q, n, [levels], k, alpha, F, G, k_f, tau, slope)[int(levels)]


def _floor_by_pixel(ff, fvalid, y, x, ch, s2):
    """m_pj read at one pixel: per axis the smaller squared difference to the two neighbours when both are inside the frame and feature-valid."""
    H, W = fvalid.shape
    total = []
    for (dy, dx) in ((0, 1), (1, 0)):  # the row's neighbours (h), then the column's (v)
        ly, lx, ry, rx = y - dy, x - dx, y + dy, x + dx
        if not (0 <= ly and 0 <= lx and ry < H and rx < W and fvalid[ly, lx] and fvalid[ry, rx]):
            total.append(np.float64(0.0))
            continue
        a_l, a_r = ff[y, x, ch] - ff[ly, lx, ch], ff[ry, rx, ch] - ff[y, x, ch]
        l2, r2 = a_l * a_l, a_r * a_r
        total.append(l2 if l2 < r2 else r2)
    return np.float64(s2) * (total[0] + total[1])


def atrous_slope_by_pixel(S, Q, n, levels=5, k=3.0, alpha=1.0, F=None, G=None, k_f=1.0, tau=1e-2, slope=0.0):
    """The second reading: every valid pixel's denominators and taps one after another, in Python floats.  It shares u, v, f, g and the masks with the
    first reading and nothing else: the floor and the denominator are read here from the header's lines."""
    S, Q = np.asarray(S, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    n = np.asarray(n)
    u, v, valid = mean_and_variance(S, Q, n)
    ff = gg = fvalid = None
    if F is not None:
        ff, gg, fvalid = feature_mean_and_variance(np.asarray(F, dtype=np.float64), np.asarray(G, dtype=np.float64), n, valid)
    H, W = valid.shape
    k2, alpha, kf2, tau, s2 = float(k) * float(k), float(alpha), float(k_f) * float(k_f), float(tau), float(slope) * float(slope)
    c, var = u.copy(), v.copy()
    old = np.seterr(all="ignore")
    try:
        den = np.zeros((H, W, CHANNELS))
        if ff is not None:  # once: the features are every level's
            for y in range(H):
                for x in range(W):
                    if not fvalid[y, x]:
                        continue
                    for ch in range(CHANNELS):
                        a = np.float64(tau) * (np.float64(1.0) if ch < CHANNELS - 1 else ff[y, x, ch] * ff[y, x, ch])
                        t = a if a > gg[y, x, ch] else gg[y, x, ch]
                        m = _floor_by_pixel(ff, fvalid, y, x, ch, s2)
                        if m > t:
                            t = m
                        den[y, x, ch] = np.float64(EPS) + np.float64(kf2) * t
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
        raw = S / n.astype(np.float64)[..., None]
    finally:
        np.seterr(**old)
    return np.where(valid[..., None], c, raw)


# ---------------------------------------------------------------- the dual calls
def dual_inputs(S_a, Q_a, S_b, Q_b, n_a, n_b, F, G, n_f, k_f, tau, slope):
    """denoise_atrous_dual_ref._inputs' values with the floored denominator in the guide (None without features)."""
    S_a, S_b, n_a, n_b, u_a, v_a, u_b, v_b, dual, _ = adref._inputs(S_a, Q_a, S_b, Q_b, n_a, n_b, None, None, None, k_f, tau)
    guide = None
    if F is not None:
        ff, gg, _, fvalid = feature_planes(F, G, n_f, dual, k_f, tau)
        guide = (ff, gg, floored_den(ff, gg, fvalid, k_f, tau, slope), fvalid)
    return S_a, S_b, n_a, n_b, u_a, v_a, u_b, v_b, dual, guide


def filtered_halves_slope_all(S_a, Q_a, S_b, Q_b, n_a, n_b, levels, k=3.0, alpha=1.0, F=None, G=None, n_f=None, k_f=1.0, tau=1e-2, slope=0.0):
    """{count: (f_A, f_B)} after each of the level counts in `levels`, from one run to the largest of them, and the dual-validity mask (as
    denoise_atrous_dual_ref.filtered_halves_all)."""
    _, _, _, _, u_a, v_a, u_b, v_b, dual, guide = dual_inputs(S_a, Q_a, S_b, Q_b, n_a, n_b, F, G, n_f, k_f, tau, slope)
    k2, alpha = float(k) * float(k), float(alpha)
    wanted = {int(l) for l in levels}
    halves = {0: (u_a, u_b)} if 0 in wanted else {}
    state = [u_a.copy(), v_a.copy(), u_b.copy(), v_b.copy()]
    with np.errstate(all="ignore"):
        for level in range(max(wanted)):
            state = rref._level(state, dual, guide, 1 << level, k2, alpha)
            if level + 1 in wanted:
                halves[level + 1] = (state[0], state[2])
    return halves, dual


def atrous_dual_slope_all(S_a, Q_a, S_b, Q_b, n_a, n_b, levels, k=3.0, alpha=1.0, F=None, G=None, n_f=None, k_f=1.0, tau=1e-2, slope=0.0):
    """{count: (out, err)} after each of the level counts in `levels`, from one run to the largest of them."""
    halves, dual = filtered_halves_slope_all(S_a, Q_a, S_b, Q_b, n_a, n_b, levels, k, alpha, F, G, n_f, k_f, tau, slope)
    S_a, S_b = np.asarray(S_a, dtype=np.float64), np.asarray(S_b, dtype=np.float64)
    return {lv: combine(f_a, f_b, S_a, S_b, np.asarray(n_a), np.asarray(n_b), dual) for lv, (f_a, f_b) in halves.items()}


def atrous_dual_slope(S_a, Q_a, S_b, Q_b, n_a, n_b, levels=5, k=3.0, alpha=1.0, F=None, G=None, n_f=None, k_f=1.0, tau=1e-2, slope=0.0):
    """rmd_denoise_atrous_dual_slope -> (out (H, W, 3), err (H, W))."""
    return atrous_dual_slope_all(S_a, Q_a, S_b, Q_b, n_a, n_b, [levels], k, alpha, F, G, n_f, k_f, tau, slope)[int(levels)]


def atrous_dual_slope_region(S_a, Q_a, S_b, Q_b, n_a, n_b, region, levels=5, k=3.0, alpha=1.0, F=None, G=None, n_f=None, k_f=1.0, tau=1e-2, slope=0.0):
    """rmd_denoise_atrous_dual_slope_region -> (out, err), NaN outside the region.  The state lives on the needed sets as in
    denoise_atrous_dual_region_ref.atrous_dual_region; f and g on the prologue's set P; the floors are made from THAT f, with a neighbour's presence still
    the whole frame's feature-validity, and kept on level 0's set R_0 alone.  A floor that read an f outside P is NaN and makes its denominator NaN."""
    S_a, S_b, n_a, n_b, u_a, v_a, u_b, v_b, dual, guide = dual_inputs(S_a, Q_a, S_b, Q_b, n_a, n_b, F, G, n_f, k_f, tau, 0.0)
    H, W = dual.shape
    P, R = rref.needed_sets(region, levels, W, H)
    state = rref._keep([u_a, v_a, u_b, v_b], P)
    if guide is not None and levels > 0:
        ff, gg, _, fvalid = guide
        ff, gg = np.where(P[..., None], ff, np.nan), np.where(P[..., None], gg, np.nan)
        with np.errstate(all="ignore"):
            den = floored_den(ff, gg, fvalid, k_f, tau, slope)
            if float(slope) > 0.0:  # (slope 0 makes no floors: the denominator then exists wherever f and g do)
                m = slope_planes(ff, fvalid, slope)
                den = np.where(np.isnan(m) | ~R[0][..., None], np.nan, den)
        guide = (ff, gg, den, fvalid)
    k2, alpha = float(k) * float(k), float(alpha)
    with np.errstate(all="ignore"):
        for level in range(levels):
            state = rref._keep(rref._level(state, dual, guide, 1 << level, k2, alpha), R[level])
    out, err = combine(state[0], state[2], S_a, S_b, n_a, n_b, dual)
    inside = rref.region_mask(region, W, H)
    return np.where(inside[..., None], out, np.nan), np.where(inside, err, np.nan)
