"""A plain numpy float64 restatement of the four _slope calls (include/raymond_hip.h states the definition): rmd_denoise_guided_slope,
rmd_denoise_dual_guided_slope, its region form and rmd_denoise_dual_select_slope.

Only the denominator of Phi_j(p, .) changes, so everything else is the existing restatements' own code: `slope_planes` makes m_pj = (slope * slope) *
(h_j + v_j) from the feature means and the feature-validity mask in exact IEEE operations in the header's order (the device's seven planes can be held
to it bit for bit), `floored_den` puts it under max(tau * s_pj, g_pj), and the filters are denoise_dual_guided_ref.cross_filter /
denoise_dual_select_ref.cross_filter_gain with that denominator in their guide.  The filtered frames differ from the kernels' only by the device's exp.
A select candidate is denoise_dual_select_ref's dict with one more key, slope (0.0).
"""
import numpy as np

import denoise_dual_guided_ref as dgref
import denoise_dual_ref
import denoise_dual_select_ref as sref
import denoise_guided_ref as gref
from denoise_guided_ref import CHANNELS
from denoise_ref import EPS, mean_and_variance


def _axis_min(ff, fvalid, axis):
    """Per pixel and channel: the smaller of the squared differences to the two neighbours along `axis` (0: rows, 1: columns) where the pixel and both
    neighbours are feature-valid and inside the frame, else 0.0."""
    out = np.zeros(ff.shape)
    if ff.shape[axis] < 3:
        return out
    sl = lambda a, b: tuple([slice(None)] * axis + [slice(a, b)])  # noqa: E731
    lo, mid, hi = sl(0, -2), sl(1, -1), sl(2, None)
    with np.errstate(all="ignore"):
        a_l, a_r = ff[mid] - ff[lo], ff[hi] - ff[mid]
        l2, r2 = a_l * a_l, a_r * a_r
        both = fvalid[mid] & fvalid[lo] & fvalid[hi]
        out[mid] = np.where(both[..., None], np.where(l2 < r2, l2, r2), 0.0)
    return out


def slope_planes(ff, fvalid, slope):
    """m (H, W, 7) = (slope * slope) * (h + v); zeros at a pixel that is not feature-valid."""
    s2 = float(slope) * float(slope)
    with np.errstate(all="ignore"):
        m = s2 * (_axis_min(ff, fvalid, 1) + _axis_min(ff, fvalid, 0))
    return np.where(fvalid[..., None], m, 0.0)


def floored_den(ff, gg, fvalid, k_f, tau, slope):
    """eps + k_f^2 * t with t = max(tau * s, g) in the existing comparison, then t = m where m > t."""
    kf2 = float(k_f) * float(k_f)
    with np.errstate(all="ignore"):
        s = np.ones_like(ff)
        s[..., CHANNELS - 1] = ff[..., CHANNELS - 1] * ff[..., CHANNELS - 1]
        a = float(tau) * s
        t = np.where(a > gg, a, gg)
        m = slope_planes(ff, fvalid, slope)
        t = np.where(m > t, m, t)
        return EPS + kf2 * t


def denoise_guided_slope(S, Q, F, G, n, radius=10, patch_radius=3, k=0.45, alpha=1.0, k_f=1.0, tau=1e-2, slope=0.0):
    """rmd_denoise_guided_slope: denoise_guided_ref.denoise_guided's operations (its loop is cross_filter's with the frame as both halves) with the
    floored denominator.  F = G = None: denoise_guided_ref.denoise_guided itself."""
    if F is None:
        return gref.denoise_guided(S, Q, None, None, n, radius, patch_radius, k, alpha)
    S, Q, F, G = (np.asarray(x, dtype=np.float64) for x in (S, Q, F, G))
    n = np.asarray(n)
    u, v, valid = mean_and_variance(S, Q, n)
    ff, gg, fvalid = gref.feature_mean_and_variance(F, G, n, valid)
    guide = (ff, gg, floored_den(ff, gg, fvalid, k_f, tau, slope), fvalid)
    out = dgref.cross_filter(u, v, u, valid, radius, patch_radius, k, alpha, guide)
    with np.errstate(all="ignore"):
        raw = S / n.astype(np.float64)[..., None]
    return np.where(valid[..., None], out, raw)


def _dual_guide(F, G, n_f, dual, k_f, tau, slope):
    ff, gg, _, fvalid = dgref.feature_planes(F, G, n_f, dual, k_f, tau)
    return ff, gg, floored_den(ff, gg, fvalid, k_f, tau, slope), fvalid


def denoise_dual_guided_slope(S_a, Q_a, S_b, Q_b, n_a, n_b, F, G, n_f, radius=10, patch_radius=3, k=0.45, alpha=1.0, k_f=1.0, tau=1e-2, slope=0.0):
    """rmd_denoise_dual_guided_slope -> (out (H, W, 3), err (H, W)); its region form writes these values at the region's pixels."""
    S_a, Q_a, S_b, Q_b = (np.asarray(x, dtype=np.float64) for x in (S_a, Q_a, S_b, Q_b))
    n_a, n_b = np.asarray(n_a), np.asarray(n_b)
    u_a, v_a, ok_a = mean_and_variance(S_a, Q_a, n_a)
    u_b, v_b, ok_b = mean_and_variance(S_b, Q_b, n_b)
    dual = ok_a & ok_b
    guide = None if F is None else _dual_guide(F, G, n_f, dual, k_f, tau, slope)
    f_a = dgref.cross_filter(u_b, v_b, u_a, dual, radius, patch_radius, k, alpha, guide)
    f_b = dgref.cross_filter(u_a, v_a, u_b, dual, radius, patch_radius, k, alpha, guide)
    return denoise_dual_ref.combine(f_a, f_b, S_a, S_b, n_a, n_b, dual)


def select_candidate(planes, n_a, n_b, cand, F, G, n_f, radius, patch_radius):
    """denoise_dual_select_ref.candidate with the candidate's slope in a guided one's denominator."""
    u_a, v_a, u_b, v_b, dual = planes
    k, alpha, guided, k_f, tau = sref._cand(cand)
    guide = _dual_guide(F, G, n_f, dual, k_f, tau, float(cand.get("slope", 0.0))) if guided else None
    f_a, g_a = sref.cross_filter_gain(u_b, v_b, u_a, dual, radius, patch_radius, k, alpha, guide)
    f_b, g_b = sref.cross_filter_gain(u_a, v_a, u_b, dual, radius, patch_radius, k, alpha, guide)
    na, nb = n_a.astype(np.float64), n_b.astype(np.float64)
    with np.errstate(all="ignore"):
        sure = (na * sref.half_sure(f_a, u_a, v_a, g_a) + nb * sref.half_sure(f_b, u_b, v_b, g_b)) / (na + nb)
    return f_a, f_b, np.where(dual, sure, np.nan)


def denoise_dual_select_slope(S_a, Q_a, S_b, Q_b, n_a, n_b, cands, F=None, G=None, n_f=None, radius=10, patch_radius=3, sure_window=2, select_window=2,
                              win=None, parts=None):
    """rmd_denoise_dual_select_slope: denoise_dual_select_ref.denoise_dual_select over select_candidate's parts (same result dict)."""
    S_a, Q_a, S_b, Q_b = (np.asarray(x, dtype=np.float64) for x in (S_a, Q_a, S_b, Q_b))
    n_a, n_b = np.asarray(n_a), np.asarray(n_b)
    if parts is None:
        planes = sref._planes(S_a, Q_a, S_b, Q_b, n_a, n_b)
        parts = [select_candidate(planes, n_a, n_b, c, F, G, n_f, radius, patch_radius) for c in cands]
    return sref.denoise_dual_select(S_a, Q_a, S_b, Q_b, n_a, n_b, cands, F, G, n_f, radius=radius, patch_radius=patch_radius, sure_window=sure_window,
                                    select_window=select_window, win=win, parts=parts)


# ---------------------------------------------------------------- the frame the host and the device tests share
DOME_CENTRE, DOME_RADIUS = (23.5, 15.5), 14.0


def dome_frame(seed):
    """48 x 32, 16 samples: colour 0.5 everywhere with per-sample noise sigma 0.4; noise-free features (G = F * f) of a dome — albedo 0.5, depth 3, normal
    (0, 0, 1) outside the disc of radius 14 px around (23.5, 15.5) and (dx, dy, sqrt(1 - dx^2 - dy^2)) inside it, dx, dy the offsets from the centre
    divided by 14: normals that change from pixel to pixel on a surface whose colour does not.  -> S, Q, F, G, n, truth, disc (the (H, W) mask)"""
    rng = np.random.default_rng(seed)
    W, H, n = 48, 32, 16
    truth = np.full((H, W, 3), 0.5)
    smp = truth[None] + rng.normal(0, 0.4, (n, H, W, 3))
    S, Q = smp.sum(0), (smp * smp).sum(0)
    dx = (np.arange(W)[None, :] - DOME_CENTRE[0]) / DOME_RADIUS + np.zeros((H, 1))
    dy = (np.arange(H)[:, None] - DOME_CENTRE[1]) / DOME_RADIUS + np.zeros((1, W))
    disc = dx * dx + dy * dy < 1.0
    f = np.zeros((H, W, CHANNELS))
    f[..., 2] = 1.0
    f[disc, 0], f[disc, 1] = dx[disc], dy[disc]
    f[disc, 2] = np.sqrt(1.0 - dx[disc] ** 2 - dy[disc] ** 2)
    f[..., 3:6] = 0.5
    f[..., 6] = 3.0
    F = f * n
    return S, Q, F, F * f, np.full((H, W), n), truth, disc


def disc_rmse(img, truth, disc):
    return float(np.sqrt(np.mean((img[disc] - truth[disc]) ** 2)))
