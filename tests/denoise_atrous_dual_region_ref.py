"""A numpy float64 restatement of rmd_denoise_atrous_dual_region (include/raymond_hip.h states the definition, DESIGN.md section 19 the needed sets).

needed_sets restates the dilation rule as boolean images, one step at a time.  atrous_dual_region runs tests/denoise_atrous_dual_ref.py's level — the
same operations in the same order — level by level, and after every level keeps the result on that level's needed set only: every state value outside
it is NaN.  A NaN that a needed pixel's taken tap read would reach the region's output, so "equal to the whole-frame restatement inside the region"
proves that the sets are large enough.
"""
import numpy as np

from denoise_atrous_dual_ref import _colour_weight, _inputs
from denoise_atrous_ref import H5
from denoise_dual_ref import combine
from denoise_guided_ref import CHANNELS


def region_mask(region, W, H):
    m = np.zeros((H, W), dtype=bool)
    for (l, t, w, h) in region:
        m[t : t + h, l : l + w] = True
    return m


def dilate(mask, d):
    """Every pixel within d pixels, each way, of a pixel of `mask`, inside the frame."""
    H, W = mask.shape
    out = np.zeros_like(mask)
    ys, xs = np.nonzero(mask)
    for y, x in zip(ys, xs):
        out[max(0, y - d) : min(H, y + d + 1), max(0, x - d) : min(W, x + d + 1)] = True
    return out


def needed_sets(region, levels, W, H):
    """(P, [R_0 .. R_{levels-1}]): R_{levels-1} is the region, R_l is R_{l+1} dilated by 2 * 2^(l+1) — a level-(l+1) tap reaches two steps of 2^(l+1) —
    and P, where the prologue's planes are needed, is R_0 dilated by 2 (the region itself at levels = 0)."""
    R = [None] * levels
    cur = region_mask(region, W, H)
    for l in range(levels - 1, -1, -1):
        R[l] = cur
        cur = dilate(cur, 2 * (1 << l))  # what level l reads: two steps of 2^l (= 2 * 2^((l-1)+1), the set of level l - 1; at l = 0 the prologue's)
    return cur, R


def _level(state, dual, guide, s, k2, alpha):
    """One level of denoise_atrous_dual_ref.filtered_halves_all, word for word."""
    H, W = dual.shape
    py, px = np.arange(H)[:, None], np.arange(W)[None, :]
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
                    Df = np.where(phi > Df, phi, Df)
                wf = np.exp(-Df)
                both = fvalid & fvalid[qyc, qxc]
                w_a = np.where(both & (wf < w_a), wf, w_a)
                w_b = np.where(both & (wf < w_b), wf, w_b)
            h = H5[i + 2] * H5[j + 2]
            for w, cq, vq, o in ((w_b, caq, vaq, 0), (w_a, cbq, vbq, 3)):
                hw = h * w
                acc[o] = np.where(take[..., None], acc[o] + hw[..., None] * cq, acc[o])
                acc[o + 1] = np.where(take[..., None], acc[o + 1] + (hw * hw)[..., None] * vq, acc[o + 1])
                acc[o + 2] = np.where(take, acc[o + 2] + hw, acc[o + 2])
    return [acc[0] / acc[2][..., None], acc[1] / (acc[2] * acc[2])[..., None], acc[3] / acc[5][..., None], acc[4] / (acc[5] * acc[5])[..., None]]


def _keep(state, mask):
    return [np.where(mask[..., None], x, np.nan) for x in state]


def atrous_dual_region(S_a, Q_a, S_b, Q_b, n_a, n_b, region, levels=5, k=3.0, alpha=1.0, F=None, G=None, n_f=None, k_f=1.0, tau=1e-2, sets=None):
    """-> (out (H, W, 3), err (H, W), state): out and err NaN outside the region; state the four images (c_A, v_A, c_B, v_B) after the last level, NaN
    outside the region.  `sets`: needed sets other than needed_sets' own (a test that shrinks one)."""
    S_a, S_b, n_a, n_b, u_a, v_a, u_b, v_b, dual, guide = _inputs(S_a, Q_a, S_b, Q_b, n_a, n_b, F, G, n_f, k_f, tau)
    H, W = dual.shape
    P, R = sets if sets is not None else needed_sets(region, levels, W, H)
    state = _keep([u_a, v_a, u_b, v_b], P)
    if guide is not None:  # the feature planes exist on the prologue's set only
        ff, gg, den, fvalid = guide
        guide = (np.where(P[..., None], ff, np.nan), np.where(P[..., None], gg, np.nan), np.where(P[..., None], den, np.nan), fvalid)
    k2, alpha = float(k) * float(k), float(alpha)
    with np.errstate(all="ignore"):
        for level in range(levels):
            state = _keep(_level(state, dual, guide, 1 << level, k2, alpha), R[level])
    out, err = combine(state[0], state[2], S_a, S_b, n_a, n_b, dual)
    inside = region_mask(region, W, H)
    return np.where(inside[..., None], out, np.nan), np.where(inside, err, np.nan), state
