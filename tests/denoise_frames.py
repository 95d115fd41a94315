"""Adversarial frames for the denoise family (rmd_denoise, its guided, dual, region, slope and select forms, and the a-trous calls), and the bar a
device result is held to on them.  Seeded and pure numpy, in the style of sphere_scenes.py and grid_meshes.py.

Every class is a function of its name alone and returns a Frame: the two halves' sums and sums of squares, the feature sums, one rect list with a
sample count per rect for half A, half B and the features, and the three count images the restatements take.  The single-buffer calls take half A.

    shape_*   test_gpu_denoise._moments content (two halves, counts with a 0 and a 1, poison) on frames one short of, equal to and one past the kernels'
              tile widths (32 and 24) and height (16), single rows and columns, and frames smaller than the patch
    seam_*    invalid pixels where the kernels' structure is — the tile seams, the frame border, a whole tile, the whole frame, all but one pixel, a
              checkerboard, a ring around one pixel — by each route in turn (n = 0, n = 1, NaN in S, inf in Q), in half A, half B, both at different
              places, or in the features only (n_f = 0, n_f = 1, NaN in F, inf in G)
    scale_*   the _moments frame times a power of two (S by s, Q by s^2) until eps = 1e-10 dominates the distance's denominator or vanishes in it,
              (du)^2 overflowing between two regions, two scales in one frame, a flat dyadic frame, negative means, Q under S^2 / n, and counts of 2, 3
              and 2^32 - 1 side by side
    region_*  region sets for the _region calls on a SEAM-sized frame (region_sets)

The frames are small (no side over 72, no area over about 3,000 pixels): two tiles each way at either tile width.
"""
import zlib

import numpy as np

from denoise_ref import mean_and_variance

CHANNELS = 7
SEAM = (40, 20)  # W, H of the seam_*, scale_* and region_* frames: tile seams at x = 24 (TW = 24), x = 32 (TW = 32) and y = 16, two tiles each way
RING_DEPTH = 4   # kDenoiseMaxPatch: the ringed pixel's patch holds no other valid pixel at any f
RING_PIXEL = (9, 12)  # (y, x)
SHAPES = ((31, 17), (32, 16), (33, 15), (23, 17), (24, 16), (25, 15), (47, 9), (48, 33), (49, 5), (1, 40), (40, 1), (2, 2), (3, 70), (70, 3))
SCALES = (40, -40, 200, -200, 500, -500)
UINT32_MAX = 2**32 - 1


# ---------------------------------------------------------------- content
def moments(rng, n_img, floor=False):
    """test_gpu_denoise._moments, operation for operation (tests/test_denoise_frames_host.py holds the two to each other): sums and sums of squares of
    n samples per pixel, a smooth image plus noise whose level varies over the frame.  `floor`: no pixel's noise level below 0.05 and no Q halved, so
    that every variance estimate is positive (the scale_* frames, whose point is the size of v beside eps)."""
    H, W = n_img.shape
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([0.5 + 0.4 * np.sin(x / 5.0), 0.3 + 0.2 * np.cos(y / 3.0), 0.2 + 0.1 * ((x + y) % 7)], axis=-1)
    sigma = rng.uniform(0.05 if floor else 0.0, 0.6, (H, W, 1)) * (1 + (x % 9 == 0))[..., None]
    n = np.maximum(n_img, 0).astype(np.float64)[..., None]
    mean = base + rng.normal(0.0, 1.0, (H, W, 3)) * sigma / np.sqrt(np.maximum(n, 1.0))
    S = mean * n
    Q = S * mean + rng.uniform(0.25 if floor else 0.0, 1.0, (H, W, 3)) * sigma * sigma * np.maximum(n - 1.0, 0.0)
    halve = rng.uniform(size=(H, W, 3)) < 0.02
    if not floor:
        Q[halve] *= 0.5  # some below S^2 / n: a negative variance estimate, clamped to 0
    return S, Q


def poison(S, Q, rng):
    """test_gpu_denoise._poison: NaN and inf in S, inf in Q, at a few random pixels."""
    H, W = S.shape[:2]
    for value, arr in ((np.nan, S), (np.inf, S), (-np.inf, S), (np.inf, Q)):
        for _ in range(max(1, H * W // 400)):
            arr[rng.integers(0, H), rng.integers(0, W), rng.integers(0, 3)] = value


def feature_means(rng, W, H):
    """Per-pixel feature means, per-sample noise levels and the variance factors: a normal that turns slowly over the frame (about 0.02 a pixel: at the
    shipped k_f = 1, tau = 1e-2 the feature weight falls from 1 to nothing over the filter's window instead of isolating every pixel), steps as albedos
    have, a depth ramp with a step, misses (all-zero pixels), noise in every fifth column."""
    y, x = np.mgrid[0:H, 0:W]
    f = np.zeros((H, W, CHANNELS))
    f[..., 0], f[..., 1] = 0.3 * np.sin(x / 9.0 + y / 13.0), 0.3 * np.cos(x / 11.0 - y / 7.0)
    f[..., 2] = np.sqrt(1.0 - f[..., 0] * f[..., 0] - f[..., 1] * f[..., 1])
    f[..., 3:6] = np.stack([np.where(x < W // 2, 0.8, 0.7), 0.2 + 0.0 * x, np.where(y < H // 2, 0.2, 0.8)], axis=-1)
    f[..., 6] = 3.0 + 0.01 * x + np.where(x % 13 < 6, 0.0, 0.5)
    f[(x + 2 * y) % 17 == 0] = 0.0
    sigma = rng.uniform(0.0, 0.05, (H, W, 1)) * (x % 5 == 0)[..., None]
    return f + rng.normal(0.0, 1.0, (H, W, CHANNELS)) * sigma, sigma, rng.uniform(0.0, 1.0, (H, W, CHANNELS))


def feature_sums(fmean, fsig, fjit, n_img, f_nan=None, g_inf=None):
    """F, G: the sums and sums of squares of n_img samples of feature_means' features; a NaN in F at the pixels of f_nan, an infinite G at those of g_inf."""
    n = np.maximum(n_img, 0).astype(np.float64)[..., None]
    F = fmean * n
    G = F * fmean + fjit * fsig * fsig * np.maximum(n - 1.0, 0.0)
    if f_nan is not None:
        F[f_nan, 1] = np.nan
    if g_inf is not None:
        G[g_inf, 5] = np.inf
    return F, G


def block_counts(rng, W, H, tw=8, th=16, lo=2, hi=65):
    """One count from [lo, hi) per tw x th block of the frame."""
    by, bx = -(-H // th), -(-W // tw)
    return np.kron(rng.integers(lo, hi, (by, bx)), np.ones((th, tw), dtype=np.int64))[:H, :W]


def rects_of(n_a, n_b, n_f):
    """The frame as rects over which all three counts are constant: the runs of each row.  A run at 0 in all three is a rect at count 0 on an even row
    and left uncovered on an odd one (both are n = 0 to the kernels).  -> rects, counts_a, counts_b, counts_f"""
    H, W = n_a.shape
    rects, ca, cb, cf = [], [], [], []
    key = np.stack([n_a, n_b, n_f], axis=-1)
    for y in range(H):
        x = 0
        while x < W:
            e = x + 1
            while e < W and (key[y, e] == key[y, x]).all():
                e += 1
            if key[y, x].any() or y % 2 == 0:
                rects.append((x, y, e - x, 1))
                ca.append(int(n_a[y, x])), cb.append(int(n_b[y, x])), cf.append(int(n_f[y, x]))
            x = e
    return rects, ca, cb, cf


class Frame:
    """One frame of a class.  halves = (S_a, Q_a, S_b, Q_b); F, G with their own counts n_f for the dual guided calls; single_features() for the
    single-buffer guided calls, whose features share half A's counts.  k, alpha: the colour parameters the class is meant for."""

    def __init__(self, name, halves, n_a, n_b, fmean, fsig, fjit, n_f, f_nan=None, g_inf=None, k=0.45, alpha=1.0, note=None):
        self.name, self.halves, self.k, self.alpha, self.note = name, tuple(halves), float(k), float(alpha), note or {}
        self.n_a, self.n_b, self.n_f = (np.asarray(n, dtype=np.int64) for n in (n_a, n_b, n_f))
        self.H, self.W = self.n_a.shape
        self._f = (fmean, fsig, fjit, np.zeros((self.H, self.W), bool) if f_nan is None else f_nan, np.zeros((self.H, self.W), bool) if g_inf is None else g_inf)
        self.rects, self.counts_a, self.counts_b, self.counts_f = rects_of(self.n_a, self.n_b, self.n_f)
        self.F, self.G = self._features(self.n_f)

    def _features(self, n_img):
        return feature_sums(*self._f[:3], n_img, self._f[3], self._f[4])

    def single(self):
        """-> S, Q, rects, counts, n: half A alone."""
        return self.halves[0], self.halves[1], self.rects, self.counts_a, self.n_a

    def single_features(self):
        """The features as sums of half A's own counts (rmd_denoise_guided and rmd_denoise_atrous read them at the frame's counts)."""
        return self._features(self.n_a)

    def valid(self):
        """-> valid_a, valid_b, dual"""
        ok_a = mean_and_variance(self.halves[0], self.halves[1], self.n_a)[2]
        ok_b = mean_and_variance(self.halves[2], self.halves[3], self.n_b)[2]
        return ok_a, ok_b, ok_a & ok_b

    def crop(self, x0, y0, w, h):
        """The frame cut to the w x h pixels at (x0, y0): small enough for the pixel-by-pixel readings."""
        sl = (slice(y0, y0 + h), slice(x0, x0 + w))
        return Frame("%s[%d:%d,%d:%d]" % (self.name, y0, y0 + h, x0, x0 + w), [a[sl].copy() for a in self.halves], self.n_a[sl], self.n_b[sl],
                     *(a[sl].copy() for a in self._f[:3]), self.n_f[sl], self._f[3][sl].copy(), self._f[4][sl].copy(), self.k, self.alpha, self.note)


def _seed(name):
    return zlib.crc32(name.encode())


def _plain(name, W, H, floor=False):
    """The content every class starts from: two independent halves over block counts of their own (all >= 2), features at a third set of counts."""
    rng = np.random.default_rng(_seed(name))
    n_a, n_b, n_f = block_counts(rng, W, H), block_counts(rng, W, H), block_counts(rng, W, H, 16, 8, hi=100)
    S_a, Q_a = moments(rng, n_a, floor)
    S_b, Q_b = moments(rng, n_b, floor)
    return rng, [S_a, Q_a, S_b, Q_b], n_a, n_b, n_f, feature_means(rng, W, H)


# ---------------------------------------------------------------- shape_*
def _shape(name, W, H):
    rng, halves, n_a, n_b, n_f, feats = _plain(name, W, H)
    if W * H >= 64:  # _two_halves-style: a block at 1 and a block at 0 in each half and in the features, at different places
        for n, (y, x) in ((n_a, (0, 8)), (n_b, (0, 16)), (n_f, (H - 1, W - 1))):
            n[n == n[min(y, H - 1), min(x, W - 1)]] = 1
        n_a[n_a == n_a[H - 1, 0]] = 0
        n_b[n_b == n_b[H // 2, W // 2]] = 0
    if W * H > 4:
        poison(halves[0], halves[1], rng)
        poison(halves[2], halves[3], rng)
    return Frame(name, halves, n_a, n_b, *feats, n_f)


# ---------------------------------------------------------------- seam_*
def _patterns(W, H):
    """name -> (H, W) mask of the pixels made invalid."""
    y, x = np.mgrid[0:H, 0:W]
    ry, rx = RING_PIXEL
    ring = (np.maximum(np.abs(y - ry), np.abs(x - rx)) <= RING_DEPTH) & ((y != ry) | (x != rx))
    one_in = np.ones((H, W), bool)
    one_in[H // 2, W // 2 + 5] = False
    one_corner = np.ones((H, W), bool)
    one_corner[H - 1, W - 1] = False
    return {"columns": np.isin(x, (23, 24, 31, 32)), "row": np.isin(y, (15, 16)), "border": (x == 0) | (x == W - 1) | (y == 0) | (y == H - 1),
            "tile": (x < 32) & (y < 16), "all": np.ones((H, W), bool), "one_inside": one_in, "one_corner": one_corner, "checker": (x + y) % 2 == 1, "ring": ring}


PATTERNS = tuple(_patterns(*SEAM))
VARIANTS = ("a", "b", "ab", "f")  # the pattern in half A only, in half B only, in A and (mirrored) in B, in the features only


def _invalidate(S, Q, n, mask):
    """Each pixel of the mask by one route, in turn along the raster: n = 0 (the sums stay: S / 0), n = 1, a NaN in S, an infinite Q."""
    route = (np.cumsum(mask.ravel()).reshape(mask.shape) - 1) % 4
    n[mask & (route == 0)] = 0
    n[mask & (route == 1)] = 1
    S[mask & (route == 2), 1] = np.nan
    Q[mask & (route == 3), 2] = np.inf


def _seam(name, pattern, variant):
    W, H = SEAM
    rng, halves, n_a, n_b, n_f, feats = _plain(name, W, H)
    mask = _patterns(W, H)[pattern]
    f_nan = g_inf = None
    if variant in ("a", "ab"):
        _invalidate(halves[0], halves[1], n_a, mask)
    if variant in ("b", "ab"):
        _invalidate(halves[2], halves[3], n_b, mask[::-1, ::-1] if variant == "ab" else mask)
    if variant == "f":
        route = (np.cumsum(mask.ravel()).reshape(mask.shape) - 1) % 4
        n_f[mask & (route == 0)] = 0
        n_f[mask & (route == 1)] = 1
        f_nan, g_inf = mask & (route == 2), mask & (route == 3)
    return Frame(name, halves, n_a, n_b, *feats, n_f, f_nan, g_inf, note=dict(mask=mask, pattern=pattern, variant=variant))


# ---------------------------------------------------------------- scale_*
def _scaled(halves, s):
    return [a * (s if i % 2 == 0 else s * s) for i, a in enumerate(halves)]


def _scale(name, kind):
    W, H = SEAM
    rng, halves, n_a, n_b, n_f, feats = _plain(name, W, H, floor=True)
    k = 0.45
    if isinstance(kind, int):
        halves = _scaled(halves, 2.0**kind)
    elif kind == "mixed":  # the left half at 2^200, the right half at 2^-200
        left, right = _scaled(halves, 2.0**200), _scaled(halves, 2.0**-200)
        halves = [np.concatenate([l[:, : W // 2], r[:, W // 2 :]], axis=1) for l, r in zip(left, right)]
    elif kind == "overflow":
        # Channel 0 is +a left of the middle column and -a right of it, a = 2^511: du = 2^512 and (du)^2 = 2^1024 overflows across the middle.  At n = 2 and
        # Q = 1.9 * 2^1023 the variance of the mean is 0.9 * 2^1022, so with k = 2 the denominator eps + k^2 (v + v) = 1.8 * 2^1024 overflows as well:
        # the term is inf / inf = NaN, D is NaN, and D > 0 ? D : 0 makes the weight exp(-0) = 1.  Channels 1 and 2 keep the _moments content.
        k = 2.0
        n_a[:], n_b[:] = 2, 2
        S_a, Q_a = moments(rng, n_a, True)
        S_b, Q_b = moments(rng, n_b, True)
        a = np.where(np.arange(W) < W // 2, 1.0, -1.0)[None, :] * 2.0**511 + np.zeros((H, 1))
        for S, Q in ((S_a, Q_a), (S_b, Q_b)):
            S[..., 0], Q[..., 0] = 2.0 * a, 1.9 * 2.0**1023
        halves = [S_a, Q_a, S_b, Q_b]
    elif kind == "flat":  # a dyadic constant with Q = S^2 / n exactly: v = 0, every difference 0, every weight 1
        n_a[:], n_b[:] = 8, 4
        halves = [np.full((H, W, 3), 0.75 * 8), np.full((H, W, 3), 0.75 * 0.75 * 8), np.full((H, W, 3), 0.75 * 4), np.full((H, W, 3), 0.75 * 0.75 * 4)]
    elif kind == "negative":  # the means below zero: S - 2 n, Q + (-4 S + 4 n) leaves every sample's deviation as it was
        for S, Q, n in ((halves[0], halves[1], n_a), (halves[2], halves[3], n_b)):
            nd = n.astype(np.float64)[..., None]
            Q += -4.0 * S + 4.0 * nd
            S -= 2.0 * nd
    elif kind == "cancel":  # Q slightly under S^2 / n: t < 0 everywhere, clamped to v = 0
        for S, Q, n in ((halves[0], halves[1], n_a), (halves[2], halves[3], n_b)):
            Q[:] = S * (S / n.astype(np.float64)[..., None]) * (1.0 - 2.0**-30)
    elif kind == "counts":  # columns in thirds: 2 | 2^32 - 1 | 3 samples in half A (2 beside 2^32 - 1, 2^32 - 1 beside 3), 3 | 2 | 2^32 - 1 in half B
        third = np.minimum(np.arange(W) * 3 // W, 2)[None, :] + np.zeros((H, 1), dtype=np.int64)
        n_a, n_b = np.choose(third, (2, UINT32_MAX, 3)), np.choose(third, (3, 2, UINT32_MAX))
        n_f = np.choose(third, (UINT32_MAX, 3, 2))
        S_a, Q_a = moments(rng, n_a, True)
        S_b, Q_b = moments(rng, n_b, True)
        halves = [S_a, Q_a, S_b, Q_b]
    else:
        raise KeyError(kind)
    return Frame(name, halves, n_a, n_b, *feats, n_f, k=k, note=dict(kind=kind))


def _scale_name(kind):
    return "scale_%s" % (("2p%d" % kind if kind > 0 else "2m%d" % -kind) if isinstance(kind, int) else kind)


CLASSES = {}
for _W, _H in SHAPES:
    CLASSES["shape_%dx%d" % (_W, _H)] = (_shape, (_W, _H))
for _p in PATTERNS:
    for _v in VARIANTS:
        CLASSES["seam_%s_%s" % (_p, _v)] = (_seam, (_p, _v))
for _k in SCALES + ("overflow", "mixed", "flat", "negative", "cancel", "counts"):
    CLASSES[_scale_name(_k)] = (_scale, (_k,))

_CACHE = {}


def frame(name):
    """The class's frame (built once; treat it as read-only)."""
    if name not in _CACHE:
        make, args = CLASSES[name]
        _CACHE[name] = make(name, *args)
    return _CACHE[name]


def names(prefix):
    return [n for n in CLASSES if n.startswith(prefix)]


# ---------------------------------------------------------------- region_*
def region_sets(W=SEAM[0], H=SEAM[1], invalid=None, seed=5):
    """name -> a list of pairwise disjoint rects.  `invalid`: an (H, W) mask; region_invalid_only is the largest rect inside its first run of rows."""
    rng = np.random.default_rng(seed)
    sets = {"region_seam_columns": [(x, 0, 1, H) for x in (23, 24, 31, 32) if x < W],
            "region_beside_columns": [(x, 0, 1, H) for x in (22, 25, 30, 33) if x < W],
            "region_seam_rows": [(0, y, W, 1) for y in (15, 16) if y < H],
            "region_beside_rows": [(0, y, W, 1) for y in (14, 17) if y < H],
            "region_last_column": [(W - 1, 0, 1, H)]}
    cells = rng.permutation(W * H)[: min(200, W * H)]
    sets["region_single_pixels"] = [(int(c % W), int(c // W), 1, 1) for c in cells]
    if invalid is not None:
        ys, xs = np.nonzero(invalid)
        y0, x0 = int(ys[0]), int(xs[0])
        w = 1
        while x0 + w < W and invalid[y0, x0 + w]:
            w += 1
        h = 1
        while y0 + h < H and invalid[y0 + h, x0 : x0 + w].all():
            h += 1
        sets["region_invalid_only"] = [(x0, y0, w, h)]
    return sets


# ---------------------------------------------------------------- the comparison bar
def local_scale(us, valid, reach):
    """Per pixel and channel: the largest finite |u_q| over the valid pixels q of the (2 reach + 1)^2 window around the pixel, over every (H, W, 3) array
    of `us`.  An output pixel is a weighted mean of exactly those values."""
    H, W = valid.shape
    m = np.zeros((H, W, 3))
    for u in us:
        a = np.abs(u)
        m = np.maximum(m, np.where(valid[..., None] & np.isfinite(a), a, 0.0))
    reach = int(min(reach, max(H, W)))
    for axis, size in ((0, H), (1, W)):
        out = m.copy()
        for d in range(1, reach + 1):
            if d >= size:
                break
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, size - d), slice(d, size)
            out[tuple(lo)] = np.maximum(out[tuple(lo)], m[tuple(hi)])
            out[tuple(hi)] = np.maximum(out[tuple(hi)], m[tuple(lo)])
        m = out
    return m


def differences(dev, ref, scale):
    """-> (number of values outside the bar, the worst relative difference among the finite ones, |ref| / scale where that one lies: how far the mean there
    has cancelled against the values it is a mean of).  The bar: NaN exactly where `ref` has NaN, infinities equal, every finite value within
    1e-9 |ref| + 1e-12 scale (scale: local_scale's array, or anything that broadcasts)."""
    dev, ref = np.asarray(dev), np.asarray(ref)
    fin = np.isfinite(ref)
    bad = int((np.isnan(dev) != np.isnan(ref)).sum())
    inf = ~fin & ~np.isnan(ref)
    with np.errstate(all="ignore"):
        bad += int((dev[inf] != ref[inf]).sum())
        err = np.where(fin, np.abs(dev - ref), 0.0)
        sc = np.broadcast_to(scale, ref.shape)
        tol = 1e-9 * np.abs(ref) + 1e-12 * sc
        out = fin & ~np.isnan(dev) & ~(err <= tol)  # (a dev NaN is counted above; a dev inf against a finite ref is outside)
        rel = np.nan_to_num(np.where(fin & (ref != 0.0), err / np.abs(ref), 0.0), nan=0.0, posinf=np.inf)
        if not rel.size:
            return bad, 0.0, 1.0
        at = np.unravel_index(np.argmax(rel), rel.shape)
        share = float(np.abs(ref[at]) / sc[at]) if sc[at] > 0.0 else 1.0
    return bad + int(out.sum()), float(rel[at]), share


def agree(dev, ref, scale, what=""):
    """Asserts the bar -> (the worst relative difference, |ref| / scale where it lies)."""
    bad, worst, share = differences(dev, ref, scale)
    assert bad == 0, "%s: %d values outside the bar, worst relative difference %.3g" % (what, bad, worst)
    return worst, share


def err_scale(scale):
    """The scale of the dual calls' err = mean_c h_c^2, h_c = (f_Ac - f_Bc) / 2: mean_c scale_c^2 of local_scale's array.  |h_c| <= scale_c, since both
    filtered values are means of values no larger than scale_c, so err <= err_scale; and the bar above already lets each filtered value move by
    1e-12 scale_c, which moves err by up to 2 |h_c| 1e-12 scale_c per channel — 1e-12 err_scale asks no less of err than the bar asks of the frame."""
    with np.errstate(all="ignore"):
        return (scale[..., 0] * scale[..., 0] + scale[..., 1] * scale[..., 1] + scale[..., 2] * scale[..., 2]) / 3.0


def agree_err(err, err_ref, dual, scale, what=""):
    """err of rmd_denoise_dual and its guided, slope and select forms: the same bar as the frame — 1e-9 relative, NaN exactly at the pixels that are not
    dual-valid — with 1e-12 err_scale(scale) as the absolute allowance."""
    assert np.array_equal(np.isnan(err), ~dual), "%s: err is NaN at other pixels than those not dual-valid" % what
    return agree(err, err_ref, err_scale(scale), what + " (err)")


def agree_err_propagated(err, f_a, f_b, dual, scale, what=""):
    """err of the a-trous dual calls, as their own file holds it (test_gpu_denoise_atrous_dual._agree_err's reasoning with the local scale), against the
    restatement's filtered halves.  Each filtered value may be off by
    d = 1e-9 |f| + 1e-12 scale (the bar above), h_c then by t_c = (d_Ac + d_Bc) / 2 and err by mean_c (2 |h_c| t_c + t_c^2); 1e-9 err is added for the
    operations of err itself.  NaN exactly where the pixel is not dual-valid."""
    assert np.array_equal(np.isnan(err), ~dual), "%s: err is NaN at other pixels than those not dual-valid" % what
    if not dual.any():
        return 0.0
    with np.errstate(all="ignore"):
        fa, fb, sc = f_a[dual], f_b[dual], np.broadcast_to(scale, f_a.shape)[dual]
        t = ((1e-9 * np.abs(fa) + 1e-12 * sc) + (1e-9 * np.abs(fb) + 1e-12 * sc)) / 2.0
        h = (fa - fb) / 2.0
        ref = (h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1] + h[:, 2] * h[:, 2]) / 3.0
        tol = (2.0 * np.abs(h) * t + t * t).sum(axis=1) / 3.0 + 1e-9 * ref
        diff = np.abs(err[dual] - ref)
        same = (err[dual] == ref) | (np.isnan(ref) & np.isnan(err[dual]))  # (an overflowing h^2 is inf in both)
        bad = ~same & ~(diff <= tol)
        of_tol = np.where(bad, diff / tol, 0.0)
        rel = np.where(same | (ref == 0.0), 0.0, diff / np.abs(ref))
    assert not bad.any(), "%s: %d err values differ, worst %.3g of its tolerance" % (what, bad.sum(), np.nanmax(of_tol))
    return float(np.nanmax(rel))
