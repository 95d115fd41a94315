"""The frames and rect lists tests/test_gpu_tile_error.py sends to rmd_tile_error and rmd_tile_error_dual, seeded and made once;
tests/test_tile_error_host.py checks on the CPU that each class is what it names.

Frames are 67 x 45 (odd width, rows that are no multiple of 64), and 300 x 300 for the long shapes.  Every (S, Q) case carries the sample count and the floor
it is made for.  The err classes that cancel (`chain`, `pairs`) plant their values per rect, in rects that do not overlap, and come with that list alone: the
header does not say what a negative total gives, so no rect may gather cancelling values it was not made for."""
import functools
from collections import namedtuple

import numpy as np

from raymond_amd.scene import generate_tiles

W, H = 67, 45
WIDE = 300
FLOOR = 1e-3

TILE = (3, 5, 32, 32)  # a 32 x 32 tile at an odd offset: 1,024 pixels, four a lane
RAGGED = [r for r in generate_tiles(W, H, (32, 32)) if r[2] < 32 or r[3] < 32]  # the right and bottom tiles of the frame's own tiling
RECTS = (
    [(10, 20, 0, 5)]                                                       # without pixels, at the front
    + [(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1)]  # lane 0 alone, at the four corners
    + [(2, 3, 51, 5), (30, 10, 32, 8), (1, 20, 32, 16), (40, 1, 27, 19)]   # 255, 256, 512 and 513 pixels
    + [(7, 0, 1, H), (0, 9, W, 1)]                                         # a column and a row
    + [(W, H, 0, 0)]                                                       # without pixels, in the middle and at the frame's far corner
    + [TILE]
    + RAGGED
    + [(8, 8, 20, 12), (18, 14, 20, 12)]                                   # two that overlap
    + [(0, 0, W, H)]                                                       # the whole frame: chains of 12
    + [(5, 5, 3, 0)]                                                       # without pixels, at the end
)
EMPTY = [j for j, r in enumerate(RECTS) if r[2] * r[3] == 0]
# the 300 x 300 frame: 257 and 511 pixels (a prime, and 7 x 73), a rect wider than 256, the long row and column, the whole frame (90,000 pixels, chains of 352)
WIDE_RECTS = [(20, 3, 257, 1), (100, 50, 73, 7), (5, 100, 270, 3), (0, 7, WIDE, 1), (11, 0, 1, WIDE), (0, 0, 0, 0), (0, 0, WIDE, WIDE), (299, 299, 1, 1)]
PLANT_RECTS = [TILE, (40, 1, 27, 19)]  # planted(): a width that is a power of two and one that is not
PLANT_INDICES = (0, 63, 64, 127, 128, 255, 256, 257, -1)  # each wave, each end of a wave, the second trip of lanes 0 and 1, the last pixel

Case = namedtuple("Case", "name S Q n floor")


def pixel_of(rect, index):
    """(x, y) of the pixel with row-major `index` in `rect` (-1: its last)."""
    l, t, w, h = rect
    index = index % (w * h)
    return l + index % w, t + index // w


def mean_to_sum(p, n):
    """A sum s with fl(s / n) == p, searched among the doubles around p * n; raises if there is none."""
    p, nd = np.float64(p), np.float64(n)
    lo = hi = p * nd
    cands = [lo]
    for _ in range(8):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        cands += [lo, hi]
    for s in cands:
        if s / nd == p:
            return float(s)
    raise ValueError("no sum gives the mean %r at n = %d" % (p, n))


# ---------------------------------------------------------------- (S, Q) for rmd_tile_error
@functools.lru_cache(maxsize=None)
def _samples(width, height):
    rng = np.random.default_rng(11)
    return rng.exponential(0.3, (64, height, width, 3)) * (rng.uniform(size=(64, height, width, 1)) < 0.7)


def random_sums(n, width=W, height=H):
    """tests/test_gpu_moments.py's frame: the sums of min(n, 64) samples (64 for n = 0), scaled by a power of two above 64 so that m stays in range; with its
    black block, its pixel that rounds below zero and its pixel below the floor."""
    L = _samples(width, height)
    k = min(n, 64) if n else 64
    S, Q = L[:k].sum(axis=0), (L[:k] * L[:k]).sum(axis=0)
    scale = 2.0 ** max(0, int(np.floor(np.log2(max(n, 1) / 64.0))))
    S, Q = S * scale, Q * scale
    nn = float(max(n, 1))
    S[0:4, 20:30] = 0.0
    Q[0:4, 20:30] = 0.0
    S[6, 4] = (3.0, 0.0, 1e-9)
    Q[6, 4] = (3.0 * 3.0 / nn * (1.0 - 4e-16), 0.0, 1e-18 / nn * (1.0 - 4e-16))
    S[40, 50] = (1e-7, 2e-7, 5e-6)
    return S, Q


COUNTS = (0, 1, 2, 3, 64, 2**24 + 1, 2**32 - 1)
CLAMP_N, TINY_N, HUGE_N, NEGATIVE_N, QUIET_N = 7, 4, 4, 5, 8
FLOOR_EDGES = ((64, 0.25), (3, 0.75), (64, 2.0**-10))  # floor * n exact, and fl(S / n) reaches the floor's two neighbours


def kinds(k, width=W, height=H):
    """(x + y) % k per pixel: which kind of a class's pixels each one is."""
    ys, xs = np.mgrid[0:height, 0:width]
    return (xs + ys) % k


def clamp_frame():
    """Kind 0: Q = fl(S * fl(S / n)) exactly, v == 0.  Kind 1: Q one ulp below, v < 0 before the clamp.  Kind 2: Q one ulp above, v tiny and positive."""
    rng = np.random.default_rng(21)
    S = rng.uniform(0.5, 4.0, (H, W, 3)) * CLAMP_N
    Q0 = S * (S / np.float64(CLAMP_N))
    kind = kinds(3)[..., None]
    Q = np.where(kind == 0, Q0, np.where(kind == 1, np.nextafter(Q0, 0.0), np.nextafter(Q0, np.inf)))
    return S, Q


def floor_edge_frame(n, floor):
    """|m| == floor (kind 0), one ulp below (1) and above (2), S > 0 in even rows and < 0 in odd ones; Q = 1.5 S^2 / n leaves a positive variance."""
    targets = [floor, float(np.nextafter(floor, 0.0)), float(np.nextafter(floor, np.inf))]
    sums = np.array([mean_to_sum(p, n) for p in targets])
    ys = np.mgrid[0:H, 0:W][0]
    S = (sums[kinds(3)] * np.where(ys % 2 == 0, 1.0, -1.0))[..., None] * np.ones(3)
    Q = S * S / np.float64(n) * 1.5
    return S, Q


def tiny_frame():
    """Kind 0: S near 1e-155, so that S*m, Q, v and v / n are subnormal.  Kind 1: S subnormal, Q near 1e-300.  Kind 2: S near 1e-300, Q subnormal."""
    rng = np.random.default_rng(22)
    u = rng.uniform(0.5, 2.0, (2, H, W, 3))
    kind = kinds(3)[..., None]
    S0 = u[0] * 1e-155
    with np.errstate(under="ignore"):
        Q0 = S0 * S0 / np.float64(TINY_N) * 1.5
    S = np.where(kind == 0, S0, np.where(kind == 1, u[0] * 1e-310, u[0] * 1e-300))
    Q = np.where(kind == 0, Q0, np.where(kind == 1, u[1] * 1e-300, u[1] * 1e-315))
    return S, Q


def huge_frame():
    """Kind 0: S near +-1e200, Q near 1e300: S*m overflows, v is -inf and clamped, the error 0.  Kind 1: S near 1, Q near 1e308: large and finite."""
    rng = np.random.default_rng(23)
    u = rng.uniform(0.5, 1.7, (2, H, W, 3))
    kind = kinds(2)[..., None]
    sign = np.where(kinds(4)[..., None] < 2, 1.0, -1.0)
    S = np.where(kind == 0, sign * u[0] * 1e200, u[0])
    Q = np.where(kind == 0, u[1] * 1e300, u[1] * 1e308)
    return S, Q


def negative_frame():
    """Kind 0: S < 0, Q > 0.  Kind 1: S > 0, Q < 0.  Kind 2: both negative.  Kind 3: S = -0.0, Q > 0.  Kind 4: S > 0, Q = -0.0.
    (S = +-0 with Q = -0.0 gives v = -0.0, which is not negative: its root is -0.0, a zero whose sign the header leaves open.  Three pixels carry that
    pair in channel 0 only, next to two channels with a positive error.)"""
    rng = np.random.default_rng(24)
    u = rng.uniform(0.5, 2.0, (H, W, 3)) * NEGATIVE_N
    q = u * u / np.float64(NEGATIVE_N) * 1.5
    kind = kinds(5)[..., None]
    S = np.where((kind == 0) | (kind == 2), -u, np.where(kind == 3, -0.0, u))
    Q = np.where((kind == 1) | (kind == 2), -q, np.where(kind == 4, -0.0, q))
    for (x, y), s0 in zip(((4, 6), (35, 20), (66, 44)), (0.0, -0.0, 0.0)):
        S[y, x], Q[y, x] = u[y, x], q[y, x]
        S[y, x, 0], Q[y, x, 0] = s0, -0.0
    return S, Q


def quiet_frame(width=W, height=H):
    """Every pixel's relative error between 0.0037 and 0.0054 at QUIET_N samples (sqrt(d / (n - 1)), d in 1e-4 .. 2e-4)."""
    rng = np.random.default_rng(25)
    S = rng.uniform(0.5, 1.0, (height, width, 3)) * QUIET_N
    Q = S * S / np.float64(QUIET_N) * (1.0 + 1e-4 * rng.uniform(1.0, 2.0, (height, width, 3)))
    return S, Q


def planted(S, Q, rect, index):
    """A copy of the quiet (S, Q) in which the pixel with row-major `index` of `rect` has Q = S^2: a relative error near 1."""
    x, y = pixel_of(rect, index)
    S2, Q2 = S.copy(), Q.copy()
    Q2[y, x] = S[y, x] * S[y, x]
    return S2, Q2


# specials: each value alone in an otherwise quiet rect, at the rect's pixel 0, its last pixel and its index 256 — the first and last pixels of lane 0's chain
SPECIAL_RECTS = [((0, 0, 20, 15), 0), ((25, 0, 20, 15), -1), ((0, 20, 20, 15), 256)]
SPECIAL_VALUES = (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf))


def special_frame(value, in_q, channel):
    S, Q = (a.copy() for a in quiet_frame())
    for rect, index in SPECIAL_RECTS:
        x, y = pixel_of(rect, index)
        (Q if in_q else S)[y, x, channel] = value
    return S, Q


def special_rects():
    return [r for r, _ in SPECIAL_RECTS] + RECTS


@functools.lru_cache(maxsize=None)
def cases():
    """Every (S, Q) case on the 67 x 45 frame, as Case(name, S, Q, n, floor); a name begins with its class."""
    out = [Case("random/n=%d" % n, *random_sums(n), n, FLOOR) for n in COUNTS]
    out.append(Case("random/n=64/floor=0.25", *random_sums(64), 64, 0.25))
    out.append(Case("clamp", *clamp_frame(), CLAMP_N, FLOOR))
    out += [Case("floor_edge/n=%d/floor=%r" % (n, f), *floor_edge_frame(n, f), n, f) for n, f in FLOOR_EDGES]
    out.append(Case("tiny", *tiny_frame(), TINY_N, FLOOR))
    out.append(Case("huge", *huge_frame(), HUGE_N, FLOOR))
    out.append(Case("negative", *negative_frame(), NEGATIVE_N, FLOOR))
    out.append(Case("quiet", *quiet_frame(), QUIET_N, FLOOR))
    for label, value in SPECIAL_VALUES:
        for in_q in (False, True):
            for c in range(3):
                out.append(Case("specials/%s/%s/%d" % (label, "Q" if in_q else "S", c), *special_frame(value, in_q, c), QUIET_N, FLOOR))
    for c in out:
        c.S.setflags(write=False), c.Q.setflags(write=False)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def case_rects(c):
    return special_rects() if c.name.startswith("specials") else RECTS


@functools.lru_cache(maxsize=None)
def wide_case():
    S, Q = random_sums(64, WIDE, WIDE)
    S.setflags(write=False), Q.setflags(write=False)
    return Case("wide/random/n=64", S, Q, 64, FLOOR)


# ---------------------------------------------------------------- err images for rmd_tile_error_dual
ErrCase = namedtuple("ErrCase", "name err rects designated")  # designated: the indices of the rects the cancelling values are planted in (None: no such values)
BIG, BIGGER = 2.0**60, 2.0**70


def background(width=W, height=H, seed=31):
    return np.random.default_rng(seed).exponential(1e-3, (height, width))


def put(err, rect, index, value):
    x, y = pixel_of(rect, index)
    err[y, x] = value


def plant_chain(err, rect, lane, trip=0):
    """+2^60, 1, -2^60 at three successive places of `lane`'s chain, from its trip `trip`: the 1 is absorbed, and the sum returns to where it was."""
    for k, v in enumerate((BIG, 1.0, -BIG)):
        put(err, rect, lane + 256 * (trip + k), v)


def plant_pair(err, rect, plus, minus):
    """+2^70 and -2^70 at two row-major indices: each swallows whatever is added to it until the two meet."""
    put(err, rect, plus, BIGGER)
    put(err, rect, minus, -BIGGER)


CHAIN_RECTS = [(0, 0, 40, 30), (40, 0, 27, 45)]  # 1,200 and 1,215 pixels: chains of four and five
CHAIN_LANES = [(0, 5, 63), (64, 200, 255)]
PAIR_RECTS = [(0, 0, 33, 20), (33, 0, 34, 20), (0, 20, 67, 25)]
WIDE_CHAIN_RECT = (0, 0, WIDE, 100)  # chains of 117: room for several triples down one lane's chain


def chain_image():
    err = background()
    for rect, lanes, pair in zip(CHAIN_RECTS, CHAIN_LANES, ((17, 49), (130, 162))):
        for lane in lanes:
            plant_chain(err, rect, lane)
        plant_pair(err, rect, pair[0] + 768, pair[1] + 768)  # lanes 32 apart, in their fourth trip
    return err


def pairs_image():
    err = background()
    plant_pair(err, PAIR_RECTS[0], 7, (7 ^ 32) + 256)      # lanes t and t ^ 32: they meet in the first halving step
    plant_pair(err, PAIR_RECTS[1], 100, (100 ^ 1) + 256)   # lanes t and t ^ 1: they meet in the last one, after each has swallowed half its wave
    # wave 0 and wave 2 meet in the very last addition, which no order within a wave changes.  So wave 0's half is the negative one, and its wave also holds
    # +-2^130 in lanes 12 and 13: in the header's order lane 12 has gathered every even lane of its wave, the -2^70 among them, before it meets lane 13, and
    # the total is wave 2's +2^70; a sum that lets 12 and 13 meet first keeps the -2^70 and ends at 0
    plant_pair(err, PAIR_RECTS[2], 128 + 10, 10 + 256)
    put(err,PAIR_RECTS[2], 12, 2.0**130)
    put(err, PAIR_RECTS[2], 13 + 512, -(2.0**130))
    return err


def wide_chain_image():
    err = background(WIDE, WIDE, seed=32)
    for trip in (0, 3, 6, 60):
        plant_chain(err, WIDE_CHAIN_RECT, 5, trip)
    plant_chain(err, WIDE_CHAIN_RECT, 255, 100)
    plant_pair(err, WIDE_CHAIN_RECT, 20 + 256 * 50, (20 ^ 32) + 256 * 7)
    return err


def absorb_image():
    """Ones, with a 2^53 at the first pixel of every fifth row of the frame and of TILE: 2^53 + 1 rounds back to 2^53."""
    err = np.ones((H, W))
    err[0::5, 0] = 2.0**53
    err[TILE[1] : TILE[1] + TILE[3] : 5, TILE[0]] = 2.0**53
    return err


def nan_image(index):
    err = background()
    put(err, TILE, index, np.nan)
    return err


def inf_image():
    err = background()
    err[10, 10] = np.inf
    return err


def zeros_image():
    return np.where(kinds(2) == 0, 0.0, -0.0)


@functools.lru_cache(maxsize=None)
def err_cases():
    out = [
        ErrCase("positive", np.random.default_rng(30).exponential(1.0, (H, W)), RECTS, None),
        ErrCase("chain", chain_image(), [(0, 0, 0, 0)] + CHAIN_RECTS, [1, 2]),
        ErrCase("pairs", pairs_image(), PAIR_RECTS + [(5, 5, 0, 0)], [0, 1, 2]),
        ErrCase("absorb", absorb_image(), RECTS, None),
        ErrCase("nan/0", nan_image(0), RECTS, None),
        ErrCase("nan/last", nan_image(-1), RECTS, None),
        ErrCase("nan/256", nan_image(256), RECTS, None),
        ErrCase("inf", inf_image(), RECTS, None),
        ErrCase("zeros", zeros_image(), RECTS, None),
    ]
    for c in out:
        c.err.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def wide_err_cases():
    out = [
        ErrCase("wide/positive", np.random.default_rng(33).exponential(1.0, (WIDE, WIDE)), WIDE_RECTS, None),
        ErrCase("wide/chain", wide_chain_image(), [WIDE_CHAIN_RECT], [0]),
    ]
    for c in out:
        c.err.setflags(write=False)
    return tuple(out)


def err_case(name):
    return next(c for c in err_cases() + wide_err_cases() if c.name == name)


# rects whose total / pixels is the exact square of a small dyadic number: (rect, the result)
EXACT_RECTS = [((2, 3, 51, 5), 2.0), ((1, 10, 64, 9), 0.75), ((0, 20, 32, 24), 0.5)]


def exact_image():
    """255 pixels of 4 (total 1,020, mean 4); 576 of 9/16 (every partial sum a multiple of 1/16); and 768 pixels, three a lane, where every fourth lane holds
    +2^60, 1, -2^60 and the others 0, 1, 0: the header's order leaves 192 — mean 1/4 — of an exact sum of 256."""
    err = np.zeros((H, W))
    (l, t, w, h), _ = EXACT_RECTS[0]
    err[t : t + h, l : l + w] = 4.0
    (l, t, w, h), _ = EXACT_RECTS[1]
    err[t : t + h, l : l + w] = 0.5625
    rect = EXACT_RECTS[2][0]
    for lane in range(256):
        if lane % 4 == 3:
            plant_chain(err, rect, lane)
        else:
            put(err, rect, lane + 256, 1.0)
    return err
