"""Frames for the rmd_despike_dual tests, over tests/despike_frames.py's helpers: the rect layout with its four count pairs, the random frames the mirror and
the device are held to tests/despike_dual_ref.py on, the hand-made ones, and one shared cache of the restatement's results.  No GPU, no library."""
import functools

import numpy as np

import despike_dual_ref
from despike_frames import S2, sums_of

SIZES = ((1, 1), (3, 2), (37, 21), (131, 70))
RADII = (1, 2, 3)


def ranks(radius):
    return (0, 2, (2 * radius + 1) ** 2 - 2)


def layout(width, height):
    """The rects and their (n_A, n_B): the quadrants of the covered part at (8, 8), (8, 16), (1, 1) and (8, 8) — so (8, 8) | (8, 16) and (8, 8) / (1, 1) are
    neighbours with different counts: a donor across the first edge is bit-copied in half A and scaled in half B —, a strip under them at (0, 8) (from 3 rows
    on) and an uncovered strip on the right (from 3 columns on).  Rects without pixels stay in the list: they cover nothing."""
    strip = max(1, width // 8) if width >= 3 else 0
    low = max(1, height // 8) if height >= 3 else 0
    cw, ch = width - strip, height - low
    mx, my = cw // 2, ch // 2
    rects = [(0, 0, mx, my), (mx, 0, cw - mx, my), (0, my, mx, ch - my), (mx, my, cw - mx, ch - my), (0, ch, cw, low)]
    return rects, [8, 8, 1, 8, 0], [8, 16, 1, 8, 8]


def count_planes(width, height, rects, counts_a, counts_b):
    na, nb = np.zeros((height, width)), np.zeros((height, width))
    for (l, t, w, h), a, b in zip(rects, counts_a, counts_b):
        na[t : t + h, l : l + w] = a
        nb[t : t + h, l : l + w] = b
    return na, nb


def random_frame(width, height, seed, counts=None):
    """(SA, QA, SB, QB, rects, counts_a, counts_b): two halves of one smooth base, each with noise of its own; exact-tie plateaus; fireflies, pairs and lines
    planted in ONE half; a block of negative sums; zeros of both signs; NaN and infinities in one half only; two finite halves whose sum overflows.
    counts: (counts_a, counts_b) for layout()'s five rects in place of its own."""
    rng = np.random.default_rng(seed)
    rects, counts_a, counts_b = layout(width, height)
    if counts is not None:
        counts_a, counts_b = list(counts[0]), list(counts[1])
    n = count_planes(width, height, rects, counts_a, counts_b)
    yy, xx = np.mgrid[0:height, 0:width]
    base = 0.75 + 0.25 * np.sin(0.21 * xx) + 0.125 * np.cos(0.33 * yy)
    halves = []
    plateaus = [(int(rng.integers(0, width)), int(rng.integers(0, height)), int(rng.integers(1, 6)), int(rng.integers(1, 6)), rng.integers(1, 9) / 8.0)
                for _ in range(max(1, width * height // 150))]
    for h in range(2):
        nh = np.maximum(n[h], 1.0)[:, :, None]
        mean = base[:, :, None] * np.array([1.0, 0.75, 0.5]) * (1.0 + 0.02 * rng.standard_normal((height, width, 3)))
        for x, y, w, hh, v in plateaus:  # one exact value in both halves over a small block: exact ties of the merged Y inside one rect
            mean[y : y + hh, x : x + w] = v
        s2 = (0.05 + 0.05 * rng.random((height, width, 1))) ** 2
        S = mean * nh
        Q = S * S / nh + np.maximum(nh - 1.0, 0.0) * s2
        halves.append([np.ascontiguousarray(S), np.ascontiguousarray(Q), mean, nh])

    def firefly(x, y):  # one sample of 50 times the pixel's mean, times its count, in one half
        S, Q, mean, nh = halves[int(rng.integers(0, 2))]
        b = 50.0 * np.abs(mean[y, x]) * nh[y, x] + 1.0
        S[y, x] += b
        Q[y, x] += b * b

    for _ in range(max(1, width * height // 60)):
        x, y = int(rng.integers(0, width)), int(rng.integers(0, height))
        kind = int(rng.integers(0, 4))
        if kind <= 1:
            firefly(x, y)
        elif kind == 2:
            firefly(x, y)
            firefly(min(x + 1, width - 1), y)
        else:
            for j in range(int(rng.integers(3, 9))):
                if y + j < height:
                    firefly(x, y + j)
    if width >= 8 and height >= 8:
        (_, _, mx, my) = rects[0]
        for y in range(1, my - 1, 3):  # along the (8, 8) | (8, 16) edge, on either side: donors across it, scaled in one half and copied in the other
            firefly(mx - 1, y)
            firefly(mx, y + 1)
        for x in range(1, mx - 1, 5):  # along the (8, 8) / (1, 1) edge
            firefly(x, my - 1)
        x, y = width // 3, height // 3
        for S, _, _, _ in halves:  # a block of negative sums, a brighter (less negative) pixel and a darker one inside
            S[y : y + 5, x : x + 5] = -np.abs(S[y : y + 5, x : x + 5])
            S[y + 2, x + 2] *= 0.5
            S[y + 3, x + 1] *= 1.5
        x, y = (2 * width) // 3, height // 4  # zeros of both signs: +0 + -0 is +0, -0 + -0 is -0
        halves[0][0][y, x], halves[1][0][y, x] = 0.0, -0.0
        halves[0][0][y, x + 1], halves[1][0][y, x + 1] = -0.0, -0.0
        halves[0][1][y, x], halves[1][1][y, x] = 0.0, 0.0
        x, y = width // 5, height // 5  # two finite halves whose sum overflows: not valid, a bit copy
        halves[0][0][y, x, 1] = halves[1][0][y, x, 1] = 1.5e308
        halves[0][1][y + 1, x, 2] = halves[1][1][y + 1, x, 2] = 1.0e308
    for _ in range(max(1, width * height // 200)):  # not finite in one half only
        h = int(rng.integers(0, 2))
        flatS, flatQ = halves[h][0].reshape(-1), halves[h][1].reshape(-1)
        flatS[int(rng.integers(0, flatS.size))] = np.nan
        flatQ[int(rng.integers(0, flatQ.size))] = np.inf
        flatS[int(rng.integers(0, flatS.size))] = -np.inf
    if width * height >= 4:
        halves[1][1].reshape(-1)[0] = np.float64(np.uint64(0x7FF8000000000ABC).view(np.float64))  # a NaN with a payload: a bit copy keeps it
    return halves[0][0], halves[0][1], halves[1][0], halves[1][1], rects, counts_a, counts_b


@functools.lru_cache(maxsize=None)
def frame(size):
    """The random frame of one of SIZES (shared, never written to)."""
    out = random_frame(size[0], size[1], seed=1000 + size[0])
    for a in out[:4]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(size, radius, rank):
    """The restatement on frame(size) at the starting k, ratio and floor (shared, never written to)."""
    SA, QA, SB, QB, rects, ca, cb = frame(size)
    out = despike_dual_ref.despike_dual(SA, QA, SB, QB, rects, ca, cb, radius, rank)
    for a in out[:5]:
        a.setflags(write=False)
    return out


def flat_dual(width, height, rects, counts_a, counts_b, value=1.0):
    """A constant frame under the given rects: every covered half holds `value` per sample, with a per-sample variance of its own per pixel and half, so
    every pixel's Q has bits of its own.  Uncovered pixels and empty halves hold zero sums."""
    na, nb = count_planes(width, height, rects, counts_a, counts_b)
    out = []
    for h, n in enumerate((na, nb)):
        s2 = S2 * (1.0 + 1e-3 * (np.arange(width * height, dtype=np.float64).reshape(height, width) + 0.5 * h))
        S, Q = sums_of(np.full((height, width), value), np.maximum(n, 1.0), s2)
        S[n == 0], Q[n == 0] = 0.0, 0.0
        out += [S, Q]
    return out[0], out[1], out[2], out[3]


def plant_half(S, Q, x, y, value, n):
    """Half (S, Q)'s pixel (x, y) gains one sample of `value` in place of one of its own: S += value - S / n, Q += value^2 - Q / n (n >= 1)."""
    s, q = S[y, x].copy(), Q[y, x].copy()
    S[y, x] = s - s / n + value
    Q[y, x] = q - q / n + value * value


# ---------------------------------------------------------------- the hand-made frames
HAND_W, HAND_H = 40, 24
# (8, 8) | (8, 16) | (0, 8) | two uncovered columns; the kernel's tile seams x = 31 | 32 and y = 15 | 16 lie inside the (8, 16) rect
HAND_RECTS, HAND_A, HAND_B = [(0, 0, 20, 24), (20, 0, 14, 24), (34, 0, 4, 24)], [8, 8, 0], [8, 16, 8]
FIREFLY = 400.0  # one sample of it in a half of 8 puts the merged mean of a (8, 8) pixel at 25.9, of a (8, 16) pixel at 17.6: far above twice a donor of 3


def hand_frame():
    """The flat frame of mean 1 under HAND_RECTS, writable: (SA, QA, SB, QB)."""
    return flat_dual(HAND_W, HAND_H, HAND_RECTS, HAND_A, HAND_B)


def set_mean(planes, x, y, value):
    """Pixel (x, y) becomes a noise-free pixel of mean `value` in both halves, at its rect's counts (an empty half stays zero)."""
    na, nb = count_planes(HAND_W, HAND_H, HAND_RECTS, HAND_A, HAND_B)
    for (S, Q), n in ((planes[0:2], na[y, x]), (planes[2:4], nb[y, x])):
        if n:
            s, q = sums_of(np.full((1, 1), value), n)
            S[y, x], Q[y, x] = s[0, 0], q[0, 0]


def spike_with_donor(planes, x, y, qx, qy, half=0, others=((-1, -1), (1, -1))):
    """A firefly in one half of (x, y) whose donor at radius 2, rank 2 is (qx, qy): that pixel at mean 3, the two `others` (offsets from the spike) at means
    3.25 and 3.5.  All three are neighbours of the spike, so each has the other two and the firefly in its own window: its donor is at least 3, twice
    which is above its own mean, and none of the three is a spike itself."""
    na, nb = count_planes(HAND_W, HAND_H, HAND_RECTS, HAND_A, HAND_B)
    assert all(max(abs(dx), abs(dy)) == 1 for dx, dy in tuple(others) + ((qx - x, qy - y),))
    set_mean(planes, qx, qy, 3.0)
    for (dx, dy), v in zip(others, (3.25, 3.5)):
        set_mean(planes, x + dx, y + dy, v)
    plant_half(planes[2 * half], planes[2 * half + 1], x, y, FIREFLY, (na, nb)[half][y, x])


def hand_frames():
    """name -> (planes, expected spikes [(x, y, donor x, donor y)]): the classes of the issue, each a frame of its own."""
    out = {}
    p = hand_frame()  # a spike planted in half A alone: every other is a tie at mean 1, so the donor is raster index 2 of the window, (x, y - 2)
    plant_half(p[0], p[1], 5, 5, FIREFLY, 8)
    out["half_a_alone"] = (p, [(5, 5, 5, 3)])
    for (x, y), (qx, qy) in (((31, 15), (32, 16)), ((32, 15), (31, 16)), ((31, 16), (32, 15)), ((32, 16), (31, 15))):
        p = hand_frame()  # on both tile seams, the donor diagonally across them; the two brighter others lie on the spike's own side of each seam
        spike_with_donor(p, x, y, qx, qy, half=(x + y) & 1, others=((x - qx, 0), (0, y - qy)))
        out["seam_%d_%d" % (x, y)] = (p, [(x, y, qx, qy)])
    p = hand_frame()  # the spike in the (8, 8) rect, its donor across the rect edge in the (8, 16) rect: half A is a bit copy, half B is scaled
    spike_with_donor(p, 19, 10, 20, 10, half=1)
    out["donor_in_8_16"] = (p, [(19, 10, 20, 10)])
    p = hand_frame()  # the reverse: the spike at (8, 16), the donor at (8, 8)
    spike_with_donor(p, 20, 10, 19, 10, half=0, others=((1, -1), (1, 1)))
    out["donor_in_8_8"] = (p, [(20, 10, 19, 10)])
    p = hand_frame()  # next to the (0, 8) rect: its pixels, however bright in half B, are no others; (34, 12) holds a firefly of its own and is copied
    spike_with_donor(p, 33, 10, 32, 10, half=0, others=((-1, -1), (-1, 1)))
    for y in (9, 10, 11):
        set_mean(p, 34, y, 9.0)
    plant_half(p[2], p[3], 34, 12, FIREFLY, 8)
    out["next_to_0_8"] = (p, [(33, 10, 32, 10)])
    p = hand_frame()  # a NaN (with a payload) in half B only: not valid, copied bit for bit, and no donor — the spike beside it takes the next other
    spike_with_donor(p, 10, 10, 9, 10, half=0)
    set_mean(p, 11, 10, 3.75)  # (valid, it would stand first among the others and push the donor to the 3.25)
    p[2][10, 11, 1] = np.float64(np.uint64(0x7FF8000000000ABC).view(np.float64))
    out["nan_in_half_b"] = (p, [(10, 10, 9, 10)])
    return out


HAND = hand_frames()


def rect_of(rects, x, y):
    return next(j for j, (l, t, w, h) in enumerate(rects) if l <= x < l + w and t <= y < t + h)


def check_hand(name, planes, result):
    """What every class is held to, whoever made `result` = (S'_A, Q'_A, S'_B, Q'_B, replaced): the expected spikes and nothing else changed, each spike's
    halves from its donor's halves by the rule written out, the count in the spike's rect — and then what the class is named for."""
    _, expected = HAND[name]
    na, nb = count_planes(HAND_W, HAND_H, HAND_RECTS, HAND_A, HAND_B)
    changed = np.zeros((HAND_H, HAND_W), dtype=bool)
    for got, src in zip(result[:4], planes):
        changed |= (got.view(np.uint64) != src.view(np.uint64)).any(axis=2)
    assert sorted((int(x), int(y)) for y, x in zip(*np.nonzero(changed))) == sorted((x, y) for x, y, _, _ in expected), name
    want_replaced = [0] * len(HAND_RECTS)
    for x, y, qx, qy in expected:
        want_replaced[rect_of(HAND_RECTS, x, y)] += 1
        for h, n in ((0, na), (1, nb)):
            for got, src in ((result[2 * h], planes[2 * h]), (result[2 * h + 1], planes[2 * h + 1])):
                if n[y, x] == n[qy, qx]:
                    assert despike_dual_ref.same_bits(got[y, x], src[qy, qx]), (name, h)
                else:
                    assert despike_dual_ref.same_bits(got[y, x], (src[qy, qx] / np.float64(n[qy, qx])) * np.float64(n[y, x])), (name, h)
    assert [int(v) for v in result[4]] == want_replaced, name
    if name == "half_a_alone":  # planted in half A alone (half B's input is the flat frame's), replaced in both halves
        flat = hand_frame()
        assert despike_dual_ref.same_bits(planes[2], flat[2]) and despike_dual_ref.same_bits(planes[3], flat[3]) and not despike_dual_ref.same_bits(planes[0], flat[0])
        assert not despike_dual_ref.same_bits(result[3][5, 5], planes[3][5, 5]) and not despike_dual_ref.same_bits(result[0][5, 5], planes[0][5, 5])  # (every pixel's Q has bits of its own)
    if name.startswith("seam"):  # the donor lies across both seams of the 32 x 16 tiles
        (x, y, qx, qy), = expected
        assert x // 32 != qx // 32 and y // 16 != qy // 16
    if name == "donor_in_8_16":  # bit-copied in half A, scaled in half B
        assert (na[10, 19], nb[10, 19], na[10, 20], nb[10, 20]) == (8, 8, 8, 16)
        assert despike_dual_ref.same_bits(result[0][10, 19], planes[0][10, 20]) and despike_dual_ref.same_bits(result[2][10, 19], (planes[2][10, 20] / np.float64(16)) * np.float64(8))
    if name == "next_to_0_8":  # the (0, 8) pixels are brighter than the donor, beside the spike, and yet no donor; their own firefly stays
        assert (na[10, 34], nb[10, 34]) == (0, 8) and planes[2][10, 34, 0] / 8 == 9.0 and planes[2][12, 34, 0] > 400.0
    if name == "nan_in_half_b":
        assert np.isnan(planes[2][10, 11, 1]) and np.isfinite(planes[0][10, 11]).all() and result[2][10, 11].view(np.uint64)[1] == 0x7FF8000000000ABC
