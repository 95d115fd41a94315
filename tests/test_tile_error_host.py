"""What tests/test_gpu_tile_error.py stands on, checked without a GPU: the restatements of tests/tile_error_ref.py and the frames of tests/tile_error_frames.py.

  * the three restatements of rmd_tile_error — tile_error_ref.tile_error, numpy_tile_error of tests/test_gpu_moments.py and despike_ref.tile_error — agree
    bit for bit on every class;
  * on `random` the restatement lies within 4 ulp of the rule in exact rational arithmetic;
  * every frame class is what it names (the clamp's three kinds, the floor's three sides, subnormal v / n, an overflowing S*m, a planted strict maximum);
  * ordered_total on `chain` and `pairs` is far from np.sum, math.fsum and the ascending butterfly; on `positive` it is math.fsum's within rounding;
  * no rect of any class has a negative restated total;
  * ordered_total depends on the rect's values alone, not on where they lie or how wide the frame is."""
import math
from fractions import Fraction

import numpy as np
import pytest

import despike_ref
import tile_error_frames as frames
import tile_error_ref as ref
from test_gpu_moments import numpy_tile_error

CASES = [c.name for c in frames.cases()]


@pytest.mark.parametrize("name", CASES)
def test_the_three_restatements_agree_bit_for_bit(name):
    c = frames.case(name)
    rects = frames.case_rects(c)
    new = ref.tile_error(c.S, c.Q, c.n, c.floor, rects)
    moments = np.array([numpy_tile_error(c.S, c.Q, c.n, c.floor, r) for r in rects])
    assert ref.same_bits(new, moments), (name, new, moments)
    # (the third is a Python loop per pixel: the specials are held to it on the rects made for them and the tile, the other classes on the whole list)
    some = list(range(len(rects))) if not name.startswith("specials") else [0, 1, 2, 3 + frames.RECTS.index(frames.TILE)]
    loops = despike_ref.tile_error(c.S, c.Q, c.n, c.floor, [rects[j] for j in some])
    assert ref.same_bits(new[some], loops), (name, new[some], loops)
    assert (new[[j for j, r in enumerate(rects) if r[2] * r[3] == 0]] == 0.0).all()
    if c.n < 2:
        assert (new[[j for j, r in enumerate(rects) if r[2] * r[3]]] == np.inf).all()


def test_the_restatements_agree_on_the_wide_frame():
    c = frames.wide_case()
    new = ref.tile_error(c.S, c.Q, c.n, c.floor, frames.WIDE_RECTS)
    assert ref.same_bits(new, np.array([numpy_tile_error(c.S, c.Q, c.n, c.floor, r) for r in frames.WIDE_RECTS]))
    short = [j for j, r in enumerate(frames.WIDE_RECTS) if r[2] * r[3] < 3000]
    assert ref.same_bits(new[short], despike_ref.tile_error(c.S, c.Q, c.n, c.floor, [frames.WIDE_RECTS[j] for j in short]))


def exact_error(s, q, n, floor):
    """The rule for one channel in rational arithmetic, rounded once at the end (the root taken at 60 digits)."""
    import decimal

    s, q = Fraction(float(s)), Fraction(float(q))
    m = s / n
    v = max(Fraction(0), (q - s * m) / (n - 1))
    x = v / n / max(abs(m), Fraction(float(floor))) ** 2  # the error squared
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        return float((decimal.Decimal(x.numerator) / decimal.Decimal(x.denominator)).sqrt())


def test_the_restatement_is_within_4_ulp_of_the_exact_rule_on_random():
    """m, S*m, the difference, the two divisions of v: at most 2.5 ulp of v / n where the difference does not cancel (here Q is about 2.9 S*m), halved by
    the root; then the root, the denominator's m and the last division, half an ulp each: under 3.  4 ulp bounds the restatement, not the device."""
    c = frames.case("random/n=64")
    got = ref.pixel_errors(c.S, c.Q, c.n, c.floor)
    worst = 0
    for y in range(0, frames.H, 2):  # every second row: 1,541 pixels, the black block and the three special pixels among them
        for x in range(frames.W):
            want = max(exact_error(c.S[y, x, ch], c.Q[y, x, ch], c.n, c.floor) for ch in range(3))
            worst = max(worst, int(ref.ulp_distance(got[y, x], want).max()))
    print("largest ulp distance from the exact rule:", worst)
    assert worst <= 4


def channel_steps(c):
    """m, S*m and v before the clamp, as the restatement rounds them."""
    nd = np.float64(c.n)
    with np.errstate(all="ignore"):
        m = c.S / nd
        sm = c.S * m
        return m, sm, (c.Q - sm) / (nd - 1.0)


def test_clamp_pixels_are_zero_negative_and_positive_and_an_exact_product_would_differ():
    c = frames.case("clamp")
    m, _, v = channel_steps(c)
    kind = frames.kinds(3)
    assert (v[kind == 0] == 0.0).all() and (v[kind == 1] < 0.0).all() and (v[kind == 2] > 0.0).all()
    e = ref.pixel_errors(c.S, c.Q, c.n, c.floor)
    assert (e[kind != 2] == 0.0).all() and (e[kind == 2] > 0.0).all()
    # with S*m unrounded — what a fused multiply-add computes — the `v == 0` kind is not zero: a build that contracts Q - S*m shows in these pixels
    ys, xs = np.nonzero(kind == 0)
    for y, x in zip(ys[::7], xs[::7]):
        for ch in range(3):
            assert Fraction(float(c.Q[y, x, ch])) - Fraction(float(c.S[y, x, ch])) * Fraction(float(m[y, x, ch])) != 0


@pytest.mark.parametrize("n,floor", frames.FLOOR_EDGES)
def test_floor_edge_means_are_at_below_and_above_the_floor(n, floor):
    c = frames.case("floor_edge/n=%d/floor=%r" % (n, floor))
    assert float(np.float64(floor) * np.float64(n)) == Fraction(floor) * n  # floor * n is exact
    m = np.abs(channel_steps(c)[0])
    kind = frames.kinds(3)
    assert (m[kind == 0] == floor).all()
    assert (m[kind == 1] == np.nextafter(floor, 0.0)).all() and (m[kind == 1] < floor).all()
    assert (m[kind == 2] == np.nextafter(floor, np.inf)).all() and (m[kind == 2] > floor).all()
    assert (c.S[0::2] > 0).all() and (c.S[1::2] < 0).all()
    assert (ref.pixel_errors(c.S, c.Q, c.n, c.floor) > 0).all()


def test_tiny_huge_and_negative_reach_what_they_name():
    tiny = np.finfo(np.float64).tiny
    c = frames.case("tiny")
    _, sm, v = channel_steps(c)
    with np.errstate(all="ignore"):
        vn = v / np.float64(c.n)
    assert ((vn > 0) & (vn < tiny)).any() and ((sm > 0) & (sm < tiny)).any()
    assert ((np.abs(c.S) < tiny) & (c.S != 0)).any() and ((c.Q < tiny) & (c.Q != 0)).any()
    e = ref.pixel_errors(c.S, c.Q, c.n, c.floor)
    assert np.isfinite(e).all() and (e > 0).any()
    c = frames.case("huge")
    _, sm, v = channel_steps(c)
    kind = frames.kinds(2)
    assert (sm[kind == 0] == np.inf).all() and (v[kind == 0] == -np.inf).all() and np.isfinite(c.S).all() and np.isfinite(c.Q).all()
    e = ref.pixel_errors(c.S, c.Q, c.n, c.floor)
    assert (e[kind == 0] == 0.0).all() and np.isfinite(e).all() and (e[kind == 1] > 1e100).all()
    c = frames.case("negative")
    assert (c.S < 0).any() and (c.Q < 0).any() and ((c.S < 0) & (c.Q < 0)).any()
    assert ((c.S == 0) & np.signbit(c.S)).any() and ((c.Q == 0) & np.signbit(c.Q)).any()
    e = ref.pixel_errors(c.S, c.Q, c.n, c.floor)
    assert np.isfinite(e).all() and not np.signbit(e).any()


def test_specials_stand_alone_in_their_rects():
    seen = 0
    for c in frames.cases():
        if not c.name.startswith("specials"):
            continue
        seen += 1
        bad = ~(np.isfinite(c.S).all(axis=2) & np.isfinite(c.Q).all(axis=2))
        assert bad.sum() == 3
        for rect, index in frames.SPECIAL_RECTS:
            l, t, w, h = rect
            x, y = frames.pixel_of(rect, index)
            assert bad[t : t + h, l : l + w].sum() == 1 and bad[y, x]
        assert frames.pixel_of(frames.SPECIAL_RECTS[2][0], 256) == (16, 32)
    assert seen == 18


@pytest.mark.parametrize("rect", frames.PLANT_RECTS)
def test_a_planted_pixel_is_the_strict_maximum_of_its_rect_by_a_factor_of_2(rect):
    q = frames.case("quiet")
    l, t, w, h = rect
    quiet = ref.pixel_errors(q.S, q.Q, q.n, q.floor)
    assert 0.0037 < quiet.min() and quiet.max() < 0.0054
    places = set()
    for index in frames.PLANT_INDICES:
        x, y = frames.pixel_of(rect, index)
        places.add((x, y))
        e = ref.pixel_errors(*frames.planted(q.S, q.Q, rect, index), q.n, q.floor)
        inside = e[t : t + h, l : l + w].copy()
        assert inside[y - t, x - l] == inside.max()
        inside[y - t, x - l] = 0.0
        assert e[y, x] >= 2.0 * inside.max() and e[y, x] >= 2.0 * quiet.max()
    assert len(places) == len(frames.PLANT_INDICES)


# ---------------------------------------------------------------- the sum order
def ascending_total(partials):
    """The other butterfly: t with t ^ 1, ^ 2, ... ^ 32."""
    lane = np.arange(256)
    s = np.asarray(partials, dtype=np.float64)
    for off in (1, 2, 4, 8, 16, 32):
        s = s + s[lane ^ off]
    return float((s[0] + s[64]) + (s[128] + s[192]))


def apart(a, b):
    """The relative difference of two totals, by the larger one."""
    return abs(a - b) / max(abs(a), abs(b)) if a != b else 0.0


@pytest.mark.parametrize("name", ["chain", "pairs", "wide/chain"])
def test_the_header_order_is_far_from_every_other_sum_on_the_cancelling_classes(name):
    c = frames.err_case(name)
    for j in c.designated:
        values = ref.rect_values(c.err, c.rects[j])
        ours = ref.ordered_total(c.err, c.rects[j])
        others = {"np.sum": float(np.sum(values)), "math.fsum": math.fsum(values), "ascending": ascending_total(ref.partial_sums(values)[0])}
        print(name, c.rects[j], "header's order", ours, others)
        assert ours >= 0.0
        for what, other in others.items():
            assert apart(ours, other) > 1e-3, (name, c.rects[j], what, ours, other)
    # the designated rects do not overlap, and the list holds nothing else with pixels
    cover = np.zeros(c.err.shape, dtype=int)
    for l, t, w, h in c.rects:
        cover[t : t + h, l : l + w] += 1
    assert cover.max() == 1 and sorted(c.designated) == [j for j, r in enumerate(c.rects) if r[2] * r[3]]


def test_on_positive_data_the_header_order_is_the_exact_sum_within_rounding():
    for c in (frames.err_case("positive"), frames.err_case("wide/positive")):
        for rect in c.rects:
            n_px = rect[2] * rect[3]
            exact = math.fsum(ref.rect_values(c.err, rect))
            assert abs(ref.ordered_total(c.err, rect) - exact) <= n_px * 2.0**-53 * exact, (c.name, rect)


def test_no_restated_total_is_negative():
    for c in frames.err_cases() + frames.wide_err_cases():
        for rect in c.rects:
            total, nan = ref.ordered_sum(ref.rect_values(c.err, rect))
            assert total >= 0.0 or total == np.inf, (c.name, rect, total)
            assert nan == bool(np.isnan(ref.rect_values(c.err, rect)).any())
        want = ref.tile_error_dual(c.err, c.rects)
        assert not np.isnan(want).any() and (want >= 0).all()
        if c.name.startswith("nan") or c.name == "inf":
            hit = [j for j, r in enumerate(c.rects) if not np.isfinite(ref.rect_values(c.err, r)).all()]
            assert len(hit) >= 2 and (want[hit] == np.inf).all() and np.isfinite(np.delete(want, hit)).all()
    err = frames.exact_image()
    assert [float(v) for v in ref.tile_error_dual(err, [r for r, _ in frames.EXACT_RECTS])] == [w for _, w in frames.EXACT_RECTS]
    assert math.fsum(ref.rect_values(err, frames.EXACT_RECTS[2][0])) == 256.0 and ref.ordered_total(err, frames.EXACT_RECTS[2][0]) == 192.0


def test_the_nan_classes_sit_at_the_ends_of_lane_0s_chain():
    l, t, w, h = frames.TILE
    for name, index in (("nan/0", 0), ("nan/last", w * h - 1), ("nan/256", 256)):
        flat = ref.rect_values(frames.err_case(name).err, frames.TILE)
        assert list(np.nonzero(np.isnan(flat))[0]) == [index]


def test_ordered_total_depends_on_the_rects_values_alone():
    for name, j in (("chain", 1), ("pairs", 2), ("positive", frames.RECTS.index((40, 1, 27, 19)))):
        c = frames.err_case(name)
        l, t, w, h = c.rects[j]
        other = np.full((frames.WIDE, frames.WIDE), 123.0)
        other[101 : 101 + h, 7 : 7 + w] = c.err[t : t + h, l : l + w]
        a, b = ref.ordered_total(c.err, c.rects[j]), ref.ordered_total(other, (7, 101, w, h))
        assert ref.same_bits(np.float64(a), np.float64(b))
        assert ref.same_bits(ref.tile_error_dual(c.err, [c.rects[j]]), ref.tile_error_dual(other, [(7, 101, w, h)]))
