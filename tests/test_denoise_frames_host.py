"""tests/denoise_frames.py without a GPU: every class is what its name says (asserted from the restatements), the vectorised restatements equal the
pixel-by-pixel readings on the classes cut down to sizes Python loops can take, and the frames discriminate — four deliberately wrong variants of
denoise_ref.denoise each leave the comparison bar on a named class.  (No wrong variant of a kernel is ever run on a device: this is its stand-in.)"""
import numpy as np
import pytest

import denoise_atrous_dual_ref as adref
import denoise_atrous_ref as aref
import denoise_dual_guided_ref as dgref
import denoise_dual_ref
import denoise_frames as df
import denoise_guided_ref as gref
import denoise_ref
from denoise_ref import EPS, mean_and_variance


def _bytes_equal(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---------------------------------------------------------------- denoise_ref.denoise with switches
MUTANTS = ("skip_outside", "full_count", "clamp_q", "own_variance")


def _variant(S, Q, n, radius, patch_radius, k, alpha, mutant=None, probe=None):
    """denoise_ref.denoise's loop, line for line, with one deliberate error per `mutant`:
        skip_outside   a patch position outside the frame is skipped instead of clamped
        full_count     D is divided by 3 (2f + 1)^2 instead of by three times the offsets taken
        clamp_q        a neighbour q outside the frame is clamped into it instead of left out
        own_variance   min(v_a, v_b) is replaced by v_a
    mutant=None is the restatement itself (held to it bit for bit below).  probe=(dy, dx): -> (D, cnt) of that offset instead of the frame."""
    H, W = n.shape
    r, f = int(radius), int(patch_radius)
    k2, alpha = float(k) * float(k), float(alpha)
    u, v, valid = mean_and_variance(S, Q, n)
    ys, xs = np.arange(-f, H + f), np.arange(-f, W + f)
    ya, xa = np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)
    ua, va, oka = u[ya][:, xa], v[ya][:, xa], valid[ya][:, xa]
    if mutant == "skip_outside":
        oka = oka & ((ys == ya)[:, None] & (xs == xa)[None, :])
    acc = np.full((H, W, 3), -0.0)
    wsum = np.full((H, W), -0.0)
    py, px = np.arange(H)[:, None], np.arange(W)[None, :]
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            yb = np.clip(ys + dy, 0, H - 1)
            for dx in range(-r, r + 1):
                xb = np.clip(xs + dx, 0, W - 1)
                ub, vb, okb = u[yb][:, xb], v[yb][:, xb], valid[yb][:, xb]
                if mutant == "skip_outside":
                    okb = okb & ((ys + dy == yb)[:, None] & (xs + dx == xb)[None, :])
                t = None
                for c in range(3):
                    du = ua[..., c] - ub[..., c]
                    other = va[..., c] if mutant == "own_variance" else np.minimum(va[..., c], vb[..., c])
                    term = (du * du - alpha * (va[..., c] + other)) / (EPS + k2 * (va[..., c] + vb[..., c]))
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
                D = ds / (3.0 * (float((2 * f + 1) ** 2) if mutant == "full_count" else cnt.astype(np.float64)))
                if probe == (dy, dx):
                    return D, cnt
                w = np.exp(-np.where(D > 0.0, D, 0.0))
                qy, qx = py + dy, px + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                if mutant == "clamp_q":
                    inside = inside | True
                qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                use = valid & inside & valid[qyc, qxc]
                uq = u[qyc, qxc]
                acc = np.where(use[..., None], acc + w[..., None] * uq, acc)
                wsum = np.where(use, wsum + w, wsum)
        out = acc / wsum[..., None]
        raw = S / n.astype(np.float64)[..., None]
    return np.where(valid[..., None], out, raw)


def _single_scale(fr, r):
    S, Q, _, _, n = fr.single()
    u, _, valid = mean_and_variance(S, Q, n)
    return df.local_scale([u], valid, r)


@pytest.mark.parametrize("name", ["shape_33x15", "seam_checker_a", "scale_overflow", "scale_2m200"])
def test_the_variant_without_a_mutation_is_the_restatement(name):
    fr = df.frame(name)
    S, Q, _, _, n = fr.single()
    for r, f in ((3, 1), (2, 2)):
        assert _bytes_equal(_variant(S, Q, n, r, f, fr.k, fr.alpha), denoise_ref.denoise(S, Q, n, r, f, fr.k, fr.alpha)), name


# mutant -> the class that must catch it (others may as well)
CAUGHT_BY = {"skip_outside": "shape_2x2", "full_count": "seam_checker_a", "clamp_q": "shape_33x15", "own_variance": "shape_24x16"}


@pytest.mark.parametrize("mutant", MUTANTS)
def test_each_wrong_variant_leaves_the_bar_on_a_named_class(mutant):
    name = CAUGHT_BY[mutant]
    fr = df.frame(name)
    S, Q, _, _, n = fr.single()
    r, f = 3, 1
    ref = denoise_ref.denoise(S, Q, n, r, f, fr.k, fr.alpha)
    bad, worst, _ = df.differences(_variant(S, Q, n, r, f, fr.k, fr.alpha, mutant), ref, _single_scale(fr, r))
    print("mutant %s on %s: %d values outside the bar, worst relative difference %.3g" % (mutant, name, bad, worst))
    assert bad > 0, "the wrong variant %s stays within the bar on class %s" % (mutant, name)


def test_the_bar_is_local():
    """A difference of 1e-3 relative in the dim half of scale_mixed is outside the bar, though it is 2^-400 of the frame's largest value."""
    fr = df.frame("scale_mixed")
    S, Q, _, _, n = fr.single()
    ref = denoise_ref.denoise(S, Q, n, 3, 1, fr.k, fr.alpha)
    scale = _single_scale(fr, 3)
    assert df.differences(ref, ref, scale)[0] == 0
    off = ref.copy()
    off[5, fr.W - 3, 1] *= 1.0 + 1e-3  # further than the radius from the bright half
    assert df.differences(off, ref, scale)[0] == 1, "class scale_mixed: the dim half is hidden by the bright one"
    assert np.abs(off - ref).max() <= 1e-12 * np.abs(ref[np.isfinite(ref)]).max()  # (the frame-wide allowance would have let it pass)
    nan = ref.copy()
    nan[2, 2, 0] = np.nan
    assert df.differences(nan, ref, scale)[0] == 1


# ---------------------------------------------------------------- every class is what it names
def test_the_content_is_test_gpu_denoises_own():
    import test_gpu_denoise as tgd

    n_img = df.block_counts(np.random.default_rng(1), 37, 23)
    a, b = df.moments(np.random.default_rng(2), n_img), tgd._moments(np.random.default_rng(2), n_img)
    assert _bytes_equal(a[0], b[0]) and _bytes_equal(a[1], b[1])
    ra, rb = np.random.default_rng(3), np.random.default_rng(3)
    pa, pb = [x.copy() for x in a], [x.copy() for x in a]
    df.poison(*pa, ra), tgd._poison(*pb, rb)
    assert _bytes_equal(pa[0], pb[0]) and _bytes_equal(pa[1], pb[1])


@pytest.mark.parametrize("name", ["shape_48x33", "seam_checker_a", "scale_2p200"])
def test_the_features_cut_weights_without_isolating_pixels(name):
    """Features drawn at random per pixel give every pair a feature weight of nothing: each pixel comes back as itself and a guided kernel is compared
    on no arithmetic at all.  These turn slowly: at either guide the tests use most pixels differ from the unguided result and from their own mean."""
    fr = df.frame(name)
    S, Q, _, _, n = fr.single()
    F1, G1 = fr.single_features()
    u, _, valid = mean_and_variance(S, Q, n)
    plain = denoise_ref.denoise(S, Q, n, 3, 1, fr.k, fr.alpha)
    for k_f, tau in ((1.0, 1e-2), (0.6, 1e-3)):
        guided = gref.denoise_guided(S, Q, F1, G1, n, 3, 1, fr.k, fr.alpha, k_f, tau)
        assert (guided[valid] != plain[valid]).mean() > 0.2 and (guided[valid] != u[valid]).mean() > 0.6, "class %s at k_f %g" % (name, k_f)


@pytest.mark.parametrize("name", list(df.CLASSES))
def test_frames_are_small_seeded_and_their_rects_give_their_counts(name):
    fr = df.frame(name)
    assert max(fr.W, fr.H) <= 72 and fr.W * fr.H <= 3000, name
    for counts, n in ((fr.counts_a, fr.n_a), (fr.counts_b, fr.n_b), (fr.counts_f, fr.n_f)):
        assert np.array_equal(denoise_ref.count_image(fr.W, fr.H, fr.rects, counts), n), name
    make, args = df.CLASSES[name]
    again = make(name, *args)
    assert all(_bytes_equal(a, b) for a, b in zip(fr.halves + (fr.F, fr.G), again.halves + (again.F, again.G))), name
    assert all(np.isfinite(h).any() or "all" in name for h in fr.halves), name


def test_shape_classes_sit_at_the_tile_edges():
    assert [(df.frame(n).W, df.frame(n).H) for n in df.names("shape_")] == list(df.SHAPES)
    for tw in (24, 32):
        assert {tw - 1, tw, tw + 1} <= {W for W, _ in df.SHAPES}
    assert {15, 16, 17} <= {H for _, H in df.SHAPES} and {47, 48, 49} <= {W for W, _ in df.SHAPES}
    for name in ("shape_31x17", "shape_48x33"):  # valid and invalid pixels in both halves, by count and by value
        fr = df.frame(name)
        ok_a, ok_b, dual = fr.valid()
        assert dual.any() and not ok_a.all() and not ok_b.all(), name
        assert (fr.n_a == 0).any() and (fr.n_a == 1).any() and np.isnan(fr.halves[0]).any() and np.isinf(fr.halves[1]).any(), name


@pytest.mark.parametrize("name", df.names("seam_"))
def test_seam_classes_are_invalid_exactly_on_their_pattern(name):
    fr = df.frame(name)
    mask, variant = fr.note["mask"], fr.note["variant"]
    ok_a, ok_b, dual = fr.valid()
    fvalid = dgref.feature_planes(fr.F, fr.G, fr.n_f, dual, 1.0, 1e-2)[3]
    none = np.zeros_like(mask)
    want_a = mask if variant in ("a", "ab") else none
    want_b = mask if variant == "b" else mask[::-1, ::-1] if variant == "ab" else none
    assert np.array_equal(~ok_a, want_a) and np.array_equal(~ok_b, want_b), "class %s" % name
    if variant == "f":  # feature-valid and colour-valid sets differ: the colours are whole
        assert dual.all() and np.array_equal(~fvalid, mask), "class %s" % name
        routes = ((fr.n_f == 0) & mask, (fr.n_f == 1) & mask, np.isnan(fr.F).any(-1), np.isinf(fr.G).any(-1))
    else:
        S, Q, n = (fr.halves[0], fr.halves[1], fr.n_a) if variant != "b" else (fr.halves[2], fr.halves[3], fr.n_b)
        routes = (n == 0, n == 1, np.isnan(S).any(-1), np.isinf(Q).any(-1))
    if mask.sum() >= 4:  # every route to an invalid pixel is taken
        assert all(r.any() for r in routes), "class %s" % name
    assert sum(int(r.sum()) for r in routes) == mask.sum(), "class %s" % name


def test_seam_patterns_lie_where_the_kernels_structure_is():
    W, H = df.SEAM
    p = df._patterns(W, H)
    assert W > 33 and H > 17  # a tile seam of either width and of the height, with pixels on both sides
    assert p["columns"][:, [23, 24, 31, 32]].all() and p["columns"].sum() == 4 * H and p["row"][[15, 16]].all() and p["row"].sum() == 2 * W
    assert p["border"].sum() == 2 * W + 2 * H - 4 and not p["border"][1:-1, 1:-1].any()
    assert p["tile"][:16, :32].all() and p["tile"].sum() == 32 * 16 and p["all"].all()
    assert p["one_inside"].sum() == W * H - 1 and not p["one_inside"][1:-1, 1:-1].all() and p["one_corner"].sum() == W * H - 1 and not p["one_corner"][-1, -1]
    assert not (p["checker"][:, 1:] & p["checker"][:, :-1]).any() and not (p["checker"][1:] & p["checker"][:-1]).any() and p["checker"].sum() == W * H // 2
    y, x = df.RING_PIXEL
    d = df.RING_DEPTH
    assert not p["ring"][y, x] and p["ring"][y - d : y + d + 1, x - d : x + d + 1].sum() == (2 * d + 1) ** 2 - 1 == p["ring"].sum()


@pytest.mark.parametrize("r,f", [(4, 4), (3, 1), (1, 0)])
def test_the_ringed_pixel_has_offset_count_one_and_comes_back_bit_for_bit(r, f):
    """seam_ring_a: within RING_DEPTH of the pixel nothing else is valid, so of D(p, p)'s (2f + 1)^2 offsets only the centre is taken, no other q is in a
    window of radius r <= RING_DEPTH, and out = (1 * u) / 1 = u."""
    fr = df.frame("seam_ring_a")
    S, Q, _, _, n = fr.single()
    y, x = df.RING_PIXEL
    u, _, valid = mean_and_variance(S, Q, n)
    assert valid[y, x]
    _, cnt = _variant(S, Q, n, r, f, fr.k, fr.alpha, probe=(0, 0))
    assert cnt[y, x] == 1, "class seam_ring_a: %d offsets taken" % cnt[y, x]
    out = denoise_ref.denoise(S, Q, n, r, f, fr.k, fr.alpha)
    assert _bytes_equal(out[y, x], u[y, x]), "class seam_ring_a"
    assert not _bytes_equal(out[valid], u[valid]) or r == 0  # (elsewhere the filter filters)


def test_the_all_invalid_frame_returns_the_means():
    for name in ("seam_all_a", "seam_all_ab"):
        fr = df.frame(name)
        S, Q, _, _, n = fr.single()
        with np.errstate(all="ignore"):
            raw = S / n.astype(np.float64)[..., None]
        assert _bytes_equal(denoise_ref.denoise(S, Q, n, 3, 1), raw), "class %s" % name
        out, err = denoise_dual_ref.denoise_dual(*fr.halves, fr.n_a, fr.n_b, 3, 1)
        with np.errstate(all="ignore"):
            merged = (fr.halves[0] + fr.halves[2]) / (fr.n_a + fr.n_b).astype(np.float64)[..., None]
        assert _bytes_equal(out, merged) and np.isnan(err).all(), "class %s" % name


def test_the_one_pixel_frames_have_one_valid_pixel():
    for name, where in (("seam_one_inside_a", (df.SEAM[1] // 2, df.SEAM[0] // 2 + 5)), ("seam_one_corner_a", (df.SEAM[1] - 1, df.SEAM[0] - 1))):
        fr = df.frame(name)
        S, Q, _, _, n = fr.single()
        u, _, valid = mean_and_variance(S, Q, n)
        assert valid.sum() == 1 and valid[where], "class %s" % name
        assert _bytes_equal(denoise_ref.denoise(S, Q, n, 12, 4)[where], u[where]), "class %s" % name


def _eps_share(fr):
    """The smallest and the largest share eps has of a denominator eps + k^2 (v_p + v_q), over the pairs of valid pixels and the channels (the extremes
    are reached at the pixels of smallest and largest v: the pair of a pixel with itself is a taken pair)."""
    S, Q, _, _, n = fr.single()
    _, v, valid = mean_and_variance(S, Q, n)
    k2 = fr.k * fr.k
    vv = v[valid]
    return EPS / (EPS + k2 * 2.0 * vv.max()), EPS / (EPS + k2 * 2.0 * vv.min())


def test_eps_passes_from_negligible_to_dominant_over_the_scales():
    lo, hi = _eps_share(df.frame("scale_2m200"))
    assert hi > 0.99, "class scale_2m200: eps is at most %.3g of a denominator" % hi
    lo, hi = _eps_share(df.frame("scale_2p200"))
    assert hi < 1e-9, "class scale_2p200: eps is %.3g of some denominator" % hi
    shares = {k: _eps_share(df.frame(df._scale_name(k))) for k in df.SCALES}
    assert shares[500][1] < shares[200][1] < shares[40][1] < shares[-40][1] <= shares[-200][1] <= shares[-500][1] <= 1.0
    # powers of two keep u exact: the scaled frame's means are the unscaled frame's, scaled
    base = df._plain("scale_2p40", *df.SEAM, floor=True)[1]
    fr = df.frame("scale_2p40")
    assert _bytes_equal(fr.halves[0], base[0] * 2.0**40) and _bytes_equal(fr.halves[1], base[1] * 2.0**80)
    assert _bytes_equal(mean_and_variance(fr.halves[0], fr.halves[1], fr.n_a)[0], mean_and_variance(base[0], base[1], fr.n_a)[0] * 2.0**40)


def test_the_overflow_frame_has_a_taken_pair_with_nan_distance():
    fr = df.frame("scale_overflow")
    S, Q, _, _, n = fr.single()
    u, v, valid = mean_and_variance(S, Q, n)
    assert valid.all() and np.isfinite(u).all() and np.isfinite(v).all()
    D, cnt = _variant(S, Q, n, 1, 1, fr.k, fr.alpha, probe=(0, 1))
    assert (np.isnan(D) & (cnt > 0)).any(), "class scale_overflow: no taken pair has a NaN distance"
    assert np.isfinite(D).any()
    out = denoise_ref.denoise(S, Q, n, 3, 1, fr.k, fr.alpha)
    assert np.isfinite(out).all()  # D > 0 ? D : 0 turns the NaN into w = exp(-0) = 1
    # w = 1 across the middle: a pixel beside it averages +a and -a
    mid = fr.W // 2
    assert np.abs(out[:, mid - 1, 0]).max() < np.abs(u[:, mid - 1, 0]).min()


def test_the_other_scale_classes():
    fr = df.frame("scale_mixed")
    u = mean_and_variance(fr.halves[0], fr.halves[1], fr.n_a)[0]
    assert np.abs(u[:, : fr.W // 2]).min() > 2.0**190 and np.abs(u[:, fr.W // 2 :]).max() < 2.0**-190, "class scale_mixed"
    fr = df.frame("scale_flat")
    S, Q, _, _, n = fr.single()
    u, v, valid = mean_and_variance(S, Q, n)
    assert valid.all() and (v == 0.0).all() and (u == 0.75).all() and _bytes_equal(Q, S * S / 8.0), "class scale_flat"
    assert _bytes_equal(denoise_ref.denoise(S, Q, n, 12, 4), u), "class scale_flat"
    fr = df.frame("scale_negative")
    for S, Q, n in ((fr.halves[0], fr.halves[1], fr.n_a), (fr.halves[2], fr.halves[3], fr.n_b)):
        u, v, valid = mean_and_variance(S, Q, n)
        assert valid.all() and (u < 0.0).all() and (v > 0.0).any(), "class scale_negative"
    fr = df.frame("scale_cancel")
    S, Q, _, _, n = fr.single()
    u, v, valid = mean_and_variance(S, Q, n)
    assert valid.all() and (v == 0.0).all() and (Q < S * u).all(), "class scale_cancel"
    fr = df.frame("scale_counts")
    assert set(fr.counts_a) == set(fr.counts_b) == set(fr.counts_f) == {2, 3, df.UINT32_MAX}, "class scale_counts"
    row = fr.n_a[0]
    beside = {(int(a), int(b)) for a, b in zip(row[:-1], row[1:]) if a != b}
    assert (2, df.UINT32_MAX) in beside and (df.UINT32_MAX, 3) in beside, "class scale_counts: 2 does not lie beside 2^32 - 1"
    assert (np.diff(fr.n_a[0]) != 0).sum() == 2 and fr.valid()[2].all(), "class scale_counts"


def test_region_sets_are_disjoint_and_lie_on_the_seams():
    fr = df.frame("seam_ring_ab")  # test_gpu_denoise_frames.REGION_FRAME
    W, H = fr.W, fr.H
    dual = fr.valid()[2]
    sets = df.region_sets(W, H, ~dual)
    assert len(sets) == 7 and all(name.startswith("region_") for name in sets)
    for name, rects in sets.items():
        cover = np.zeros((H, W), dtype=np.int64)
        for (l, t, w, h) in rects:
            assert w > 0 and h > 0 and l >= 0 and t >= 0 and l + w <= W and t + h <= H, name
            cover[t : t + h, l : l + w] += 1
        assert cover.max() == 1, name
    assert [r[0] for r in sets["region_seam_columns"]] == [23, 24, 31, 32] and all(r[2] == 1 and r[3] == H for r in sets["region_seam_columns"])
    assert [r[0] for r in sets["region_beside_columns"]] == [22, 25, 30, 33]
    assert [r[1] for r in sets["region_seam_rows"]] == [15, 16] and [r[1] for r in sets["region_beside_rows"]] == [14, 17]
    assert len(sets["region_single_pixels"]) == 200 and sets["region_last_column"] == [(W - 1, 0, 1, H)]
    (l, t, w, h), = sets["region_invalid_only"]
    assert w * h >= 36 and not dual[t : t + h, l : l + w].any(), "region_invalid_only"
    assert dual.sum() > 0.75 * W * H and all(dual[:, x].any() and not dual[:, x].all() for x in (23, 24, 31)) and dual[[15, 16]].any()


# ---------------------------------------------------------------- which window takes which tile
def test_every_window_but_the_largest_takes_the_32_wide_tile(product_lib):
    """denoise_tile_width / denoise_lds_bytes, the functions the launchers size their launch with (through rmd_probe_denoise_tile): 24 wide at (12, 4)
    alone; the largest 32-wide layouts are (11, 4) and (12, 3); nothing exceeds the budget; and the sizes are the kernel's own carving of its LDS."""
    from raymond_amd import probe

    def carved(tw, r, f):  # denoise_kernel: six apron planes, the term image and its row sums in doubles, their taken-counts in 32-bit words
        AA = (tw + 2 * (r + f)) * (16 + 2 * (r + f))
        PP, HH = (tw + 2 * f) * (16 + 2 * f), (16 + 2 * f) * tw
        return (6 * AA + PP + HH) * 8 + (PP + HH) * 4

    table = {(r, f): probe.denoise_tile(r, f) for r in range(13) for f in range(5)}
    assert len(table) == 65
    for (r, f), (tw, lds, lds32, budget) in table.items():
        assert budget == 160 * 1024 and lds <= budget, (r, f)
        assert tw == (24 if (r, f) == (12, 4) else 32), (r, f)
        assert lds == carved(tw, r, f) and lds32 == carved(32, r, f), (r, f)
        assert (16 + 2 * f) * (tw + 2 * f) <= 3 * 16 * tw, (r, f)  # every term-image position has one of a thread's three slots
    assert table[(12, 3)][1] == 155376 and table[(11, 4)][1] == 157632 and table[(12, 4)][1:3] == (145152, 168192)
    assert sorted(table, key=lambda w: table[w][1] if table[w][0] == 32 else 0)[-2:] == [(12, 3), (11, 4)]
    for bad in ((13, 0), (0, 5)):
        with pytest.raises(RuntimeError):
            probe.denoise_tile(*bad)


# ---------------------------------------------------------------- the vectorised restatements against the pixel-by-pixel readings
CUT = (20, 10, 12, 9)  # x0, y0, w, h: columns 23, 24 and 31 and rows 15 and 16 of a SEAM frame
CUT_CLASSES = ["seam_columns_ab", "seam_row_b", "seam_checker_a", "seam_border_f", "seam_all_ab", "scale_2p200", "scale_2m200", "scale_mixed", "scale_overflow",
               "scale_cancel", "scale_counts", "shape_2x2", "shape_1x40", "shape_40x1"]


def _cut(name):
    fr = df.frame(name)
    if fr.W * fr.H <= 108 and min(fr.W, fr.H) <= 9 and max(fr.W, fr.H) <= 12:
        return fr
    if name == "scale_mixed":  # both scales in the cut
        return fr.crop(fr.W // 2 - 6, 10, 12, 9)
    if name == "scale_overflow":
        return fr.crop(fr.W // 2 - 6, 0, 12, 9)
    if name == "scale_counts":
        return fr.crop(fr.W // 3 - 5, 0, 12, 9)  # (two of the three counts)
    if fr.H == 1 or fr.W == 1:
        return fr.crop(0, 0, min(fr.W, 12), min(fr.H, 9)) if fr.H == 1 else fr.crop(0, 0, 1, 9)
    return fr.crop(*CUT)


@pytest.mark.parametrize("name", CUT_CLASSES)
def test_dual_restatements_equal_the_naive_readings_on_cut_classes(name):
    """The bars of test_denoise_dual_host.py and test_denoise_dual_guided_host.py: NaN at the same places, 4 ulp on the weighted means (numpy's exp of an
    array and of a scalar may differ in the last bit), err to 1e-9 relative."""
    fr = _cut(name)
    assert fr.W <= 12 and fr.H <= 9
    n_f = fr.n_f
    for r, f in ((2, 2), (1, 0)):
        params = dict(radius=r, patch_radius=f, k=fr.k, alpha=fr.alpha)
        pairs = [(denoise_dual_ref.denoise_dual(*fr.halves, fr.n_a, fr.n_b, **params), denoise_dual_ref.denoise_dual_naive(*fr.halves, fr.n_a, fr.n_b, **params)),
                 (dgref.denoise_dual_guided(*fr.halves, fr.n_a, fr.n_b, fr.F, fr.G, n_f, k_f=0.6, tau=1e-3, **params),
                  dgref.denoise_dual_guided_naive(*fr.halves, fr.n_a, fr.n_b, fr.F, fr.G, n_f, r, f, fr.k, fr.alpha, 0.6, 1e-3))]
        for (out, err), (out_n, err_n) in pairs:
            assert np.array_equal(np.isnan(out), np.isnan(out_n)) and np.array_equal(np.isnan(err), np.isnan(err_n)), name
            inf = np.isinf(out_n)
            assert np.array_equal(out[inf], out_n[inf]), name
            fin = np.isfinite(out_n)
            assert np.all(np.abs(out[fin] - out_n[fin]) <= 4 * np.spacing(np.abs(out_n[fin]))), name
            fin = np.isfinite(err_n)
            assert np.allclose(err[fin], err_n[fin], rtol=1e-9, atol=1e-30), name


@pytest.mark.parametrize("name", CUT_CLASSES)
def test_atrous_restatements_equal_the_by_pixel_readings_on_cut_classes(name):
    """The bar of test_denoise_atrous_host.py and test_denoise_atrous_dual_host.py: the same bytes."""
    fr = _cut(name)
    S, Q, _, _, n = fr.single()
    F1, G1 = fr.single_features()
    for levels in (1, 3):
        for feats in ((None, None), (F1, G1)):
            a = aref.atrous(S, Q, n, levels=levels, F=feats[0], G=feats[1])
            b = aref.atrous_by_pixel(S, Q, n, levels=levels, F=feats[0], G=feats[1])
            assert _bytes_equal(a, b), (name, levels, feats[0] is not None)
        for guide in ({}, dict(F=fr.F, G=fr.G, n_f=fr.n_f)):
            a = adref.atrous_dual(*fr.halves, fr.n_a, fr.n_b, levels=levels, **guide)
            b = adref.atrous_dual_by_pixel(*fr.halves, fr.n_a, fr.n_b, levels=levels, **guide)
            assert _bytes_equal(a[0], b[0]) and _bytes_equal(a[1], b[1]), (name, levels, bool(guide))


# ---------------------------------------------------------------- the table tool reads what the GPU file prints
def test_the_table_tool_reads_the_gpu_files_lines(capsys, tmp_path):
    import importlib.util
    import os

    import test_gpu_denoise_frames as tgf

    spec = importlib.util.spec_from_file_location("denoise_frames_table", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "denoise_frames_table.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tgf._note("rmd_denoise", "seam_ring_a", (3, 1), (3.4e-14, 0.002))
    tgf._note("rmd_denoise_atrous_dual:err", "shape_1x40", "8 levels, guided", 1.5e-13)
    tgf._note("rmd_denoise", "seam_ring_a", (12, 4), (1e-16, 0.5))
    log = tmp_path / "log"
    log.write_text("." + capsys.readouterr().out)  # (pytest's progress dot stands before a test's first line)
    tool.main(str(log), False)
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 2 and lines[0].split() == ["rmd_denoise", "seam_ring_a", "3.4e-14", "at", "3,1", "share", "0.002"], lines
    assert lines[1].split()[:3] == ["rmd_denoise_atrous_dual:err", "shape_1x40", "1.5e-13"], lines
