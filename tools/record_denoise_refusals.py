#!/usr/bin/env python3
"""What the ten denoise entry points and rmd_tile_error_dual answer to bad arguments, and in which order they check them:

    RAYMOND_HIP_LIB=<a build of the commit to record> python tools/record_denoise_refusals.py --recorded-from <that commit> \\
        --out tests/golden/denoise_refusals.json

Every call has a NULL context, an 8 x 8 frame and fake addresses that do not overlap, so no device is touched: a refused argument comes back with its
own text, an accepted call with "null context".  Per entry point the fixed list holds every single fault, every ordered pair (a, b) of two different
faults — the arguments of a, then those of b on top — and the valid variants.  Each case is recorded as its status and last-error text;
tests/test_denoise_refusals_host.py replays the list against the library under test and wants every case equal.

The file, per entry point: "outcomes" is its table of (status, text) pairs, "singles" and "valid" are {case id: outcome index}, "pairs" a matrix over the
single faults in their order, a string per row: character j of pairs[i] is the outcome index of case "<single i> + <single j>" (CELLS), "." on the
diagonal.  No case is left out.
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import abi, lib  # noqa: E402

W = H = 8
SPAN, FSPAN = W * H * 3 * 8, W * H * 7 * 8
BASE = 0x100000
SA, QA, SB, QB, OUT, ERR = (BASE + i * SPAN for i in range(6))  # (err_dev's W*H doubles get a span of their own)
FE = BASE + 6 * SPAN
GE, SURE = FE + FSPAN, FE + 2 * FSPAN
WIN = SURE + SPAN
FULL, SOME = ((0, 0, 8, 8),), ((1, 2, 3, 4),)
NAN, INF = float("nan"), float("inf")
CAND = dict(k=3.0, alpha=1.0, k_f=1.0, tau=1e-2, guided=0, reserved=0)
GUIDED = dict(CAND, guided=1)

# the arguments after the context, in the header's order, with the value of a good call
_SUMS1 = [("S", SA), ("Q", QA)]
_SUMS2 = [("SA", SA), ("QA", QA), ("SB", SB), ("QB", QB)]
_FEAT = [("F", FE), ("G", GE)]
_FRAME1 = [("w", W), ("h", H), ("rects", FULL), ("ca", "counts"), ("n_rects", 1)]
_FRAME2 = [("w", W), ("h", H), ("rects", FULL), ("ca", "counts"), ("cb", "counts"), ("n_rects", 1)]
_FRAME3 = [("w", W), ("h", H), ("rects", FULL), ("ca", "counts"), ("cb", "counts"), ("cf", "counts"), ("n_rects", 1)]
_REGION = [("region", SOME), ("n_region", 1)]
_WINDOW = [("radius", 5), ("patch", 1)]
_LEVELS = [("levels", 5)]
_KA, _KT = [("k", 3.0), ("alpha", 1.0)], [("kf", 1.0), ("tau", 1e-2)]
_OUT1, _OUT2 = [("out", OUT)], [("out", OUT), ("err", ERR)]
ENTRY_POINTS = {
    "rmd_denoise": _SUMS1 + _FRAME1 + _WINDOW + _KA + _OUT1,
    "rmd_denoise_guided": _SUMS1 + _FEAT + _FRAME1 + _WINDOW + _KA + _KT + _OUT1,
    "rmd_denoise_atrous": _SUMS1 + _FEAT + _FRAME1 + _LEVELS + _KA + _KT + _OUT1,
    "rmd_denoise_dual": _SUMS2 + _FRAME2 + _WINDOW + _KA + _OUT2,
    "rmd_denoise_dual_region": _SUMS2 + _FRAME2 + _REGION + _WINDOW + _KA + _OUT2,
    "rmd_denoise_dual_guided": _SUMS2 + _FEAT + _FRAME3 + _WINDOW + _KA + _KT + _OUT2,
    "rmd_denoise_dual_guided_region": _SUMS2 + _FEAT + _FRAME3 + _REGION + _WINDOW + _KA + _KT + _OUT2,
    "rmd_denoise_dual_select": _SUMS2 + _FEAT + _FRAME3 + _WINDOW + [("cands", (CAND, GUIDED)), ("n_cands", 2), ("sure_window", 2), ("select_window", 1)] + _OUT2
    + [("sure", SURE), ("win", WIN)],
    "rmd_denoise_atrous_dual": _SUMS2 + _FEAT + _FRAME3 + _LEVELS + _KA + _KT + _OUT2,
    "rmd_denoise_atrous_dual_region": _SUMS2 + _FEAT + _FRAME3 + _REGION + _LEVELS + _KA + _KT + _OUT2,
    "rmd_tile_error_dual": [("err", ERR), ("w", W), ("h", H), ("rects", FULL), ("n_rects", 1), ("out_host", "host")],
}


def _dedup(items):
    seen, out = set(), []
    for kw in items:
        if case_id(kw) not in seen:
            seen.add(case_id(kw))
            out.append(kw)
    return out


def _faults(name):
    """The single faults of one entry point and its valid variants: every one that the argument-rule tests of the suite try on any entry point of its
    family (tests/test_denoise*_host.py: *argument_rules_without_a_device), restated in this file's addresses and given to every entry point that
    has the argument."""
    good = dict(ENTRY_POINTS[name])
    has = set(good)
    if name == "rmd_tile_error_dual":
        f = [dict(err=None), dict(w=0), dict(h=0), dict(rects=None), dict(out_host=None), dict(rects=((0, 0, 9, 8),)), dict(rects=((4, 4, 4, 5),)),
             dict(rects=((1, 0, 8, 8),)), dict(rects=((0, 7, 1, 2),)), dict(rects=((2**32 - 1, 0, 2, 1),))]
        return f, [{}, dict(rects=None, out_host=None, n_rects=0), dict(rects=((0, 0, 4, 4), (3, 3, 2, 2)), n_rects=2), dict(rects=((8, 8, 0, 0),))]
    dual, select = "SB" in has, name == "rmd_denoise_dual_select"
    s, q = ("SA", "QA") if dual else ("S", "Q")
    f = [{k: None} for k in (s, q, "SB", "QB", "out", "rects", "ca", "cb") if k in has] + [dict(w=0), dict(h=0)]
    valid = [{}, dict(rects=((0, 0, 4, 8), (4, 0, 4, 8)), n_rects=2), dict(rects=((0, 0, 0, 8), (0, 0, 8, 8)), n_rects=2),
             {k: None for k in ("rects", "ca", "cb", "cf") if k in has} | dict(n_rects=0)]
    # aliasing: every buffer in every other's place, then partial overlaps; err_dev inside out_dev, reaching into it, its last double on accum_a_dev's first
    ptrs = [k for k in (s, q, "SB", "QB", "out", "err", "sure", "win") if k in has]
    f += [{a: good[b]} for a in ptrs for b in ptrs if a != b]
    f += [{q: BASE + SPAN - 8}, {s: BASE + SPAN - 8}, {q: BASE + 8}, dict(out=BASE + 8), dict(out=BASE + 2 * SPAN - 8)]
    if dual:
        f += [dict(SB=BASE + SPAN - 8), dict(QB=BASE + 8), dict(err=OUT + 8), dict(err=ERR - 8), dict(err=ERR - SPAN // 3 + 8), dict(err=BASE - W * H * 8 + 8)]
        valid += [dict(err=None), dict(err=BASE - W * H * 8)]
    if "F" in has:
        f += [dict(F=None), dict(G=None), dict(G=FE), dict(G=FE + 8), dict(G=GE - 8), dict(F=ERR + 8 if dual else OUT + 8)]
        # a feature range on another buffer: the dual forms refuse every one, the single-buffer forms only out_dev's (their sums are not compared with it)
        on_buffers = [{k: good[b]} for b in ptrs for k in ("F", "G")] + [dict(G=BASE - FSPAN + 8)]
        f += [kw for kw in on_buffers if dual or OUT in kw.values()]
        valid += [kw for kw in on_buffers if not (dual or OUT in kw.values())]
        f += [dict(out=GE - 8, err=None), dict(out=GE + FSPAN - 8, err=None)] if dual else [dict(out=GE - 8), dict(out=GE - 8, Q=BASE + 8 * SPAN)]
        if dual:
            f += [dict(F=ERR + W * H * 8 - 8)]
        valid += [dict(G=BASE - FSPAN)]
        (f if select else valid).append(dict(F=None, G=None))  # (the good call of rmd_denoise_dual_select has a guided candidate)
        if "cf" in has:
            f += [dict(cf=None)]
            (f if select else valid).append(dict(F=None, G=None, cf=None))
    if "radius" in has:
        f += [dict(radius=13), dict(radius=2**32 - 1), dict(patch=5)]
        valid += [dict(radius=12, patch=4), dict(radius=0, patch=0)]
    if "levels" in has:
        f += [dict(levels=9), dict(levels=2**32 - 1)]
        valid += [dict(levels=0), dict(levels=8)]
    if "k" in has:
        f += [dict(k=bad) for bad in (0.0, -3.0, -0.45, NAN, INF)] + [dict(alpha=bad) for bad in (-1e-300, -1.0, NAN, INF)]
        valid += [dict(alpha=0.0), dict(k=1e-300)]
    if "kf" in has:
        f += [dict(kf=bad) for bad in (0.0, -3.0, -0.6, -1.0, NAN, INF)] + [dict(tau=bad) for bad in (0.0, -3.0, -0.6, -1.0, NAN, INF)]
        valid += [dict(F=None, G=None, kf=NAN, tau=-1.0), dict(F=None, G=None, cf=None, kf=NAN, tau=-1.0) if "cf" in has else dict(kf=1e-300, tau=1e-300),
                  dict(kf=1e-300, tau=1e-300)]
    if select:
        f += [dict(cands=None), dict(n_cands=0), dict(n_cands=5), dict(n_cands=5, cands=(CAND,) * 5), dict(sure_window=6), dict(select_window=6), dict(sure=OUT + 8),
              dict(sure=ERR + 8), dict(win=ERR + 8), dict(win=SURE + 8), dict(win=BASE - W * H * 4 + 4)]
        f += [dict(cands=(CAND, dict(GUIDED, reserved=1))), dict(cands=(CAND, dict(CAND, reserved=1))), dict(cands=(dict(CAND, reserved=7), dict(GUIDED, tau=0.0)))]
        for v in (0.0, -0.45, -3.0, NAN, INF):
            f += [dict(cands=(dict(CAND, k=v), GUIDED)), dict(cands=(CAND, dict(CAND, k=v))), dict(cands=(CAND, dict(GUIDED, k=v))), dict(cands=(CAND, dict(GUIDED, k_f=v))),
                  dict(cands=(CAND, dict(GUIDED, tau=v)))]
        f += [dict(cands=(dict(CAND, alpha=a), GUIDED)) for a in (-1e-300, -1.0, NAN, INF)] + [dict(cands=(CAND, dict(GUIDED, alpha=a))) for a in (-1.0, INF)]
        valid += [dict(F=None, G=None, cf=None, cands=(CAND, dict(CAND, k_f=NAN, tau=-1.0))), dict(cf=None, cands=(CAND, dict(CAND, k=1.0))), dict(n_cands=1),
                  dict(n_cands=4, cands=tuple(dict(CAND, guided=i & 1) for i in range(4))), dict(err=None), dict(sure=None), dict(win=None),
                  dict(sure=None, win=None, err=None), dict(radius=12, patch=4, sure_window=5, select_window=5), dict(radius=0, patch=0, sure_window=0, select_window=0)]
    f += [dict(rects=((0, 0, 9, 8),)), dict(rects=((4, 4, 4, 5),)), dict(rects=((0, 0, 4, 4), (8, 0, 1, 1)), n_rects=2), dict(rects=((0, 0, 4, 4), (3, 3, 2, 2)), n_rects=2),
          dict(rects=((0, 0, 8, 8), (0, 0, 8, 8)), n_rects=2)]
    if "region" in has:
        f += [dict(region=None), dict(region=((0, 0, 9, 8),)), dict(region=((0, 0, 4, 4), (8, 0, 1, 1)), n_region=2), dict(region=((2**32 - 1, 0, 2, 1),)),
              dict(region=((0, 0, 4, 4), (3, 3, 2, 2)), n_region=2)]
        valid += [dict(region=None, n_region=0), dict(n_region=0), dict(region=FULL), dict(region=((0, 0, 1, 1), (7, 7, 1, 1), (3, 1, 4, 5)), n_region=3),
                  dict(region=((1, 1, 3, 5), (5, 0, 3, 3)), n_region=2), dict(region=((8, 8, 0, 0), (0, 0, 0, 8), (0, 0, 8, 8)), n_region=3),
                  dict(rects=((0, 0, 4, 8), (4, 0, 4, 8)), n_rects=2, region=((3, 0, 2, 8),))]
    return _dedup(f), _dedup(valid)


def case_id(kw):
    return ", ".join("%s=%r" % (k, v) for k, v in kw.items()) or "good"


def cases(name):
    """[(kind, case id, arguments that differ from the good call)] of one entry point, in the file's order."""
    faults, valid = _faults(name)
    out = [("singles", case_id(a), a) for a in faults]
    out += [("pairs", case_id(a) + " + " + case_id(b), {**a, **b}) for a in faults for b in faults if a is not b]
    return out + [("valid", case_id(v), v) for v in valid]


def _rects(rs):
    if rs is None:
        return None
    arr = (abi.TileRect * max(1, len(rs)))()
    for i, (l, t, w, h) in enumerate(rs):
        arr[i].left, arr[i].top, arr[i].width, arr[i].height = l, t, w, h
    return arr


def call(L, name, kw):
    """-> (status, last-error text) of one case."""
    keep, args = [], []
    for key, good in ENTRY_POINTS[name]:
        v = kw.get(key, good)
        if key in ("rects", "region"):
            v = _rects(v)
        elif key == "cands" and v is not None:
            v = (abi.DenoiseCandidate * len(v))(*(abi.DenoiseCandidate(**c) for c in v))
        elif v == "counts":
            v = (C.c_uint32 * 4)(4, 4, 4, 4)
        elif v == "host":
            v = C.cast((C.c_double * 4)(), C.c_void_p)
        keep.append(v)
        args.append(v)
    status = getattr(L, name)(None, *args)
    del keep
    return int(status), (L.rmd_last_error(None) or b"").decode()


CELLS = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"  # a pair's outcome, one character: its index in the entry point's own outcomes


def record(L, recorded_from):
    about = ("tools/record_denoise_refusals.py; recorded from: %s.  Per entry point: outcomes = its [status, last-error text] pairs; singles / valid = "
             "{case id: outcome index}; pairs = one string per single fault i, whose character j is the outcome index (in 0-9A-Za-z) of the case "
             "'<single i> + <single j>' (j's arguments on top of i's), '.' on the diagonal.  Every ordered pair is kept." % recorded_from)
    doc = {"about": about, "frame": [W, H], "entry_points": {}}
    for name in ENTRY_POINTS:
        n = len(_faults(name)[0])
        outcomes = []
        e = {"outcomes": outcomes, "singles": {}, "pairs": [["."] * n for _ in range(n)], "valid": {}}
        pair = ((i, j) for i in range(n) for j in range(n) if i != j)
        for kind, cid, kw in cases(name):
            o = list(call(L, name, kw))
            if o not in outcomes:
                outcomes.append(o)
            if kind == "pairs":
                i, j = next(pair)
                e["pairs"][i][j] = CELLS[outcomes.index(o)]
            else:
                e[kind][cid] = outcomes.index(o)
        e["pairs"] = ["".join(row) for row in e["pairs"]]
        doc["entry_points"][name] = e
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--recorded-from", required=True, help="what RAYMOND_HIP_LIB was built from, for the file's header (a commit, say)")
    a = ap.parse_args()
    doc = record(lib.load(), a.recorded_from)
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    n = sum(len(e["singles"]) ** 2 + len(e["valid"]) for e in doc["entry_points"].values())
    print("%d cases -> %s (%d bytes)" % (n, a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
