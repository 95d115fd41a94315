"""rmd_despike_dual's refusals, without a GPU: every rule of include/raymond_hip.h comes with its own text, in the stated order — the frame and the rects
with both count arrays, the two counts' sum, the radius, the rank, k, ratio, floor, the eight buffers, and only then the context — and all of it before the
device is touched: every call here passes a NULL context (and pointers that are no allocations), and a call that breaks no rule is refused for that
context alone.  The parameter rules carry rmd_despike's texts."""
import ctypes as C
import itertools

import pytest

from raymond_amd import abi

W, H = 8, 8
SPAN = W * H * 3 * 8
BASE = 0x100000
NAMES = ("SA", "QA", "SB", "QB", "oSA", "oQA", "oSB", "oQB")
BUFS = {name: C.c_void_p(BASE + i * SPAN) for i, name in enumerate(NAMES)}  # eight ranges side by side: no two overlap


def rects_of(*rs):
    arr = (abi.TileRect * max(1, len(rs)))()
    for i, (l, t, w, h) in enumerate(rs):
        arr[i].left, arr[i].top, arr[i].width, arr[i].height = l, t, w, h
    return arr


FULL = rects_of((0, 0, W, H))
COUNTS = (C.c_uint32 * 2)(4, 4)
NOT_NULL = "the eight sum buffers must not be NULL"
ALIAS = "the four input and the four output sum buffers must not alias"


def call(L, w=W, h=H, rects=FULL, ca=COUNTS, cb=COUNTS, n_rects=1, radius=2, rank=2, k=6.0, ratio=2.0, floor=0.0, replaced=None, **bufs):
    b = dict(BUFS, **bufs)
    return L.rmd_despike_dual(None, b["SA"], b["QA"], b["SB"], b["QB"], w, h, rects, ca, cb, n_rects, radius, rank, k, ratio, floor, b["oSA"], b["oQA"], b["oSB"], b["oQB"],
                              replaced)


def last_error(L):
    return (L.rmd_last_error(None) or b"").decode()


def refused(L, text, **kw):
    assert call(L, **kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
    assert last_error(L) == ("rmd_despike_dual: " + text if text != "null context" else text), (kw, last_error(L))


def u32(*v):
    return (C.c_uint32 * max(2, len(v)))(*v)


RULES = [  # in the header's order: (the rule's text, arguments that break it and nothing before it)
    ("bad argument", [dict(w=0), dict(h=0), dict(rects=None), dict(ca=None), dict(cb=None)]),
    ("tile rectangle outside the framebuffer", [dict(rects=rects_of((0, 0, W + 1, H))), dict(rects=rects_of((4, 4, 4, 5))), dict(rects=rects_of((2**32 - 4, 0, 8, 8)))]),
    ("tile rectangles overlap", [dict(rects=rects_of((0, 0, 5, 5), (4, 4, 4, 4)), n_rects=2)]),
    ("a rect's two counts must not add to more than 2^32 - 1",
     [dict(ca=u32(2**32 - 1), cb=u32(1)), dict(ca=u32(2**31), cb=u32(2**31)), dict(rects=rects_of((0, 0, 4, 8), (4, 0, 4, 8)), n_rects=2, ca=u32(1, 2**32 - 2), cb=u32(1, 2)),
      dict(rects=rects_of((3, 3, 0, 2)), ca=u32(2**32 - 1), cb=u32(2**32 - 1))]),  # (a rect without pixels is held to the rule too)
    ("radius must be 1 .. 3", [dict(radius=0), dict(radius=4), dict(radius=2**32 - 1)]),
    ("rank must be <= (2 * radius + 1)^2 - 2", [dict(radius=1, rank=8), dict(radius=2, rank=24), dict(radius=3, rank=48), dict(rank=2**32 - 1)]),
    ("k must be finite and >= 0", [dict(k=-1e-300), dict(k=float("nan")), dict(k=float("inf"))]),
    ("ratio must be finite and >= 1", [dict(ratio=0.999), dict(ratio=float("nan")), dict(ratio=float("inf")), dict(ratio=-2.0)]),
    ("floor must be finite and >= 0", [dict(floor=-1e-300), dict(floor=float("nan")), dict(floor=float("inf"))]),
    (NOT_NULL, [{name: None} for name in NAMES]),
    (ALIAS, [dict(oSA=C.c_void_p(BASE + SPAN - 8)), dict(oQB=C.c_void_p(BASE + 6 * SPAN + 8)), dict(SA=C.c_void_p(BASE + 7 * SPAN + SPAN - 8))]),
    ("null context", [dict(), dict(rects=None, ca=None, cb=None, n_rects=0), dict(n_rects=0), dict(rects=rects_of((3, 3, 0, 2))), dict(radius=1, rank=7), dict(radius=3, rank=47),
                      dict(k=0.0, ratio=1.0, floor=0.0), dict(replaced=(C.c_uint32 * 2)()), dict(ca=u32(0), cb=u32(0)), dict(ca=u32(2**32 - 2), cb=u32(1)),
                      dict(ca=u32(0), cb=u32(2**32 - 1)), dict(rects=rects_of((0, 0, 4, 8), (4, 0, 4, 8)), n_rects=2)]),
]


@pytest.mark.parametrize("text,breaking", RULES, ids=[r[0].replace(" ", "_")[:40] for r in RULES])
def test_every_rule_has_its_text_and_comes_before_the_context(product_lib, text, breaking):
    for kw in breaking:
        refused(product_lib, text, **kw)


@pytest.mark.parametrize("first,second", list(itertools.combinations(NAMES, 2)), ids=lambda n: n)
def test_no_two_of_the_eight_ranges_may_overlap(product_lib, first, second):
    """One test per pair: the second buffer at the first's address, one double into it, and one double before its end."""
    at = BUFS[first].value
    for address in (at, at + 8, at + SPAN - 8):
        refused(product_lib, ALIAS, **{second: C.c_void_p(address)})
    at = BUFS[second].value  # ... and the other way round, where the neighbours' own ranges allow it
    refused(product_lib, ALIAS, **{first: C.c_void_p(at)})


def test_the_rules_are_checked_in_the_stated_order(product_lib):
    """One breaking argument of every rule, accumulated from the last rule to the first: the earliest broken rule is the one reported."""
    firsts = [(text, breaking[0]) for text, breaking in RULES]
    broken = {}
    for text, kw in reversed(firsts):
        if text == "tile rectangles overlap":  # (it shares its arguments with the rule before it: checked on its own below)
            continue
        broken.update(kw)
        refused(product_lib, text, **broken)
    # the rects come before the counts' sum, every parameter and buffer; an overlap after a rect outside the frame
    later = dict(ca=u32(2**32 - 1, 1), cb=u32(1, 1), radius=0, rank=99, k=-1.0, ratio=0.0, floor=-1.0, SA=None, oQB=BUFS["SA"])
    refused(product_lib, "tile rectangles overlap", rects=rects_of((0, 0, 5, 5), (4, 4, 4, 4)), n_rects=2, **later)
    refused(product_lib, "tile rectangle outside the framebuffer", rects=rects_of((0, 0, 5, 5), (4, 4, 4, 5)), n_rects=2, **later)
    # the counts' sum before the radius
    refused(product_lib, "a rect's two counts must not add to more than 2^32 - 1", ca=u32(2**32 - 1), cb=u32(1), radius=0, SA=None)
    # the rank is judged against the radius given, once that is legal
    refused(product_lib, "radius must be 1 .. 3", radius=4, rank=79)
    refused(product_lib, "rank must be <= (2 * radius + 1)^2 - 2", radius=1, rank=23)
    # NULL buffers before aliasing ones
    refused(product_lib, NOT_NULL, SB=None, oSA=BUFS["QA"])


def test_replaced_host_is_untouched_by_a_refused_call(product_lib):
    replaced = (C.c_uint32 * 2)(0xABABABAB, 0xABABABAB)
    for kw in (dict(), dict(radius=0), dict(oSA=None), dict(ca=u32(2**32 - 1), cb=u32(1))):
        assert call(product_lib, replaced=replaced, **kw) == abi.RMD_ERR_INVALID_ARGUMENT
        assert list(replaced) == [0xABABABAB, 0xABABABAB]
