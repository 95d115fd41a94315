"""rmd_despike's refusals, without a GPU: every rule of include/raymond_hip.h comes with its own text, in the stated order — the frame and the rects, the
radius, the rank, k, ratio, floor, the four buffers, and only then the context — and all of it before the device is touched: every call here passes a
NULL context (and pointers that are no allocations), and a call that breaks no rule is refused for that context alone."""
import ctypes as C

import pytest

from raymond_amd import abi

W, H = 8, 8
SPAN = W * H * 3 * 8
BASE = 0x100000
BUFS = [C.c_void_p(BASE + i * SPAN) for i in range(4)]  # four ranges side by side: no two overlap


def rects_of(*rs):
    arr = (abi.TileRect * max(1, len(rs)))()
    for i, (l, t, w, h) in enumerate(rs):
        arr[i].left, arr[i].top, arr[i].width, arr[i].height = l, t, w, h
    return arr


FULL = rects_of((0, 0, W, H))
COUNTS = (C.c_uint32 * 2)(4, 4)


def call(L, S=BUFS[0], Q=BUFS[1], w=W, h=H, rects=FULL, cnt=COUNTS, n_rects=1, radius=2, rank=2, k=6.0, ratio=2.0, floor=0.0, oS=BUFS[2], oQ=BUFS[3], replaced=None):
    return L.rmd_despike(None, S, Q, w, h, rects, cnt, n_rects, radius, rank, k, ratio, floor, oS, oQ, replaced)


def last_error(L):
    return (L.rmd_last_error(None) or b"").decode()


def refused(L, text, **kw):
    assert call(L, **kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
    assert last_error(L) == ("rmd_despike: " + text if text != "null context" else text), (kw, last_error(L))


RULES = [  # in the header's order: (the rule's text, arguments that break it and nothing before it)
    ("bad argument", [dict(w=0), dict(h=0), dict(rects=None), dict(cnt=None)]),
    ("tile rectangle outside the framebuffer", [dict(rects=rects_of((0, 0, W + 1, H))), dict(rects=rects_of((4, 4, 4, 5))), dict(rects=rects_of((2**32 - 4, 0, 8, 8)))]),
    ("tile rectangles overlap", [dict(rects=rects_of((0, 0, 5, 5), (4, 4, 4, 4)), n_rects=2)]),
    ("radius must be 1 .. 3", [dict(radius=0), dict(radius=4), dict(radius=2**32 - 1)]),
    ("rank must be <= (2 * radius + 1)^2 - 2", [dict(radius=1, rank=8), dict(radius=2, rank=24), dict(radius=3, rank=48), dict(rank=2**32 - 1)]),
    ("k must be finite and >= 0", [dict(k=-1e-300), dict(k=float("nan")), dict(k=float("inf"))]),
    ("ratio must be finite and >= 1", [dict(ratio=0.999), dict(ratio=float("nan")), dict(ratio=float("inf")), dict(ratio=-2.0)]),
    ("floor must be finite and >= 0", [dict(floor=-1e-300), dict(floor=float("nan")), dict(floor=float("inf"))]),
    ("the four sum buffers must not be NULL", [dict(S=None), dict(Q=None), dict(oS=None), dict(oQ=None)]),
    ("accum_dev, accum_sq_dev, out_accum_dev and out_accum_sq_dev must not alias",
     [dict(Q=BUFS[0]), dict(oS=BUFS[0]), dict(oQ=BUFS[1]), dict(oQ=BUFS[2]), dict(oS=C.c_void_p(BASE + SPAN - 8)), dict(oQ=C.c_void_p(BASE + 2 * SPAN + 8)),
      dict(S=C.c_void_p(BASE + 3 * SPAN + SPAN - 8))]),
    ("null context", [dict(), dict(rects=None, cnt=None, n_rects=0), dict(n_rects=0), dict(rects=rects_of((3, 3, 0, 2))), dict(radius=1, rank=7), dict(radius=3, rank=47),
                      dict(k=0.0, ratio=1.0, floor=0.0), dict(replaced=(C.c_uint32 * 2)()), dict(cnt=(C.c_uint32 * 2)(0, 0)),
                      dict(rects=rects_of((0, 0, 4, 8), (4, 0, 4, 8)), n_rects=2)]),
]


@pytest.mark.parametrize("text,breaking", RULES, ids=[r[0].replace(" ", "_")[:40] for r in RULES])
def test_every_rule_has_its_text_and_comes_before_the_context(product_lib, text, breaking):
    for kw in breaking:
        refused(product_lib, text, **kw)


def test_the_rules_are_checked_in_the_stated_order(product_lib):
    """One breaking argument of every rule, accumulated from the last rule to the first: the earliest broken rule is the one reported."""
    firsts = [(text, breaking[0]) for text, breaking in RULES]
    broken = {}
    for text, kw in reversed(firsts):
        if text == "tile rectangles overlap":  # (it shares its arguments with the rule before it: checked on its own below)
            continue
        broken.update(kw)
        refused(product_lib, text, **broken)
    # the rects come before every parameter and buffer, an overlap after a rect outside the frame
    later = dict(radius=0, rank=99, k=-1.0, ratio=0.0, floor=-1.0, S=None, oQ=BUFS[0])
    refused(product_lib, "tile rectangles overlap", rects=rects_of((0, 0, 5, 5), (4, 4, 4, 4)), n_rects=2, **later)
    refused(product_lib, "tile rectangle outside the framebuffer", rects=rects_of((0, 0, 5, 5), (4, 4, 4, 5)), n_rects=2, **later)
    # the rank is judged against the radius given, once that is legal
    refused(product_lib, "radius must be 1 .. 3", radius=4, rank=79)
    refused(product_lib, "rank must be <= (2 * radius + 1)^2 - 2", radius=1, rank=23)
    # NULL buffers before aliasing ones
    refused(product_lib, "the four sum buffers must not be NULL", S=None, oS=BUFS[1])


def test_replaced_host_is_untouched_by_a_refused_call(product_lib):
    replaced = (C.c_uint32 * 2)(0xABABABAB, 0xABABABAB)
    for kw in (dict(), dict(radius=0), dict(oS=None)):
        assert call(product_lib, replaced=replaced, **kw) == abi.RMD_ERR_INVALID_ARGUMENT
        assert list(replaced) == [0xABABABAB, 0xABABABAB]
