"""The refusals of the frame calls that only a live context reaches, by status and by the exact text of rmd_last_error: the tile transfers,
rmd_resolve_tonemap, rmd_resolve_tonemap_tiles, rmd_tile_error's and rmd_render_tiles's rect rule.  Each of these calls looks at its context first, so
the host-only tests, which pass a NULL context, never get this far.  The texts are written out here as the C header's callers see them.  After the
refusals the tile transfers still work: a refused transfer has taken one of the two staging slots, and the slots keep rotating.  A 16 x 16 frame."""
import ctypes as C

import numpy as np
import pytest

from raymond_amd import abi, render, scenes
from raymond_amd.scene import Settings, tile_array

pytestmark = pytest.mark.gpu

W = H = 16
INVALID, UNSUPPORTED = abi.RMD_ERR_INVALID_ARGUMENT, abi.RMD_ERR_UNSUPPORTED
PAST_RIGHT_EDGE = (W - 7, 0, 8, 8)
WRAPS = (2**32 - 4, 0, 8, 8)  # left + width = 4 in 32 bits
OUTSIDE = "tile rectangle outside the framebuffer"


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _refused(ctx, status, want_status, want_text, what):
    text = (ctx.L.rmd_last_error(ctx.handle) or b"").decode()
    assert (status, text) == (want_status, want_text), what


@pytest.fixture()
def fb(gpu_ctx):
    f = render.Framebuffer(gpu_ctx, W, H)
    yield f
    f.close()


def test_tile_transfers_refuse_and_then_still_work(gpu_ctx, fb):
    L, h = gpu_ctx.L, gpu_ctx.handle
    two = [(0, 0, 8, 8), (8, 8, 8, 8)]
    packed = np.full(2 * 64 * 3, 7.0)

    def download(dev=fb.ptr, width=W, rects=two, n=None, host=packed, rects_ptr=True):
        return L.rmd_framebuffer_download_tiles(h, dev, width, H, tile_array(rects) if rects_ptr else None, len(rects) if n is None else n, _ptr(host))

    def upload(dev=fb.ptr, width=W, rects=two, n=None, host=packed, rects_ptr=True):
        return L.rmd_framebuffer_upload_tiles(h, _ptr(host), dev, width, H, tile_array(rects) if rects_ptr else None, len(rects) if n is None else n)

    for name, call in (("rmd_framebuffer_download_tiles", download), ("rmd_framebuffer_upload_tiles", upload)):
        for what, kw in (("NULL buffer", dict(dev=None)), ("NULL host buffer", dict(host=None)), ("zero width", dict(width=0)),
                         ("NULL rects with n_rects > 0", dict(rects_ptr=False, n=2))):
            _refused(gpu_ctx, call(**kw), INVALID, name + ": bad argument", (name, what))
        for what, rect in (("past the right edge", PAST_RIGHT_EDGE), ("left + width wraps", WRAPS)):
            _refused(gpu_ctx, call(rects=[two[0], rect]), INVALID, "tile transfer: " + OUTSIDE, (name, what))
        assert call(rects=[], rects_ptr=False) == abi.RMD_OK, name  # n_rects = 0 with NULL rects
    assert (packed == 7.0).all()  # no refused download wrote
    # download, upload, download: what was uploaded comes back, and the pixels outside the rects stay what they were
    rng = np.random.default_rng(11)
    frame = rng.uniform(size=(H, W, 3))
    fb.upload(frame)
    first = [t.copy() for t in fb.download_tiles(two)]
    assert all(np.array_equal(t, frame[y : y + th, x : x + tw]) for t, (x, y, tw, th) in zip(first, two))
    fresh = [rng.uniform(size=(8, 8, 3)) for _ in two]
    fb.upload_tiles(two, fresh)
    assert all(np.array_equal(a, b) for a, b in zip(fb.download_tiles(two), fresh))
    want = frame.copy()
    for t, (x, y, tw, th) in zip(fresh, two):
        want[y : y + th, x : x + tw] = t
    assert np.array_equal(fb.download(), want)
    # the slot rotation: two downloads nobody has waited for, then a third, which takes the first one's slot
    lists = ([(0, 0, 8, 8)], [(8, 0, 8, 8), (0, 8, 8, 8)], [(3, 5, 9, 6)])
    outs = [np.zeros(sum(tw * th for _, _, tw, th in r) * 3) for r in lists]
    for rects, out in zip(lists[:2], outs[:2]):
        assert L.rmd_framebuffer_download_tiles_async(h, fb.ptr, W, H, tile_array(rects), len(rects), _ptr(out)) == abi.RMD_OK
    assert L.rmd_framebuffer_download_tiles(h, fb.ptr, W, H, tile_array(lists[2]), 1, _ptr(outs[2])) == abi.RMD_OK
    for rects, out in zip(lists, outs):
        assert np.array_equal(out, np.concatenate([want[y : y + th, x : x + tw].reshape(-1) for x, y, tw, th in rects])), rects


def test_resolve_tonemap_refusals(gpu_ctx, fb):
    L, h = gpu_ctx.L, gpu_ctx.handle
    out = np.full(W * H * 3, 0xAB, dtype=np.uint8)
    for what, args in (("NULL sums", (None, W, H, 4, 1.0, 2.2, _ptr(out))), ("NULL output", (fb.ptr, W, H, 4, 1.0, 2.2, None)),
                       ("sample_count 0", (fb.ptr, W, H, 0, 1.0, 2.2, _ptr(out)))):
        _refused(gpu_ctx, L.rmd_resolve_tonemap(h, *args), INVALID, "rmd_resolve_tonemap: bad argument", what)
    assert (out == 0xAB).all()


def test_resolve_tonemap_tiles_refusals_by_their_texts(gpu_ctx, fb):
    L, h = gpu_ctx.L, gpu_ctx.handle
    name = "rmd_resolve_tonemap_tiles: "
    out = np.full(W * H * 3, 0xAB, dtype=np.uint8)
    ok = [(0, 0, 8, 8), (8, 8, 8, 8)]

    def call(dev=fb.ptr, second=None, width=W, height=H, rects=ok, counts_ptr=True, host=out):
        counts = np.full(len(rects), 2, dtype=np.uint32)
        return L.rmd_resolve_tonemap_tiles(h, dev, second, width, height, tile_array(rects), counts.ctypes.data_as(C.POINTER(C.c_uint32)) if counts_ptr else None,
                                           len(rects), 1.0, 2.2, _ptr(host))

    inside = C.c_void_p(fb.ptr.value + 8 * 3 * W * (H // 2))  # half a frame further
    for what, kw, text in (("NULL sums", dict(dev=None), "bad argument"), ("zero width", dict(width=0), "bad argument"), ("NULL counts", dict(counts_ptr=False), "bad argument"),
                           ("second buffer is the first", dict(second=fb.ptr), "accum2_dev overlaps accum_dev"), ("second buffer inside the first", dict(second=inside), "accum2_dev overlaps accum_dev"),
                           ("rect past the right edge", dict(rects=[ok[0], PAST_RIGHT_EDGE]), OUTSIDE), ("left + width wraps", dict(rects=[WRAPS, ok[1]]), OUTSIDE),
                           ("NULL output", dict(host=None), "null output for rects that hold pixels")):
        _refused(gpu_ctx, call(**kw), INVALID, name + text, what)
    big = 70000  # a frame description large enough, never touched: the call is refused before the device is
    _refused(gpu_ctx, call(width=big, height=big, rects=[(0, 0, big, big)]), UNSUPPORTED, name + "more than 2^32-1 packed pixels", "2^32 - 1")
    assert (out == 0xAB).all()


def test_rects_outside_the_frame_in_tile_error_and_render(gpu_ctx, fb):
    L, h = gpu_ctx.L, gpu_ctx.handle
    sq = render.Framebuffer(gpu_ctx, W, H)
    ds = render.DeviceScene(gpu_ctx, scenes.reflective_spheres())
    try:
        err = np.zeros(2)
        for what, rect in (("past the right edge", PAST_RIGHT_EDGE), ("left + width wraps", WRAPS)):
            status = L.rmd_tile_error(h, fb.ptr, sq.ptr, W, H, 4, 1e-3, tile_array([(0, 0, 8, 8), rect]), 2, _ptr(err))
            _refused(gpu_ctx, status, INVALID, "rmd_tile_error: " + OUTSIDE, what)
        st = Settings(scenes.camera(W, H), sample_count=1, bounce_limit=1, seed=scenes.SEED)
        cam, pod = st.camera_settings.pod(), st.pod(0, 1)

        def render_rects(rects):
            return L.rmd_render_tiles(h, ds.handle, C.byref(cam), C.byref(pod), tile_array(rects), len(rects), fb.ptr)

        _refused(gpu_ctx, render_rects([(W, 0, 8, 8)]), INVALID, "rmd_render_tiles: tile rectangle outside the backbuffer", "a rect with pixels right of the frame")
        assert render_rects([(W, 0, 0, 8)]) == abi.RMD_OK  # a rect without pixels at the same place renders nothing
        assert (fb.download() == 0.0).all()
    finally:
        ds.close(), sq.close()
