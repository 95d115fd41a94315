"""Host-side mirror of the reference's render API over the C-ABI.

`render_tiled(scene, settings) -> TaskHandle` keeps the reference's shape (src/trace.rs:137-230,
TaskHandle :70-135): the framebuffer is split into tiles in the reference's column-major order
(:142-173), tiles are handed to workers, finished tiles come back as `Message.TileFinished` and
`TaskHandle.await_()` assembles the W*H image divided by the sample count (:82-113).  The one
difference is what a worker is: a GPU context that runs rmd_render_tiles over its share of the
tiles (the per-pixel body :197-205 for ALL pixels of those tiles at once) instead of an OS thread
looping over pixels.
"""
import ctypes as C

import numpy as np

from . import abi
from . import lib as _lib
from .scene import generate_tiles, tile_array


class Context:
    """rmd_context: one per GPU."""

    def __init__(self, device=0, stream=None):
        self.L = _lib.load()
        self.handle = C.c_void_p()
        if stream is None:
            _lib.check(self.L.rmd_context_create(device, C.byref(self.handle)))
        else:
            _lib.check(self.L.rmd_context_create_on_stream(device, C.c_void_p(stream), C.byref(self.handle)))
        self.device = device

    def close(self):
        if self.handle:
            self.L.rmd_context_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def check(self, status):
        _lib.check(status, self.handle)

    def set_tunable(self, key, value):
        """rmd_context_set_tunable: scheduling knobs (abi.RMD_TUNE_*); no setting changes a result.  0 = the library's choice."""
        self.check(self.L.rmd_context_set_tunable(self.handle, key, int(value)))

    def get_tunable(self, key):
        v = C.c_int64()
        self.check(self.L.rmd_context_get_tunable(self.handle, key, C.byref(v)))
        return v.value

    def memory_info(self):
        """(free, total) bytes of the device's memory."""
        free, total = C.c_uint64(), C.c_uint64()
        self.check(self.L.rmd_context_memory_info(self.handle, C.byref(free), C.byref(total)))
        return free.value, total.value

    def synchronize(self):
        self.check(self.L.rmd_context_synchronize(self.handle))

    def last_launch_info(self):
        """rmd_last_launch_info: how the most recent render was launched (passes, split_k, persistent, end_black_paths, has_grid)."""
        info = abi.LaunchInfo()
        self.check(self.L.rmd_last_launch_info(self.handle, C.byref(info)))
        return info

    def last_kernel_ms(self):
        ms = C.c_float()
        self.check(self.L.rmd_last_kernel_ms(self.handle, C.byref(ms)))
        return ms.value


class DeviceScene:
    """rmd_scene: the Scene resident in one GPU's HBM."""

    def __init__(self, ctx, scene):
        self.ctx = ctx
        objs, n, descs, ng, keep = scene.flatten()
        self.handle = C.c_void_p()
        ctx.check(ctx.L.rmd_scene_create(ctx.handle, objs, n, descs, ng, C.byref(self.handle)))

    def close(self):
        if self.handle:
            self.ctx.L.rmd_scene_destroy(self.handle)
            self.handle = C.c_void_p()


class Framebuffer:
    """W*H*3 f64 accumulation buffer in HBM (library-allocated, or wrapping a caller's device pointer)."""

    def __init__(self, ctx, width, height, device_ptr=None):
        self.ctx, self.width, self.height = ctx, width, height
        self.n = width * height * 3
        self.owned = device_ptr is None
        if self.owned:
            p = C.c_void_p()
            ctx.check(ctx.L.rmd_framebuffer_alloc(ctx.handle, width, height, C.byref(p)))
            self.ptr = p
        else:
            self.ptr = C.c_void_p(device_ptr)

    def zero(self):
        self.ctx.check(self.ctx.L.rmd_framebuffer_zero(self.ctx.handle, self.ptr, self.n))

    def download(self):
        out = np.empty((self.height, self.width, 3), dtype=np.float64)
        self.ctx.check(self.ctx.L.rmd_framebuffer_download(self.ctx.handle, self.ptr, out.ctypes.data_as(C.c_void_p), self.n))
        return out

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        assert arr.size == self.n
        self.ctx.check(self.ctx.L.rmd_framebuffer_upload(self.ctx.handle, arr.ctypes.data_as(C.c_void_p), self.ptr, self.n))

    def download_tiles(self, tiles):
        """rmd_framebuffer_download_tiles: the pixels of `tiles` (left, top, width, height) as ONE packed array, tile after tile, each
        row-major (height, width, 3) — core::tile::Tile.data's layout; returns the list of per-tile views."""
        arr = tile_array(tiles)
        n = sum(w * h for (_, _, w, h) in tiles)
        out = np.empty(n * 3, dtype=np.float64)
        self.ctx.check(self.ctx.L.rmd_framebuffer_download_tiles(self.ctx.handle, self.ptr, self.width, self.height, arr, len(tiles), out.ctypes.data_as(C.c_void_p)))
        views, at = [], 0
        for (_, _, w, h) in tiles:
            views.append(out[at : at + w * h * 3].reshape(h, w, 3))
            at += w * h * 3
        return views

    def upload_tiles(self, tiles, datas):
        """rmd_framebuffer_upload_tiles: the inverse (datas: one (height, width, 3) array per tile)."""
        packed = np.ascontiguousarray(np.concatenate([np.asarray(d, dtype=np.float64).reshape(-1) for d in datas]))
        self.ctx.check(self.ctx.L.rmd_framebuffer_upload_tiles(self.ctx.handle, packed.ctypes.data_as(C.c_void_p), self.ptr, self.width, self.height, tile_array(tiles), len(tiles)))

    def close(self):
        if self.owned and self.ptr:
            self.ctx.L.rmd_framebuffer_free(self.ctx.handle, self.ptr)
            self.ptr = C.c_void_p()


class FeatureBuffer(Framebuffer):
    """W*H*7 f64 first-hit feature sums in HBM (rmd_feature_buffer_alloc): per pixel normal xyz, albedo rgb, depth."""

    def __init__(self, ctx, width, height):
        self.ctx, self.width, self.height = ctx, width, height
        self.n = width * height * abi.RMD_FEATURE_CHANNELS
        self.owned = True
        p = C.c_void_p()
        ctx.check(ctx.L.rmd_feature_buffer_alloc(ctx.handle, width, height, C.byref(p)))
        self.ptr = p

    def download(self):
        out = np.empty((self.height, self.width, abi.RMD_FEATURE_CHANNELS), dtype=np.float64)
        self.ctx.check(self.ctx.L.rmd_framebuffer_download(self.ctx.handle, self.ptr, out.ctypes.data_as(C.c_void_p), self.n))
        return out

    def download_tiles(self, tiles):
        raise NotImplementedError("feature buffers have no tile-rect transfers")

    def upload_tiles(self, tiles, datas):
        raise NotImplementedError("feature buffers have no tile-rect transfers")


def render_features(ctx, dscene, camera_settings, settings, tiles, features, sample_begin=0, sample_count=None, sync=True, features_sq=None):
    """rmd_render_features[_async]: add the first-hit features (normal, albedo, depth) of `sample_count` samples per pixel of `tiles` into the
    FeatureBuffer `features`, and their squares into `features_sq` when given."""
    cam = camera_settings.pod()
    st = settings.pod(sample_begin, sample_count)
    arr = tiles if isinstance(tiles, tuple) and len(tiles) == 2 and hasattr(tiles[0], "_length_") else (tile_array(tiles), len(tiles))
    fn = ctx.L.rmd_render_features if sync else ctx.L.rmd_render_features_async
    ctx.check(fn(ctx.handle, dscene.handle, C.byref(cam), C.byref(st), arr[0], arr[1], features.ptr, None if features_sq is None else features_sq.ptr))


def render_tiles(ctx, dscene, camera_settings, settings, tiles, framebuffer, sample_begin=0, sample_count=None, sync=True, framebuffer_sq=None):
    """rmd_render_tiles[_async]: add `sample_count` samples per pixel of `tiles` into `framebuffer`.  With `framebuffer_sq`:
    rmd_render_tiles_moments[_async], which also adds every sample's square to it."""
    cam = camera_settings.pod()
    st = settings.pod(sample_begin, sample_count)
    arr = tiles if isinstance(tiles, tuple) and len(tiles) == 2 and hasattr(tiles[0], "_length_") else (tile_array(tiles), len(tiles))
    if framebuffer_sq is None:
        fn = ctx.L.rmd_render_tiles if sync else ctx.L.rmd_render_tiles_async
        ctx.check(fn(ctx.handle, dscene.handle, C.byref(cam), C.byref(st), arr[0], arr[1], framebuffer.ptr))
    else:
        fn = ctx.L.rmd_render_tiles_moments if sync else ctx.L.rmd_render_tiles_moments_async
        ctx.check(fn(ctx.handle, dscene.handle, C.byref(cam), C.byref(st), arr[0], arr[1], framebuffer.ptr, framebuffer_sq.ptr))


def tile_error(ctx, framebuffer, framebuffer_sq, sample_count, floor, tiles):
    """rmd_tile_error: per tile, the relative standard error of its worst pixel and channel after `sample_count` samples (float64 array)."""
    out = np.empty(max(1, len(tiles)), dtype=np.float64)
    ctx.check(ctx.L.rmd_tile_error(ctx.handle, framebuffer.ptr, framebuffer_sq.ptr, framebuffer.width, framebuffer.height, int(sample_count), float(floor),
                                   tile_array(tiles), len(tiles), out.ctypes.data_as(C.c_void_p)))
    return out[: len(tiles)]


def despike(ctx, framebuffer, framebuffer_sq, rects, counts, radius=2, rank=2, k=6.0, ratio=2.0, floor=0.0, out=None, want_replaced=True):
    """rmd_despike: firefly rejection from the moments.  A pixel whose luminance stands more than `k` standard errors of its DONOR — the other of its
    (2 * radius + 1)^2 window at 0-based index `rank` by luminance — above `ratio` times the donor's plus `floor` takes the donor's sums, at its own count.
    Returns (Framebuffer S', Framebuffer Q', replaced): the two new sum buffers (the caller closes them), which every call takes in place of the inputs
    with the same rects and counts, and the number of pixels replaced in each rect (uint32 array).  `out`: a (Framebuffer, Framebuffer) pair to write into
    instead of two new ones.  want_replaced=False passes NULL for the counts and returns None for them."""
    rects = list(rects)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if len(counts) != len(rects):
        raise ValueError("one sample count per rect")
    W, H = framebuffer.width, framebuffer.height
    made = []
    try:
        if out is None:
            made.append(Framebuffer(ctx, W, H))
            made.append(Framebuffer(ctx, W, H))
            out = tuple(made)
        replaced = np.zeros(max(1, len(rects)), dtype=np.uint32) if want_replaced else None
        ctx.check(ctx.L.rmd_despike(ctx.handle, framebuffer.ptr, framebuffer_sq.ptr, W, H, tile_array(rects), counts.ctypes.data_as(C.POINTER(C.c_uint32)),
                                    len(rects), int(radius), int(rank), float(k), float(ratio), float(floor), out[0].ptr, out[1].ptr,
                                    None if replaced is None else replaced.ctypes.data_as(C.POINTER(C.c_uint32))))
    except Exception:
        for b in made:
            b.close()
        raise
    return out[0], out[1], None if replaced is None else replaced[: len(rects)]


def despike_arrays(ctx, sums, sums_sq, rects, counts, **params):
    """despike() for host arrays: (H, W, 3) sums and sums of squares in; the (H, W, 3) despiked sums, sums of squares and the per-rect replaced counts out."""
    H, W = sums.shape[0], sums.shape[1]
    bufs = [Framebuffer(ctx, W, H) for _ in range(4)]
    try:
        bufs[0].upload(sums)
        bufs[1].upload(sums_sq)
        _, _, replaced = despike(ctx, bufs[0], bufs[1], rects, counts, out=(bufs[2], bufs[3]), **params)
        return bufs[2].download(), bufs[3].download(), replaced
    finally:
        for b in bufs:
            b.close()


def denoise(ctx, framebuffer, framebuffer_sq, rects, counts, out_framebuffer, radius=10, patch_radius=3, k=0.45, alpha=1.0):
    """rmd_denoise: `out_framebuffer` = the variance-guided non-local means of the frame whose sums are `framebuffer` and sums of squares
    `framebuffer_sq`; rect i of `rects` (left, top, width, height) holds counts[i] samples per pixel.  The result holds means, not sums."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if len(counts) != len(rects):
        raise ValueError("one sample count per rect")
    ctx.check(ctx.L.rmd_denoise(ctx.handle, framebuffer.ptr, framebuffer_sq.ptr, framebuffer.width, framebuffer.height, tile_array(rects),
                                counts.ctypes.data_as(C.POINTER(C.c_uint32)), len(rects), int(radius), int(patch_radius), float(k), float(alpha),
                                out_framebuffer.ptr))


def denoise_arrays(ctx, sums, sums_sq, rects, counts, **params):
    """denoise() for host arrays: (H, W, 3) sums and sums of squares in, the (H, W, 3) denoised means out."""
    H, W = sums.shape[0], sums.shape[1]
    bufs = [Framebuffer(ctx, W, H) for _ in range(3)]
    try:
        bufs[0].upload(sums)
        bufs[1].upload(sums_sq)
        denoise(ctx, bufs[0], bufs[1], rects, counts, bufs[2], **params)
        return bufs[2].download()
    finally:
        for b in bufs:
            b.close()


def denoise_guided(ctx, framebuffer, framebuffer_sq, features, features_sq, rects, counts, out_framebuffer, radius=10, patch_radius=3, k=0.45, alpha=1.0,
                   k_f=1.0, tau=1e-2, slope=None):
    """rmd_denoise_guided: denoise() with the feature weight of the FeatureBuffers `features` / `features_sq` (both None: exactly denoise()).
    `slope` (a number; None: the call above): rmd_denoise_guided_slope, the same with the feature-slope term at that many pixels (0: the same bytes);
    without features it is passed and not read, as the header states."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if len(counts) != len(rects):
        raise ValueError("one sample count per rect")
    head = (ctx.handle, framebuffer.ptr, framebuffer_sq.ptr, None if features is None else features.ptr, None if features_sq is None else features_sq.ptr,
            framebuffer.width, framebuffer.height, tile_array(rects), counts.ctypes.data_as(C.POINTER(C.c_uint32)), len(rects), int(radius), int(patch_radius),
            float(k), float(alpha), float(k_f), float(tau))
    if slope is None:
        ctx.check(ctx.L.rmd_denoise_guided(*head, out_framebuffer.ptr))
    else:
        ctx.check(ctx.L.rmd_denoise_guided_slope(*head, float(slope), out_framebuffer.ptr))


def denoise_guided_arrays(ctx, sums, sums_sq, feats, feats_sq, rects, counts, **params):
    """denoise_guided() for host arrays: (H, W, 3) sums and sums of squares and (H, W, 7) feature sums and sums of squares in (the latter two may
    both be None), the (H, W, 3) denoised means out."""
    H, W = sums.shape[0], sums.shape[1]
    bufs = [Framebuffer(ctx, W, H) for _ in range(3)]
    fbufs = [FeatureBuffer(ctx, W, H) for _ in range(2)] if feats is not None else [None, None]
    try:
        bufs[0].upload(sums)
        bufs[1].upload(sums_sq)
        if feats is not None:
            fbufs[0].upload(feats)
            fbufs[1].upload(feats_sq)
        denoise_guided(ctx, bufs[0], bufs[1], fbufs[0], fbufs[1], rects, counts, bufs[2], **params)
        return bufs[2].download()
    finally:
        for b in bufs + fbufs:
            if b is not None:
                b.close()


def denoise_atrous(ctx, framebuffer, framebuffer_sq, rects, counts, out_framebuffer, levels=5, k=3.0, alpha=1.0, features=None, features_sq=None, k_f=1.0,
                   tau=1e-2, slope=None):
    """rmd_denoise_atrous: `out_framebuffer` = the frame after `levels` levels of the edge-avoiding a-trous filter (the fast filter for previews), with
    the feature weight of the FeatureBuffers `features` / `features_sq` when they are given.  The result holds means, not sums.
    `slope` (a number; None: the call above): rmd_denoise_atrous_slope, the same with the feature-slope term at that many pixels (0: the same bytes)."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if len(counts) != len(rects):
        raise ValueError("one sample count per rect")
    head = (ctx.handle, framebuffer.ptr, framebuffer_sq.ptr, None if features is None else features.ptr, None if features_sq is None else features_sq.ptr,
            framebuffer.width, framebuffer.height, tile_array(rects), counts.ctypes.data_as(C.POINTER(C.c_uint32)), len(rects), int(levels), float(k),
            float(alpha), float(k_f), float(tau))
    if slope is None:
        ctx.check(ctx.L.rmd_denoise_atrous(*head, out_framebuffer.ptr))
    else:
        ctx.check(ctx.L.rmd_denoise_atrous_slope(*head, float(slope), out_framebuffer.ptr))


def denoise_atrous_arrays(ctx, sums, sums_sq, feats, feats_sq, rects, counts, **params):
    """denoise_atrous() for host arrays: (H, W, 3) sums and sums of squares and (H, W, 7) feature sums and sums of squares in (the latter two may
    both be None), the (H, W, 3) filtered means out."""
    H, W = sums.shape[0], sums.shape[1]
    bufs = [Framebuffer(ctx, W, H) for _ in range(3)]
    fbufs = [FeatureBuffer(ctx, W, H) for _ in range(2)] if feats is not None else [None, None]
    try:
        bufs[0].upload(sums)
        bufs[1].upload(sums_sq)
        if feats is not None:
            fbufs[0].upload(feats)
            fbufs[1].upload(feats_sq)
        denoise_atrous(ctx, bufs[0], bufs[1], rects, counts, bufs[2], features=fbufs[0], features_sq=fbufs[1], **params)
        return bufs[2].download()
    finally:
        for b in bufs + fbufs:
            if b is not None:
                b.close()


class ErrorImage(Framebuffer):
    """W*H f64 in HBM: rmd_denoise_dual's per-pixel error estimate (the allocation is a framebuffer's; its first W*H doubles are used)."""

    def __init__(self, ctx, width, height):
        Framebuffer.__init__(self, ctx, width, height)
        self.n = width * height

    def download(self):
        out = np.empty((self.height, self.width), dtype=np.float64)
        self.ctx.check(self.ctx.L.rmd_framebuffer_download(self.ctx.handle, self.ptr, out.ctypes.data_as(C.c_void_p), self.n))
        return out

    def download_tiles(self, tiles):
        raise NotImplementedError("error images have no tile-rect transfers")

    def upload_tiles(self, tiles, datas):
        raise NotImplementedError("error images have no tile-rect transfers")


def denoise_dual(ctx, half_a, half_b, rects, counts_a, counts_b, out_framebuffer, error_image=None, radius=10, patch_radius=3, k=0.45, alpha=1.0, region=None,
                 features=None, features_sq=None, counts_f=None, k_f=1.0, tau=1e-2, slope=None):
    """rmd_denoise_dual: `out_framebuffer` = the cross-filtered means of the two sample halves `half_a` and `half_b`, each a (sums, sums of squares)
    pair of Framebuffers; rect i holds counts_a[i] and counts_b[i] samples per pixel in them.  `error_image` (an ErrorImage, optional) receives the
    per-pixel error estimate.  `region` (a list of rects, possibly empty): rmd_denoise_dual_region — only the pixels of those rects are written, with
    the bytes the whole-frame call gives them; None is the whole-frame call.  `features` / `features_sq` (FeatureBuffers; rect i holds counts_f[i]
    feature samples per pixel): rmd_denoise_dual_guided[_region], the same with rmd_denoise_guided's feature weight; features=None makes the calls above.
    `slope` (a number; None: the calls above): rmd_denoise_dual_guided_slope[_region], the same with the feature-slope term.  Without features the slope
    is not read, as in the C calls and in denoise_guided: the unguided calls above are made."""
    counts_a = np.ascontiguousarray(counts_a, dtype=np.uint32)
    counts_b = np.ascontiguousarray(counts_b, dtype=np.uint32)
    if len(counts_a) != len(rects) or len(counts_b) != len(rects):
        raise ValueError("one sample count per rect and half")
    fb = half_a[0]
    head = (ctx.handle, half_a[0].ptr, half_a[1].ptr, half_b[0].ptr, half_b[1].ptr, fb.width, fb.height, tile_array(rects),
            counts_a.ctypes.data_as(C.POINTER(C.c_uint32)), counts_b.ctypes.data_as(C.POINTER(C.c_uint32)), len(rects))
    tail = (int(radius), int(patch_radius), float(k), float(alpha), out_framebuffer.ptr, None if error_image is None else error_image.ptr)
    if features is not None or features_sq is not None:
        counts_f = np.ascontiguousarray([] if counts_f is None else counts_f, dtype=np.uint32)
        if len(counts_f) != len(rects):
            raise ValueError("one feature sample count per rect")
        head = head[:5] + (None if features is None else features.ptr, None if features_sq is None else features_sq.ptr) + head[5:10] + (
            counts_f.ctypes.data_as(C.POINTER(C.c_uint32)), len(rects))
        tail = tail[:4] + (float(k_f), float(tau)) + (() if slope is None else (float(slope),)) + tail[4:]
        whole, regional = ((ctx.L.rmd_denoise_dual_guided, ctx.L.rmd_denoise_dual_guided_region) if slope is None else
                           (ctx.L.rmd_denoise_dual_guided_slope, ctx.L.rmd_denoise_dual_guided_slope_region))
        if region is None:
            ctx.check(whole(*head, *tail))
        else:
            region = list(region)
            ctx.check(regional(*head, tile_array(region), len(region), *tail))
    elif region is None:
        ctx.check(ctx.L.rmd_denoise_dual(*head, *tail))
    else:
        region = list(region)
        ctx.check(ctx.L.rmd_denoise_dual_region(*head, tile_array(region), len(region), *tail))


def denoise_dual_arrays(ctx, sums_a, sums_sq_a, sums_b, sums_sq_b, rects, counts_a, counts_b, region=None, out_init=None, err_init=None, features=None,
                        features_sq=None, **params):
    """denoise_dual() for host arrays: the two halves' (H, W, 3) sums and sums of squares in; the (H, W, 3) means and the (H, W) error estimate out.
    `out_init` (H, W, 3) and `err_init` (H, W): what the two outputs hold before the call — what a pixel outside `region` still holds after it.
    `features` / `features_sq`: (H, W, 7) feature sums and sums of squares for the guided forms (with counts_f, k_f, tau among the params)."""
    H, W = sums_a.shape[0], sums_a.shape[1]
    opened = []
    try:
        for arr in (sums_a, sums_sq_a, sums_b, sums_sq_b, out_init):
            opened.append(Framebuffer(ctx, W, H))
            if arr is not None:
                opened[-1].upload(arr)
        opened.append(ErrorImage(ctx, W, H))
        if err_init is not None:
            opened[-1].upload(err_init)
        fbufs = [None, None]
        if features is not None:
            for i, arr in enumerate((features, features_sq)):
                opened.append(FeatureBuffer(ctx, W, H))
                opened[-1].upload(arr)
                fbufs[i] = opened[-1]
        denoise_dual(ctx, (opened[0], opened[1]), (opened[2], opened[3]), rects, counts_a, counts_b, opened[4], opened[5], region=region, features=fbufs[0],
                     features_sq=fbufs[1], **params)
        return opened[4].download(), opened[5].download()
    finally:
        for b in opened:
            b.close()


def denoise_atrous_dual(ctx, half_a, half_b, rects, counts_a, counts_b, out_framebuffer, error_image=None, levels=5, k=3.0, alpha=1.0, features=None,
                        features_sq=None, counts_f=None, k_f=1.0, tau=1e-2, region=None, slope=None):
    """rmd_denoise_atrous_dual: `out_framebuffer` = the two sample halves `half_a` and `half_b` (as denoise_dual's) after `levels` levels of the
    edge-avoiding a-trous filter, each half under the other's weights, combined as denoise_dual combines them; `error_image` (an ErrorImage,
    optional) receives the per-pixel error estimate.  `features` / `features_sq` (FeatureBuffers; rect i holds counts_f[i] feature samples per
    pixel) add the feature weight; without them counts_f, k_f and tau are not read.  `region` (a list of rects, possibly empty):
    rmd_denoise_atrous_dual_region — only the pixels of those rects are written, with the bytes the whole-frame call gives them; None is the whole-frame
    call.  `slope` (a number; None: the calls above): rmd_denoise_atrous_dual_slope[_region], the same with the feature-slope term."""
    counts_a = np.ascontiguousarray(counts_a, dtype=np.uint32)
    counts_b = np.ascontiguousarray(counts_b, dtype=np.uint32)
    if len(counts_a) != len(rects) or len(counts_b) != len(rects):
        raise ValueError("one sample count per rect and half")
    p_f = None
    if features is not None or features_sq is not None:
        counts_f = np.ascontiguousarray([] if counts_f is None else counts_f, dtype=np.uint32)
        if len(counts_f) != len(rects):
            raise ValueError("one feature sample count per rect")
        p_f = counts_f.ctypes.data_as(C.POINTER(C.c_uint32))
    fb = half_a[0]
    head = (ctx.handle, half_a[0].ptr, half_a[1].ptr, half_b[0].ptr, half_b[1].ptr, None if features is None else features.ptr,
            None if features_sq is None else features_sq.ptr, fb.width, fb.height, tile_array(rects), counts_a.ctypes.data_as(C.POINTER(C.c_uint32)),
            counts_b.ctypes.data_as(C.POINTER(C.c_uint32)), p_f, len(rects))
    tail = ((int(levels), float(k), float(alpha), float(k_f), float(tau)) + (() if slope is None else (float(slope),)) +
            (out_framebuffer.ptr, None if error_image is None else error_image.ptr))
    whole, regional = ((ctx.L.rmd_denoise_atrous_dual, ctx.L.rmd_denoise_atrous_dual_region) if slope is None else
                       (ctx.L.rmd_denoise_atrous_dual_slope, ctx.L.rmd_denoise_atrous_dual_slope_region))
    if region is None:
        ctx.check(whole(*head, *tail))
    else:
        region = list(region)
        ctx.check(regional(*head, tile_array(region), len(region), *tail))


def denoise_atrous_dual_arrays(ctx, sums_a, sums_sq_a, sums_b, sums_sq_b, rects, counts_a, counts_b, out_init=None, err_init=None, features=None,
                               features_sq=None, want_err=True, region=None, **params):
    """denoise_atrous_dual() for host arrays: the two halves' (H, W, 3) sums and sums of squares in; the (H, W, 3) means and the (H, W) error estimate
    out (None for the latter with want_err=False: the call is then made without an error image).  `out_init` / `err_init`: what the two outputs hold
    before the call — what a pixel outside `region` still holds after it.  `features` / `features_sq`: (H, W, 7) feature sums and sums of squares (with
    counts_f, k_f, tau among the params)."""
    H, W = sums_a.shape[0], sums_a.shape[1]
    opened = []
    try:
        for arr in (sums_a, sums_sq_a, sums_b, sums_sq_b, out_init):
            opened.append(Framebuffer(ctx, W, H))
            if arr is not None:
                opened[-1].upload(arr)
        opened.append(ErrorImage(ctx, W, H))
        if err_init is not None:
            opened[-1].upload(err_init)
        fbufs = [None, None]
        if features is not None:
            for i, arr in enumerate((features, features_sq)):
                opened.append(FeatureBuffer(ctx, W, H))
                opened[-1].upload(arr)
                fbufs[i] = opened[-1]
        denoise_atrous_dual(ctx, (opened[0], opened[1]), (opened[2], opened[3]), rects, counts_a, counts_b, opened[4], opened[5] if want_err else None,
                            features=fbufs[0], features_sq=fbufs[1], region=region, **params)
        return opened[4].download(), opened[5].download() if want_err else None
    finally:
        for b in opened:
            b.close()


class WinnerImage(ErrorImage):
    """W*H uint32 in HBM: rmd_denoise_dual_select's per-pixel winners (the allocation is a framebuffer's; its first W*H words are used)."""

    def download(self):
        out = np.empty((self.n + 1) // 2, dtype=np.float64)  # (transfers count doubles)
        self.ctx.check(self.ctx.L.rmd_framebuffer_download(self.ctx.handle, self.ptr, out.ctypes.data_as(C.c_void_p), out.size))
        return out.view(np.uint32)[: self.n].reshape(self.height, self.width).copy()

    def upload(self, words):
        buf = np.zeros(2 * ((self.n + 1) // 2), dtype=np.uint32)
        buf[: self.n] = np.asarray(words, dtype=np.uint32).reshape(-1)
        arr = buf.view(np.float64)
        self.ctx.check(self.ctx.L.rmd_framebuffer_upload(self.ctx.handle, arr.ctypes.data_as(C.c_void_p), self.ptr, arr.size))


def candidate_array(candidates):
    """An abi.DenoiseCandidate array from dicts with k and, optionally, alpha (1.0), guided (False), k_f (1.0), tau (1e-2) and reserved (0)."""
    arr = (abi.DenoiseCandidate * max(1, len(candidates)))()
    for i, c in enumerate(candidates):
        arr[i] = abi.DenoiseCandidate(float(c["k"]), float(c.get("alpha", 1.0)), float(c.get("k_f", 1.0)), float(c.get("tau", 1e-2)), int(bool(c.get("guided", False))),
                                      int(c.get("reserved", 0)))
    return arr


def denoise_dual_select(ctx, half_a, half_b, rects, counts_a, counts_b, candidates, out_framebuffer, error_image=None, sure_image=None, winner_image=None,
                        radius=10, patch_radius=3, sure_window=2, select_window=2, features=None, features_sq=None, counts_f=None):
    """rmd_denoise_dual_select: per pixel, the best of `candidates` (dicts, see candidate_array: parameter sets of denoise_dual, `guided` ones with the
    feature weight) by Stein's unbiased risk estimate, blended over the winners around the pixel.  `error_image` and `sure_image` (ErrorImages) and
    `winner_image` (a WinnerImage) are optional; `features`, `features_sq` and `counts_f` are needed by a guided candidate.  A candidate with a `slope`
    key makes the call rmd_denoise_dual_select_slope, with that candidate's slope (0.0 for one without the key)."""
    counts_a = np.ascontiguousarray(counts_a, dtype=np.uint32)
    counts_b = np.ascontiguousarray(counts_b, dtype=np.uint32)
    if len(counts_a) != len(rects) or len(counts_b) != len(rects):
        raise ValueError("one sample count per rect and half")
    cf = None
    if counts_f is not None:
        counts_f = np.ascontiguousarray(counts_f, dtype=np.uint32)
        if len(counts_f) != len(rects):
            raise ValueError("one feature sample count per rect")
        cf = counts_f.ctypes.data_as(C.POINTER(C.c_uint32))
    candidates = list(candidates)
    fb = half_a[0]
    opt = lambda o: None if o is None else o.ptr  # noqa: E731
    head = (ctx.handle, half_a[0].ptr, half_a[1].ptr, half_b[0].ptr, half_b[1].ptr, opt(features), opt(features_sq), fb.width, fb.height, tile_array(rects),
            counts_a.ctypes.data_as(C.POINTER(C.c_uint32)), counts_b.ctypes.data_as(C.POINTER(C.c_uint32)), cf, len(rects), int(radius), int(patch_radius),
            candidate_array(candidates))
    tail = (len(candidates), int(sure_window), int(select_window), out_framebuffer.ptr, opt(error_image), opt(sure_image), opt(winner_image))
    if any("slope" in c for c in candidates):
        slopes = (C.c_double * len(candidates))(*[float(c.get("slope", 0.0)) for c in candidates])
        ctx.check(ctx.L.rmd_denoise_dual_select_slope(*head, slopes, *tail))
    else:
        ctx.check(ctx.L.rmd_denoise_dual_select(*head, *tail))


def denoise_dual_select_arrays(ctx, sums_a, sums_sq_a, sums_b, sums_sq_b, rects, counts_a, counts_b, candidates, features=None, features_sq=None,
                               want=("err", "sure", "win"), init=None, **params):
    """denoise_dual_select() for host arrays: the two halves' (H, W, 3) sums and sums of squares in (and (H, W, 7) `features` / `features_sq` with counts_f
    among the params for guided candidates); a dict out with "out" (H, W, 3) and those of "err" (H, W), "sure" (H, W) and "win" (H, W) uint32 named in
    `want` — one left out is passed as NULL.  `init`: a dict of what the named outputs hold before the call."""
    H, W = sums_a.shape[0], sums_a.shape[1]
    init = init or {}
    opened = []
    try:
        for arr in (sums_a, sums_sq_a, sums_b, sums_sq_b, init.get("out")):
            opened.append(Framebuffer(ctx, W, H))
            if arr is not None:
                opened[-1].upload(arr)
        imgs = {}
        for name in ("err", "sure", "win"):
            if name in want:
                imgs[name] = (WinnerImage if name == "win" else ErrorImage)(ctx, W, H)
                opened.append(imgs[name])
                if init.get(name) is not None:
                    imgs[name].upload(init[name])
        fbufs = [None, None]
        if features is not None:
            for i, arr in enumerate((features, features_sq)):
                opened.append(FeatureBuffer(ctx, W, H))
                opened[-1].upload(arr)
                fbufs[i] = opened[-1]
        denoise_dual_select(ctx, (opened[0], opened[1]), (opened[2], opened[3]), rects, counts_a, counts_b, candidates, opened[4], imgs.get("err"),
                            imgs.get("sure"), imgs.get("win"), features=fbufs[0], features_sq=fbufs[1], **params)
        res = {"out": opened[4].download()}
        for name, img in imgs.items():
            res[name] = img.download()
        return res
    finally:
        for b in opened:
            b.close()


def tile_error_dual(ctx, error_image, tiles):
    """rmd_tile_error_dual: per tile, the root mean square of `error_image` (rmd_denoise_dual's estimate) over its pixels; +inf for a tile with a
    pixel that is not dual-valid (float64 array)."""
    out = np.empty(max(1, len(tiles)), dtype=np.float64)
    ctx.check(ctx.L.rmd_tile_error_dual(ctx.handle, error_image.ptr, error_image.width, error_image.height, tile_array(tiles), len(tiles),
                                        out.ctypes.data_as(C.c_void_p)))
    return out[: len(tiles)]


def resolve_tonemap(ctx, framebuffer, sample_count, exposure=1.0, gamma=2.2):
    """TaskHandle::await's divide + cli_old's tone-map/gamma/u8 cast (cli_old/src/main.rs:161-181) -> (H, W, 3) uint8."""
    out = np.empty((framebuffer.height, framebuffer.width, 3), dtype=np.uint8)
    ctx.check(
        ctx.L.rmd_resolve_tonemap(ctx.handle, framebuffer.ptr, framebuffer.width, framebuffer.height, sample_count, exposure, gamma,
                                  out.ctypes.data_as(C.c_void_p))
    )
    return out


def resolve_tonemap_tiles(ctx, framebuffer, rects, counts, exposure=1.0, gamma=2.2, second=None):
    """rmd_resolve_tonemap_tiles: resolve_tonemap over the tile rects (left, top, width, height), rect i at counts[i] samples per pixel -> one
    (h, w, 3) uint8 array per rect (views of one packed block, in download_tiles's order).  `second` (a Framebuffer): a dual-buffer render's other
    half, whose sums are added to `framebuffer`'s before the division; counts then hold both halves' samples."""
    rects = list(rects)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if len(counts) != len(rects):
        raise ValueError("one sample count per rect")
    n = sum(w * h for (_, _, w, h) in rects)
    out = np.empty(n * 3, dtype=np.uint8)
    ctx.check(ctx.L.rmd_resolve_tonemap_tiles(ctx.handle, framebuffer.ptr, None if second is None else second.ptr, framebuffer.width, framebuffer.height,
                                              tile_array(rects), counts.ctypes.data_as(C.POINTER(C.c_uint32)), len(rects), float(exposure), float(gamma),
                                              out.ctypes.data_as(C.c_void_p)))
    views, at = [], 0
    for (_, _, w, h) in rects:
        views.append(out[at : at + w * h * 3].reshape(h, w, 3))
        at += w * h * 3
    return views


def scatter_tiles(rects, tiles, width=None, height=None, out=None):
    """The per-rect arrays `tiles` ((h, w, c) each, as resolve_tonemap_tiles or download_tiles return them) written into a (height, width, c) frame at
    their rects: `out` when given, else a new zeroed frame of the tiles' dtype.  Later rects overwrite earlier ones where they overlap."""
    rects = list(rects)
    if len(rects) != len(tiles):
        raise ValueError("one array per rect")
    if out is None:
        if width is None or height is None:
            raise ValueError("scatter_tiles needs a frame: out, or width and height")
        first = np.asarray(tiles[0]) if len(tiles) else np.empty((0, 0, 3), dtype=np.uint8)
        out = np.zeros((height, width, first.shape[2] if first.ndim == 3 else 3), dtype=first.dtype)
    H, W = out.shape[0], out.shape[1]
    for (l, t, w, h), data in zip(rects, tiles):
        if l < 0 or t < 0 or w < 0 or h < 0 or l + w > W or t + h > H:
            raise ValueError("rect (%d, %d, %d, %d) outside the %d x %d frame" % (l, t, w, h, W, H))
        if w and h:
            out[t : t + h, l : l + w] = np.asarray(data).reshape(h, w, -1)
    return out


class LumaHistogram:
    """rmd_luma_histogram as numpy counters: `bins` (256 uint64: bin i holds the luminances in [2^e (1 + m / 4), 2^e (1 + (m + 1) / 4)), e = i // 4 - 32,
    m = i % 4) and the integers `below`, `above`, `zero`, `negative`, `not_finite`, `pixels`."""

    SIDE = ("below", "above", "zero", "negative", "not_finite", "pixels")

    def __init__(self, bins=None, below=0, above=0, zero=0, negative=0, not_finite=0, pixels=0):
        self.bins = np.zeros(abi.RMD_LUMA_BINS, dtype=np.uint64) if bins is None else np.array(bins, dtype=np.uint64)
        if self.bins.shape != (abi.RMD_LUMA_BINS,):
            raise ValueError("a luminance histogram has %d bins" % abi.RMD_LUMA_BINS)
        self.below, self.above, self.zero, self.negative, self.not_finite, self.pixels = (int(v) for v in (below, above, zero, negative, not_finite, pixels))

    @staticmethod
    def from_struct(s):
        return LumaHistogram(np.ctypeslib.as_array(s.bins).copy(), s.below, s.above, s.zero, s.negative, s.not_finite, s.pixels)

    def to_struct(self):
        s = abi.LumaHistogram()
        s.bins[:] = [int(v) for v in self.bins]
        s.below, s.above, s.zero, s.negative, s.not_finite, s.pixels = self.below, self.above, self.zero, self.negative, self.not_finite, self.pixels
        return s

    def counters(self):
        """All 262 integers in the struct's order, as one uint64 array."""
        return np.concatenate([self.bins, np.array([getattr(self, n) for n in self.SIDE], dtype=np.uint64)])

    def __eq__(self, other):
        return isinstance(other, LumaHistogram) and np.array_equal(self.counters(), other.counters())

    def __repr__(self):
        nz = np.flatnonzero(self.bins)
        return "LumaHistogram(%s, bins %s)" % (", ".join("%s=%d" % (n, getattr(self, n)) for n in self.SIDE), {int(i): int(self.bins[i]) for i in nz})


def luminance_histogram(ctx, framebuffer, rects, counts, second=None):
    """rmd_luminance_histogram_tiles: the luminance histogram of the pixels resolve_tonemap_tiles would resolve with the same arguments -> LumaHistogram."""
    rects = list(rects)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if len(counts) != len(rects):
        raise ValueError("one sample count per rect")
    out = abi.LumaHistogram()
    ctx.check(ctx.L.rmd_luminance_histogram_tiles(ctx.handle, framebuffer.ptr, None if second is None else second.ptr, framebuffer.width, framebuffer.height,
                                                  tile_array(rects), counts.ctypes.data_as(C.POINTER(C.c_uint32)), len(rects), C.byref(out)))
    return LumaHistogram.from_struct(out)


def add_histograms(a, b):
    """The histogram of two rect lists together from the histograms of each (several devices, each over its own tiles): every counter added — integers,
    so exact in any order."""
    return LumaHistogram(a.bins + b.bins, *(getattr(a, n) + getattr(b, n) for n in LumaHistogram.SIDE))


def exposure_from_histogram(hist, percentile=0.99, target=0.8):
    """rmd_exposure_from_histogram: the exposure that puts the histogram's `percentile` of luminance at `target` before gamma (a host function)."""
    out = C.c_double()
    _lib.check(_lib.load().rmd_exposure_from_histogram(C.byref(hist.to_struct()), float(percentile), float(target), C.byref(out)))
    return out.value


# ---------------------------------------------------------------- the reference-shaped API
class Tile:  # core/src/tile.rs:7-14
    def __init__(self, left, top, width, height, sample_count, data, error=None, data_sq=None):
        self.left, self.top, self.width, self.height = left, top, width, height
        self.sample_count = sample_count
        self.data = data  # (height, width, 3) running sums, like Tile.data
        self.error = error  # adaptive renders (an extension): the tile's rmd_tile_error at sample_count when it was checked, else None
        self.data_sq = data_sq  # denoised renders (an extension): the finished tile's running sums of squares, like data; else None
        # dual-buffer renders (an extension): the finished tile's two sample halves — sums, sums of squares (like data) and samples per pixel —;
        # data and data_sq are then the halves' sums added, sample_count = count_a + count_b.  Else None
        self.data_a = self.data_sq_a = self.count_a = self.data_b = self.data_sq_b = self.count_b = None


class Message:  # src/trace.rs:62-66
    def __init__(self, kind, tile):
        self.kind, self.tile = kind, tile

    @staticmethod
    def TileFinished(tile):
        return Message("TileFinished", tile)

    @staticmethod
    def TileProgressed(tile):
        return Message("TileProgressed", tile)

    @staticmethod
    def FramePreview(frame, pass_index, sample_count, exposure=None):
        """An extension (settings.preview_every): `frame` — the whole (H, W, 3) uint8 frame after pass `pass_index` (counted from 1), every tile
        tone-mapped at its own sample count; `sample_count`: the samples per pixel of a tile that is still live.  `tile` is None.  `exposure`: with
        settings.preview_auto_exposure the exposure this frame's histogram asked for and was tone-mapped with; None when the setting is off."""
        m = Message("FramePreview", None)
        m.frame, m.pass_index, m.sample_count, m.exposure = frame, pass_index, sample_count, exposure
        return m


class TaskHandle:  # src/trace.rs:70-135
    def __init__(self, settings, messages, device=0, scene=None):
        self.settings = settings
        self.scene = scene  # settings.denoise_features / denoise_dual_features: await_() uploads it to `device` for the feature pass
        self._messages = list(messages)
        self.callback = None
        self.preview_callback = None
        self.device = device  # settings.denoise: the GPU await_() denoises on (render_tiled's first)

    def set_callback(self, callback):
        self.callback = callback

    def poll(self):
        return self._messages.pop(0) if self._messages else None

    def set_preview_callback(self, callback):
        """`callback(message)` for every Message.FramePreview that async_await meets."""
        self.preview_callback = callback

    def async_await(self):
        while self._messages and self._messages[0].kind in ("TileProgressed", "FramePreview"):
            m = self._messages.pop(0)
            if m.kind == "FramePreview":
                if self.preview_callback:
                    self.preview_callback(m)
            elif self.callback:
                self.callback(m.tile)

    def await_(self):
        """`await`: W*H radiance values, row-major, each the tile sum divided by its sample count (:93-99).

        With settings.denoise (an extension): the finished tiles' sums, sums of squares and sample counts are assembled and the frame comes
        back through rmd_denoise on `device` — means as well; a pixel that no finished tile covers has n = 0 and comes back as 0 / 0.  With
        settings.denoise_features as well: the scene is uploaded to `device`, the finished tiles' first-hit features are rendered there
        (finished_tile_features) and the filter is rmd_denoise_guided.  With settings.denoise_atrous the filter is rmd_denoise_atrous instead, at
        denoise_atrous_levels and denoise_atrous_k, guided by the same features when denoise_features is on.
        With settings.despike: the assembled sums and sums of squares first go through rmd_despike on `device`, and the plain divide or whichever filter
        is on takes its outputs in their place."""
        cam = self.settings.camera_settings
        shape = (cam.backbuffer_height, cam.backbuffer_width, 3)
        out = np.zeros(shape, dtype=np.float64)
        if self.settings.denoise and self.settings.denoise_dual:
            return self._await_dual()
        denoised = self.settings.denoise
        if denoised and self.settings.denoise_atrous:
            self.settings.check_denoise()
        if denoised and self.settings.denoise_features:
            self.settings.check_denoise()
            if self.scene is None:
                raise ValueError("settings.denoise_features: this TaskHandle was made without the scene whose features await_() has to render")
        despiked = self.settings.despike
        if despiked:
            self.settings.check_despike()
        if denoised or despiked:
            sums, sums_sq, rects, counts = np.zeros(shape), np.zeros(shape), [], []
        while self._messages:
            m = self._messages.pop(0)
            if m.kind != "TileFinished":
                break  # the reference stops collecting at the first non-TileFinished message (:101-103)
            t = m.tile
            if denoised or despiked:
                sums[t.top : t.top + t.height, t.left : t.left + t.width] = t.data
                sums_sq[t.top : t.top + t.height, t.left : t.left + t.width] = t.data_sq
                rects.append((t.left, t.top, t.width, t.height))
                counts.append(t.sample_count)
            else:
                out[t.top : t.top + t.height, t.left : t.left + t.width] = t.data / float(t.sample_count)
        if despiked and not denoised:  # the plain divide, of the despiked sums
            with Context(self.device) as ctx:
                sums, _, _ = despike_arrays(ctx, sums, sums_sq, rects, counts, want_replaced=False, **self.settings.despike_keywords())
            for (l, t, w, h), n in zip(rects, counts):
                out[t : t + h, l : l + w] = sums[t : t + h, l : l + w] / float(n)
        if denoised:
            st = self.settings
            with Context(self.device) as ctx:
                if despiked:  # before anything else: every filter below takes the despiked sums in place of the raw ones
                    sums, sums_sq, _ = despike_arrays(ctx, sums, sums_sq, rects, counts, want_replaced=False, **st.despike_keywords())
                params = dict(radius=st.denoise_radius, patch_radius=st.denoise_patch, k=st.denoise_k, alpha=st.denoise_alpha)
                if st.denoise_atrous:
                    feats, feats_sq = finished_tile_features(ctx, self.scene, st, rects, counts) if st.denoise_features else (None, None)
                    out = denoise_atrous_arrays(ctx, sums, sums_sq, feats, feats_sq, rects, counts, levels=st.denoise_atrous_levels, k=st.denoise_atrous_k,
                                                alpha=st.denoise_alpha, k_f=st.denoise_feature_k, tau=st.denoise_feature_tau, **st.atrous_slope_keyword())
                elif st.denoise_features:
                    feats, feats_sq = finished_tile_features(ctx, self.scene, st, rects, counts)
                    out = denoise_guided_arrays(ctx, sums, sums_sq, feats, feats_sq, rects, counts, k_f=st.denoise_feature_k, tau=st.denoise_feature_tau,
                                                **st.slope_keyword(), **params)
                else:
                    out = denoise_arrays(ctx, sums, sums_sq, rects, counts, **params)
        return out


    def _await_dual(self):
        """await_() with settings.denoise_dual: the finished tiles' two halves through rmd_denoise_dual on `device`.  With settings.denoise_dual_features:
        the finished tiles' first-hit features are rendered there at count_a + count_b samples per tile (finished_tile_features) and the filter is
        rmd_denoise_dual_guided.  With settings.denoise_dual_select: the features are rendered the same way and the frame is
        rmd_denoise_dual_select's at settings.select_candidates(), both windows 2.  With settings.denoise_dual_atrous the frame is
        rmd_denoise_atrous_dual's at denoise_atrous_levels and denoise_atrous_k, guided by the same features when denoise_dual_features is on."""
        st = self.settings
        st.check_denoise()
        if (st.denoise_dual_features or st.denoise_dual_select) and self.scene is None:
            raise ValueError("settings.denoise_dual_features / denoise_dual_select: this TaskHandle was made without the scene whose features await_() has to render")
        cam = st.camera_settings
        shape = (cam.backbuffer_height, cam.backbuffer_width, 3)
        halves = [np.zeros(shape) for _ in range(4)]
        rects, counts_a, counts_b = [], [], []
        while self._messages:
            m = self._messages.pop(0)
            if m.kind != "TileFinished":
                break
            t = m.tile
            for dst, src in zip(halves, (t.data_a, t.data_sq_a, t.data_b, t.data_sq_b)):
                dst[t.top : t.top + t.height, t.left : t.left + t.width] = src
            rects.append((t.left, t.top, t.width, t.height))
            counts_a.append(t.count_a)
            counts_b.append(t.count_b)
        with Context(self.device) as ctx:
            params = dict(radius=st.denoise_radius, patch_radius=st.denoise_patch, k=st.denoise_k, alpha=st.denoise_alpha)
            if st.denoise_dual_atrous:
                guide = {}
                if st.denoise_dual_features:
                    counts_f = [a + b for a, b in zip(counts_a, counts_b)]
                    feats, feats_sq = finished_tile_features(ctx, self.scene, st, rects, counts_f)
                    guide = dict(features=feats, features_sq=feats_sq, counts_f=counts_f, k_f=st.denoise_feature_k, tau=st.denoise_feature_tau,
                                 **st.atrous_slope_keyword())
                out, _ = denoise_atrous_dual_arrays(ctx, *halves, rects, counts_a, counts_b, levels=st.denoise_atrous_levels, k=st.denoise_atrous_k,
                                                    alpha=st.denoise_alpha, **guide)
            elif st.denoise_dual_select:
                counts_f = [a + b for a, b in zip(counts_a, counts_b)]
                feats, feats_sq = finished_tile_features(ctx, self.scene, st, rects, counts_f)
                out = denoise_dual_select_arrays(ctx, *halves, rects, counts_a, counts_b, st.select_candidates(), features=feats, features_sq=feats_sq,
                                                 counts_f=counts_f, want=(), radius=st.denoise_radius, patch_radius=st.denoise_patch, sure_window=2,
                                                 select_window=2)["out"]
            elif st.denoise_dual_features:
                counts_f = [a + b for a, b in zip(counts_a, counts_b)]
                feats, feats_sq = finished_tile_features(ctx, self.scene, st, rects, counts_f)
                out, _ = denoise_dual_arrays(ctx, *halves, rects, counts_a, counts_b, features=feats, features_sq=feats_sq, counts_f=counts_f,
                                             k_f=st.denoise_feature_k, tau=st.denoise_feature_tau, **st.slope_keyword(), **params)
            else:
                out, _ = denoise_dual_arrays(ctx, *halves, rects, counts_a, counts_b, **params)
        return out


def finished_tile_features(ctx, scene, settings, rects, counts):
    """The (H, W, 7) first-hit feature sums and sums of squares of a frame whose rect i holds counts[i] samples: one rmd_render_features call per
    distinct sample count, each tile at its own count, with the settings' seed and DOF flag.  Pixels no rect covers stay zero."""
    cam = settings.camera_settings
    W, H = cam.backbuffer_width, cam.backbuffer_height
    opened = []  # closed in reverse order whichever way the body leaves, each on its own
    try:
        ds = DeviceScene(ctx, scene)
        opened.append(ds)
        fb = FeatureBuffer(ctx, W, H)
        opened.append(fb)
        fb_sq = FeatureBuffer(ctx, W, H)
        opened.append(fb_sq)
        for n in sorted(set(int(c) for c in counts)):
            share = [r for r, c in zip(rects, counts) if int(c) == n]
            if n > 0:
                render_features(ctx, ds, cam, settings, share, fb, 0, n, sync=False, features_sq=fb_sq)
        ctx.synchronize()
        return fb.download(), fb_sq.download()
    finally:
        for o in reversed(opened):
            try:
                o.close()
            except Exception:  # noqa: BLE001 (a failing close must not keep the others open, nor hide the body's own error)
                pass


def render_tiled(scene, settings, devices=(0,)):
    """render_tiled (src/trace.rs:137): tiles -> workers -> TaskHandle.  Workers are GPU contexts.

    Adaptive (settings.adaptive_threshold > 0, an extension): every pass renders the tiles that are still live with their second moments, and
    after each pass that leaves them below sample_count a tile whose rmd_tile_error is at most the threshold is sent as TileFinished at its
    current sample count and takes no further passes; the others are sent as TileProgressed and go on.

    Denoised (settings.denoise, an extension): the passes render with second moments, every TileFinished tile carries them as `data_sq`, and
    TaskHandle.await_() denoises the assembled frame on the first of `devices`.

    Previews (settings.preview_every > 0, an extension): after every preview_every-th pass that leaves live tiles below sample_count, one
    Message.FramePreview follows that pass's TileProgressed messages — each device resolves and tone-maps the tiles of its share with
    rmd_resolve_tonemap_tiles, live ones at the current count and those that finished early at theirs, and the packed tiles are scattered into one
    (H, W, 3) uint8 frame here.  With settings.preview_denoise the frame is rmd_denoise_atrous's (one device; the passes then render with second
    moments).  With settings.progress_tiles = False no TileProgressed message is made and only converged tiles' pixels are downloaded.  With
    settings.preview_auto_exposure every device first histograms the buffers, rects and counts its resolve call is about to use
    (rmd_luminance_histogram_tiles), the devices' histograms are added and the exposure of the sum (rmd_exposure_from_histogram at
    auto_exposure_percentile and auto_exposure_target) replaces preview_exposure in that preview, which carries it as `exposure`.

    Despiked (settings.despike, an extension): the passes render with second moments and every TileFinished tile carries them, as for denoise;
    TaskHandle.await_() despikes the assembled frame (rmd_despike) before its divide or filter.  With adaptive_threshold the check calls rmd_despike over
    all tiles — live ones at the current count, those that finished early at theirs — into two spare buffers and rmd_tile_error reads those; the buffers the
    passes add to, every message's data and the previews stay the raw sums.

    Dual-buffer (settings.denoise_dual, an extension): _render_tiled_dual."""
    settings.check_adaptive()
    settings.check_denoise()
    settings.check_preview(len(devices))
    settings.check_despike(len(devices))
    if settings.denoise_dual:
        return _render_tiled_dual(scene, settings, devices)
    adaptive = settings.adaptive_threshold > 0.0
    preview_filtered = settings.preview_every > 0 and settings.preview_denoise
    moments = adaptive or settings.denoise or preview_filtered or settings.despike
    with_sq = settings.denoise or settings.despike  # the finished tiles carry their sums of squares: await_() reads them
    cam = settings.camera_settings
    W, H = cam.backbuffer_width, cam.backbuffer_height
    tiles = generate_tiles(W, H, settings.tile_size)
    workers = []
    for d in devices:
        ctx = Context(d)
        workers.append((ctx, DeviceScene(ctx, scene), Framebuffer(ctx, W, H), Framebuffer(ctx, W, H) if moments else None))
    filtered_fb = Framebuffer(workers[0][0], W, H) if preview_filtered else None  # (one device: check_preview)
    # despike with the adaptive check: two spare buffers for the despiked sums the check reads (one device: check_despike); the passes' own stay raw
    spare = (Framebuffer(workers[0][0], W, H), Framebuffer(workers[0][0], W, H)) if settings.despike and adaptive else None
    shares = [tiles[i :: len(workers)] for i in range(len(workers))]  # adaptive: the tiles of a share that are still live
    early = [[] for _ in workers]  # previews: per worker, the (rect, sample count) of the tiles that finished early
    step = settings.samples_per_iteration if settings.samples_per_iteration else settings.sample_count
    messages = []
    finished = []
    done = passes = 0
    try:
        while done < settings.sample_count:
            n = min(step, settings.sample_count - done)
            for (ctx, ds, fb, fb_sq), share in zip(workers, shares):
                if share:
                    render_tiles(ctx, ds, cam, settings, share, fb, done, n, sync=False, framebuffer_sq=fb_sq)
            for ctx, _, _, _ in workers:
                ctx.synchronize()
            done += n
            passes += 1
            if done < settings.sample_count and settings.samples_per_iteration:
                for i, (ctx, ds, fb, fb_sq) in enumerate(workers):
                    share = shares[i]
                    if adaptive and share and spare is not None:  # all tiles at their current counts; the error of the live ones on the despiked sums
                        despike(ctx, fb, fb_sq, [r for r, _ in early[i]] + share, [c for _, c in early[i]] + [done] * len(share), out=spare,
                                want_replaced=False, **settings.despike_keywords())
                        errors = tile_error(ctx, spare[0], spare[1], done, settings.adaptive_floor, share)
                    else:
                        errors = tile_error(ctx, fb, fb_sq, done, settings.adaptive_floor, share) if adaptive and share else [None] * len(share)
                    if not settings.progress_tiles:  # no snapshots: only the converged tiles' pixels come to the host
                        is_conv = [adaptive and e <= settings.adaptive_threshold for e in errors]
                        conv = [r for r, c in zip(share, is_conv) if c]
                        data = fb.download_tiles(conv) if conv else []
                        data_sq = fb_sq.download_tiles(conv) if conv and with_sq else [None] * len(conv)
                        for (l, t, w, h), e, d, d_sq in zip(conv, [e for e, c in zip(errors, is_conv) if c], data, data_sq):
                            finished.append(Message.TileFinished(Tile(l, t, w, h, done, d.copy(), float(e), None if d_sq is None else d_sq.copy())))
                            early[i].append(((l, t, w, h), done))
                        shares[i] = [r for r, c in zip(share, is_conv) if not c]
                        continue
                    img = fb.download()
                    img_sq = fb_sq.download() if with_sq else None
                    live = []
                    for (l, t, w, h), e in zip(share, errors):
                        tile = Tile(l, t, w, h, done, img[t : t + h, l : l + w].copy(), None if e is None else float(e))
                        if adaptive and e <= settings.adaptive_threshold:
                            if img_sq is not None:
                                tile.data_sq = img_sq[t : t + h, l : l + w].copy()
                            finished.append(Message.TileFinished(tile))  # converged: finished at the samples it has
                            early[i].append(((l, t, w, h), done))
                        else:
                            messages.append(Message.TileProgressed(tile))
                            live.append((l, t, w, h))
                    shares[i] = live
                if settings.preview_every and passes % settings.preview_every == 0 and any(shares):  # (no live tile: the render is finished)
                    # every device resolves the tiles of its share — live ones at `done`, those that finished early at their own counts — and the
                    # packed 8-bit tiles are scattered into one frame here
                    frame = np.zeros((H, W, 3), dtype=np.uint8)
                    calls = []  # per device with tiles: what its resolve call takes
                    for i, (ctx, ds, fb, fb_sq) in enumerate(workers):
                        rects = [r for r, _ in early[i]] + shares[i]
                        counts = [c for _, c in early[i]] + [done] * len(shares[i])
                        if not rects:
                            continue
                        if preview_filtered:
                            denoise_atrous(ctx, fb, fb_sq, rects, counts, filtered_fb, levels=settings.denoise_atrous_levels, k=settings.denoise_atrous_k,
                                           alpha=settings.denoise_alpha)
                            fb, counts = filtered_fb, [1] * len(rects)  # (means)
                        calls.append((ctx, fb, rects, counts))
                    exposure = None
                    if settings.preview_auto_exposure:  # one exposure for the frame: the devices' histograms added
                        hist = LumaHistogram()
                        for ctx, fb, rects, counts in calls:
                            hist = add_histograms(hist, luminance_histogram(ctx, fb, rects, counts))
                        exposure = exposure_from_histogram(hist, settings.auto_exposure_percentile, settings.auto_exposure_target)
                    for ctx, fb, rects, counts in calls:
                        scatter_tiles(rects, resolve_tonemap_tiles(ctx, fb, rects, counts, settings.preview_exposure if exposure is None else exposure,
                                                                   settings.preview_gamma), out=frame)
                    messages.append(Message.FramePreview(frame, passes, done, exposure))
        for (ctx, ds, fb, fb_sq), share in zip(workers, shares):
            img = fb.download()
            img_sq = fb_sq.download() if with_sq else None
            for (l, t, w, h) in share:
                sq = None if img_sq is None else img_sq[t : t + h, l : l + w].copy()
                finished.append(Message.TileFinished(Tile(l, t, w, h, settings.sample_count, img[t : t + h, l : l + w].copy(), data_sq=sq)))
        messages = messages + finished  # progress snapshots (and previews) first, then the finished tiles
    finally:
        if filtered_fb is not None:
            filtered_fb.close()
        for b in spare or ():
            b.close()
        for ctx, ds, fb, fb_sq in workers:
            fb.close()
            if fb_sq is not None:
                fb_sq.close()
            ds.close()
            ctx.close()
    handle = TaskHandle(settings, messages, devices[0], scene if settings.denoise_features else None)
    return handle


def _render_tiled_dual(scene, settings, devices):
    """render_tiled with settings.denoise_dual: one device, four framebuffers.  Pass j (counted from 0; every live tile takes every pass) adds its
    samples to half A when j is even and to half B when j is odd, so after an even NUMBER of full passes both halves hold the same count.  Every
    TileFinished tile carries both halves; await_() returns rmd_denoise_dual's frame.

    With settings.adaptive_denoised_threshold > 0: after every even number of passes that leaves live tiles below sample_count with at least
    adaptive_min_samples samples, rmd_denoise_dual_region filters the live tiles' pixels of the whole frame (finished tiles at the counts they
    finished with: the bytes rmd_denoise_dual would give those pixels), rmd_tile_error_dual runs over the live tiles, and a live tile at or below the threshold is sent as TileFinished, with that error, and takes no further passes.

    With settings.denoise_dual_features the adaptive check needs the features: two feature buffers beside the four, into which rmd_render_features
    adds, after each pass, the live tiles' first-hit features of the same samples [done, done + n), so a tile's features hold count_a + count_b
    samples; the check is rmd_denoise_dual_guided_region with those counts.  (Without an adaptive threshold nothing in this loop would read them and
    none are rendered.)  await_() renders the finished tiles' features itself (finished_tile_features) and returns rmd_denoise_dual_guided's frame.

    With settings.denoise_dual_atrous the check is rmd_denoise_atrous_dual on the WHOLE frame instead, at the same rects and counts, guided by the same
    feature buffers; rmd_tile_error_dual then runs over the live tiles as before.  With settings.denoise_dual_atrous_region the check passes
    region=live — rmd_denoise_atrous_dual_region, the same bytes at the live tiles' pixels —; nothing else changes.

    With settings.preview_every > 0 a Message.FramePreview follows the snapshots of every preview_every-th pass that leaves live tiles: the two halves'
    sums added on the device (rmd_resolve_tonemap_tiles with the other half as its second buffer) at n_A + n_B, finished tiles at the counts they
    finished with; with settings.preview_denoise, rmd_denoise_atrous_dual's frame at those counts, guided when this loop keeps the feature buffers.  With
    settings.preview_auto_exposure the exposure comes from rmd_luminance_histogram_tiles on what that resolve call takes, as in render_tiled."""
    if len(devices) != 1:
        raise ValueError("denoise_dual renders on one device: the filter's window crosses the tiles that several devices would own")
    st = settings
    cam = st.camera_settings
    W, H = cam.backbuffer_width, cam.backbuffer_height
    tiles = generate_tiles(W, H, st.tile_size)
    adaptive = st.adaptive_denoised_threshold > 0.0
    params = dict(radius=st.denoise_radius, patch_radius=st.denoise_patch, k=st.denoise_k, alpha=st.denoise_alpha)
    opened = []  # closed in reverse order whichever way the body leaves
    messages, finished = [], []
    try:
        ctx = Context(devices[0])
        opened.append(ctx)
        ds = DeviceScene(ctx, scene)
        opened.append(ds)
        fbs = [Framebuffer(ctx, W, H) for _ in range(4)]  # S_A, Q_A, S_B, Q_B
        opened.extend(fbs)
        if adaptive:
            out_fb, err_img = Framebuffer(ctx, W, H), ErrorImage(ctx, W, H)
            opened.extend([out_fb, err_img])
        guided = adaptive and st.denoise_dual_features
        guide = {}
        if guided:
            feat_fbs = [FeatureBuffer(ctx, W, H) for _ in range(2)]
            opened.extend(feat_fbs)
        preview_fb = None
        if st.preview_every and st.preview_denoise:
            preview_fb = Framebuffer(ctx, W, H)
            opened.append(preview_fb)
        live = list(tiles)
        done_rects, done_a, done_b = [], [], []  # the finished tiles and the counts they finished with
        n_half = [0, 0]  # samples per pixel of a live tile in A and B
        done, j = 0, 0

        def finish(rects, errors=None):
            """TileFinished for `rects`: both halves' sums and sums of squares, the tiles' pixels only."""
            if not rects:
                return
            packed = [fb.download_tiles(rects) for fb in fbs]
            for i, rect in enumerate(rects):
                l, t, w, h = rect
                a, a_sq, b, b_sq = (p[i].copy() for p in packed)
                tile = Tile(l, t, w, h, n_half[0] + n_half[1], a + b, None if errors is None else errors[i], a_sq + b_sq)
                tile.data_a, tile.data_sq_a, tile.count_a, tile.data_b, tile.data_sq_b, tile.count_b = a, a_sq, n_half[0], b, b_sq, n_half[1]
                finished.append(Message.TileFinished(tile))
                done_rects.append(rect), done_a.append(n_half[0]), done_b.append(n_half[1])

        while done < st.sample_count and live:
            n = min(st.samples_per_iteration, st.sample_count - done)
            half = j & 1
            render_tiles(ctx, ds, cam, st, live, fbs[2 * half], done, n, sync=False, framebuffer_sq=fbs[2 * half + 1])
            if guided:
                render_features(ctx, ds, cam, st, live, feat_fbs[0], done, n, sync=False, features_sq=feat_fbs[1])
            ctx.synchronize()
            done, j = done + n, j + 1
            n_half[half] += n
            if done < st.sample_count:
                errors = [None] * len(live)
                if adaptive and j % 2 == 0 and done >= st.adaptive_min_samples:
                    # only the live tiles' filtered pixels are read below: the region form writes those, with the whole-frame call's bytes
                    all_a, all_b = done_a + [n_half[0]] * len(live), done_b + [n_half[1]] * len(live)
                    if guided:
                        guide = dict(features=feat_fbs[0], features_sq=feat_fbs[1], counts_f=[a + b for a, b in zip(all_a, all_b)], k_f=st.denoise_feature_k,
                                     tau=st.denoise_feature_tau)
                    if st.denoise_dual_atrous:
                        where = dict(region=live) if st.denoise_dual_atrous_region else {}  # (off: exactly the call made before the region form existed)
                        slope = st.atrous_slope_keyword() if guided else {}  # (set: the check is rmd_denoise_atrous_dual_slope[_region])
                        denoise_atrous_dual(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), done_rects + live, all_a, all_b, out_fb, err_img,
                                            levels=st.denoise_atrous_levels, k=st.denoise_atrous_k, alpha=st.denoise_alpha, **guide, **where, **slope)
                    else:
                        slope = st.slope_keyword() if guided else {}  # (set: the check is rmd_denoise_dual_guided_slope_region)
                        denoise_dual(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), done_rects + live, all_a, all_b, out_fb, err_img, region=live, **params, **guide, **slope)
                    errors = tile_error_dual(ctx, err_img, live)
                conv = [e is not None and e <= st.adaptive_denoised_threshold for e in errors]
                finish([r for r, c in zip(live, conv) if c], [float(e) for e, c in zip(errors, conv) if c])  # converged: finished at the samples they have
                still = [r for r, c in zip(live, conv) if not c]
                if still and st.progress_tiles:  # progress snapshots: the two halves' sums added
                    pa, pb = fbs[0].download_tiles(still), fbs[2].download_tiles(still)
                    for (l, t, w, h), e, a, b in zip(still, [e for e, c in zip(errors, conv) if not c], pa, pb):
                        messages.append(Message.TileProgressed(Tile(l, t, w, h, done, a + b, None if e is None else float(e))))
                if still and st.preview_every and j % st.preview_every == 0:
                    # the whole frame: finished tiles at the counts they finished with, live ones at n_A + n_B, the two halves' sums added on the device
                    rects = done_rects + still
                    all_a, all_b = done_a + [n_half[0]] * len(still), done_b + [n_half[1]] * len(still)
                    if preview_fb is None:
                        src, src_counts, second = fbs[0], [a + b for a, b in zip(all_a, all_b)], fbs[2]
                    else:
                        if guided:
                            guide = dict(features=feat_fbs[0], features_sq=feat_fbs[1], counts_f=[a + b for a, b in zip(all_a, all_b)], k_f=st.denoise_feature_k,
                                         tau=st.denoise_feature_tau)
                        slope = st.atrous_slope_keyword() if guided else {}  # (set: the preview is rmd_denoise_atrous_dual_slope's)
                        denoise_atrous_dual(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), rects, all_a, all_b, preview_fb, None, levels=st.denoise_atrous_levels,
                                            k=st.denoise_atrous_k, alpha=st.denoise_alpha, **guide, **slope)
                        src, src_counts, second = preview_fb, [1] * len(rects), None  # (means)
                    exposure = None
                    if st.preview_auto_exposure:
                        exposure = exposure_from_histogram(luminance_histogram(ctx, src, rects, src_counts, second=second), st.auto_exposure_percentile,
                                                           st.auto_exposure_target)
                    packed = resolve_tonemap_tiles(ctx, src, rects, src_counts, st.preview_exposure if exposure is None else exposure, st.preview_gamma,
                                                   second=second)
                    messages.append(Message.FramePreview(scatter_tiles(rects, packed, W, H), j, done, exposure))
                live = still
        finish(live)
        messages = messages + finished  # progress snapshots first, then the finished tiles
    finally:
        for o in reversed(opened):
            try:
                o.close()
            except Exception:  # noqa: BLE001 (a failing close must not keep the others open, nor hide the body's own error)
                pass
    return TaskHandle(settings, messages, devices[0], scene if settings.denoise_dual_features or settings.denoise_dual_select else None)
