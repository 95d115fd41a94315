"""The Python binding of the C-ABI (include/raymond_hip.h), and the reference-shaped render API on top of it.

Bottom up:
  * the device objects — Context, DeviceScene, Framebuffer and its kinds FeatureBuffer, IdBuffer, AoBuffer, ErrorImage, WinnerImage, and RayBuffer / HitBuffer —, each a context manager;
  * one thin wrapper per entry point: render_tiles, render_features, render_ids, ids_matte, render_ao, ao_resolve, intersect_rays[_dev[_async]], camera_rays, pick, tile_error[_dual], tile_luma_error, tile_weighted_error[_dual], display_weights, despike[_dual], the denoise family (every rmd_denoise* call is laid out
    by _denoise_call), resolve_tonemap[_tiles], luminance_histogram;
  * the *_arrays helpers, the same calls for host arrays (_staged puts the arrays on the device);
  * `render_tiled(scene, settings) -> TaskHandle`, which keeps the reference's shape (src/trace.rs:137-230, TaskHandle :70-135): the framebuffer is split
    into tiles in the reference's column-major order (:142-173), tiles are handed to workers, finished tiles come back as `Message.TileFinished` and
    `TaskHandle.await_()` assembles the W*H image divided by the sample count (:82-113).  The one difference is what a worker is: a GPU context that
    runs rmd_render_tiles over its share of the tiles (the per-pixel body :197-205 for ALL pixels of those tiles at once) instead of an OS thread
    looping over pixels.  The extensions — adaptive sampling, denoising, the dual-buffer loop, previews, despiking — are steps of the two loops
    (_TiledLoop, _DualLoop), named as the C++ mirror names them; which filter runs for which Settings is decided by Settings.nlm_keywords /
    atrous_keywords / guide_keywords and _guide, nowhere else.

tests/binding_trace.py pins which C call every function here makes, with which arguments in which order, against a recording stand-in for the library.
"""
import collections
import contextlib
import ctypes as C

import numpy as np

from . import abi
from . import lib as _lib
from .scene import generate_tiles, tile_array


class _Scoped:
    """`with` for the device objects: close() on the way out.  A failing close is dropped, so that inside an ExitStack it neither keeps the objects
    opened before it open nor takes the place of the body's own error."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class Context(_Scoped):
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
        """rmd_last_launch_info: how the most recent render was launched, as an abi.LaunchInfo (passes, split_k, persistent, end_black_paths, has_grid,
        waves_per_workgroup, buffered, chained, queued)."""
        info = abi.LaunchInfo()
        self.check(self.L.rmd_last_launch_info(self.handle, C.byref(info)))
        return info

    def last_kernel_ms(self):
        ms = C.c_float()
        self.check(self.L.rmd_last_kernel_ms(self.handle, C.byref(ms)))
        return ms.value


class DeviceScene(_Scoped):
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


def _ptr(buffer):
    return None if buffer is None else buffer.ptr


def _tile_views(packed, rects, channels=3):
    """One (h, w, channels) view per rect of a block that holds the rects' pixels packed, tile after tile."""
    views, at = [], 0
    for (_, _, w, h) in rects:
        views.append(packed[at : at + w * h * channels].reshape(h, w, channels))
        at += w * h * channels
    return views


def _no_tile_transfers(what):
    def refuse(self, *args):
        raise NotImplementedError("%s have no tile-rect transfers" % what)

    return refuse


class Framebuffer(_Scoped):
    """W*H*3 f64 accumulation buffer in HBM (library-allocated, or wrapping a caller's device pointer).  Its kinds below differ in `shape`, what
    download() returns, and in the call that allocates them."""

    ALLOC = "rmd_framebuffer_alloc"

    def __init__(self, ctx, width, height, device_ptr=None):
        self.ctx, self.width, self.height = ctx, width, height
        self.shape = self._shape()
        self.n = int(np.prod(self.shape))
        self.owned = device_ptr is None
        if self.owned:
            p = C.c_void_p()
            ctx.check(getattr(ctx.L, self.ALLOC)(ctx.handle, width, height, C.byref(p)))
            self.ptr = p
        else:
            self.ptr = C.c_void_p(device_ptr)

    def _shape(self):
        return (self.height, self.width, 3)

    def zero(self):
        self.ctx.check(self.ctx.L.rmd_framebuffer_zero(self.ctx.handle, self.ptr, self.n))

    def download(self):
        out = np.empty(self.shape, dtype=np.float64)
        self.ctx.check(self.ctx.L.rmd_framebuffer_download(self.ctx.handle, self.ptr, out.ctypes.data_as(C.c_void_p), out.size))
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
        return _tile_views(out, tiles)

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

    ALLOC = "rmd_feature_buffer_alloc"
    download_tiles = upload_tiles = _no_tile_transfers("feature buffers")

    def __init__(self, ctx, width, height):
        Framebuffer.__init__(self, ctx, width, height)

    def _shape(self):
        return (self.height, self.width, abi.RMD_FEATURE_CHANNELS)


class IdBuffer(Framebuffer):
    """W*H*10 uint32 first-hit object IDs with coverage in HBM (rmd_id_buffer_alloc): per pixel key_0 count_0 .. key_3 count_3 other samples.  A key is
    0 (empty), object index + 1, or abi.RMD_ID_MISS.  The framebuffer calls serve it with 5 doubles a pixel."""

    ALLOC = "rmd_id_buffer_alloc"
    download_tiles = upload_tiles = _no_tile_transfers("ID buffers")

    def __init__(self, ctx, width, height):
        Framebuffer.__init__(self, ctx, width, height)
        self.n = self.n // 2  # (in doubles: what zero() and the transfers count in)

    def _shape(self):
        return (self.height, self.width, abi.RMD_ID_WORDS)

    def download(self):
        out = np.empty(self.shape, dtype=np.uint32)
        self.ctx.check(self.ctx.L.rmd_framebuffer_download(self.ctx.handle, self.ptr, out.ctypes.data_as(C.c_void_p), self.n))
        return out

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint32)
        assert arr.size == 2 * self.n
        self.ctx.check(self.ctx.L.rmd_framebuffer_upload(self.ctx.handle, arr.ctypes.data_as(C.c_void_p), self.ptr, self.n))


class AoBuffer(IdBuffer):
    """W*H*4 uint32 ambient-occlusion counts of the first hit in HBM (rmd_ao_buffer_alloc): per pixel occluded open none samples.  The framebuffer
    calls serve it with 2 doubles a pixel."""

    ALLOC = "rmd_ao_buffer_alloc"
    download_tiles = upload_tiles = _no_tile_transfers("AO buffers")

    def _shape(self):
        return (self.height, self.width, abi.RMD_AO_WORDS)


def _render_call(ctx, stem, sync, dscene, camera_settings, settings, tiles, sample_begin, sample_count, *buffers):
    """rmd_render_*[_async]: `stem` or its _async form over `tiles` — a list of rects, or a ready (abi.TileRect array, n) pair."""
    cam = camera_settings.pod()
    st = settings.pod(sample_begin, sample_count)
    arr, n = tiles if isinstance(tiles, tuple) and len(tiles) == 2 and hasattr(tiles[0], "_length_") else (tile_array(tiles), len(tiles))
    fn = getattr(ctx.L, stem if sync else stem + "_async")
    ctx.check(fn(ctx.handle, dscene.handle, C.byref(cam), C.byref(st), arr, n, *buffers))


def render_features(ctx, dscene, camera_settings, settings, tiles, features, sample_begin=0, sample_count=None, sync=True, features_sq=None):
    """rmd_render_features[_async]: add the first-hit features (normal, albedo, depth) of `sample_count` samples per pixel of `tiles` into the
    FeatureBuffer `features`, and their squares into `features_sq` when given."""
    _render_call(ctx, "rmd_render_features", sync, dscene, camera_settings, settings, tiles, sample_begin, sample_count, features.ptr, _ptr(features_sq))


def render_ids(ctx, dscene, camera_settings, settings, tiles, ids, sample_begin=0, sample_count=None, sync=True):
    """rmd_render_ids[_async]: enter the first-hit object of `sample_count` samples per pixel of `tiles` into the IdBuffer `ids`."""
    _render_call(ctx, "rmd_render_ids", sync, dscene, camera_settings, settings, tiles, sample_begin, sample_count, ids.ptr)


def ids_matte(ctx, ids, objects):
    """rmd_ids_matte: the share of each pixel's samples whose first hit is one of `objects` — object indices, abi.RMD_ID_MISS for the background; a set,
    duplicates allowed, at most 2048 — from the IdBuffer `ids`.  Returns ((H, W) float64, other_pixels): the matte and the number of pixels whose table
    overflowed (other != 0), where the matte is a lower bound; at 0 it is exact.  Alpha is 1 - ids_matte(ctx, ids, [abi.RMD_ID_MISS])[0]."""
    objects = np.ascontiguousarray(objects, dtype=np.uint32).reshape(-1)
    W, H = ids.width, ids.height
    other = C.c_uint64()
    with ErrorImage(ctx, W, H) as matte:
        ctx.check(ctx.L.rmd_ids_matte(ctx.handle, ids.ptr, W, H, _u32(objects) if len(objects) else None, len(objects), matte.ptr, C.byref(other)))
        return matte.download(), other.value


def render_ao(ctx, dscene, camera_settings, settings, tiles, max_distance, ao, sample_begin=0, sample_count=None, sync=True):
    """rmd_render_ao[_async]: count, for `sample_count` samples per pixel of `tiles`, whether the diffuse bounce ray off the first hit meets an object
    nearer than `max_distance` (> 0; inf: any hit) into the AoBuffer `ao`."""
    _render_call(ctx, "rmd_render_ao", sync, dscene, camera_settings, settings, tiles, sample_begin, sample_count, C.c_double(max_distance), ao.ptr)


def ao_resolve(ctx, ao, empty_value=1.0):
    """rmd_ao_resolve: open / (open + occluded) per pixel of the AoBuffer `ao`, `empty_value` where no sample has a first hit.  Returns ((H, W)
    float64, empty_pixels): the openness and the number of such pixels."""
    W, H = ao.width, ao.height
    empty = C.c_uint64()
    with ErrorImage(ctx, W, H) as out:
        ctx.check(ctx.L.rmd_ao_resolve(ctx.handle, ao.ptr, W, H, C.c_double(empty_value), out.ptr, C.byref(empty)))
        return out.download(), empty.value


class RayBuffer(_Scoped):
    """n rays in HBM (rmd_ray_buffer_alloc): 6 f64 a ray, origin xyz then direction xyz.  The framebuffer calls serve it with 6 doubles a ray."""

    ALLOC, DOUBLES = "rmd_ray_buffer_alloc", abi.RMD_RAY_DOUBLES

    def __init__(self, ctx, n):
        self.ctx, self.count = ctx, int(n)
        self.n = self.count * self.DOUBLES  # (in doubles: what the transfers count in)
        self.ptr = C.c_void_p()
        ctx.check(getattr(ctx.L, self.ALLOC)(ctx.handle, self.count, C.byref(self.ptr)))

    def _host(self, arr=None):
        return np.empty((self.count, self.DOUBLES), dtype=np.float64) if arr is None else np.ascontiguousarray(arr, dtype=np.float64)

    def download(self):
        out = self._host()
        self.ctx.check(self.ctx.L.rmd_framebuffer_download(self.ctx.handle, self.ptr, out.ctypes.data_as(C.c_void_p), self.n))
        return out

    def upload(self, arr):
        arr = self._host(arr)
        assert arr.nbytes == 8 * self.n
        self.ctx.check(self.ctx.L.rmd_framebuffer_upload(self.ctx.handle, arr.ctypes.data_as(C.c_void_p), self.ptr, self.n))

    def close(self):
        if self.ptr:
            self.ctx.L.rmd_framebuffer_free(self.ctx.handle, self.ptr)
            self.ptr = C.c_void_p()


HIT_DTYPE = np.dtype([("t", "<f8"), ("normal", "<f8", (3,)), ("object", "<i4"), ("triangle", "<u4")])  # rmd_ray_hit, 40 bytes
Hits = collections.namedtuple("Hits", "object triangle t normal")


def hits_of(records):
    """The Hits views — object int32, triangle uint32, t f64, normal (n, 3) f64 — of one structured array of HIT_DTYPE records."""
    return Hits(records["object"], records["triangle"], records["t"], records["normal"])


class HitBuffer(RayBuffer):
    """n rmd_ray_hit records in HBM (rmd_hit_buffer_alloc), 40 bytes each.  The framebuffer calls serve it with 5 doubles a record; download() returns
    a structured array of HIT_DTYPE and upload() takes one."""

    ALLOC, DOUBLES = "rmd_hit_buffer_alloc", abi.RMD_HIT_DOUBLES

    def _host(self, arr=None):
        return np.empty(self.count, dtype=HIT_DTYPE) if arr is None else np.ascontiguousarray(arr, dtype=HIT_DTYPE)


def intersect_rays_dev(ctx, dscene, rays, hits, n=None, sync=True):
    """rmd_intersect_rays[_async]: the closest hit of each of the first `n` (default: all) rays of the RayBuffer `rays` into the HitBuffer `hits`."""
    n = rays.count if n is None else int(n)
    fn = ctx.L.rmd_intersect_rays if sync else ctx.L.rmd_intersect_rays_async
    ctx.check(fn(ctx.handle, dscene.handle, rays.ptr, n, hits.ptr))


def intersect_rays_dev_async(ctx, dscene, rays, hits, n=None):
    """rmd_intersect_rays_async: only enqueued on the context's stream; ctx.synchronize() ends it."""
    intersect_rays_dev(ctx, dscene, rays, hits, n, sync=False)


def intersect_rays(ctx, dscene, rays):
    """rmd_intersect_rays_host: the closest hit of each ray of the (n, 6) array `rays` (origin xyz, direction xyz; the direction is used as given).
    Returns Hits(object, triangle, t, normal), views of one structured download; a miss is object -1, t 0, a zero normal and triangle 0."""
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, abi.RMD_RAY_DOUBLES)
    out = np.empty(len(rays), dtype=HIT_DTYPE)
    if len(rays):
        ctx.check(ctx.L.rmd_intersect_rays_host(ctx.handle, dscene.handle, rays.ctypes.data_as(C.c_void_p), len(rays), out.ctypes.data_as(C.c_void_p)))
    return hits_of(out)


def camera_rays(ctx, camera, xy, uv=None, out=None):
    """rmd_camera_rays: the pinhole primary rays of the pixels `xy` ((n, 2) x, y) at the jitter uniforms `uv` ((n, 2), or None: 0.5, 0.5, the pixel
    centres) into a RayBuffer — `out`, or a new one the caller closes."""
    xy = np.ascontiguousarray(xy, dtype=np.uint32).reshape(-1, 2)
    if uv is not None:
        uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
        assert len(uv) == len(xy)
    rays = RayBuffer(ctx, len(xy)) if out is None else out
    assert rays.count >= len(xy)
    try:
        ctx.check(ctx.L.rmd_camera_rays(ctx.handle, C.byref(camera.pod()), xy.ctypes.data_as(C.c_void_p), None if uv is None else uv.ctypes.data_as(C.c_void_p),
                                        len(xy), rays.ptr))
    except Exception:
        if out is None:
            rays.close()
        raise
    return rays


def pick(ctx, dscene, camera, x, y):
    """What pixel (x, y) sees through its centre: (object, triangle, t, normal) of the closest hit, object -1 for the background.  The ray is made and
    intersected on the device (rmd_camera_rays, rmd_intersect_rays)."""
    with camera_rays(ctx, camera, [[x, y]]) as rays, HitBuffer(ctx, 1) as hits:
        intersect_rays_dev(ctx, dscene, rays, hits)
        h = hits.download()[0]
    return int(h["object"]), int(h["triangle"]), float(h["t"]), h["normal"].copy()


def _first_hit_arrays(ctx, scene, settings, rects, counts, buffer_types, render):
    """A first-hit pass over a frame whose rect i holds counts[i] samples, into zeroed buffers of `buffer_types`: one render(dscene, camera, rects, n,
    *buffers) per distinct non-zero sample count n over the rects that share it, then a synchronize.  Returns the buffers' downloads."""
    cam = settings.camera_settings
    with contextlib.ExitStack() as stack:
        ds = stack.enter_context(DeviceScene(ctx, scene))
        buffers = [stack.enter_context(t(ctx, cam.backbuffer_width, cam.backbuffer_height)) for t in buffer_types]
        for n in sorted(set(int(c) for c in counts)):
            if n > 0:
                render(ds, cam, [r for r, c in zip(rects, counts) if int(c) == n], n, *buffers)
        ctx.synchronize()
        return tuple(b.download() for b in buffers)


def render_ids_arrays(ctx, scene, settings, rects, counts):
    """The (H, W, 10) uint32 ID words of a frame whose rect i holds counts[i] samples: one rmd_render_ids call per distinct sample count, each tile at
    its own count, with the settings' seed and DOF flag (as finished_tile_features renders the features).  Pixels no rect covers stay zero."""
    return _first_hit_arrays(ctx, scene, settings, rects, counts, (IdBuffer,),
                             lambda ds, cam, share, n, ids: render_ids(ctx, ds, cam, settings, share, ids, 0, n, sync=False))[0]


def render_ao_arrays(ctx, scene, settings, rects, counts, max_distance):
    """The (H, W, 4) uint32 AO words of a frame whose rect i holds counts[i] samples: one rmd_render_ao call per distinct sample count, each tile at
    its own count, with the settings' seed and DOF flag (as render_ids_arrays renders the IDs).  Pixels no rect covers stay zero."""
    return _first_hit_arrays(ctx, scene, settings, rects, counts, (AoBuffer,),
                             lambda ds, cam, share, n, ao: render_ao(ctx, ds, cam, settings, share, max_distance, ao, 0, n, sync=False))[0]


def ids_ranked(words):
    """Plain numpy: the slots of (..., 10) ID words ordered per pixel by count descending, ties by slot -> (keys, counts), each (..., 4).  Empty slots
    (key 0, count 0) trail unless a count has wrapped to 0."""
    words = np.asarray(words, dtype=np.uint32)
    keys, counts = words[..., 0:8:2], words[..., 1:8:2]
    order = np.argsort(-counts.astype(np.int64), axis=-1, kind="stable")
    return np.take_along_axis(keys, order, axis=-1), np.take_along_axis(counts, order, axis=-1)


def render_tiles(ctx, dscene, camera_settings, settings, tiles, framebuffer, sample_begin=0, sample_count=None, sync=True, framebuffer_sq=None):
    """rmd_render_tiles[_async]: add `sample_count` samples per pixel of `tiles` into `framebuffer`.  With `framebuffer_sq`:
    rmd_render_tiles_moments[_async], which also adds every sample's square to it."""
    if framebuffer_sq is None:
        _render_call(ctx, "rmd_render_tiles", sync, dscene, camera_settings, settings, tiles, sample_begin, sample_count, framebuffer.ptr)
    else:
        _render_call(ctx, "rmd_render_tiles_moments", sync, dscene, camera_settings, settings, tiles, sample_begin, sample_count, framebuffer.ptr, framebuffer_sq.ptr)


def tile_error(ctx, framebuffer, framebuffer_sq, sample_count, floor, tiles):
    """rmd_tile_error: per tile, the relative standard error of its worst pixel and channel after `sample_count` samples (float64 array)."""
    out = np.empty(max(1, len(tiles)), dtype=np.float64)
    ctx.check(ctx.L.rmd_tile_error(ctx.handle, framebuffer.ptr, framebuffer_sq.ptr, framebuffer.width, framebuffer.height, int(sample_count), float(floor),
                                   tile_array(tiles), len(tiles), out.ctypes.data_as(C.c_void_p)))
    return out[: len(tiles)]


def _counts(rects, *counts, what="one sample count per rect"):
    """Each of `counts` as a uint32 array, one per rect."""
    arrays = [np.ascontiguousarray(c, dtype=np.uint32) for c in counts]
    if any(len(a) != len(rects) for a in arrays):
        raise ValueError(what)
    return arrays


def _u32(array):
    return None if array is None else array.ctypes.data_as(C.POINTER(C.c_uint32))


def despike(ctx, framebuffer, framebuffer_sq, rects, counts, radius=2, rank=2, k=6.0, ratio=2.0, floor=0.0, out=None, want_replaced=True):
    """rmd_despike: firefly rejection from the moments.  A pixel whose luminance stands more than `k` standard errors of its DONOR — the other of its
    (2 * radius + 1)^2 window at 0-based index `rank` by luminance — above `ratio` times the donor's plus `floor` takes the donor's sums, at its own count.
    Returns (Framebuffer S', Framebuffer Q', replaced): the two new sum buffers (the caller closes them), which every call takes in place of the inputs
    with the same rects and counts, and the number of pixels replaced in each rect (uint32 array).  `out`: a (Framebuffer, Framebuffer) pair to write into
    instead of two new ones.  want_replaced=False passes NULL for the counts and returns None for them."""
    rects = list(rects)
    (counts,) = _counts(rects, counts)
    W, H = framebuffer.width, framebuffer.height
    with contextlib.ExitStack() as made:
        if out is None:
            out = (made.enter_context(Framebuffer(ctx, W, H)), made.enter_context(Framebuffer(ctx, W, H)))
        replaced = np.zeros(max(1, len(rects)), dtype=np.uint32) if want_replaced else None
        ctx.check(ctx.L.rmd_despike(ctx.handle, framebuffer.ptr, framebuffer_sq.ptr, W, H, tile_array(rects), _u32(counts), len(rects), int(radius), int(rank),
                                    float(k), float(ratio), float(floor), out[0].ptr, out[1].ptr, _u32(replaced)))
        made.pop_all()  # (the call went through: the new buffers are the caller's)
    return out[0], out[1], None if replaced is None else replaced[: len(rects)]


def _staged(stack, ctx, like, *buffers):
    """One device buffer per (kind, host array or None) of `buffers`, of the frame size of the (H, W, ..) array `like`: all allocated, then every array
    that is given uploaded to its buffer.  `stack` (an ExitStack) closes them."""
    H, W = like.shape[0], like.shape[1]
    made = [stack.enter_context(kind(ctx, W, H)) for kind, _ in buffers]
    for buf, (_, arr) in zip(made, buffers):
        if arr is not None:
            buf.upload(arr)
    return made


def despike_arrays(ctx, sums, sums_sq, rects, counts, **params):
    """despike() for host arrays: (H, W, 3) sums and sums of squares in; the (H, W, 3) despiked sums, sums of squares and the per-rect replaced counts out."""
    with contextlib.ExitStack() as stack:
        s, q, s_out, q_out = _staged(stack, ctx, sums, (Framebuffer, sums), (Framebuffer, sums_sq), (Framebuffer, None), (Framebuffer, None))
        _, _, replaced = despike(ctx, s, q, rects, counts, out=(s_out, q_out), **params)
        return s_out.download(), q_out.download(), replaced


def despike_dual(ctx, half_a, half_b, rects, counts_a, counts_b, radius=2, rank=2, k=6.0, ratio=2.0, floor=0.0, out=None, want_replaced=True):
    """rmd_despike_dual: firefly rejection for the two halves of a dual-buffer frame.  half_a and half_b are (Framebuffer S, Framebuffer Q) pairs.  The
    decision is despike()'s on the merged pixel (S_A + S_B, Q_A + Q_B at n_A + n_B; both halves must hold a sample); a spike takes, half by half, its
    donor's sums of that half at its own half count, so the halves stay independent sample sets.
    Returns ((S'_A, Q'_A), (S'_B, Q'_B), replaced): four new sum buffers (the caller closes them), which every dual call takes in place of the inputs with
    the same rects and counts, and the number of pixels replaced in each rect (uint32 array).  `out`: ((Framebuffer, Framebuffer), (Framebuffer,
    Framebuffer)) to write into instead of four new ones.  want_replaced=False passes NULL for the counts and returns None for them."""
    rects = list(rects)
    counts_a, counts_b = _counts(rects, counts_a, counts_b, what="one sample count per rect and half")
    W, H = half_a[0].width, half_a[0].height
    with contextlib.ExitStack() as made:
        if out is None:
            out = tuple((made.enter_context(Framebuffer(ctx, W, H)), made.enter_context(Framebuffer(ctx, W, H))) for _ in range(2))
        replaced = np.zeros(max(1, len(rects)), dtype=np.uint32) if want_replaced else None
        ctx.check(ctx.L.rmd_despike_dual(ctx.handle, half_a[0].ptr, half_a[1].ptr, half_b[0].ptr, half_b[1].ptr, W, H, tile_array(rects), _u32(counts_a),
                                         _u32(counts_b), len(rects), int(radius), int(rank), float(k), float(ratio), float(floor), out[0][0].ptr, out[0][1].ptr,
                                         out[1][0].ptr, out[1][1].ptr, _u32(replaced)))
        made.pop_all()  # (the call went through: the new buffers are the caller's)
    return (out[0][0], out[0][1]), (out[1][0], out[1][1]), None if replaced is None else replaced[: len(rects)]


def despike_dual_arrays(ctx, sums_a, sums_sq_a, sums_b, sums_sq_b, rects, counts_a, counts_b, **params):
    """despike_dual() for host arrays: four (H, W, 3) arrays in; the four despiked ones, in the same order, and the per-rect replaced counts out."""
    with contextlib.ExitStack() as stack:
        bufs = _staged(stack, ctx, sums_a, (Framebuffer, sums_a), (Framebuffer, sums_sq_a), (Framebuffer, sums_b), (Framebuffer, sums_sq_b), *[(Framebuffer, None)] * 4)
        _, _, replaced = despike_dual(ctx, bufs[0:2], bufs[2:4], rects, counts_a, counts_b, out=(bufs[4:6], bufs[6:8]), **params)
        return bufs[4].download(), bufs[5].download(), bufs[6].download(), bufs[7].download(), replaced


TILE_LUMA_DTYPE = np.dtype([("tile_rms", "<f8"), ("pixel_rms", "<f8"), ("mean_luma", "<f8"), ("mean_variance", "<f8"), ("mean_rel_variance", "<f8"),
                            ("valid", "<u4"), ("invalid", "<u4")])  # rmd_tile_luma, field for field
assert TILE_LUMA_DTYPE.itemsize == C.sizeof(abi.TileLuma)


def _tile_measure(entry, dtype, result, ctx, framebuffer, framebuffer_sq, tiles, counts, parameter):
    """One per-tile measure: `entry` of the library over the tiles at their own counts, into a structured array of `dtype` (the C struct `result`, field for
    field).  parameter(): the measure's own argument as ctypes takes it, made once the counts are checked."""
    tiles = list(tiles)
    (counts,) = _counts(tiles, counts)
    parameter = parameter()
    out = np.zeros(max(1, len(tiles)), dtype=dtype)
    ctx.check(getattr(ctx.L, entry)(ctx.handle, framebuffer.ptr, framebuffer_sq.ptr, framebuffer.width, framebuffer.height, tile_array(tiles), _u32(counts), len(tiles),
                                    parameter, out.ctypes.data_as(C.POINTER(result))))
    return out[: len(tiles)]


def _tile_measure_arrays(measure, ctx, sums, sums_sq, tiles, counts, parameter):
    """`measure` (tile_luma_error, tile_weighted_error) for host arrays: (H, W, 3) sums and sums of squares in, the structured array out."""
    with contextlib.ExitStack() as stack:
        s, q = _staged(stack, ctx, sums, (Framebuffer, sums), (Framebuffer, sums_sq))
        return measure(ctx, s, q, tiles, counts, parameter)


def tile_luma_error(ctx, framebuffer, framebuffer_sq, tiles, counts, floor):
    """rmd_tile_luma_error: per tile, at its own sample count, the aggregated noise of its luminance — a numpy structured array with rmd_tile_luma's fields:
    tile_rms (the RMS standard error of the luminance over the tile's mean luminance), pixel_rms (the RMS of the pixels' relative luminance errors), the
    three means they are made of, and the valid / invalid pixel counts.  Tiles may overlap or repeat."""
    return _tile_measure("rmd_tile_luma_error", TILE_LUMA_DTYPE, abi.TileLuma, ctx, framebuffer, framebuffer_sq, tiles, counts, lambda: float(floor))


def tile_luma_error_arrays(ctx, sums, sums_sq, tiles, counts, floor):
    """tile_luma_error() for host arrays: (H, W, 3) sums and sums of squares in, the structured array out."""
    return _tile_measure_arrays(tile_luma_error, ctx, sums, sums_sq, tiles, counts, floor)


TILE_WEIGHTED_DTYPE = np.dtype([("rms", "<f8"), ("mean_weighted_variance", "<f8"), ("mean_luma", "<f8"), ("mean_variance", "<f8"), ("valid", "<u4"),
                                ("invalid", "<u4")])  # rmd_tile_weighted, field for field
assert TILE_WEIGHTED_DTYPE.itemsize == C.sizeof(abi.TileWeighted)


def _weights(weights):
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    if weights.shape != (abi.LUMA_WEIGHTS,):
        raise ValueError("a weight table has %d entries" % abi.LUMA_WEIGHTS)
    return weights


def tile_weighted_error(ctx, framebuffer, framebuffer_sq, tiles, counts, weights):
    """rmd_tile_weighted_error: per tile, at its own sample count, the variance of its pixels' luminance weighted by `weights` — abi.LUMA_WEIGHTS doubles,
    one per counter of the luminance histogram (256 bins, below, above, zero, negative); a pixel takes the entry its luminance's bits name — as a numpy
    structured array with rmd_tile_weighted's fields: rms (what an adaptive check compares with its threshold), mean_weighted_variance, mean_luma,
    mean_variance and the valid / invalid pixel counts.  display_weights() makes the table of the displayed error.  Tiles may overlap or repeat."""
    return _tile_measure("rmd_tile_weighted_error", TILE_WEIGHTED_DTYPE, abi.TileWeighted, ctx, framebuffer, framebuffer_sq, tiles, counts,
                         lambda: _weights(weights).ctypes.data_as(C.POINTER(C.c_double)))


def tile_weighted_error_arrays(ctx, sums, sums_sq, tiles, counts, weights):
    """tile_weighted_error() for host arrays: (H, W, 3) sums and sums of squares in, the structured array out."""
    return _tile_measure_arrays(tile_weighted_error, ctx, sums, sums_sq, tiles, counts, weights)


def display_weights(exposure=1.0, gamma=2.2, display_floor=1.0 / 255.0):
    """rmd_display_weights: the table that makes tile_weighted_error measure the displayed error — per luminance counter the squared slope of the tone curve
    (1 - exp(-y exposure))^(1 / gamma), capped at the luminance that displays at `display_floor` (a host function) -> abi.LUMA_WEIGHTS float64."""
    out = np.zeros(abi.LUMA_WEIGHTS, dtype=np.float64)
    _lib.check(_lib.load().rmd_display_weights(float(exposure), float(gamma), float(display_floor), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


_GUIDED = {"rmd_denoise": "rmd_denoise_guided", "rmd_denoise_dual": "rmd_denoise_dual_guided"}  # the stems whose name says that the features are there


def _denoise_call(ctx, stem, sums, rects, counts, params, outputs, features=None, region=None, slope=None, after_slope=()):
    """One call of the rmd_denoise family.  Every one of its entry points is laid out as

        ctx | sum buffers | [feature buffers] | W, H | rects | counts.. | n_rects | [region rects, n] | parameters [slope] [..] | outputs

    and is named by the groups it has: `stem`, _guided where a stem's features are optional in the header (`features` is the pair of FeatureBuffers, either
    of which may be None; features=None leaves the group out), _slope for `slope` and _region for `region` (a list of rects, possibly empty).  `sums` and
    `outputs` are device buffers (an output may be None), `counts` uint32 arrays (the feature counts may be None), `params` and `after_slope` ready C
    scalars and arrays.  lib.SIGNATURES holds the header's own argument types, so a group out of place does not get past ctypes."""
    name = (stem if features is None else _GUIDED.get(stem, stem)) + ("" if slope is None else "_slope") + ("" if region is None else "_region")
    args = [ctx.handle] + [b.ptr for b in sums] + ([] if features is None else [_ptr(b) for b in features])
    args += [sums[0].width, sums[0].height, tile_array(rects)] + [_u32(c) for c in counts] + [len(rects)]
    if region is not None:
        region = list(region)
        args += [tile_array(region), len(region)]
    args += list(params) + ([] if slope is None else [slope]) + list(after_slope) + [_ptr(o) for o in outputs]
    ctx.check(getattr(ctx.L, name)(*args))


def _slope(slope):
    return None if slope is None else float(slope)


def denoise(ctx, framebuffer, framebuffer_sq, rects, counts, out_framebuffer, radius=10, patch_radius=3, k=0.45, alpha=1.0):
    """rmd_denoise: `out_framebuffer` = the variance-guided non-local means of the frame whose sums are `framebuffer` and sums of squares
    `framebuffer_sq`; rect i of `rects` (left, top, width, height) holds counts[i] samples per pixel.  The result holds means, not sums."""
    _denoise_call(ctx, "rmd_denoise", (framebuffer, framebuffer_sq), rects, _counts(rects, counts), (int(radius), int(patch_radius), float(k), float(alpha)),
                  (out_framebuffer,))


def denoise_arrays(ctx, sums, sums_sq, rects, counts, **params):
    """denoise() for host arrays: (H, W, 3) sums and sums of squares in, the (H, W, 3) denoised means out."""
    with contextlib.ExitStack() as stack:
        s, q, out = _staged(stack, ctx, sums, (Framebuffer, sums), (Framebuffer, sums_sq), (Framebuffer, None))
        denoise(ctx, s, q, rects, counts, out, **params)
        return out.download()


def denoise_guided(ctx, framebuffer, framebuffer_sq, features, features_sq, rects, counts, out_framebuffer, radius=10, patch_radius=3, k=0.45, alpha=1.0,
                   k_f=1.0, tau=1e-2, slope=None):
    """rmd_denoise_guided: denoise() with the feature weight of the FeatureBuffers `features` / `features_sq` (both None: exactly denoise()).
    `slope` (a number; None: the call above): rmd_denoise_guided_slope, the same with the feature-slope term at that many pixels (0: the same bytes);
    without features it is passed and not read, as the header states."""
    _denoise_call(ctx, "rmd_denoise", (framebuffer, framebuffer_sq), rects, _counts(rects, counts),
                  (int(radius), int(patch_radius), float(k), float(alpha), float(k_f), float(tau)), (out_framebuffer,), features=(features, features_sq),
                  slope=_slope(slope))


def _staged_guided(stack, ctx, sums, sums_sq, feats, feats_sq):
    """denoise_guided_arrays' and denoise_atrous_arrays' buffers: sums, sums of squares, the output, then the features; all allocated before any upload."""
    features = [(FeatureBuffer, feats), (FeatureBuffer, feats_sq)] if feats is not None else []
    made = _staged(stack, ctx, sums, (Framebuffer, sums), (Framebuffer, sums_sq), (Framebuffer, None), *features)
    return made + [None] * (5 - len(made))


def denoise_guided_arrays(ctx, sums, sums_sq, feats, feats_sq, rects, counts, **params):
    """denoise_guided() for host arrays: (H, W, 3) sums and sums of squares and (H, W, 7) feature sums and sums of squares in (the latter two may
    both be None), the (H, W, 3) denoised means out."""
    with contextlib.ExitStack() as stack:
        s, q, out, f, f_sq = _staged_guided(stack, ctx, sums, sums_sq, feats, feats_sq)
        denoise_guided(ctx, s, q, f, f_sq, rects, counts, out, **params)
        return out.download()


def denoise_atrous(ctx, framebuffer, framebuffer_sq, rects, counts, out_framebuffer, levels=5, k=3.0, alpha=1.0, features=None, features_sq=None, k_f=1.0,
                   tau=1e-2, slope=None):
    """rmd_denoise_atrous: `out_framebuffer` = the frame after `levels` levels of the edge-avoiding a-trous filter (the fast filter for previews), with
    the feature weight of the FeatureBuffers `features` / `features_sq` when they are given.  The result holds means, not sums.
    `slope` (a number; None: the call above): rmd_denoise_atrous_slope, the same with the feature-slope term at that many pixels (0: the same bytes)."""
    _denoise_call(ctx, "rmd_denoise_atrous", (framebuffer, framebuffer_sq), rects, _counts(rects, counts),
                  (int(levels), float(k), float(alpha), float(k_f), float(tau)), (out_framebuffer,), features=(features, features_sq), slope=_slope(slope))


def denoise_atrous_arrays(ctx, sums, sums_sq, feats, feats_sq, rects, counts, **params):
    """denoise_atrous() for host arrays: (H, W, 3) sums and sums of squares and (H, W, 7) feature sums and sums of squares in (the latter two may
    both be None), the (H, W, 3) filtered means out."""
    with contextlib.ExitStack() as stack:
        s, q, out, f, f_sq = _staged_guided(stack, ctx, sums, sums_sq, feats, feats_sq)
        denoise_atrous(ctx, s, q, rects, counts, out, features=f, features_sq=f_sq, **params)
        return out.download()


class ErrorImage(Framebuffer):
    """W*H f64 in HBM: rmd_denoise_dual's per-pixel error estimate (the allocation is a framebuffer's; its first W*H doubles are used)."""

    download_tiles = upload_tiles = _no_tile_transfers("error images")

    def __init__(self, ctx, width, height):
        Framebuffer.__init__(self, ctx, width, height)

    def _shape(self):
        return (self.height, self.width)


def _dual_counts(rects, counts_a, counts_b):
    return _counts(rects, counts_a, counts_b, what="one sample count per rect and half")


def _feature_counts(rects, counts_f):
    return _counts(rects, [] if counts_f is None else counts_f, what="one feature sample count per rect")


def denoise_dual(ctx, half_a, half_b, rects, counts_a, counts_b, out_framebuffer, error_image=None, radius=10, patch_radius=3, k=0.45, alpha=1.0, region=None,
                 features=None, features_sq=None, counts_f=None, k_f=1.0, tau=1e-2, slope=None):
    """rmd_denoise_dual: `out_framebuffer` = the cross-filtered means of the two sample halves `half_a` and `half_b`, each a (sums, sums of squares)
    pair of Framebuffers; rect i holds counts_a[i] and counts_b[i] samples per pixel in them.  `error_image` (an ErrorImage, optional) receives the
    per-pixel error estimate.  `region` (a list of rects, possibly empty): rmd_denoise_dual_region — only the pixels of those rects are written, with
    the bytes the whole-frame call gives them; None is the whole-frame call.  `features` / `features_sq` (FeatureBuffers; rect i holds counts_f[i]
    feature samples per pixel): rmd_denoise_dual_guided[_region], the same with rmd_denoise_guided's feature weight; features=None makes the calls above.
    `slope` (a number; None: the calls above): rmd_denoise_dual_guided_slope[_region], the same with the feature-slope term.  Without features the slope
    is not read, as in the C calls and in denoise_guided: the unguided calls above are made."""
    counts = _dual_counts(rects, counts_a, counts_b)
    params = (int(radius), int(patch_radius), float(k), float(alpha))
    halves = (half_a[0], half_a[1], half_b[0], half_b[1])
    if features is None and features_sq is None:
        _denoise_call(ctx, "rmd_denoise_dual", halves, rects, counts, params, (out_framebuffer, error_image), region=region)
    else:
        _denoise_call(ctx, "rmd_denoise_dual", halves, rects, counts + _feature_counts(rects, counts_f), params + (float(k_f), float(tau)),
                      (out_framebuffer, error_image), features=(features, features_sq), region=region, slope=_slope(slope))


def _staged_dual(stack, ctx, halves, out_init, images, features, features_sq):
    """The dual helpers' buffers, each allocated and filled before the next: the two halves' sums and sums of squares and the output frame (`out_init`:
    what it holds before the call, or None), one image per (kind, what it holds before the call or None) of `images`, and the two feature buffers when
    `features` is given -> half A, half B, the output, the images, (features, features_sq)."""
    def one(kind, arr):
        return _staged(stack, ctx, halves[0], (kind, arr))[0]

    fbs = [one(Framebuffer, arr) for arr in (*halves, out_init)]
    imgs = [one(kind, arr) for kind, arr in images]
    feats = [one(FeatureBuffer, arr) for arr in (features, features_sq)] if features is not None else [None, None]
    return (fbs[0], fbs[1]), (fbs[2], fbs[3]), fbs[4], imgs, feats


def denoise_dual_arrays(ctx, sums_a, sums_sq_a, sums_b, sums_sq_b, rects, counts_a, counts_b, region=None, out_init=None, err_init=None, features=None,
                        features_sq=None, **params):
    """denoise_dual() for host arrays: the two halves' (H, W, 3) sums and sums of squares in; the (H, W, 3) means and the (H, W) error estimate out.
    `out_init` (H, W, 3) and `err_init` (H, W): what the two outputs hold before the call — what a pixel outside `region` still holds after it.
    `features` / `features_sq`: (H, W, 7) feature sums and sums of squares for the guided forms (with counts_f, k_f, tau among the params)."""
    with contextlib.ExitStack() as stack:
        a, b, out, (err,), (f, f_sq) = _staged_dual(stack, ctx, (sums_a, sums_sq_a, sums_b, sums_sq_b), out_init, [(ErrorImage, err_init)], features, features_sq)
        denoise_dual(ctx, a, b, rects, counts_a, counts_b, out, err, region=region, features=f, features_sq=f_sq, **params)
        return out.download(), err.download()


def denoise_atrous_dual(ctx, half_a, half_b, rects, counts_a, counts_b, out_framebuffer, error_image=None, levels=5, k=3.0, alpha=1.0, features=None,
                        features_sq=None, counts_f=None, k_f=1.0, tau=1e-2, region=None, slope=None):
    """rmd_denoise_atrous_dual: `out_framebuffer` = the two sample halves `half_a` and `half_b` (as denoise_dual's) after `levels` levels of the
    edge-avoiding a-trous filter, each half under the other's weights, combined as denoise_dual combines them; `error_image` (an ErrorImage,
    optional) receives the per-pixel error estimate.  `features` / `features_sq` (FeatureBuffers; rect i holds counts_f[i] feature samples per
    pixel) add the feature weight; without them counts_f, k_f and tau are not read.  `region` (a list of rects, possibly empty):
    rmd_denoise_atrous_dual_region — only the pixels of those rects are written, with the bytes the whole-frame call gives them; None is the whole-frame
    call.  `slope` (a number; None: the calls above): rmd_denoise_atrous_dual_slope[_region], the same with the feature-slope term."""
    counts = _dual_counts(rects, counts_a, counts_b)
    counts += [None] if features is None and features_sq is None else _feature_counts(rects, counts_f)
    _denoise_call(ctx, "rmd_denoise_atrous_dual", (half_a[0], half_a[1], half_b[0], half_b[1]), rects, counts,
                  (int(levels), float(k), float(alpha), float(k_f), float(tau)), (out_framebuffer, error_image), features=(features, features_sq), region=region,
                  slope=_slope(slope))


def denoise_atrous_dual_arrays(ctx, sums_a, sums_sq_a, sums_b, sums_sq_b, rects, counts_a, counts_b, out_init=None, err_init=None, features=None,
                               features_sq=None, want_err=True, region=None, **params):
    """denoise_atrous_dual() for host arrays: the two halves' (H, W, 3) sums and sums of squares in; the (H, W, 3) means and the (H, W) error estimate
    out (None for the latter with want_err=False: the call is then made without an error image).  `out_init` / `err_init`: what the two outputs hold
    before the call — what a pixel outside `region` still holds after it.  `features` / `features_sq`: (H, W, 7) feature sums and sums of squares (with
    counts_f, k_f, tau among the params)."""
    with contextlib.ExitStack() as stack:
        a, b, out, (err,), (f, f_sq) = _staged_dual(stack, ctx, (sums_a, sums_sq_a, sums_b, sums_sq_b), out_init, [(ErrorImage, err_init)], features, features_sq)
        denoise_atrous_dual(ctx, a, b, rects, counts_a, counts_b, out, err if want_err else None, features=f, features_sq=f_sq, region=region, **params)
        return out.download(), err.download() if want_err else None


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
    counts = _dual_counts(rects, counts_a, counts_b)
    counts += [None] if counts_f is None else _counts(rects, counts_f, what="one feature sample count per rect")
    candidates = list(candidates)
    slopes = None  # (in this call the slopes follow the candidates they belong to, and the candidates' number follows them)
    if any("slope" in c for c in candidates):
        slopes = (C.c_double * len(candidates))(*[float(c.get("slope", 0.0)) for c in candidates])
    _denoise_call(ctx, "rmd_denoise_dual_select", (half_a[0], half_a[1], half_b[0], half_b[1]), rects, counts,
                  (int(radius), int(patch_radius), candidate_array(candidates)), (out_framebuffer, error_image, sure_image, winner_image),
                  features=(features, features_sq), slope=slopes, after_slope=(len(candidates), int(sure_window), int(select_window)))


def denoise_dual_select_arrays(ctx, sums_a, sums_sq_a, sums_b, sums_sq_b, rects, counts_a, counts_b, candidates, features=None, features_sq=None,
                               want=("err", "sure", "win"), init=None, **params):
    """denoise_dual_select() for host arrays: the two halves' (H, W, 3) sums and sums of squares in (and (H, W, 7) `features` / `features_sq` with counts_f
    among the params for guided candidates); a dict out with "out" (H, W, 3) and those of "err" (H, W), "sure" (H, W) and "win" (H, W) uint32 named in
    `want` — one left out is passed as NULL.  `init`: a dict of what the named outputs hold before the call."""
    init = init or {}
    names = [name for name in ("err", "sure", "win") if name in want]
    with contextlib.ExitStack() as stack:
        a, b, out, made, (f, f_sq) = _staged_dual(stack, ctx, (sums_a, sums_sq_a, sums_b, sums_sq_b), init.get("out"),
                                                  [(WinnerImage if name == "win" else ErrorImage, init.get(name)) for name in names], features, features_sq)
        imgs = dict(zip(names, made))
        denoise_dual_select(ctx, a, b, rects, counts_a, counts_b, candidates, out, imgs.get("err"), imgs.get("sure"), imgs.get("win"), features=f, features_sq=f_sq,
                            **params)
        res = {"out": out.download()}
        for name, img in imgs.items():
            res[name] = img.download()
        return res


def tile_error_dual(ctx, error_image, tiles):
    """rmd_tile_error_dual: per tile, the root mean square of `error_image` (rmd_denoise_dual's estimate) over its pixels; +inf for a tile with a
    pixel that is not dual-valid (float64 array)."""
    out = np.empty(max(1, len(tiles)), dtype=np.float64)
    ctx.check(ctx.L.rmd_tile_error_dual(ctx.handle, error_image.ptr, error_image.width, error_image.height, tile_array(tiles), len(tiles),
                                        out.ctypes.data_as(C.c_void_p)))
    return out[: len(tiles)]


def tile_weighted_error_dual(ctx, out_fb, err_img, tiles, weights):
    """rmd_tile_weighted_error_dual: per tile, `err_img` (a dual filter's per-pixel error estimate) weighted by `weights` — abi.LUMA_WEIGHTS doubles, a
    pixel taking the entry the luminance of its filtered means in `out_fb` names — as the structured array tile_weighted_error returns; rms is +inf for a
    tile with a pixel that is not dual-valid.  display_weights() makes the table of the displayed error.  Tiles may overlap or repeat."""
    tiles = list(tiles)
    out = np.zeros(max(1, len(tiles)), dtype=TILE_WEIGHTED_DTYPE)
    ctx.check(ctx.L.rmd_tile_weighted_error_dual(ctx.handle, out_fb.ptr, err_img.ptr, out_fb.width, out_fb.height, tile_array(tiles), len(tiles),
                                                 _weights(weights).ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(abi.TileWeighted))))
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
    (counts,) = _counts(rects, counts)
    out = np.empty(3 * sum(w * h for (_, _, w, h) in rects), dtype=np.uint8)
    ctx.check(ctx.L.rmd_resolve_tonemap_tiles(ctx.handle, framebuffer.ptr, _ptr(second), framebuffer.width, framebuffer.height, tile_array(rects), _u32(counts),
                                              len(rects), float(exposure), float(gamma), out.ctypes.data_as(C.c_void_p)))
    return _tile_views(out, rects)


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
    (counts,) = _counts(rects, counts)
    out = abi.LumaHistogram()
    ctx.check(ctx.L.rmd_luminance_histogram_tiles(ctx.handle, framebuffer.ptr, _ptr(second), framebuffer.width, framebuffer.height, tile_array(rects),
                                                  _u32(counts), len(rects), C.byref(out)))
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
def _guide(settings, features, counts_f, atrous=False):
    """The keywords that make a dual filter call (denoise_dual, or with `atrous` denoise_atrous_dual; their *_arrays forms alike) the guided one: `features`,
    a (sums, sums of squares) pair at counts_f[i] samples in rect i, with the settings' feature weight and slope.  features=None: {}, the unguided call."""
    if features is None:
        return {}
    return dict(features=features[0], features_sq=features[1], counts_f=counts_f, **settings.guide_keywords(atrous))


class Tile:  # core/src/tile.rs:7-14
    def __init__(self, left, top, width, height, sample_count, data, error=None, data_sq=None):
        self.left, self.top, self.width, self.height = left, top, width, height
        self.sample_count = sample_count
        self.data = data  # (height, width, 3) running sums, like Tile.data
        # adaptive renders (an extension): the measure that decided — the tile's rmd_tile_error, or with settings.adaptive_measure "luma_tile" / "luma_pixel"
        # its rmd_tile_luma_error tile_rms / pixel_rms — at sample_count when it was checked, else None
        self.error = error
        self.data_sq = data_sq  # denoised renders (an extension): the finished tile's running sums of squares, like data; else None
        # dual-buffer renders (an extension): the finished tile's two sample halves — sums, sums of squares (like data) and samples per pixel —;
        # data and data_sq are then the halves' sums added, sample_count = count_a + count_b.  Else None
        self.data_a = self.data_sq_a = self.count_a = self.data_b = self.data_sq_b = self.count_b = None

    @property
    def rect(self):
        return (self.left, self.top, self.width, self.height)

    def put(self, frame, data):
        """`data` into this tile's pixels of the (H, W, ..) array `frame`."""
        frame[self.top : self.top + self.height, self.left : self.left + self.width] = data


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

    def _finished_tiles(self):
        """The tiles of the TileFinished messages at the head of the queue: the reference stops collecting at the first other message (:101-103)."""
        while self._messages:
            m = self._messages.pop(0)
            if m.kind != "TileFinished":
                break
            yield m.tile

    def await_(self):
        """`await`: W*H radiance values, row-major, each the tile sum divided by its sample count (:93-99).

        With settings.denoise (an extension): the finished tiles' sums, sums of squares and sample counts are assembled and the frame comes
        back through rmd_denoise on `device` — means as well; a pixel that no finished tile covers has n = 0 and comes back as 0 / 0.  With
        settings.denoise_features as well: the scene is uploaded to `device`, the finished tiles' first-hit features are rendered there
        (finished_tile_features) and the filter is rmd_denoise_guided.  With settings.denoise_atrous the filter is rmd_denoise_atrous instead, at
        denoise_atrous_levels and denoise_atrous_k, guided by the same features when denoise_features is on.
        With settings.despike: the assembled sums and sums of squares first go through rmd_despike on `device`, and the plain divide or whichever filter
        is on takes its outputs in their place."""
        st = self.settings
        cam = st.camera_settings
        shape = (cam.backbuffer_height, cam.backbuffer_width, 3)
        if st.denoise and st.denoise_dual:
            return self._await_dual()
        if st.denoise and (st.denoise_atrous or st.denoise_features):
            st.check_denoise()
        if st.denoise and st.denoise_features and self.scene is None:
            raise ValueError("settings.denoise_features: this TaskHandle was made without the scene whose features await_() has to render")
        if st.despike:
            st.check_despike()
        out = np.zeros(shape, dtype=np.float64)
        if not (st.denoise or st.despike):
            for t in self._finished_tiles():
                t.put(out, t.data / float(t.sample_count))
            return out
        sums, sums_sq, rects, counts = np.zeros(shape), np.zeros(shape), [], []
        for t in self._finished_tiles():
            t.put(sums, t.data)
            t.put(sums_sq, t.data_sq)
            rects.append(t.rect)
            counts.append(t.sample_count)
        with Context(self.device) as ctx:
            if st.despike:  # before anything else: the divide or filter below takes the despiked sums in place of the raw ones
                sums, sums_sq, _ = despike_arrays(ctx, sums, sums_sq, rects, counts, want_replaced=False, **st.despike_keywords())
            if st.denoise:
                return self._filtered(ctx, sums, sums_sq, rects, counts)
        for (l, t, w, h), n in zip(rects, counts):  # the plain divide, of the despiked sums
            out[t : t + h, l : l + w] = sums[t : t + h, l : l + w] / float(n)
        return out

    def _filtered(self, ctx, sums, sums_sq, rects, counts):
        """await_()'s frame through the single-buffer filter the settings name."""
        st = self.settings
        feats = finished_tile_features(ctx, self.scene, st, rects, counts) if st.denoise_features else (None, None)
        if st.denoise_atrous:
            return denoise_atrous_arrays(ctx, sums, sums_sq, *feats, rects, counts, **st.atrous_keywords(), **st.guide_keywords(atrous=True))
        if st.denoise_features:
            return denoise_guided_arrays(ctx, sums, sums_sq, *feats, rects, counts, **st.guide_keywords(), **st.nlm_keywords())
        return denoise_arrays(ctx, sums, sums_sq, rects, counts, **st.nlm_keywords())

    def _await_dual(self):
        """await_() with settings.denoise_dual: the finished tiles' two halves through rmd_denoise_dual on `device`.  With settings.denoise_dual_features:
        the finished tiles' first-hit features are rendered there at count_a + count_b samples per tile (finished_tile_features) and the filter is
        rmd_denoise_dual_guided.  With settings.denoise_dual_select: the features are rendered the same way and the frame is
        rmd_denoise_dual_select's at settings.select_candidates(), both windows 2.  With settings.denoise_dual_atrous the frame is
        rmd_denoise_atrous_dual's at denoise_atrous_levels and denoise_atrous_k, guided by the same features when denoise_dual_features is on."""
        st = self.settings
        st.check_denoise()
        featured = st.denoise_dual_features or st.denoise_dual_select
        if featured and self.scene is None:
            raise ValueError("settings.denoise_dual_features / denoise_dual_select: this TaskHandle was made without the scene whose features await_() has to render")
        cam = st.camera_settings
        shape = (cam.backbuffer_height, cam.backbuffer_width, 3)
        halves = [np.zeros(shape) for _ in range(4)]
        rects, counts_a, counts_b = [], [], []
        for t in self._finished_tiles():
            for dst, src in zip(halves, (t.data_a, t.data_sq_a, t.data_b, t.data_sq_b)):
                t.put(dst, src)
            rects.append(t.rect)
            counts_a.append(t.count_a)
            counts_b.append(t.count_b)
        counts_f = [a + b for a, b in zip(counts_a, counts_b)]
        with Context(self.device) as ctx:
            if st.despike_dual:  # before anything else: whichever dual filter is on takes the despiked halves in place of the raw ones
                st.check_despike()
                halves = list(despike_dual_arrays(ctx, *halves, rects, counts_a, counts_b, want_replaced=False, **st.despike_keywords())[:4])
            feats = finished_tile_features(ctx, self.scene, st, rects, counts_f) if featured else None
            if st.denoise_dual_atrous:
                out, _ = denoise_atrous_dual_arrays(ctx, *halves, rects, counts_a, counts_b, **st.atrous_keywords(), **_guide(st, feats, counts_f, atrous=True))
            elif st.denoise_dual_select:
                out = denoise_dual_select_arrays(ctx, *halves, rects, counts_a, counts_b, st.select_candidates(), features=feats[0], features_sq=feats[1],
                                                 counts_f=counts_f, want=(), radius=st.denoise_radius, patch_radius=st.denoise_patch, sure_window=2,
                                                 select_window=2)["out"]
            else:
                out, _ = denoise_dual_arrays(ctx, *halves, rects, counts_a, counts_b, **st.nlm_keywords(), **_guide(st, feats, counts_f))
        return out


def finished_tile_features(ctx, scene, settings, rects, counts):
    """The (H, W, 7) first-hit feature sums and sums of squares of a frame whose rect i holds counts[i] samples: one rmd_render_features call per
    distinct sample count, each tile at its own count, with the settings' seed and DOF flag.  Pixels no rect covers stay zero."""
    return _first_hit_arrays(ctx, scene, settings, rects, counts, (FeatureBuffer, FeatureBuffer),
                             lambda ds, cam, share, n, fb, fb_sq: render_features(ctx, ds, cam, settings, share, fb, 0, n, sync=False, features_sq=fb_sq))


def _preview(settings, W, H, pass_index, sample_count, calls):
    """The Message.FramePreview of one pass.  `calls`: per device, the (ctx, framebuffer, rects, counts, second) its rmd_resolve_tonemap_tiles call takes.
    With preview_auto_exposure every device first histograms exactly that, the histograms are added and the sum's exposure replaces preview_exposure;
    then every device resolves its tiles and the packed 8-bit tiles are scattered into one frame here."""
    st = settings
    exposure = None
    if st.preview_auto_exposure:
        hist = LumaHistogram()
        for ctx, fb, rects, counts, second in calls:
            hist = add_histograms(hist, luminance_histogram(ctx, fb, rects, counts, second=second))
        exposure = exposure_from_histogram(hist, st.auto_exposure_percentile, st.auto_exposure_target)
    frame = np.zeros((H, W, 3), dtype=np.uint8)
    for ctx, fb, rects, counts, second in calls:
        scatter_tiles(rects, resolve_tonemap_tiles(ctx, fb, rects, counts, st.preview_exposure if exposure is None else exposure, st.preview_gamma, second=second),
                      out=frame)
    return Message.FramePreview(frame, pass_index, sample_count, exposure)


class _Worker:
    """One device of render_tiled: its context, scene and sum buffers; `live`, the tiles of its share that still take passes; `early`, the
    (rect, sample count) of those that finished before the last pass."""

    def __init__(self, stack, device, scene, W, H, moments):
        self.ctx = stack.enter_context(Context(device))
        self.ds = stack.enter_context(DeviceScene(self.ctx, scene))
        self.fb = stack.enter_context(Framebuffer(self.ctx, W, H))
        self.fb_sq = stack.enter_context(Framebuffer(self.ctx, W, H)) if moments else None
        self.live, self.early = [], []

    def whole_frame(self, done):
        """The rects and counts of everything this device holds: the tiles that finished early at their counts, the live ones at `done`."""
        return [r for r, _ in self.early] + self.live, [c for _, c in self.early] + [done] * len(self.live)


class _TiledLoop:
    """render_tiled's single-buffer loop: the state its steps share.  Every device object is opened on `stack`."""

    def __init__(self, stack, scene, settings, devices):
        st = self.st = settings
        cam = st.camera_settings
        self.W, self.H = cam.backbuffer_width, cam.backbuffer_height
        self.display = st.adaptive_display_threshold > 0.0  # the check is rmd_tile_weighted_error under the tone curve's weights
        self.adaptive = st.adaptive_threshold > 0.0 or self.display
        self.threshold = st.adaptive_display_threshold if self.display else st.adaptive_threshold  # what a tile's measure has to meet
        # with a fixed exposure the weights are made once; with adaptive_display_auto_exposure every check makes its own (check_weights)
        self.weights = display_weights(st.adaptive_display_exposure, st.adaptive_display_gamma, st.adaptive_display_floor) if self.display else None
        self.despiked_at = None  # the pass whose despiked sums the spare buffers hold
        self.preview_filtered = st.preview_every > 0 and st.preview_denoise
        moments = self.adaptive or st.denoise or self.preview_filtered or st.despike
        self.with_sq = st.denoise or st.despike  # the finished tiles carry their sums of squares: await_() reads them
        self.workers = [_Worker(stack, d, scene, self.W, self.H, moments) for d in devices]
        first = self.workers[0].ctx
        self.filtered_fb = stack.enter_context(Framebuffer(first, self.W, self.H)) if self.preview_filtered else None  # (one device: check_preview)
        # despike with the adaptive check: two spare buffers for the despiked sums the check reads (one device: check_despike); the passes' own stay raw
        self.spare = tuple(stack.enter_context(Framebuffer(first, self.W, self.H)) for _ in range(2)) if st.despike and self.adaptive else None
        tiles = generate_tiles(self.W, self.H, st.tile_size)
        for i, w in enumerate(self.workers):
            w.live = tiles[i :: len(self.workers)]
        self.messages, self.finished = [], []
        self.done = self.passes = 0

    def render_pass(self, n):
        st = self.st
        for w in self.workers:
            if w.live:
                render_tiles(w.ctx, w.ds, st.camera_settings, st, w.live, w.fb, self.done, n, sync=False, framebuffer_sq=w.fb_sq)
        for w in self.workers:
            w.ctx.synchronize()
        self.done += n
        self.passes += 1

    def check_buffers(self, w):
        """The sums this pass's check reads on `w`: its own, or with despike the despiked sums of all its tiles at their counts, made once a pass."""
        if self.spare is None:
            return w.fb, w.fb_sq
        if self.despiked_at != self.passes:
            rects, counts = w.whole_frame(self.done)
            despike(w.ctx, w.fb, w.fb_sq, rects, counts, out=self.spare, want_replaced=False, **self.st.despike_keywords())
            self.despiked_at = self.passes
        return self.spare

    def check_weights(self):
        """adaptive_display_auto_exposure: before a check, every device histograms its whole frame at its tiles' own counts — the sums the check reads —,
        the histograms are added, and the weights are the tone curve's at the exposure the sum asks for."""
        st = self.st
        if not (self.display and st.adaptive_display_auto_exposure and any(w.live for w in self.workers)):
            return
        hist = LumaHistogram()
        for w in self.workers:
            rects, counts = w.whole_frame(self.done)
            if rects:
                hist = add_histograms(hist, luminance_histogram(w.ctx, self.check_buffers(w)[0], rects, counts))
        exposure = exposure_from_histogram(hist, st.auto_exposure_percentile, st.auto_exposure_target)
        self.weights = display_weights(exposure, st.adaptive_display_gamma, st.adaptive_display_floor)

    def adaptive_check(self, w):
        """The settings' adaptive measure of `w`'s live tiles (None each without a threshold): rmd_tile_error, or with a luma measure one
        rmd_tile_luma_error call's tile_rms or pixel_rms, or with adaptive_display_threshold one rmd_tile_weighted_error call's rms under the tone curve's
        weights; with despike, on the despiked sums of all its tiles at their counts."""
        st = self.st
        if not (self.adaptive and w.live):
            return [None] * len(w.live)
        fb, fb_sq = self.check_buffers(w)
        if self.display:
            return tile_weighted_error(w.ctx, fb, fb_sq, w.live, [self.done] * len(w.live), self.weights)["rms"]
        if st.adaptive_measure != "channel_max":
            luma = tile_luma_error(w.ctx, fb, fb_sq, w.live, [self.done] * len(w.live), st.adaptive_floor)
            return luma["tile_rms" if st.adaptive_measure == "luma_tile" else "pixel_rms"]
        return tile_error(w.ctx, fb, fb_sq, self.done, st.adaptive_floor, w.live)

    def finish(self, w, rect, sample_count, data, error=None, data_sq=None):
        l, t, width, height = rect
        self.finished.append(Message.TileFinished(Tile(l, t, width, height, sample_count, data, error, data_sq)))
        if sample_count < self.st.sample_count:  # converged between passes: the previews and the despiked check go on reading it at this count
            w.early.append((rect, sample_count))

    def snapshots(self, w, errors):
        """After a pass that leaves the render unfinished: `w`'s converged tiles finish at the samples they have, the others are sent as TileProgressed —
        from one download of the whole frame, or with progress_tiles off from the converged tiles' pixels alone and without a message for the rest."""
        st, done = self.st, self.done
        converged = [self.adaptive and e <= self.threshold for e in errors]
        conv = [r for r, c in zip(w.live, converged) if c]
        if not st.progress_tiles:
            data = w.fb.download_tiles(conv) if conv else []
            data_sq = w.fb_sq.download_tiles(conv) if conv and self.with_sq else [None] * len(conv)
            for rect, e, d, d_sq in zip(conv, [e for e, c in zip(errors, converged) if c], data, data_sq):
                self.finish(w, rect, done, d.copy(), float(e), None if d_sq is None else d_sq.copy())
        else:
            img = w.fb.download()
            img_sq = w.fb_sq.download() if self.with_sq else None
            for (l, t, width, height), e, c in zip(w.live, errors, converged):
                data = img[t : t + height, l : l + width].copy()
                if c:
                    self.finish(w, (l, t, width, height), done, data, float(e), None if img_sq is None else img_sq[t : t + height, l : l + width].copy())
                else:
                    self.messages.append(Message.TileProgressed(Tile(l, t, width, height, done, data, None if e is None else float(e))))
        w.live = [r for r, c in zip(w.live, converged) if not c]

    def preview(self):
        """Every device with tiles resolves its whole frame; with preview_denoise, rmd_denoise_atrous's means of it at count 1."""
        st = self.st
        calls = []
        for w in self.workers:
            rects, counts = w.whole_frame(self.done)
            if not rects:
                continue
            fb = w.fb
            if self.preview_filtered:
                denoise_atrous(w.ctx, w.fb, w.fb_sq, rects, counts, self.filtered_fb, **st.atrous_keywords())
                fb, counts = self.filtered_fb, [1] * len(rects)  # (means)
            calls.append((w.ctx, fb, rects, counts, None))
        self.messages.append(_preview(st, self.W, self.H, self.passes, self.done, calls))

    def finish_all(self):
        """The last pass is through: every tile still live finishes at sample_count."""
        for w in self.workers:
            img = w.fb.download()
            img_sq = w.fb_sq.download() if self.with_sq else None
            for (l, t, width, height) in w.live:
                sq = None if img_sq is None else img_sq[t : t + height, l : l + width].copy()
                self.finish(w, (l, t, width, height), self.st.sample_count, img[t : t + height, l : l + width].copy(), data_sq=sq)

    def run(self):
        st = self.st
        step = st.samples_per_iteration if st.samples_per_iteration else st.sample_count
        while self.done < st.sample_count:
            self.render_pass(min(step, st.sample_count - self.done))
            if self.done < st.sample_count and st.samples_per_iteration:
                self.check_weights()
                for w in self.workers:
                    self.snapshots(w, self.adaptive_check(w))
                if st.preview_every and self.passes % st.preview_every == 0 and any(w.live for w in self.workers):  # (no live tile: the render is finished)
                    self.preview()
        self.finish_all()
        return self.messages + self.finished  # progress snapshots (and previews) first, then the finished tiles


def render_tiled(scene, settings, devices=(0,)):
    """render_tiled (src/trace.rs:137): tiles -> workers -> TaskHandle.  Workers are GPU contexts.

    Adaptive (settings.adaptive_threshold > 0, an extension): every pass renders the tiles that are still live with their second moments, and
    after each pass that leaves them below sample_count a tile whose rmd_tile_error is at most the threshold is sent as TileFinished at its
    current sample count and takes no further passes; the others are sent as TileProgressed and go on.  With settings.adaptive_measure "luma_tile" or
    "luma_pixel" the check is one rmd_tile_luma_error call over the live tiles instead, and its tile_rms or pixel_rms is what meets the threshold.
    With settings.adaptive_display_threshold > 0 (instead of adaptive_threshold) the check is one rmd_tile_weighted_error call over the live tiles under
    rmd_display_weights' table — the tile's RMS error after exposure and gamma, in fractions of the display's full scale — at adaptive_display_exposure, or
    with adaptive_display_auto_exposure at the exposure every check's own histogram of the whole frame asks for (several devices' histograms are added).

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

    Dual-buffer (settings.denoise_dual, an extension): _render_tiled_dual.

    Whichever way a loop ends, the device objects it opened are closed in reverse order of opening."""
    settings.check_adaptive()
    settings.check_denoise()
    settings.check_preview(len(devices))
    settings.check_despike(len(devices))
    if settings.denoise_dual:
        return _render_tiled_dual(scene, settings, devices)
    with contextlib.ExitStack() as stack:
        messages = _TiledLoop(stack, scene, settings, devices).run()
    return TaskHandle(settings, messages, devices[0], scene if settings.denoise_features else None)


class _DualLoop:
    """The dual-buffer loop (_render_tiled_dual, which describes it): the state its steps share.  Every device object is opened on `stack`."""

    def __init__(self, stack, scene, settings, device):
        st = self.st = settings
        cam = st.camera_settings
        W, H = self.W, self.H = cam.backbuffer_width, cam.backbuffer_height
        self.display = st.adaptive_denoised_display_threshold > 0.0  # the check is rmd_tile_weighted_error_dual under the tone curve's weights
        self.adaptive = st.adaptive_denoised_threshold > 0.0 or self.display
        self.threshold = st.adaptive_denoised_display_threshold if self.display else st.adaptive_denoised_threshold  # what a tile's measure has to meet
        # with a fixed exposure the weights are made once; with adaptive_display_auto_exposure every check makes its own (check_weights)
        self.weights = display_weights(st.adaptive_display_exposure, st.adaptive_display_gamma, st.adaptive_display_floor) if self.display else None
        ctx = self.ctx = stack.enter_context(Context(device))
        self.ds = stack.enter_context(DeviceScene(ctx, scene))
        self.fbs = [stack.enter_context(Framebuffer(ctx, W, H)) for _ in range(4)]  # S_A, Q_A, S_B, Q_B
        if self.adaptive:
            self.out_fb, self.err_img = stack.enter_context(Framebuffer(ctx, W, H)), stack.enter_context(ErrorImage(ctx, W, H))
        # the feature buffers (sums, sums of squares) the guided check reads, or None: this loop keeps none
        self.feat_fbs = [stack.enter_context(FeatureBuffer(ctx, W, H)) for _ in range(2)] if self.adaptive and st.denoise_dual_features else None
        self.preview_fb = stack.enter_context(Framebuffer(ctx, W, H)) if st.preview_every and st.preview_denoise else None
        # despike_dual: four spare buffers for the despiked halves every dual filter call of this loop reads (the check, the filtered preview); the passes' own stay raw
        filters = self.adaptive or self.preview_fb is not None
        self.spare = [stack.enter_context(Framebuffer(ctx, W, H)) for _ in range(4)] if st.despike_dual and filters else None
        self.despiked_at = None  # the pass whose despiked halves the spare buffers hold
        self.live = generate_tiles(W, H, st.tile_size)
        self.done_rects, self.done_a, self.done_b = [], [], []  # the finished tiles and the counts they finished with
        self.n_half = [0, 0]  # samples per pixel of a live tile in A and B
        self.done = self.passes = 0
        self.messages, self.finished = [], []

    def render_pass(self, n):
        st, cam, half = self.st, self.st.camera_settings, self.passes & 1
        render_tiles(self.ctx, self.ds, cam, st, self.live, self.fbs[2 * half], self.done, n, sync=False, framebuffer_sq=self.fbs[2 * half + 1])
        if self.feat_fbs is not None:
            render_features(self.ctx, self.ds, cam, st, self.live, self.feat_fbs[0], self.done, n, sync=False, features_sq=self.feat_fbs[1])
        self.ctx.synchronize()
        self.done, self.passes = self.done + n, self.passes + 1
        self.n_half[half] += n

    def whole_frame(self, live):
        """The rects and the two halves' counts of the whole frame: the finished tiles at the counts they finished with, `live` ones at n_A and n_B."""
        return self.done_rects + live, self.done_a + [self.n_half[0]] * len(live), self.done_b + [self.n_half[1]] * len(live)

    def filter_whole_frame(self, live, out_fb, err_img, atrous, **where):
        """The dual filter over whole_frame(live) into `out_fb` (and `err_img`): rmd_denoise_atrous_dual with `atrous`, else rmd_denoise_dual; guided when
        the loop keeps the feature buffers.  `where`: region=..., or nothing for the whole-frame call."""
        st = self.st
        rects, all_a, all_b = self.whole_frame(live)
        guide = _guide(st, self.feat_fbs, [a + b for a, b in zip(all_a, all_b)], atrous)
        halves = self.filter_halves(rects, all_a, all_b)
        if atrous:
            denoise_atrous_dual(self.ctx, *halves, rects, all_a, all_b, out_fb, err_img, **st.atrous_keywords(), **guide, **where)
        else:
            denoise_dual(self.ctx, *halves, rects, all_a, all_b, out_fb, err_img, **where, **st.nlm_keywords(), **guide)

    def filter_halves(self, rects, all_a, all_b):
        """The two halves a dual filter call of this pass reads: the loop's own, or with despike_dual the despiked halves of the whole frame at its counts,
        made once a pass by one rmd_despike_dual call (a later call of the same pass has the same tiles at the same counts)."""
        if self.spare is None:
            return (self.fbs[0], self.fbs[1]), (self.fbs[2], self.fbs[3])
        out = (self.spare[0], self.spare[1]), (self.spare[2], self.spare[3])
        if self.despiked_at != self.passes:
            despike_dual(self.ctx, (self.fbs[0], self.fbs[1]), (self.fbs[2], self.fbs[3]), rects, all_a, all_b, out=out, want_replaced=False, **self.st.despike_keywords())
            self.despiked_at = self.passes
        return out

    def check_weights(self):
        """adaptive_display_auto_exposure: before a check, one histogram of the whole frame on the RAW sums — S_A with S_B as the second buffer, live tiles at
        n_A + n_B, finished ones at the counts they finished with: what a raw preview of this moment resolves; the region forms leave the filtered
        frame's finished tiles unwritten — and the weights are the tone curve's at the exposure it asks for."""
        st = self.st
        rects, all_a, all_b = self.whole_frame(self.live)
        hist = luminance_histogram(self.ctx, self.fbs[0], rects, [a + b for a, b in zip(all_a, all_b)], self.fbs[2])
        exposure = exposure_from_histogram(hist, st.auto_exposure_percentile, st.auto_exposure_target)
        self.weights = display_weights(exposure, st.adaptive_display_gamma, st.adaptive_display_floor)

    def adaptive_check(self):
        """rmd_tile_error_dual of the live tiles after the settings' filter — with adaptive_denoised_display_threshold one rmd_tile_weighted_error_dual call's
        rms on the filtered frame and the error image instead —, or None each when no check is due."""
        st = self.st
        if not (self.adaptive and self.passes % 2 == 0 and self.done >= st.adaptive_min_samples):
            return [None] * len(self.live)
        if st.denoise_dual_atrous:  # the whole frame; (region off: exactly the call made before the region form existed)
            self.filter_whole_frame(self.live, self.out_fb, self.err_img, True, **(dict(region=self.live) if st.denoise_dual_atrous_region else {}))
        else:  # only the live tiles' filtered pixels are read below: the region form writes those, with the whole-frame call's bytes
            self.filter_whole_frame(self.live, self.out_fb, self.err_img, False, region=self.live)
        if self.display:
            if st.adaptive_display_auto_exposure:
                self.check_weights()
            return tile_weighted_error_dual(self.ctx, self.out_fb, self.err_img, self.live, self.weights)["rms"]
        return tile_error_dual(self.ctx, self.err_img, self.live)

    def finish(self, rects, errors=None):
        """TileFinished for `rects`: both halves' sums and sums of squares, the tiles' pixels only."""
        if not rects:
            return
        n_a, n_b = self.n_half
        packed = [fb.download_tiles(rects) for fb in self.fbs]
        for i, rect in enumerate(rects):
            l, t, w, h = rect
            a, a_sq, b, b_sq = (p[i].copy() for p in packed)
            tile = Tile(l, t, w, h, n_a + n_b, a + b, None if errors is None else errors[i], a_sq + b_sq)
            tile.data_a, tile.data_sq_a, tile.count_a, tile.data_b, tile.data_sq_b, tile.count_b = a, a_sq, n_a, b, b_sq, n_b
            self.finished.append(Message.TileFinished(tile))
            self.done_rects.append(rect), self.done_a.append(n_a), self.done_b.append(n_b)

    def snapshots(self, still, errors):
        """TileProgressed for the tiles that go on: the two halves' sums added."""
        pa, pb = self.fbs[0].download_tiles(still), self.fbs[2].download_tiles(still)
        for (l, t, w, h), e, a, b in zip(still, errors, pa, pb):
            self.messages.append(Message.TileProgressed(Tile(l, t, w, h, self.done, a + b, None if e is None else float(e))))

    def preview(self, still):
        """The whole frame: finished tiles at the counts they finished with, live ones at n_A + n_B, the two halves' sums added on the device; with
        preview_denoise, rmd_denoise_atrous_dual's means of it at count 1."""
        rects, all_a, all_b = self.whole_frame(still)
        if self.preview_fb is None:
            call = (self.ctx, self.fbs[0], rects, [a + b for a, b in zip(all_a, all_b)], self.fbs[2])
        else:
            self.filter_whole_frame(still, self.preview_fb, None, True)
            call = (self.ctx, self.preview_fb, rects, [1] * len(rects), None)  # (means)
        self.messages.append(_preview(self.st, self.W, self.H, self.passes, self.done, [call]))

    def run(self):
        st = self.st
        while self.done < st.sample_count and self.live:
            self.render_pass(min(st.samples_per_iteration, st.sample_count - self.done))
            if self.done < st.sample_count:
                errors = self.adaptive_check()
                conv = [e is not None and e <= self.threshold for e in errors]
                self.finish([r for r, c in zip(self.live, conv) if c], [float(e) for e, c in zip(errors, conv) if c])  # converged: finished at the samples they have
                still = [r for r, c in zip(self.live, conv) if not c]
                if still and st.progress_tiles:
                    self.snapshots(still, [e for e, c in zip(errors, conv) if not c])
                if still and st.preview_every and self.passes % st.preview_every == 0:
                    self.preview(still)
                self.live = still
        self.finish(self.live)
        return self.messages + self.finished  # progress snapshots first, then the finished tiles


def _render_tiled_dual(scene, settings, devices):
    """render_tiled with settings.denoise_dual: one device, four framebuffers.  Pass j (counted from 0; every live tile takes every pass) adds its
    samples to half A when j is even and to half B when j is odd, so after an even NUMBER of full passes both halves hold the same count.  Every
    TileFinished tile carries both halves; await_() returns rmd_denoise_dual's frame.

    With settings.adaptive_denoised_threshold > 0: after every even number of passes that leaves live tiles below sample_count with at least
    adaptive_min_samples samples, rmd_denoise_dual_region filters the live tiles' pixels of the whole frame (finished tiles at the counts they
    finished with: the bytes rmd_denoise_dual would give those pixels), rmd_tile_error_dual runs over the live tiles, and a live tile at or below the
    threshold is sent as TileFinished, with that error, and takes no further passes.

    With settings.adaptive_denoised_display_threshold > 0 (instead of adaptive_denoised_threshold) the same filter call is followed by one
    rmd_tile_weighted_error_dual call over the live tiles on the filtered frame and the error image, under rmd_display_weights' table at
    adaptive_display_exposure, gamma and floor — the filtered tile's RMS error after exposure and gamma, in fractions of the display's full scale —, and its
    rms is what meets the threshold and what the tile carries.  With adaptive_display_auto_exposure every check first histograms the whole frame's RAW sums
    (S_A with S_B as the second buffer, at the counts a raw preview would resolve) and makes the weights at the exposure that histogram asks for.

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
    settings.preview_auto_exposure the exposure comes from rmd_luminance_histogram_tiles on what that resolve call takes, as in render_tiled.

    With settings.despike_dual every call of the dual filter this loop makes — the adaptive check, the filtered preview — reads despiked copies of the
    halves: four spare buffers, filled once per pass by one rmd_despike_dual call over the whole frame (finished tiles at the counts they finished with,
    live ones at n_A / n_B); the region forms then filter the live tiles of those copies.  The sums the passes add to, the TileFinished / TileProgressed
    data, raw previews and the auto-exposure histogram stay the raw sums; await_() despikes the assembled halves itself."""
    if len(devices) != 1:
        raise ValueError("denoise_dual renders on one device: the filter's window crosses the tiles that several devices would own")
    with contextlib.ExitStack() as stack:
        messages = _DualLoop(stack, scene, settings, devices[0]).run()
    return TaskHandle(settings, messages, devices[0], scene if settings.denoise_dual_features or settings.denoise_dual_select else None)
