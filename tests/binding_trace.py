"""A recording stand-in for libraymond_hip.so, and the scenarios whose C calls tests/golden/binding_trace.json pins.

FakeLibrary builds, for every name in lib.SIGNATURES, a ctypes.CFUNCTYPE(restype, *argtypes) around a Python recorder, so ctypes converts the arguments
of raymond_amd/render.py exactly as it would for the real library; no .so and no GPU is needed.  A call is recorded as one line, `name(arg, ...)`:
scalars as they arrive; what a pointer points to and never its address — rect, count, candidate and slope arrays as lists, the camera and settings
structs as their fields —; device objects as the label their fake constructor handed out (ctx0, scene0, fb3, feat1).  Host outputs are filled
deterministically: downloads with ones, rmd_tile_error[_dual] from `tile_errors`, rmd_despike[_dual]'s counts with 1, 2, ..., histograms with one bin, and
rmd_exposure_from_histogram with a value that differs from call to call, so that a trace shows which exposure reaches which resolve call.

The three tile measures (rmd_tile_luma_error, rmd_tile_weighted_error[_dual]) fill their per-rect structs from `tile_errors` as well, each deciding
field at its own offset from the hook's value e — tile_rms = e + 1/8, pixel_rms = e + 1/4; rms = e + 1/8, mean_weighted_variance = e + 3/8 —, so that both
stay on e's side of the scenarios' threshold of 0.5 and a message's Tile.error shows which field the loop read; `valid` is the rect's pixel count, every
other field 0.  rmd_display_weights fills all abi.LUMA_WEIGHTS entries with 1024 * exposure + gamma + display_floor.  A weight table, going out or coming
in, is recorded as `weights(<entry>)` when all its entries are equal (`weights(<first>..<last>)` otherwise), so that a trace shows which exposure's table
reached which measure call.

`with installed() as fake:` makes raymond_amd.lib.load() return the fake for the duration.  SCENARIOS maps a name to a function of the fake that drives
render.py and returns further lines (messages, results); run(name) gives a scenario's whole trace.  tools/record_binding_trace.py writes the golden
file, tests/test_binding_trace.py replays it.
"""
import contextlib
import ctypes as C

import numpy as np

from raymond_amd import abi, lib, render, scenes
from raymond_amd.scene import Settings, generate_tiles, tile_array

_SCALARS = (C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_size_t, C.c_double, C.c_float)
_HANDLES = {"rmd_context_create": "ctx", "rmd_context_create_on_stream": "ctx", "rmd_scene_create": "scene", "rmd_framebuffer_alloc": "fb",
            "rmd_feature_buffer_alloc": "feat"}
_RELEASES = ("rmd_context_destroy", "rmd_scene_destroy", "rmd_framebuffer_free")


def _fields(s):
    return [list(v) if isinstance(v, C.Array) else v for v in (getattr(s, n) for n, _ in s._fields_)]


def _show(v):
    """A recorded value as text: lists nested in brackets, labels bare, a NULL pointer as 0."""
    return "[%s]" % ",".join(_show(x) for x in v) if isinstance(v, list) else "0" if v is None else str(v)


def _rect_pixels(ptr, n):
    return sum(ptr[i].width * ptr[i].height for i in range(n))


def _weights_token(ptr):
    table = [ptr[i] for i in range(abi.LUMA_WEIGHTS)]
    return "weights(%r)" % table[0] if all(v == table[0] for v in table) else "weights(%r..%r)" % (table[0], table[-1])


_TABLES = {"rmd_tile_weighted_error": 8, "rmd_tile_weighted_error_dual": 7, "rmd_display_weights": 3}  # entry point: the argument that is a weight table
_MEASURES = {"rmd_tile_luma_error": (("tile_rms", 0.125), ("pixel_rms", 0.25)), "rmd_tile_weighted_error": (("rms", 0.125), ("mean_weighted_variance", 0.375)),
             "rmd_tile_weighted_error_dual": (("rms", 0.125), ("mean_weighted_variance", 0.375))}  # entry point: its deciding fields, and what each adds to tile_errors


def _fill(kind, address, n, value):
    if address and n:
        np.ctypeslib.as_array((kind * n).from_address(address))[:] = value


class FakeLibrary:
    def __init__(self):
        self.fail = ()  # entry points whose names start with one of these return RMD_ERR_INVALID_ARGUMENT (after being recorded)
        self.tile_errors = lambda rect, check: 1.0  # rmd_tile_error[_dual] and the tile measures: the error of tile `rect` at the check-th call of that entry point
        self.reset()
        for name, (res, args) in lib.SIGNATURES.items():
            if res is C.c_char_p:  # (not a callback's result type)
                setattr(self, name, lambda handle: b"the stand-in was told to fail")
            else:
                setattr(self, name, C.CFUNCTYPE(res, *args)(self._recorder(name, res, args)))

    def reset(self):
        self.lines, self.labels, self.live, self.made, self.calls = [], {}, [], {}, {}

    def rmd_abi_version(self):
        return abi.RMD_ABI_VERSION

    def _label(self, address):
        return None if address is None else self.labels.get(address, "host")

    def _new(self, prefix):
        k = self.made.get(prefix, 0)
        self.made[prefix] = k + 1
        address = 0x1000 * (len(self.labels) + 1)
        self.labels[address] = "%s%d" % (prefix, k)
        self.live.append(self.labels[address])
        return address

    def _recorder(self, name, res, argtypes):
        def count_after(i):  # the arrays' length: the first uint32 that follows them
            return next(j for j in range(i + 1, len(argtypes)) if argtypes[j] is C.c_uint32)

        def record(*args):
            shown = []
            for i, (t, a) in enumerate(zip(argtypes, args)):
                if t is C.c_void_p:
                    shown.append(self._label(a))
                elif t in _SCALARS:
                    shown.append(a)
                elif not a:
                    shown.append(None)
                elif t._type_ in (abi.Camera, abi.Settings):
                    shown.append(_fields(a[0]))
                elif t._type_ in (abi.TileRect, abi.DenoiseCandidate):
                    shown.append([_fields(a[j]) for j in range(args[count_after(i)])])
                elif t._type_ in (C.c_uint32, C.c_double) and any(argtypes[j] is C.c_uint32 for j in range(i + 1, len(argtypes))):
                    shown.append(list(a[: args[count_after(i)]]))
                elif _TABLES.get(name) == i:
                    shown.append(None)  # (read below, once the stand-in has written what it writes)
                elif t._type_ is abi.LumaHistogram and name == "rmd_exposure_from_histogram":
                    shown.append("hist(pixels=%d)" % a[0].pixels)
                else:
                    shown.append("out")
            check = self.calls.get(name, 0)
            self.calls[name] = check + 1
            failed = any(name.startswith(f) for f in self.fail)
            if not failed:
                self._act(name, args, check)
            if name in _TABLES and args[_TABLES[name]]:
                shown[_TABLES[name]] = _weights_token(args[_TABLES[name]])
            if name in _RELEASES:
                self.live.remove(shown[-1])
            self.lines.append("%s(%s)%s" % (name, _show(shown)[1:-1], " -> 1" if failed else ""))
            return None if res is None else abi.RMD_ERR_INVALID_ARGUMENT if failed else abi.RMD_OK

        return record

    def _act(self, name, a, check):
        """What the stand-in writes: handles, and every host output render.py goes on to read."""
        if name in _HANDLES:
            a[-1][0] = self._new(_HANDLES[name])
        elif name == "rmd_framebuffer_download":
            _fill(C.c_double, a[2], a[3], 1.0)
        elif name == "rmd_framebuffer_download_tiles":
            _fill(C.c_double, a[6], 3 * _rect_pixels(a[4], a[5]), 1.0)
        elif name in ("rmd_tile_error", "rmd_tile_error_dual"):
            rects, n, out = a[-3], a[-2], a[-1]
            _fill(C.c_double, out, n, [self.tile_errors(tuple(_fields(rects[i])), check) for i in range(n)])
        elif name in _MEASURES:
            rects, n, out = a[5], a[6 if name.endswith("_dual") else 7], a[-1]
            for i in range(n):
                e = self.tile_errors(tuple(_fields(rects[i])), check)
                for field, offset in _MEASURES[name]:
                    setattr(out[i], field, e + offset)
                out[i].valid = rects[i].width * rects[i].height
        elif name == "rmd_display_weights":
            _fill(C.c_double, C.addressof(a[3].contents), abi.LUMA_WEIGHTS, 1024.0 * a[0] + a[1] + a[2])
        elif name in ("rmd_despike", "rmd_despike_dual") and a[-1]:
            for i in range(a[7 if name == "rmd_despike" else 10]):
                a[-1][i] = i + 1
        elif name == "rmd_resolve_tonemap":
            _fill(C.c_uint8, a[7], 3 * a[2] * a[3], 128)
        elif name == "rmd_resolve_tonemap_tiles":
            _fill(C.c_uint8, a[10], 3 * _rect_pixels(a[5], a[7]), 128)
        elif name == "rmd_luminance_histogram_tiles":
            a[8][0].pixels = a[8][0].bins[128] = _rect_pixels(a[5], a[7])
        elif name == "rmd_exposure_from_histogram":
            a[3][0] = 1.0 + 0.125 * (check + 1)


_FAKE = None


@contextlib.contextmanager
def installed():
    """raymond_amd.lib.load() returns one (reset) FakeLibrary inside the block, and what it returned before after it."""
    global _FAKE
    if _FAKE is None:
        _FAKE = FakeLibrary()
    _FAKE.reset()
    _FAKE.fail, _FAKE.tile_errors = (), (lambda rect, check: 1.0)
    before, lib._lib = lib._lib, _FAKE
    try:
        yield _FAKE
    finally:
        lib._lib = before


# ---------------------------------------------------------------- the scenarios
W, H = 8, 6
TILE = (4, 3)
RECTS = generate_tiles(W, H, TILE)  # four tiles
COUNTS = [2, 2, 3, 3]
COUNTS_B = [1, 2, 3, 4]
COUNTS_F = [3, 4, 6, 7]
REGIONS = (None, [], [RECTS[1], RECTS[3]])
SLOPES = (None, 0, 3.0)
SCENARIOS = {}


def scenario(name):
    def add(fn):
        assert name not in SCENARIOS, name
        SCENARIOS[name] = fn
        return fn

    return add


def _raises(lines, fn, *args, **kwargs):
    """Calls fn; what it raised becomes a line (the library's calls up to there are in the trace already)."""
    try:
        fn(*args, **kwargs)
        lines.append("no exception")
    except Exception as e:  # noqa: BLE001
        lines.append("raised %s: %s" % (type(e).__name__, e))
    return lines


class Bench:
    """One context and the device buffers a wrapper scenario hands to render.py; closed by the scenario's end."""

    def __init__(self):
        self.ctx = render.Context(0)
        self.fbs = [render.Framebuffer(self.ctx, W, H) for _ in range(6)]
        self.feats = [render.FeatureBuffer(self.ctx, W, H) for _ in range(2)]
        self.err, self.sure = render.ErrorImage(self.ctx, W, H), render.ErrorImage(self.ctx, W, H)
        self.win = render.WinnerImage(self.ctx, W, H)
        self.half_a, self.half_b = (self.fbs[0], self.fbs[1]), (self.fbs[2], self.fbs[3])

    def close(self):
        for o in [self.win, self.sure, self.err] + self.feats[::-1] + self.fbs[::-1] + [self.ctx]:
            o.close()


def wrapper_scenario(name):
    """A scenario `fn(bench, lines)` over a Bench."""

    def add(fn):
        def run_it(fake):
            b, lines = Bench(), []
            try:
                fn(b, lines)
            finally:
                b.close()
            return lines

        return scenario(name)(run_it)

    return add


@wrapper_scenario("buffers")
def _(b, lines):
    fb = b.fbs[0]
    fb.zero()
    fb.upload(np.zeros((H, W, 3)))
    lines.append("download %r %s" % (fb.download().shape, fb.download().dtype))
    views = fb.download_tiles(RECTS[:3])
    lines.append("download_tiles %r" % [v.shape for v in views])
    fb.upload_tiles(RECTS[:2], [np.zeros((3, 4, 3))] * 2)
    for o, arr in ((b.feats[0], np.zeros((H, W, 7))), (b.err, np.zeros((H, W))), (b.win, np.zeros((H, W), dtype=np.uint32))):
        o.zero()
        o.upload(arr)
        got = o.download()
        lines.append("%s download %r %s" % (type(o).__name__, got.shape, got.dtype))
        _raises(lines, o.download_tiles, RECTS)
        _raises(lines, o.upload_tiles, RECTS, [])
    wrapped = render.Framebuffer(b.ctx, W, H, device_ptr=0x77)
    wrapped.zero()
    wrapped.close()  # (not owned: no free)
    ds = render.DeviceScene(b.ctx, scenes.reflective_spheres())
    ds.close()
    ds.close()  # (a second close is no call)


def _settings(**kw):
    kw.setdefault("sample_count", 2)
    kw.setdefault("samples_per_iteration", 1)
    return Settings(scenes.camera(W, H), tile_size=TILE, bounce_limit=3, seed=scenes.SEED, **kw)


@wrapper_scenario("render_tiles")
def _(b, lines):
    st = _settings()
    cam = st.camera_settings
    ds = render.DeviceScene(b.ctx, scenes.reflective_spheres())
    try:
        render.render_tiles(b.ctx, ds, cam, st, RECTS, b.fbs[0])
        render.render_tiles(b.ctx, ds, cam, st, RECTS[:2], b.fbs[0], 3, 5, sync=False)
        render.render_tiles(b.ctx, ds, cam, st, (tile_array(RECTS[1:]), 3), b.fbs[0], 1, 1, framebuffer_sq=b.fbs[1])
        render.render_tiles(b.ctx, ds, cam, st, [], b.fbs[0], sync=False, framebuffer_sq=b.fbs[1])
        render.render_features(b.ctx, ds, cam, st, RECTS, b.feats[0])
        render.render_features(b.ctx, ds, cam, st, (tile_array(RECTS[:1]), 1), b.feats[0], 2, 4, sync=False, features_sq=b.feats[1])
        render.render_features(b.ctx, ds, cam, st, [], b.feats[0], features_sq=b.feats[1])
    finally:
        ds.close()


@wrapper_scenario("tile_error")
def _(b, lines):
    lines.append(repr(render.tile_error(b.ctx, b.fbs[0], b.fbs[1], 5, 1e-3, RECTS).tolist()))
    lines.append(repr(render.tile_error(b.ctx, b.fbs[0], b.fbs[1], 5, 1e-3, []).tolist()))
    lines.append(repr(render.tile_error_dual(b.ctx, b.err, RECTS[1:]).tolist()))
    lines.append(repr(render.tile_error_dual(b.ctx, b.err, []).tolist()))


@wrapper_scenario("despike")
def _(b, lines):
    s, q, n = render.despike(b.ctx, b.fbs[0], b.fbs[1], RECTS, COUNTS)
    lines.append("new buffers %s, replaced %r" % (s is not b.fbs[0] and q is not b.fbs[1], n.tolist()))
    s.close(), q.close()
    s, q, n = render.despike(b.ctx, b.fbs[0], b.fbs[1], iter(RECTS[:2]), COUNTS[:2], 3, 1, 5.0, 1.5, 0.25, out=(b.fbs[2], b.fbs[3]), want_replaced=False)
    lines.append("out given back %s, replaced %r" % (s is b.fbs[2] and q is b.fbs[3], n))
    s, q, n = render.despike(b.ctx, b.fbs[0], b.fbs[1], [], [], out=(b.fbs[2], b.fbs[3]))
    lines.append("zero rects: replaced %r" % n.tolist())
    _raises(lines, render.despike, b.ctx, b.fbs[0], b.fbs[1], RECTS, COUNTS[:3])
    lib.load().fail = ("rmd_despike",)
    _raises(lines, render.despike, b.ctx, b.fbs[0], b.fbs[1], RECTS, COUNTS)  # its two new buffers are freed


@wrapper_scenario("denoise")
def _(b, lines):
    render.denoise(b.ctx, b.fbs[0], b.fbs[1], RECTS, COUNTS, b.fbs[4])
    render.denoise(b.ctx, b.fbs[0], b.fbs[1], RECTS[:2], np.array(COUNTS[:2]), b.fbs[4], 4, 2, 0.5, 0.75)
    render.denoise(b.ctx, b.fbs[0], b.fbs[1], [], [], b.fbs[4])
    _raises(lines, render.denoise, b.ctx, b.fbs[0], b.fbs[1], RECTS, COUNTS[:1], b.fbs[4])


@wrapper_scenario("denoise_guided")
def _(b, lines):
    for f, f_sq in ((None, None), b.feats):
        for slope in SLOPES:
            render.denoise_guided(b.ctx, b.fbs[0], b.fbs[1], f, f_sq, RECTS, COUNTS, b.fbs[4], 4, 2, 0.5, 0.75, 1.5, 0.02, slope)
    render.denoise_guided(b.ctx, b.fbs[0], b.fbs[1], b.feats[0], None, RECTS, COUNTS, b.fbs[4], slope=1)  # (the sums alone)
    render.denoise_guided(b.ctx, b.fbs[0], b.fbs[1], b.feats[0], b.feats[1], [], [], b.fbs[4])
    _raises(lines, render.denoise_guided, b.ctx, b.fbs[0], b.fbs[1], None, None, RECTS, [], b.fbs[4])


@wrapper_scenario("denoise_atrous")
def _(b, lines):
    for f, f_sq in ((None, None), b.feats):
        for slope in SLOPES:
            render.denoise_atrous(b.ctx, b.fbs[0], b.fbs[1], RECTS, COUNTS, b.fbs[4], 3, 2.5, 0.75, f, f_sq, 1.5, 0.02, slope)
    render.denoise_atrous(b.ctx, b.fbs[0], b.fbs[1], RECTS, COUNTS, b.fbs[4], features=b.feats[0])  # (the sums alone)
    render.denoise_atrous(b.ctx, b.fbs[0], b.fbs[1], [], [], b.fbs[4])
    _raises(lines, render.denoise_atrous, b.ctx, b.fbs[0], b.fbs[1], RECTS, COUNTS + [1], b.fbs[4])


def _dual_matrix(b, lines, fn, **params):
    for f, f_sq in ((None, None), b.feats):
        for region in REGIONS:
            for slope in SLOPES:
                fn(b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B, b.fbs[4], b.err, region=region, features=f, features_sq=f_sq,
                   counts_f=None if f is None else COUNTS_F, k_f=1.5, tau=0.02, slope=slope, **params)
    fn(b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B, b.fbs[4], b.err, features=b.feats[0], counts_f=COUNTS_F, slope=1)  # (the sums alone)
    fn(b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B, b.fbs[4])  # every default; no error image
    fn(b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B, b.fbs[4], None, region=iter(RECTS[:1]), features=b.feats[0], features_sq=b.feats[1], counts_f=COUNTS_F)
    fn(b.ctx, b.half_a, b.half_b, [], [], [], b.fbs[4], b.err)
    fn(b.ctx, b.half_a, b.half_b, [], [], [], b.fbs[4], b.err, features=b.feats[0], features_sq=b.feats[1], region=[])
    fn(b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B, b.fbs[4], b.err, counts_f=[1], slope=2.0)  # no features: counts_f and slope are not read
    _raises(lines, fn, b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B[:2], b.fbs[4])
    _raises(lines, fn, b.ctx, b.half_a, b.half_b, RECTS, COUNTS[:2], COUNTS_B, b.fbs[4])
    _raises(lines, fn, b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B, b.fbs[4], features=b.feats[0], features_sq=b.feats[1])
    _raises(lines, fn, b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B, b.fbs[4], features_sq=b.feats[1], counts_f=COUNTS_F[:3])


@wrapper_scenario("denoise_dual")
def _(b, lines):
    _dual_matrix(b, lines, render.denoise_dual, radius=4, patch_radius=2, k=0.5, alpha=0.75)


@wrapper_scenario("denoise_atrous_dual")
def _(b, lines):
    _dual_matrix(b, lines, render.denoise_atrous_dual, levels=3, k=2.5, alpha=0.75)


CANDIDATES = [dict(k=0.45), dict(k=1.0, alpha=0.5, guided=True, k_f=1.5, tau=0.02)]


@wrapper_scenario("denoise_dual_select")
def _(b, lines):
    sel = render.denoise_dual_select
    sloped = [CANDIDATES[0], dict(CANDIDATES[1], slope=3.0)]
    for cands in (CANDIDATES, sloped, CANDIDATES[:1], [dict(k=0.3, slope=0, reserved=0)], iter(sloped)):
        sel(b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B, cands, b.fbs[4], b.err, b.sure, b.win, 4, 2, 1, 3, b.feats[0], b.feats[1], COUNTS_F)
    sel(b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B, CANDIDATES[:1], b.fbs[4])  # every default: no image, no features
    sel(b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B, sloped, b.fbs[4], sure_image=b.sure, features=b.feats[0], counts_f=COUNTS_F)
    sel(b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B, CANDIDATES, b.fbs[4], winner_image=b.win, features_sq=b.feats[1])
    sel(b.ctx, b.half_a, b.half_b, [], [], [], [], b.fbs[4], b.err, counts_f=[])
    _raises(lines, sel, b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B[:1], CANDIDATES, b.fbs[4])
    _raises(lines, sel, b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B, CANDIDATES, b.fbs[4], counts_f=COUNTS_F[:2])


@wrapper_scenario("resolve")
def _(b, lines):
    lines.append("resolve_tonemap %r" % (render.resolve_tonemap(b.ctx, b.fbs[0], 5).shape,))
    lines.append("resolve_tonemap %r" % (render.resolve_tonemap(b.ctx, b.fbs[0], 5, 2.0, 1.8).dtype,))
    for second in (None, b.fbs[2]):
        views = render.resolve_tonemap_tiles(b.ctx, b.fbs[0], iter(RECTS[1:]), COUNTS[1:], 2.0, 1.8, second=second)
        lines.append("resolve_tonemap_tiles %r" % [v.shape for v in views])
        h = render.luminance_histogram(b.ctx, b.fbs[0], iter(RECTS[1:]), COUNTS[1:], second=second)
        lines.append("luminance_histogram pixels %d" % h.pixels)
        lines.append("exposure %r" % render.exposure_from_histogram(h, 0.9, 0.5))
    lines.append("resolve_tonemap_tiles %r" % render.resolve_tonemap_tiles(b.ctx, b.fbs[0], [], []))
    lines.append("luminance_histogram pixels %d" % render.luminance_histogram(b.ctx, b.fbs[0], [], []).pixels)
    lines.append("exposure %r" % render.exposure_from_histogram(render.LumaHistogram()))
    _raises(lines, render.resolve_tonemap_tiles, b.ctx, b.fbs[0], RECTS, COUNTS[:3])
    _raises(lines, render.luminance_histogram, b.ctx, b.fbs[0], RECTS, COUNTS[:3])


TABLE = np.full(abi.LUMA_WEIGHTS, 3.0)  # a weight table no rmd_display_weights call of the stand-in makes


@wrapper_scenario("tile_measures")
def _(b, lines):
    measures = (("tile_luma_error", lambda tiles, counts, table: render.tile_luma_error(b.ctx, b.fbs[0], b.fbs[1], tiles, counts, 1e-3)),
                ("tile_weighted_error", lambda tiles, counts, table: render.tile_weighted_error(b.ctx, b.fbs[0], b.fbs[1], tiles, counts, table)),
                ("tile_weighted_error_dual", lambda tiles, counts, table: render.tile_weighted_error_dual(b.ctx, b.fbs[4], b.err, tiles, table)))
    lib.load().tile_errors = first_converges
    for name, measure in measures:
        for tiles, counts in ((RECTS, COUNTS), (iter(RECTS[:2]), COUNTS[:2]), ([], []), (RECTS, np.array(COUNTS))):
            lines.append("%s %r" % (name, measure(tiles, counts, TABLE).tolist()))
        if name != "tile_luma_error":  # (which takes no table)
            _raises(lines, measure, RECTS, COUNTS, TABLE[:-1])
        if name != "tile_weighted_error_dual":  # (which takes no counts)
            _raises(lines, measure, RECTS, COUNTS[:3], TABLE)
    lib.load().fail = ("rmd_tile_",)
    for name, measure in measures:
        _raises(lines, measure, RECTS, COUNTS, TABLE)


@wrapper_scenario("display_weights")
def _(b, lines):
    for args in ((), (2.0, 1.8, 0.0625)):
        table = render.display_weights(*args)
        lines.append("display_weights %r %s of %r" % (table.shape, table.dtype, sorted(set(table.tolist()))))
        render.tile_weighted_error(b.ctx, b.fbs[0], b.fbs[1], RECTS, COUNTS, table)  # the table handed on is that call's
        render.tile_weighted_error_dual(b.ctx, b.fbs[4], b.err, RECTS, table)
    lib.load().fail = ("rmd_display",)
    _raises(lines, render.display_weights)


@wrapper_scenario("despike_dual")
def _(b, lines):
    a, bb, n = render.despike_dual(b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B)
    lines.append("new buffers %s, replaced %r" % (len({id(fb) for fb in a + bb + b.half_a + b.half_b}) == 8, n.tolist()))
    for fb in a + bb:
        fb.close()
    outs = ((b.fbs[4], b.fbs[5]), (b.feats[0], b.feats[1]))  # (the stand-in asks no kind of a buffer: four labels that differ)
    a, bb, n = render.despike_dual(b.ctx, b.half_a, b.half_b, iter(RECTS[:2]), COUNTS[:2], COUNTS_B[:2], 3, 1, 5.0, 1.5, 0.25, out=outs, want_replaced=False)
    lines.append("out given back %s, replaced %r" % ((a, bb) == outs, n))
    a, bb, n = render.despike_dual(b.ctx, b.half_a, b.half_b, [], [], [], out=outs)
    lines.append("zero rects: replaced %r" % n.tolist())
    _raises(lines, render.despike_dual, b.ctx, b.half_a, b.half_b, RECTS, COUNTS[:3], COUNTS_B)
    _raises(lines, render.despike_dual, b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B[:3])
    lib.load().fail = ("rmd_despike_dual",)
    _raises(lines, render.despike_dual, b.ctx, b.half_a, b.half_b, RECTS, COUNTS, COUNTS_B)  # its four new buffers are freed


# ---- the *_arrays helpers: the order of alloc, upload, call, download and free; with the filter call failing, the frees still happen
def _shapes(res):
    if isinstance(res, dict):
        return {k: _shapes(v) for k, v in res.items()}
    if isinstance(res, tuple):
        return [_shapes(v) for v in res]
    return None if res is None else "%s %s" % (res.shape, res.dtype)


def arrays_scenario(name, fn, cases):
    """One scenario per case of a helper, and one more in which the first case's filter call fails."""
    for case, (args, kwargs) in cases.items():
        def run_it(fake, args=args, kwargs=kwargs, failing=False):
            lines = []
            with render.Context(0) as ctx:
                if failing:
                    fake.fail = ("rmd_denoise", "rmd_despike", "rmd_tile_")
                    _raises(lines, fn, ctx, *args, **kwargs)
                else:
                    lines.append("-> %r" % (_shapes(fn(ctx, *args, **kwargs)),))
            return lines

        scenario("%s/%s" % (name, case))(run_it)
    args, kwargs = next(iter(cases.values()))
    scenario("%s/failing" % name)(lambda fake: run_it(fake, args, kwargs, True))


S3, S7, S1 = np.zeros((H, W, 3)), np.zeros((H, W, 7)), np.zeros((H, W))
HALVES = (S3, S3, S3, S3)
arrays_scenario("despike_arrays", render.despike_arrays, {
    "plain": ((S3, S3, RECTS, COUNTS), {}),
    "params": ((S3, S3, RECTS[:2], COUNTS[:2]), dict(radius=1, rank=0, k=5.0, ratio=1.5, floor=0.5, want_replaced=False))})
arrays_scenario("despike_dual_arrays", render.despike_dual_arrays, {
    "plain": ((*HALVES, RECTS, COUNTS, COUNTS_B), {}),
    "params": ((*HALVES, RECTS[:2], COUNTS[:2], COUNTS_B[:2]), dict(radius=1, rank=0, k=5.0, ratio=1.5, floor=0.5, want_replaced=False))})
arrays_scenario("tile_luma_error_arrays", render.tile_luma_error_arrays, {
    "plain": ((S3, S3, RECTS, COUNTS, 1e-3), {}),
    "some": ((S3, S3, iter(RECTS[1:3]), np.array(COUNTS[1:3]), 0.5), {})})
arrays_scenario("tile_weighted_error_arrays", render.tile_weighted_error_arrays, {
    "plain": ((S3, S3, RECTS, COUNTS, TABLE), {}),
    "some": ((S3, S3, iter(RECTS[1:3]), np.array(COUNTS[1:3]), TABLE.tolist()), {})})
arrays_scenario("denoise_arrays", render.denoise_arrays, {
    "plain": ((S3, S3, RECTS, COUNTS), {}),
    "params": ((S3, S3, RECTS, COUNTS), dict(radius=4, patch_radius=2, k=0.5, alpha=0.75))})
arrays_scenario("denoise_guided_arrays", render.denoise_guided_arrays, {
    "features": ((S3, S3, S7, S7, RECTS, COUNTS), dict(k_f=1.5, tau=0.02, slope=3.0, radius=4)),
    "no_features": ((S3, S3, None, None, RECTS, COUNTS), {})})
arrays_scenario("denoise_atrous_arrays", render.denoise_atrous_arrays, {
    "features": ((S3, S3, S7, S7, RECTS, COUNTS), dict(levels=3, k=2.5, k_f=1.5, tau=0.02, slope=3.0)),
    "no_features": ((S3, S3, None, None, RECTS, COUNTS), {})})
arrays_scenario("denoise_dual_arrays", render.denoise_dual_arrays, {
    "features_region": ((*HALVES, RECTS, COUNTS, COUNTS_B), dict(region=RECTS[:2], out_init=S3, err_init=S1, features=S7, features_sq=S7, counts_f=COUNTS_F,
                                                                 k_f=1.5, tau=0.02, slope=3.0)),
    "plain": ((*HALVES, RECTS, COUNTS, COUNTS_B), {}),
    "region_positional": ((*HALVES, RECTS, COUNTS, COUNTS_B, []), dict(radius=4))})
arrays_scenario("denoise_atrous_dual_arrays", render.denoise_atrous_dual_arrays, {
    "features_region": ((*HALVES, RECTS, COUNTS, COUNTS_B), dict(region=RECTS[:2], out_init=S3, err_init=S1, features=S7, features_sq=S7, counts_f=COUNTS_F,
                                                                 k_f=1.5, tau=0.02, slope=3.0)),
    "plain": ((*HALVES, RECTS, COUNTS, COUNTS_B), {}),
    "no_err": ((*HALVES, RECTS, COUNTS, COUNTS_B), dict(want_err=False, levels=3, err_init=S1))})
arrays_scenario("denoise_dual_select_arrays", render.denoise_dual_select_arrays, {
    "all": ((*HALVES, RECTS, COUNTS, COUNTS_B, CANDIDATES), dict(features=S7, features_sq=S7, counts_f=COUNTS_F, radius=4,
                                                                init=dict(out=S3, err=S1, sure=S1, win=np.zeros((H, W), dtype=np.uint32)))),
    "want_none": ((*HALVES, RECTS, COUNTS, COUNTS_B, CANDIDATES[:1]), dict(want=())),
    "want_some": ((*HALVES, RECTS, COUNTS, COUNTS_B, CANDIDATES[:1]), dict(want=("win", "err"), init=dict(sure=S1, win=np.zeros((H, W), dtype=np.uint32))))})


@scenario("finished_tile_features")
def _(fake):
    with render.Context(0) as ctx:
        feats, feats_sq = render.finished_tile_features(ctx, scenes.reflective_spheres(), _settings(), RECTS, [2, 0, 3, 2])
    return ["-> %s, %s" % (feats.shape, feats_sq.shape)]


@scenario("finished_tile_features/failing")
def _(fake):
    fake.fail = ("rmd_render_features",)
    with render.Context(0) as ctx:
        return _raises([], render.finished_tile_features, ctx, scenes.reflective_spheres(), _settings(), RECTS, COUNTS)


# ---- the render loops and await_()
def _messages(handle):
    out = []
    for m in handle._messages:
        if m.kind == "FramePreview":
            out.append("FramePreview %s pass %d at %d samples, exposure %r" % (m.frame.shape, m.pass_index, m.sample_count, m.exposure))
        else:
            t = m.tile
            out.append("%s %r at %d samples, error %r, data_sq %s, halves %r %r" % (m.kind, (t.left, t.top, t.width, t.height), t.sample_count, t.error,
                                                                                  t.data_sq is not None, t.count_a, t.count_b))
    return out


def first_converges(rect, check):
    """The first tile is below any threshold from the first check on, the second from the second, the others never."""
    return 0.0 if rect == RECTS[0] or (rect == RECTS[1] and check >= 1) else 1.0


def loop_scenario(name, devices=(0,), errors=None, **settings):
    def run_it(fake):
        if errors is not None:
            fake.tile_errors = errors
        handle = render.render_tiled(scenes.reflective_spheres(), _settings(**settings), devices)
        lines = _messages(handle)
        lines.append("leaked by render_tiled: %r" % fake.live)
        fake.lines.extend(lines)
        seen = []
        handle.set_callback(lambda tile: seen.append("tile"))
        handle.set_preview_callback(lambda m: seen.append("preview"))
        handle.async_await()
        out = handle.await_()
        return ["callbacks %r" % seen, "await_ -> %s %s" % (out.shape, out.dtype)]

    scenario("render_tiled/" + name)(run_it)


ADAPTIVE = dict(adaptive_threshold=0.5, errors=first_converges)
loop_scenario("plain")
loop_scenario("one_pass", samples_per_iteration=0)
loop_scenario("two_devices", devices=(0, 1))
loop_scenario("adaptive", sample_count=3, **ADAPTIVE)
loop_scenario("no_progress_tiles", progress_tiles=False)
loop_scenario("adaptive_no_progress_tiles", progress_tiles=False, **ADAPTIVE)
loop_scenario("denoise", denoise=True, denoise_radius=4, denoise_patch=2, denoise_k=0.5, denoise_alpha=0.75)
loop_scenario("denoise_features", denoise=True, denoise_features=True, denoise_feature_k=1.5, denoise_feature_tau=0.02)
loop_scenario("denoise_atrous", denoise=True, denoise_atrous=True, denoise_atrous_levels=3, denoise_atrous_k=2.5)
loop_scenario("denoise_atrous_features", denoise=True, denoise_atrous=True, denoise_features=True)
loop_scenario("despike", despike=True, despike_radius=1, despike_rank=1, despike_k=5.0, despike_ratio=1.5, despike_floor=0.25)
loop_scenario("despike_denoise", despike=True, denoise=True)
loop_scenario("despike_adaptive", despike=True, sample_count=3, **ADAPTIVE)
loop_scenario("preview", preview_every=1, sample_count=3, preview_exposure=2.0, preview_gamma=1.8)
loop_scenario("preview_two_devices", devices=(0, 1), preview_every=1)
loop_scenario("preview_adaptive", preview_every=1, sample_count=3, **ADAPTIVE)
loop_scenario("preview_denoise", preview_every=1, preview_denoise=True, denoise_atrous_levels=3, denoise_atrous_k=2.5, denoise_alpha=0.75)
loop_scenario("preview_auto_exposure", preview_every=1, preview_auto_exposure=True, sample_count=3, auto_exposure_percentile=0.9, auto_exposure_target=0.5)
loop_scenario("preview_denoise_auto_exposure", preview_every=1, preview_denoise=True, preview_auto_exposure=True)

LUMA = dict(sample_count=3, adaptive_threshold=0.5, errors=first_converges)
DISPLAY = dict(sample_count=3, adaptive_display_threshold=0.5, errors=first_converges)
AUTO = dict(DISPLAY, adaptive_display_auto_exposure=True, auto_exposure_percentile=0.9, auto_exposure_target=0.5, adaptive_display_gamma=1.8, adaptive_display_floor=0.0625)
DESPIKE = dict(despike_radius=1, despike_rank=1, despike_k=5.0, despike_ratio=1.5, despike_floor=0.25)
loop_scenario("adaptive_luma_tile", adaptive_measure="luma_tile", adaptive_floor=0.25, **LUMA)
loop_scenario("adaptive_luma_pixel", adaptive_measure="luma_pixel", **LUMA)
loop_scenario("adaptive_display", adaptive_display_exposure=2.0, adaptive_display_gamma=1.8, adaptive_display_floor=0.0625, **DISPLAY)
loop_scenario("adaptive_display_auto_exposure", **AUTO)
loop_scenario("adaptive_display_auto_exposure_two_devices", devices=(0, 1), **AUTO)
loop_scenario("despike_adaptive_luma_tile", despike=True, adaptive_measure="luma_tile", **DESPIKE, **LUMA)
loop_scenario("despike_adaptive_display", despike=True, adaptive_display_exposure=2.0, **DESPIKE, **DISPLAY)
loop_scenario("despike_adaptive_display_auto_exposure", despike=True, **DESPIKE, **AUTO)
loop_scenario("preview_adaptive_display_auto_exposure", preview_every=1, preview_auto_exposure=True, **AUTO)

DUAL = dict(denoise=True, denoise_dual=True, sample_count=4)
DUAL_ADAPTIVE = dict(DUAL, adaptive_denoised_threshold=0.5, adaptive_min_samples=2, sample_count=6, errors=first_converges)
loop_scenario("dual", **DUAL, denoise_radius=4, denoise_patch=2, denoise_k=0.5, denoise_alpha=0.75)
loop_scenario("dual_features", **DUAL, denoise_dual_features=True, denoise_feature_k=1.5, denoise_feature_tau=0.02)
loop_scenario("dual_select", **DUAL, denoise_dual_select=True)
loop_scenario("dual_atrous", **DUAL, denoise_dual_atrous=True, denoise_atrous_levels=3, denoise_atrous_k=2.5)
loop_scenario("dual_atrous_region", **DUAL, denoise_dual_atrous=True, denoise_dual_atrous_region=True)
loop_scenario("dual_adaptive", **DUAL_ADAPTIVE)
loop_scenario("dual_adaptive_features", **DUAL_ADAPTIVE, denoise_dual_features=True, denoise_feature_k=1.5, denoise_feature_tau=0.02)
loop_scenario("dual_adaptive_atrous", **DUAL_ADAPTIVE, denoise_dual_atrous=True)
loop_scenario("dual_adaptive_atrous_region", **DUAL_ADAPTIVE, denoise_dual_atrous=True, denoise_dual_atrous_region=True)
loop_scenario("dual_adaptive_no_progress_tiles", **DUAL_ADAPTIVE, progress_tiles=False)
loop_scenario("dual_slope_features", **DUAL, denoise_dual_features=True, denoise_feature_slope=3.0)
loop_scenario("dual_slope_select", **DUAL, denoise_dual_select=True, denoise_feature_slope=3.0)
loop_scenario("dual_slope_adaptive_features", **DUAL_ADAPTIVE, denoise_dual_features=True, denoise_feature_slope=3.0)
loop_scenario("dual_atrous_slope", **DUAL, denoise_dual_atrous=True, denoise_dual_features=True, denoise_atrous_slope=3.0)
loop_scenario("dual_atrous_slope_adaptive", **DUAL_ADAPTIVE, denoise_dual_atrous=True, denoise_dual_features=True, denoise_atrous_slope=3.0)
loop_scenario("dual_atrous_slope_adaptive_region", **DUAL_ADAPTIVE, denoise_dual_atrous=True, denoise_dual_atrous_region=True, denoise_dual_features=True,
              denoise_atrous_slope=3.0)
loop_scenario("dual_preview", **DUAL, preview_every=1, preview_exposure=2.0, preview_gamma=1.8)
loop_scenario("dual_preview_auto_exposure", **DUAL, preview_every=2, preview_auto_exposure=True)
loop_scenario("dual_preview_denoise", **DUAL, preview_every=1, preview_denoise=True, denoise_atrous_levels=3, denoise_atrous_k=2.5)
loop_scenario("dual_preview_denoise_adaptive_features", **DUAL_ADAPTIVE, preview_every=1, preview_denoise=True, denoise_dual_features=True)
loop_scenario("dual_preview_denoise_adaptive_atrous_slope", **DUAL_ADAPTIVE, preview_every=2, preview_denoise=True, denoise_dual_atrous=True,
              denoise_dual_features=True, denoise_atrous_slope=3.0)
DUAL_DISPLAY = dict(DUAL, adaptive_denoised_display_threshold=0.5, adaptive_min_samples=2, sample_count=6, errors=first_converges)
DUAL_AUTO = dict(DUAL_DISPLAY, adaptive_display_auto_exposure=True, auto_exposure_percentile=0.9, auto_exposure_target=0.5, adaptive_display_gamma=1.8)
loop_scenario("dual_adaptive_display", **DUAL_DISPLAY, adaptive_display_exposure=2.0, adaptive_display_gamma=1.8, adaptive_display_floor=0.0625)
loop_scenario("dual_adaptive_display_features", **DUAL_DISPLAY, denoise_dual_features=True, denoise_feature_k=1.5, denoise_feature_tau=0.02)
loop_scenario("dual_adaptive_display_atrous", **DUAL_DISPLAY, denoise_dual_atrous=True)
loop_scenario("dual_adaptive_display_atrous_region", **DUAL_DISPLAY, denoise_dual_atrous=True, denoise_dual_atrous_region=True)
loop_scenario("dual_adaptive_display_auto_exposure", **DUAL_AUTO)
loop_scenario("dual_adaptive_display_no_progress_tiles", **DUAL_DISPLAY, progress_tiles=False)
loop_scenario("dual_despike", **DUAL, despike_dual=True, **DESPIKE)
loop_scenario("dual_despike_adaptive", **DUAL_ADAPTIVE, despike_dual=True, **DESPIKE)
loop_scenario("dual_despike_adaptive_atrous_region", **DUAL_ADAPTIVE, despike_dual=True, denoise_dual_atrous=True, denoise_dual_atrous_region=True)
loop_scenario("dual_despike_select", **DUAL, despike_dual=True, denoise_dual_select=True)
loop_scenario("dual_despike_preview_denoise", **DUAL_ADAPTIVE, despike_dual=True, preview_every=1, preview_denoise=True)
loop_scenario("dual_despike_adaptive_display_auto_exposure", **DUAL_AUTO, despike_dual=True)


@scenario("render_tiled/failing_pass")
def _(fake):
    """A pass that fails: everything the loop opened is closed, in reverse order."""
    fake.fail = ("rmd_context_synchronize",)
    lines = _raises([], render.render_tiled, scenes.reflective_spheres(), _settings(denoise=True, preview_every=1, preview_denoise=True), (0,))
    return lines + ["leaked: %r" % fake.live]


@scenario("render_tiled/dual_failing_check")
def _(fake):
    fake.fail = ("rmd_denoise",)
    st = _settings(**{k: v for k, v in DUAL_ADAPTIVE.items() if k != "errors"}, denoise_dual_features=True)
    lines = _raises([], render.render_tiled, scenes.reflective_spheres(), st, (0,))
    return lines + ["leaked: %r" % fake.live]


@scenario("render_tiled/refusals")
def _(fake):
    lines = _raises([], render.render_tiled, scenes.reflective_spheres(), _settings(**DUAL), (0, 1))
    st = _settings(denoise=True, denoise_features=True)
    handle = render.TaskHandle(st, [])
    _raises(lines, handle.await_)
    handle = render.TaskHandle(_settings(**DUAL, denoise_dual_select=True), [])
    return _raises(lines, handle.await_)


def _later(**changed):
    """Settings that were valid when made and had `changed` set afterwards: what only render_tiled's own checks can refuse."""
    st = _settings()
    for name, value in changed.items():
        setattr(st, name, value)
    return st


@scenario("render_tiled/refusals_measures")
def _(fake):
    """Every rule of check_adaptive, check_denoise and check_despike that names adaptive_measure, adaptive_display_*, adaptive_denoised_display_threshold or
    despike_dual, by its text; none of them opens a device first."""
    dual = dict(denoise=True, denoise_dual=True)
    lines = []
    for devices, changed in (
            ((0,), dict(adaptive_measure="median")),
            ((0,), dict(adaptive_measure=None)),
            ((0,), dict(adaptive_display_threshold=-0.5)),
            ((0,), dict(adaptive_display_threshold=float("nan"))),
            ((0,), dict(adaptive_display_threshold=0.5, samples_per_iteration=0)),
            ((0,), dict(adaptive_display_threshold=0.5, adaptive_threshold=0.5)),
            ((0,), dict(adaptive_display_threshold=0.5, adaptive_measure="luma_tile")),
            ((0,), dict(adaptive_display_exposure=0.0)),
            ((0,), dict(adaptive_display_gamma=float("inf"))),
            ((0,), dict(adaptive_display_floor=1.0)),
            ((0,), dict(dual, adaptive_measure="luma_pixel")),
            ((0,), dict(dual, adaptive_display_threshold=0.5)),
            ((0,), dict(dual, adaptive_denoised_display_threshold=float("inf"))),
            ((0,), dict(adaptive_denoised_display_threshold=0.5, samples_per_iteration=0)),
            ((0,), dict(adaptive_denoised_display_threshold=0.5)),
            ((0,), dict(dual, adaptive_denoised_display_threshold=0.5, adaptive_denoised_threshold=0.5)),
            ((0,), dict(dual, adaptive_denoised_display_threshold=0.5, adaptive_threshold=0.5)),
            ((0, 1), dict(despike=True, adaptive_display_threshold=0.5)),
            ((0,), dict(despike_dual=True))):
        _raises(lines, render.render_tiled, scenes.reflective_spheres(), _later(**changed), devices)
        lines.append("C calls so far: %r" % fake.lines)
    return lines


def _releases_sorted(lines):
    """`lines` with every run of consecutive release calls (free, destroy) in sorted order: WHICH objects are released between two other calls is pinned,
    the order among them is not — nothing a caller can observe depends on it, and the binding is free to close in reverse order of opening."""
    out, run_ = [], []
    for line in lines + [""]:
        if line.startswith(_RELEASES):
            run_.append(line)
        else:
            out += sorted(run_) + [line]
            run_ = []
    return out[:-1]


def run(name):
    """The trace of one scenario: the stand-in's lines, then the scenario's own; nothing it opened may be left open."""
    with installed() as fake:
        tail = SCENARIOS[name](fake)
        return _releases_sorted(fake.lines) + list(tail) + ["left open: %r" % fake.live]
