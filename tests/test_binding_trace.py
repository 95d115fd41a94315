"""raymond_amd/render.py makes the C calls recorded in tests/golden/binding_trace.json: the same entry points, with the same arguments in the same order,
for every scenario of tests/binding_trace.py (every public wrapper at every switch it has, every *_arrays helper, the two render loops and await_()).
The library is binding_trace's recording stand-in, so this needs no GPU; it is what shows that a wrapper calls the entry point it is meant to."""
import ctypes as C
import difflib
import json
import os
import re

import pytest

import binding_trace
from raymond_amd import lib, render

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_trace.json")
with open(GOLDEN) as f:
    _DOC = json.load(f)
RECORDED = {name: [_DOC["lines"][int(i)] for i in numbers.split()] for name, numbers in _DOC["scenarios"].items()}


def test_the_recording_covers_the_scenarios():
    assert sorted(RECORDED) == sorted(binding_trace.SCENARIOS)


@pytest.mark.parametrize("name", sorted(binding_trace.SCENARIOS))
def test_calls_are_the_recorded_ones(name):
    got = binding_trace.run(name)
    assert got[-1] == "left open: []", got[-1]  # whatever the scenario opened is closed, also where a call raised
    if got != RECORDED[name]:
        pytest.fail("\n".join(difflib.unified_diff(RECORDED[name], got, "recorded", "now", lineterm="", n=1)), pytrace=False)


def test_every_denoise_entry_point_is_reached():
    """The scenarios leave no entry point of the header uncalled that takes frame data or makes a table for one that does: rmd_denoise* / rmd_despike* /
    rmd_tile_* (the errors and the measures) / rmd_display* / rmd_resolve* / rmd_luminance* / rmd_exposure*.  And lib has one signature table, which holds
    every rmd_* function of include/raymond_hip.h that render.py names."""
    called = {line.split("(", 1)[0] for lines in RECORDED.values() for line in lines}
    family = [n for n in lib.SIGNATURES
              if n.startswith(("rmd_denoise", "rmd_despike", "rmd_tile_error", "rmd_tile_", "rmd_display", "rmd_resolve", "rmd_luminance", "rmd_exposure"))]
    assert len([n for n in family if n.startswith("rmd_denoise")]) == 17
    assert {"rmd_tile_luma_error", "rmd_tile_weighted_error", "rmd_tile_weighted_error_dual", "rmd_display_weights", "rmd_despike_dual"} <= set(family)
    assert [n for n in family if n not in called] == []
    for name in ("rmd_tile_luma_error", "rmd_tile_weighted_error", "rmd_tile_weighted_error_dual", "rmd_display_weights", "rmd_despike_dual"):
        reached = {scenario.startswith("render_tiled/") for scenario, lines in RECORDED.items() if any(line.startswith(name + "(") for line in lines)}
        assert reached == {False, True}, name  # by a wrapper's scenario and by a loop's
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "raymond_hip.h")) as f:
        declared = set(re.findall(r"\b(rmd_\w+)\s*\(", f.read()))
    with open(render.__file__) as f:
        source = f.read()
    named = set(re.findall(r"\brmd_\w+\b", source)) & declared  # (the denoise family's names are put together from their stems: `named` holds the stems)
    literal = {n for found in re.findall(r"\bL\.(rmd_\w+)\(|\bload\(\)\.(rmd_\w+)\(|\"(rmd_\w+)\"", source) for n in found if n}
    assert len(named) > 40 and literal <= named and named <= set(lib.SIGNATURES)
    assert {n for n in called if n.startswith("rmd_")} <= set(lib.SIGNATURES)  # every recorded call is of that table
    tables = [n for n, v in vars(lib).items() if isinstance(v, dict) and any(str(k).startswith("rmd_") for k in v)]
    assert tables == ["SIGNATURES"]


@pytest.mark.parametrize("body", ["denoise_arrays", "render_tiled", "render_tiled_dual"])
def test_a_failing_close_keeps_nothing_else_open_and_hides_no_error(monkeypatch, body):
    """The first close (of what was opened last) raises before it frees anything: everything else is still closed, and what comes out is the body's own
    error — the failing filter call's, or the failing pass's."""
    real_close, failed = render.Framebuffer.close, []

    def close(self):
        if not failed:
            failed.append(self)
            raise RuntimeError("this close fails")
        real_close(self)

    with binding_trace.installed() as fake:
        monkeypatch.setattr(render.Framebuffer, "close", close)
        with pytest.raises(lib.RaymondError, match="told to fail"):
            if body == "denoise_arrays":
                fake.fail = ("rmd_denoise",)
                with render.Context(0) as ctx:
                    render.denoise_arrays(ctx, binding_trace.S3, binding_trace.S3, binding_trace.RECTS, binding_trace.COUNTS)
            else:
                fake.fail = ("rmd_context_synchronize",)
                dual = dict(denoise_dual=True) if body == "render_tiled_dual" else {}
                render.render_tiled(binding_trace.scenes.reflective_spheres(), binding_trace._settings(denoise=True, **dual))
        assert len(failed) == 1 and len(fake.live) == 1 and fake.live[0].startswith("fb")


@pytest.mark.parametrize("name, atrous, guided", [("dual_adaptive_features", False, True), ("dual_atrous_slope_adaptive_region", True, True),
                                                  ("dual_adaptive", False, False), ("dual_preview_denoise_adaptive_features", False, True)])
def test_the_loops_call_the_filters_through_the_module_names(monkeypatch, name, atrous, guided):
    """Spies with the signatures the GPU tests give theirs, set on raymond_amd.render for the duration of render_tiled, see the dual loop's filter and
    error calls — positional up to the error image, region and the rest as keywords — and the C calls are the recorded ones all the same."""
    seen = []

    def spy_on(fn_name):
        real = getattr(render, fn_name)

        def spy_filter(ctx, half_a, half_b, rects, counts_a, counts_b, out_fb, err_img=None, **kw):
            seen.append((fn_name, sorted(k for k, v in kw.items() if v is not None)))  # (await_() passes region=None)
            return real(ctx, half_a, half_b, rects, counts_a, counts_b, out_fb, err_img, **kw)

        monkeypatch.setattr(render, fn_name, spy_filter)

    spy_on("denoise_dual"), spy_on("denoise_atrous_dual")
    real_error = render.tile_error_dual

    def spy_error(ctx, err_img, rects):
        seen.append(("tile_error_dual", len(rects)))
        return real_error(ctx, err_img, rects)

    monkeypatch.setattr(render, "tile_error_dual", spy_error)
    assert binding_trace.run("render_tiled/" + name) == RECORDED["render_tiled/" + name]
    checks = [kw for fn, kw in seen if fn == ("denoise_atrous_dual" if atrous else "denoise_dual") and "region" in kw]
    assert len(checks) == 2 and all(("features" in kw) == guided for kw in checks)
    assert [s for s in seen if s[0] == "tile_error_dual"] == [("tile_error_dual", 4), ("tile_error_dual", 3)]
    if "preview" in name:
        # one whole-frame a-trous call per preview (five passes leave live tiles), then await_()'s filter
        assert [fn for fn, kw in seen if fn != "tile_error_dual" and "region" not in kw] == ["denoise_atrous_dual"] * 5 + ["denoise_dual"]


# ---------------------------------------------------------------- the traces tell wrong bindings apart
def _tiled_adaptive_check(raw=False, pixel_field="pixel_rms"):
    """_TiledLoop.adaptive_check; `raw`: it makes the despiked sums and then reads the pass's own; `pixel_field`: what "luma_pixel" reads."""
    def adaptive_check(self, w):
        st = self.st
        if not (self.adaptive and w.live):
            return [None] * len(w.live)
        fb, fb_sq = self.check_buffers(w)
        if raw:
            fb, fb_sq = w.fb, w.fb_sq
        if self.display:
            return render.tile_weighted_error(w.ctx, fb, fb_sq, w.live, [self.done] * len(w.live), self.weights)["rms"]
        if st.adaptive_measure != "channel_max":
            luma = render.tile_luma_error(w.ctx, fb, fb_sq, w.live, [self.done] * len(w.live), st.adaptive_floor)
            return luma["tile_rms" if st.adaptive_measure == "luma_tile" else pixel_field]
        return render.tile_error(w.ctx, fb, fb_sq, self.done, st.adaptive_floor, w.live)

    return adaptive_check


def _tiled_check_weights(raw=False, keep_first=False):
    """_TiledLoop.check_weights; `raw`: the histogram reads the pass's own sums; `keep_first`: the new table is made and not kept."""
    def check_weights(self):
        st = self.st
        if not (self.display and st.adaptive_display_auto_exposure and any(w.live for w in self.workers)):
            return
        hist = render.LumaHistogram()
        for w in self.workers:
            rects, counts = w.whole_frame(self.done)
            if rects:
                hist = render.add_histograms(hist, render.luminance_histogram(w.ctx, w.fb if raw else self.check_buffers(w)[0], rects, counts))
        exposure = render.exposure_from_histogram(hist, st.auto_exposure_percentile, st.auto_exposure_target)
        table = render.display_weights(exposure, st.adaptive_display_gamma, st.adaptive_display_floor)
        if not keep_first:
            self.weights = table

    return check_weights


def _dual_check_weights(second=True, spare=False):
    """_DualLoop.check_weights; second=False: half A alone; `spare`: the despiked halves."""
    def check_weights(self):
        st = self.st
        rects, all_a, all_b = self.whole_frame(self.live)
        a, b = (self.spare[0], self.spare[2]) if spare else (self.fbs[0], self.fbs[2])
        hist = render.luminance_histogram(self.ctx, a, rects, [x + y for x, y in zip(all_a, all_b)], b if second else None)
        exposure = render.exposure_from_histogram(hist, st.auto_exposure_percentile, st.auto_exposure_target)
        self.weights = render.display_weights(exposure, st.adaptive_display_gamma, st.adaptive_display_floor)

    return check_weights


def _filter_halves_once(self, rects, all_a, all_b):
    """_DualLoop.filter_halves with despiked_at never compared with the pass."""
    if self.spare is None:
        return (self.fbs[0], self.fbs[1]), (self.fbs[2], self.fbs[3])
    out = (self.spare[0], self.spare[1]), (self.spare[2], self.spare[3])
    if self.despiked_at is None:
        render.despike_dual(self.ctx, (self.fbs[0], self.fbs[1]), (self.fbs[2], self.fbs[3]), rects, all_a, all_b, out=out, want_replaced=False, **self.st.despike_keywords())
        self.despiked_at = self.passes
    return out


def _wrong_counts_order(mp):
    real = render.despike_dual
    mp.setattr(render, "despike_dual", lambda ctx, a, b, rects, counts_a, counts_b, *args, **kw: real(ctx, a, b, rects, counts_b, counts_a, *args, **kw))


def _wrong_outputs_order(mp):
    real = render.despike_dual

    def despike_dual(*args, out=None, **kw):
        b, a, replaced = real(*args, out=None if out is None else (out[1], out[0]), **kw)
        return a, b, replaced

    mp.setattr(render, "despike_dual", despike_dual)


def _wrong_measure_buffers(mp):
    real = render.tile_weighted_error_dual
    mp.setattr(render, "tile_weighted_error_dual", lambda ctx, out_fb, err_img, tiles, weights: real(ctx, err_img, out_fb, tiles, weights))


def _wrong_dual_threshold(mp):
    real = render._DualLoop.__init__

    def init(self, *args):
        real(self, *args)
        self.threshold = self.st.adaptive_denoised_threshold

    mp.setattr(render._DualLoop, "__init__", init)


def _wrong_await_switch(mp):
    real = render.TaskHandle._await_dual

    def await_dual(self):  # the despike step asks the single-buffer loop's switch, which is off wherever denoise_dual is on
        st = self.settings
        was, st.despike_dual = st.despike_dual, st.despike
        try:
            return real(self)
        finally:
            st.despike_dual = was

    mp.setattr(render.TaskHandle, "_await_dual", await_dual)


def _method(cls, name, wrong):
    return lambda mp: mp.setattr(getattr(render, cls), name, wrong)


WRONG = {  # a wrong variant of raymond_amd.render: (how it is put in place, the scenarios whose traces it must change)
    "despike_dual passes counts_b before counts_a": (_wrong_counts_order, ["despike_dual", "despike_dual_arrays/plain", "render_tiled/dual_despike_preview_denoise"]),
    "despike_dual writes half B's outputs first": (_wrong_outputs_order, ["despike_dual", "despike_dual_arrays/plain", "render_tiled/dual_despike_adaptive"]),
    "tile_weighted_error_dual passes err_img before out_fb": (_wrong_measure_buffers, ["tile_measures", "render_tiled/dual_adaptive_display"]),
    "luma_pixel reads tile_rms": (_method("_TiledLoop", "adaptive_check", _tiled_adaptive_check(pixel_field="tile_rms")), ["render_tiled/adaptive_luma_pixel"]),
    "the single-buffer check with despike reads the raw sums": (_method("_TiledLoop", "adaptive_check", _tiled_adaptive_check(raw=True)),
                                                               ["render_tiled/despike_adaptive_luma_tile", "render_tiled/despike_adaptive_display",
                                                                "render_tiled/despike_adaptive_display_auto_exposure"]),
    "the single-buffer histogram reads the raw sums while the check reads the despiked ones": (
        _method("_TiledLoop", "check_weights", _tiled_check_weights(raw=True)), ["render_tiled/despike_adaptive_display_auto_exposure"]),
    "auto exposure makes the new table and keeps the first": (
        _method("_TiledLoop", "check_weights", _tiled_check_weights(keep_first=True)),
        ["render_tiled/adaptive_display_auto_exposure", "render_tiled/adaptive_display_auto_exposure_two_devices", "render_tiled/preview_adaptive_display_auto_exposure"]),
    "the dual histogram drops the second buffer": (_method("_DualLoop", "check_weights", _dual_check_weights(second=False)),
                                                  ["render_tiled/dual_adaptive_display_auto_exposure"]),
    "the dual histogram reads the spare halves": (_method("_DualLoop", "check_weights", _dual_check_weights(spare=True)),
                                                 ["render_tiled/dual_despike_adaptive_display_auto_exposure"]),
    "filter_halves never despikes again after its first call": (_method("_DualLoop", "filter_halves", _filter_halves_once),
                                                               ["render_tiled/dual_despike_adaptive", "render_tiled/dual_despike_preview_denoise"]),
    "the dual display check compares with adaptive_denoised_threshold": (_wrong_dual_threshold, ["render_tiled/dual_adaptive_display"]),
    "await_() filters the raw halves with despike_dual": (_wrong_await_switch, ["render_tiled/dual_despike", "render_tiled/dual_despike_select"]),
}


@pytest.mark.parametrize("variant", sorted(WRONG))
def test_the_trace_tells_wrong_bindings_apart(monkeypatch, variant):
    """Each wrong variant of render.py — one argument pair swapped, one wrong attribute read — changes the trace of every scenario named for it; the copies
    of the loops' methods above, with their switches off, leave every trace what it is."""
    put_in_place, caught_by = WRONG[variant]
    for cls, name, right in (("_TiledLoop", "adaptive_check", _tiled_adaptive_check()), ("_TiledLoop", "check_weights", _tiled_check_weights()),
                             ("_DualLoop", "check_weights", _dual_check_weights())):
        with monkeypatch.context() as mp:  # (a copy that had drifted from render.py would tell nothing apart)
            mp.setattr(getattr(render, cls), name, right)
            for scenario in caught_by:
                assert binding_trace.run(scenario) == RECORDED[scenario], (cls, name, scenario)
    put_in_place(monkeypatch)
    for scenario in caught_by:
        got = binding_trace.run(scenario)
        assert got[-1] == "left open: []" and got != RECORDED[scenario], scenario
        changed = [line for line in difflib.unified_diff(RECORDED[scenario], got, lineterm="", n=0) if line[:1] in "+-" and line[:3] not in ("+++", "---")]
        print("%s: %s: %d lines differ, the first %s" % (variant, scenario, len(changed), changed[0]))


def test_the_stand_in_converts_arguments_as_the_library_would():
    """A wrong type is refused by ctypes before the recorder sees it, and the real loader comes back after the block."""
    before = lib._lib
    with binding_trace.installed() as fake:
        ctx = render.Context(0)
        with pytest.raises(C.ArgumentError):
            fake.rmd_framebuffer_zero(ctx.handle, 1.5, 3)  # (a float where a pointer goes)
        ctx.close()
        assert fake.live == []
    assert lib._lib is before
