"""raymond_amd/render.py makes the C calls recorded in tests/golden/binding_trace.json: the same entry points, with the same arguments in the same order,
for every scenario of tests/binding_trace.py (every public wrapper at every switch it has, every *_arrays helper, the two render loops and await_()).
The library is binding_trace's recording stand-in, so this needs no GPU; it is what shows that a wrapper calls the entry point it is meant to."""
import ctypes as C
import difflib
import json
import os

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
    """The scenarios leave no rmd_denoise* / rmd_despike / rmd_tile_error* / rmd_resolve* / rmd_luminance* entry point of the header uncalled."""
    called = {line.split("(", 1)[0] for lines in RECORDED.values() for line in lines}
    family = [n for n in lib.SIGNATURES if n.startswith(("rmd_denoise", "rmd_despike", "rmd_tile_error", "rmd_resolve", "rmd_luminance", "rmd_exposure"))]
    assert len([n for n in family if n.startswith("rmd_denoise")]) == 17
    assert [n for n in family if n not in called] == []


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
