"""The device scratch block of every denoise entry point, on the host (no GPU): denoise_host.hpp's denoise_scratch_layout — the function the entry points
carve their block with — through rmd_probe_denoise_scratch.

Every part starts on a 16-byte boundary, the parts are pairwise disjoint and lie inside the block, each form holds exactly the parts its launcher takes,
and each part has the length launch.hpp states for it.  The sizes are the ones where padding matters: W*H odd and not a multiple of 4 (a uint32 image that
ends off a 16-byte boundary), 0 .. 3 rects (counts of 0, 4 and 12 bytes), 1 and 5 table entries."""
import itertools

import numpy as np
import pytest

from raymond_amd import abi, probe

F64, U32, RECT, BLOCK = 8, 4, 16, 16
SIZES = [(1, 1), (3, 1), (45, 29), (37, 23), (70, 9)]
N_RECTS = [0, 1, 3]
N_TABLE = [0, 1, 5]
N_CANDS = [1, 4]
DUAL_FORMS = ("dual", "atrous_dual", "atrous_dual_region", "dual_select")


def expected(form, N, n_rects, guided, n_cands, n_table):
    """{part: bytes} as raymond_amd/csrc/launch.hpp documents each launcher's scratch."""
    if form == "tile_error":  # [rects][one double per rect]
        return {"rects": RECT * n_rects, "tile_errors": F64 * n_rects}
    dual = form in DUAL_FORMS
    want = {"n_img": U32 * N * (2 if dual else 1), "rects": RECT * n_rects, "counts_a": U32 * n_rects}
    if dual:
        want["counts_b"] = U32 * n_rects
    if guided:
        want["feat_planes"] = F64 * 14 * N
        if dual:
            want["n_f_img"], want["counts_f"] = U32 * N, U32 * n_rects
    if n_table and form in ("dual", "atrous_dual_region"):  # launch.hpp: launch_denoise_dual's table, launch_denoise_atrous_dual_region's tables; no other takes one
        want["table"] = BLOCK * n_table
    if form == "atrous":
        want["planes"] = F64 * 12 * N  # cv
    elif form == "dual":
        want["planes"], want["f_b"] = F64 * 12 * N, F64 * 3 * N
    elif form in ("atrous_dual", "atrous_dual_region"):
        want["planes"] = F64 * 24 * N  # state
    elif form == "dual_select":
        want["planes"], want["cand_img"], want["gain"], want["win_img"] = F64 * 12 * N, F64 * 7 * N * n_cands, F64 * 2 * N, U32 * N
    return want


def cases(form):
    tables = N_TABLE if form != "tile_error" else [0]  # (only the region launchers take a table: the other forms must ignore the count)
    cands = N_CANDS if form == "dual_select" else [0]
    return itertools.product(SIZES, N_RECTS, (False, True) if form != "tile_error" else (False,), cands, tables)


@pytest.mark.parametrize("form", probe.SCRATCH_FORMS)
def test_parts_are_aligned_disjoint_inside_and_as_long_as_documented(form):
    assert set(probe.SCRATCH_FORMS) >= {"single", "atrous", "dual", "atrous_dual", "atrous_dual_region", "dual_select"}
    n = 0
    for (W, H), n_rects, guided, n_cands, n_table in cases(form):
        parts, total = probe.denoise_scratch(form, W, H, n_rects, guided, n_cands, n_table)
        what = (form, W, H, n_rects, guided, n_cands, n_table)
        assert {k: b for k, (_, b) in parts.items()} == expected(form, W * H, n_rects, guided, n_cands, n_table), what
        spans = sorted((o, o + b) for o, b in parts.values())
        assert all(o % 16 == 0 for o, _ in spans), what
        assert all(a_end <= b_begin for (_, a_end), (b_begin, _) in zip(spans, spans[1:])), what
        assert spans[0][0] == 0 and spans[-1][1] <= total, what
        n += 1
    assert n == len(SIZES) * len(N_RECTS) * (1 if form == "tile_error" else 2) * (1 if form == "tile_error" else 3) * (2 if form == "dual_select" else 1)


def test_the_block_is_no_larger_than_its_parts_and_their_padding():
    """Nothing is carved that no launcher takes: the total is the parts' lengths, each rounded up to 16 bytes."""
    for form in probe.SCRATCH_FORMS:
        for (W, H), n_rects, guided, n_cands, n_table in cases(form):
            parts, total = probe.denoise_scratch(form, W, H, n_rects, guided, n_cands, n_table)
            assert total == sum((b + 15) // 16 * 16 for _, b in parts.values()), (form, W, H, n_rects, guided, n_cands, n_table)


def test_bad_arguments_are_refused():
    L, out = probe._L(), np.zeros(3 * len(probe.SCRATCH_PARTS), dtype=np.uint64)
    assert L.rmd_probe_denoise_scratch(len(probe.SCRATCH_FORMS), 8, 8, 1, 0, 0, 0, probe._p(out), None) == abi.RMD_ERR_INVALID_ARGUMENT
    assert L.rmd_probe_denoise_scratch(0, 8, 8, 1, 0, 0, 0, None, None) == abi.RMD_ERR_INVALID_ARGUMENT
