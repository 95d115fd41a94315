"""The two-part work list of the role-sorted spheres kernel's split launches, on the host (no GPU): raymond_amd/csrc/work_list.hpp's mapping —
the function the kernel itself evaluates for every item it draws — and api.cpp's plan, through rmd_probe_work_items / rmd_probe_work_plan.

A list is (n_tiles, n_whole, k_tail): wave tiles 0 .. n_whole - 1 are ONE item each with all samples of the pass, the other tiles k_tail items
each.  Whatever the plan says, the mapping must hand every (wave tile, sample) of the pass to exactly one item — a sample handed out twice is
added twice, one never handed out is missing from the frame, and neither would fail anywhere else than in the image.  Checked over tile counts
1 .. 3 x slots (slots = 8), sample counts 1 .. 700 and the plans the host makes for them, and over the degenerate lists (all tail, all whole,
k_tail = 1, more parts than samples):
  * every (tile, sample) is covered exactly once;
  * whole items come first, one per tile, in tile order, part 0 of 1 with every sample;
  * a tail tile's parts are next to each other, in sample order, contiguous, and there are exactly k_tail of them (tile_done counts to that);
  * numbers past the end of the list name no tile and no sample;
  * n_whole + n_tail is the tile count, the tail is 2.5 tiles per wave slot, k_tail keeps 64 samples per item unless the uniform rule's k is larger,
    and a list with no more tiles than the tail — or a pass of more than 2^20 samples — is the uniform split."""
import numpy as np
import pytest

from raymond_amd import probe

SLOTS = 8
TILE_COUNTS = range(1, 3 * SLOTS + 1)
SAMPLE_COUNTS = np.arange(1, 701)


def check_list(n_tiles, n_whole, k_tail, sample_count):
    items, n_items = probe.work_items(n_tiles, n_whole, k_tail, sample_count, extra=3)
    where = (n_tiles, n_whole, k_tail, sample_count)
    assert n_items == n_whole + (n_tiles - n_whole) * k_tail, where
    past, items = items[n_items:], items[:n_items]
    assert (past[:, 0] == n_tiles).all() and (past[:, 2] == 0).all(), where
    tile, first, count, parts, whole = items.T
    # whole items first: item i is tile i, every sample, part 0 of 1
    assert (whole[:n_whole] == 1).all() and (whole[n_whole:] == 0).all(), where
    assert (tile[:n_whole] == np.arange(n_whole)).all() and (first[:n_whole] == 0).all() and (count[:n_whole] == sample_count).all() and (parts[:n_whole] == 1).all(), where
    # tail: tile-major, k_tail parts each, contiguous and ordered
    t_tile, t_first, t_count = (a[n_whole:].reshape(n_tiles - n_whole, k_tail) for a in (tile, first, count))
    assert (parts[n_whole:] == k_tail).all(), where
    assert (t_tile == np.arange(n_whole, n_tiles)[:, None]).all(), where
    assert (t_first[:, 0] == 0).all() and (t_first[:, 1:] == (t_first + t_count)[:, :-1]).all() and ((t_first + t_count)[:, -1] == sample_count).all(), where
    assert (t_count >= 0).all() and (t_count.max(initial=0) <= -(-sample_count // k_tail)), where
    # every (tile, sample) exactly once
    cover = np.zeros((n_tiles, sample_count + 1), dtype=np.int64)
    np.add.at(cover, (tile, first), 1)
    np.add.at(cover, (tile, first + count), -1)
    assert (np.cumsum(cover, axis=1)[:, :sample_count] == 1).all() and (cover.sum(axis=1) == 0).all(), where


@pytest.mark.parametrize("n_tiles", list(TILE_COUNTS))
def test_the_planned_lists_cover_every_tile_and_sample_once(n_tiles):
    for k_uniform in (1, 2, 7):
        n_whole, n_tail, k_tail = probe.work_plan(SLOTS, n_tiles, SAMPLE_COUNTS, k_uniform)
        assert (n_whole + n_tail == n_tiles).all()
        seen = set()
        for s, w, k in zip(SAMPLE_COUNTS, n_whole, k_tail):
            if (int(w), int(k)) not in seen or s % 7 == 0 or s < 12:  # every distinct plan of this tile count, and a spread of sample counts for each
                check_list(n_tiles, int(w), int(k), int(s))
                seen.add((int(w), int(k)))


def test_the_plan_over_tile_counts_and_sample_counts():
    tiles = np.array(list(TILE_COUNTS))[:, None]
    for k_uniform in (1, 2, 3, 7, 64):
        n_whole, n_tail, k_tail = probe.work_plan(SLOTS, tiles, SAMPLE_COUNTS[None, :], k_uniform)
        assert (n_whole + n_tail == tiles).all() and (n_whole >= 0).all() and (k_tail >= 1).all() and (k_tail <= 64).all()
        tail = 5 * SLOTS // 2  # 2.5 wave tiles per wave slot
        few = np.broadcast_to(tiles <= tail, n_whole.shape)
        assert (n_whole[few] == 0).all() and (k_tail[few] == k_uniform).all()  # few tiles: the uniform split, as it was
        assert (n_tail[~few] == tail).all()
        # k_tail: 4 parts where each keeps 64 samples, fewer where not, never fewer than the uniform rule's
        want = np.maximum(np.minimum(4, SAMPLE_COUNTS // 64), k_uniform)
        assert (k_tail[~few] == np.broadcast_to(want[None, :], k_tail.shape)[~few]).all()
    # the plan scales with the slots
    w, t, k = probe.work_plan(4096, 32400, 500, 4)
    assert (int(w), int(t), int(k)) == (32400 - 10240, 10240, 4)
    w, t, k = probe.work_plan(4096, 10240, 500, 7)
    assert (int(w), int(t), int(k)) == (0, 10240, 7)
    # whole items only while a pass's pool indices keep room in 32 bits: up to 2^20 samples
    w, t, k = probe.work_plan(SLOTS, 100, [1 << 20, (1 << 20) + 1], 3)
    assert w.tolist() == [100 - 20, 0] and t.tolist() == [20, 100] and k.tolist() == [4, 3]


@pytest.mark.parametrize("n_tiles,n_whole,k_tail", [(1, 0, 1), (1, 1, 1), (1, 1, 5), (5, 0, 3), (5, 5, 3), (5, 0, 1), (5, 4, 1), (24, 12, 64), (24, 23, 7), (9, 1, 2)])
def test_degenerate_lists(n_tiles, n_whole, k_tail):
    for s in (1, 2, 3, 63, 64, 65, 127, 128, 500, 700):  # (more parts than samples: the empty parts are items too)
        check_list(n_tiles, n_whole, k_tail, s)
