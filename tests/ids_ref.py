"""The expected words of rmd_render_ids and the expected matte of rmd_ids_matte, restated in numpy from include/raymond_hip.h and nothing else.

The input is the oracle's per-sample first-hit object index (tests/first_hit_ref.py: reference(key).objs, shape (spp, H, W), -1 for a miss and for a
sample the thin lens yields no ray for).  The rule is applied sample by sample, in order; a record is key_0 count_0 .. key_3 count_3 other samples.

VARIANTS are three wrong readings of the definition, for tests/test_ids_host.py to tell the restatement from:
  sorted_by_key     the slots kept in ascending key order instead of first-seen order
  other_in_matte    `other` counted into the matte's numerator
  skip_no_ray       a sample without a ray skipped instead of counted as a miss (needs the `no_ray` mask)
"""
import numpy as np

SLOTS, WORDS, OTHER, SAMPLES = 4, 10, 8, 9
MISS = 0xFFFFFFFF
VARIANTS = ("sorted_by_key", "other_in_matte", "skip_no_ray")


def key_of(obj):
    """object indices (-1 or MISS: the background) -> keys"""
    obj = np.asarray(obj, dtype=np.int64)
    return np.where((obj < 0) | (obj == MISS), MISS, obj + 1).astype(np.uint32)


def insert(words, keys, active=None):
    """One sample per record: words (N, 10) uint32, changed in place; keys (N,) uint32; active (N,) bool or None = all."""
    open_ = np.ones(len(words), dtype=bool) if active is None else active.copy()
    counted = open_.copy()
    for j in range(SLOTS):
        take = open_ & ((words[:, 2 * j] == keys) | (words[:, 2 * j] == 0))
        words[take, 2 * j] = keys[take]
        words[take, 2 * j + 1] += np.uint32(1)
        open_ &= ~take
    words[open_, OTHER] += np.uint32(1)
    words[counted, SAMPLES] += np.uint32(1)


def sort_slots(words):
    """the wrong reading `sorted_by_key`: the used slots in ascending key order, empty slots trailing"""
    out = words.copy()
    k, c = words[:, 0:8:2].astype(np.int64), words[:, 1:8:2]
    order = np.argsort(np.where(k == 0, 1 << 40, k), axis=1, kind="stable")
    out[:, 0:8:2] = np.take_along_axis(words[:, 0:8:2], order, axis=1)
    out[:, 1:8:2] = np.take_along_axis(c, order, axis=1)
    return out


def words_from_objs(objs, base=None, no_ray=None, variant=None):
    """objs (spp, H, W) -> (H, W, 10) uint32: the records after the samples in order, from `base` (H, W, 10) or zero.  no_ray (spp, H, W) bool:
    which of the -1 are samples without a ray (read by the wrong reading skip_no_ray alone)."""
    objs = np.asarray(objs)
    spp, H, W = objs.shape
    words = np.zeros((H * W, WORDS), dtype=np.uint32) if base is None else np.ascontiguousarray(base, dtype=np.uint32).reshape(H * W, WORDS).copy()
    for s in range(spp):
        active = None
        if variant == "skip_no_ray" and no_ray is not None:
            active = ~np.asarray(no_ray[s], dtype=bool).reshape(-1)
        insert(words, key_of(objs[s].reshape(-1)), active)
        if variant == "sorted_by_key":
            words = sort_slots(words)
    return words.reshape(H, W, WORDS)


def matte(words, objects, variant=None):
    """(..., 10) words and a list of object indices (MISS or -1: the background) -> ((...) float64 matte, the number of pixels with other != 0)"""
    words = np.asarray(words, dtype=np.uint32)
    keys = np.unique(key_of(np.asarray(objects, dtype=np.int64).reshape(-1)))
    k, c = words[..., 0:8:2], words[..., 1:8:2].astype(np.uint64)
    inset = np.isin(k, keys) & (k != 0)
    num = np.where(inset, c, np.uint64(0)).sum(axis=-1, dtype=np.uint64)
    if variant == "other_in_matte":
        num = num + words[..., OTHER].astype(np.uint64)
    samples = words[..., SAMPLES]
    with np.errstate(all="ignore"):
        out = np.where(samples == 0, 0.0, num.astype(np.float64) / samples.astype(np.float64))
    return out, int((words[..., OTHER] != 0).sum())


def used_slots(words):
    """(..., 10) -> (...) the number of slots with a key"""
    return (np.asarray(words)[..., 0:8:2] != 0).sum(axis=-1)


def random_records(rng, n):
    """n records for the matte: samples == 0 (all-zero records), part-filled and full tables with and without `other`, the miss key in any slot, counts
    up to 2^32 - 1 (records need not be reachable by the rule: the matte is defined on the words)"""
    words = np.zeros((n, WORDS), dtype=np.uint32)
    kind = rng.integers(0, 6, n)
    for i in range(n):
        if kind[i] == 0:
            continue  # samples == 0
        used = SLOTS if kind[i] >= 3 else int(rng.integers(1, SLOTS + 1))
        pool = np.concatenate([rng.choice(np.arange(1, 40, dtype=np.uint32), size=SLOTS, replace=False), [MISS]]).astype(np.uint32)
        keys = rng.permutation(pool)[:used]
        big = kind[i] == 5
        counts = rng.integers(1, 0xFFFFFFFF if big else 64, used, dtype=np.uint64, endpoint=True)
        other = int(rng.integers(1, 64)) if kind[i] == 4 else 0
        words[i, 0 : 2 * used : 2], words[i, 1 : 2 * used : 2] = keys, counts.astype(np.uint32)
        words[i, OTHER] = other
        words[i, SAMPLES] = np.uint32((int(counts.sum()) + other) & 0xFFFFFFFF) or np.uint32(1)
    return words
