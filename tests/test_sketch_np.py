"""The host model of the counting sketch (tests/sketch_np.py) pinned without a GPU: known answers of the key hash worked out once
with plain Python integers from the definition in include/kmx.h, the bound estimate >= min(255, true count), the merge law and
count_solid == filter of the full count, for any sketch size."""
import numpy as np
import pytest

from tests import sketch_np as sk
from tests.count_np import table_of

K1 = 0x0123456789ABCDEF
M = (1 << 64) - 1

# (lo, hi or None for a one-word key, seed, log2_blocks) -> (h, the four cells)
KATS = [
    ((0, None, 0, 0), (0x6393D51C06C618DC, [12, 29, 40, 49])),                      # key 0, seed 0, one block: no shift by 64
    ((0, None, 0, 10), (0x6393D51C06C618DC, [25484, 25501, 25512, 25521])),
    ((K1, None, 7, 10), (0xBD09E0ABCBEB101F, [48399, 48401, 48416, 48433])),
    ((K1, 0, 7, 10), (0xBD09E0ABCBEB101F, [48399, 48401, 48416, 48433])),            # (lo, 0) IS the one-word key
    ((K1, 5, 7, 10), (0xAF0BE9F3C8D118C3, [44803, 44828, 44840, 44849])),            # the same lo under hi != 0: another block
    ((K1, None, 7, 32), (0xBD09E0ABCBEB101F, [202978634447, 202978634449, 202978634464, 202978634481])),
    ((M, M, M, 1), (0x0F8821C6BA3E4D1D, [13, 17, 45, 52])),                          # every sum wraps
    ((1, None, 0, 12), (0x8D82751399F55D54, [144900, 144917, 144941, 144949])),
]


def _key(lo, hi):
    return np.array([lo], np.uint64) if hi is None else np.array([[lo, hi]], np.uint64)


def test_fmix64_known_answers():
    assert [int(v) for v in sk.fmix64(np.array([0, 1], np.uint64))] == [0, 0xB456BCFC34C2CB2C]


@pytest.mark.parametrize("case", KATS)
def test_key_hash_and_cells_known_answers(case):
    (lo, hi, seed, lb), (h, cells) = case
    assert int(sk.key_hash(_key(lo, hi), seed)[0]) == h
    got = [int(c) for c in sk.cells_of(_key(lo, hi), lb, seed)[0]]
    assert got == cells
    assert len(set(got)) == 4 and len({c // 64 for c in got}) == 1 and [c % 64 // 16 for c in got] == [0, 1, 2, 3]


def _multiset(rng, n_distinct, n, words):
    pool = rng.integers(0, 2**63, (n_distinct, words), dtype=np.uint64)
    pick = pool[np.minimum((rng.pareto(1.2, n) * 3).astype(np.int64), n_distinct - 1)]   # a few heavy keys, many singletons
    return pick[:, 0] if words == 1 else pick


@pytest.mark.parametrize("words", (1, 2))
@pytest.mark.parametrize("log2_blocks", (0, 3, 9))
def test_estimate_is_never_below_the_clipped_count(words, log2_blocks):
    rng = np.random.default_rng(10 * log2_blocks + words)
    keys = _multiset(rng, 3000, 20000, words)
    s = sk.add(sk.new(log2_blocks), keys, log2_blocks, seed=3)
    tk, tc = table_of(keys, np.ones(len(keys), np.uint8))
    est = sk.estimate(s, tk, log2_blocks, seed=3)
    assert (est.astype(np.uint64) >= np.minimum(tc, 255)).all()
    assert tc.max() > 255 and est.max() == 255                        # the heavy keys saturate
    if log2_blocks == 9:
        assert (est.astype(np.uint64) == np.minimum(tc, 255)).mean() > 0.5   # and a roomy sketch is mostly exact
    # weights: a table added with its counts is the multiset added key by key
    assert (sk.add(sk.new(log2_blocks), tk, log2_blocks, seed=3, weights=tc) == s).all()


def test_adds_commute_and_saturate():
    key = np.array([K1], np.uint64)
    s = sk.add(sk.new(2), key, 2, weights=[200])
    s = sk.add(s, key, 2, weights=[200])
    cells = sk.cells_of(key, 2)[0]
    assert (s[cells] == 255).all() and np.count_nonzero(s) == 4
    assert (sk.add(sk.new(2), key, 2, weights=[2**40]) == s).all()    # a u64 weight above 255 is 255
    assert (sk.stats(s) == np.bincount(s, minlength=256)).all() and sk.fill(s) == 4 / 256


@pytest.mark.parametrize("words", (1, 2))
def test_merge_law(words):
    rng = np.random.default_rng(77 + words)
    keys = _multiset(rng, 500, 30000, words)
    for lb in (0, 4):
        whole = sk.add(sk.new(lb), keys, lb, seed=9)
        a = sk.add(sk.new(lb), keys[:11000], lb, seed=9)
        b = sk.add(sk.new(lb), keys[11000:], lb, seed=9)
        assert (sk.merge(a, b) == whole).all() and (sk.merge(b, a) == whole).all()
        assert whole.max() == 255


@pytest.mark.parametrize("words", (1, 2))
@pytest.mark.parametrize("log2_blocks", (0, 2, 8))
@pytest.mark.parametrize("min_count", (1, 2, 3, 255))
def test_count_solid_equals_the_filtered_full_count(words, log2_blocks, min_count):
    rng = np.random.default_rng(1000 * words + 10 * log2_blocks + min_count)
    keys = _multiset(rng, 4000, 24000, words)
    flags = (rng.random(len(keys)) < 0.95).astype(np.uint8) * 3        # some windows are not valid
    cut = [0, 5000, 5000, 13000, 24000]                                 # an empty batch among them
    batches = [(keys[a:b], flags[a:b]) for a, b in zip(cut[:-1], cut[1:])]
    gk, gc, s, sizes = sk.count_solid(batches, min_count, log2_blocks, seed=5)
    tk, tc = table_of(keys, flags)
    keep = tc >= min_count
    assert gk.shape == tk[keep].shape and (gk == tk[keep]).all() and (gc == tc[keep]).all()
    assert (s == sk.add(sk.new(log2_blocks), keys, log2_blocks, seed=5, flags=flags)).all()
    full = [len(table_of(k_, f_)[1]) for k_, f_ in batches]
    assert all(a <= b for a, b in zip(sizes, full))
    if log2_blocks == 8 and min_count == 2:
        assert max(sizes) < max(full)                                   # a roomy sketch keeps singletons out of the batch tables


def test_min_mask_edges():
    rng = np.random.default_rng(4)
    keys = _multiset(rng, 300, 2000, 1)
    flags = np.full(len(keys), 3, np.uint8)
    s = sk.add(sk.new(6), keys, 6)
    assert (sk.min_mask(s, keys, flags, 6, 0, 1) == flags).all()        # a sketch that has seen the batch passes it at 1
    assert (sk.min_mask(s, keys, flags, 6, 0, 256) == 2).all()          # nothing reaches 256
    assert (sk.min_mask(sk.new(6), keys, flags, 6, 0, 1) == 2).all()    # an empty sketch passes nothing
