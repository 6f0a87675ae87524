"""The host references of the count family's GPU tests (tests/count_np.py), pinned on the CPU.

table_of and host_lookup carry every exact u64 comparison those tests make, so they are checked here against brute force written in
this file: a collections.Counter over Python ints (one-word keys) or (high, low) tuples (two-word keys), sorted() for the order, a
dict for the lookup.  Python ints do not wrap and tuples compare high word first: neither can share a mistake with the numpy code.
The inputs are made by hand and small (at most 2,000 windows); each test asserts that its input holds the cases it is there for.
No GPU, no oracle, no library."""
import collections

import numpy as np
import pytest

from tests import count_np

M = 2**64 - 1
H = 2**63


# ---------------------------------------------------------------- brute force
def _keys_of(canon):
    """numpy canonical words -> Python ints, or (high, low) tuples of rows (low, high)"""
    return canon.tolist() if canon.ndim == 1 else [(hi, lo) for lo, hi in canon.tolist()]


def _brute_table(canon, flags):
    c = collections.Counter(key for key, f in zip(_keys_of(canon), flags.tolist()) if f & 1)
    keys = sorted(c)
    return keys, [c[key] for key in keys]


def _brute_lookup(keys, counts, queries, qflags=None):
    d = dict(zip(keys, counts if counts is not None else [1] * len(keys)))
    return [d.get(q, 0) if qflags is None or qflags[i] & 1 else 0 for i, q in enumerate(queries)]


def _as_array(keys, w):
    """Python keys -> the layout of a table: (n,) uint64, or (n, 2) rows (low, high)"""
    if w == 1:
        return np.array(keys, np.uint64).reshape(-1)
    return np.array([[lo, hi] for hi, lo in keys], np.uint64).reshape(-1, 2)


# ---------------------------------------------------------------- hand-made windows: (key, flag) pairs; bit 0 of a flag = valid
def _one_word_edges():
    valid = [0, M, H - 1, H, H + 1, 5, 5, 5, M, 0, H, 9, 6, 4]
    # invalid windows with the words of valid ones and with words of none; flag 3 is valid (bit 0 decides)
    return [(v, 1) for v in valid] + [(5, 0), (H, 2), (7, 0), (M - 1, 2), (9, 3)]


def _one_word_inner():
    """neither 0 nor 2^64 - 1: there are queries below the first key and above the last"""
    return [(v, 1) for v in (10, 12, H - 2, H + 2, M - 10, 12, H + 2, H + 2)] + [(11, 0), (0, 0), (M, 2)]


def _one_word_many():
    vals = [(i * 0x9E3779B97F4A7C15) % 2**64 for i in range(400)]                  # on both sides of 2^63
    return [(vals[(j * j) % 400], 0 if j % 7 == 0 else 1 + 2 * (j % 2)) for j in range(2000)]


def _two_word_edges():
    valid = [(0, 0), (M, M), (0, M), (M, 0), (H, H), (H, H - 1), (H - 1, H), (H - 1, H - 1),   # (high, low)
             (3, 5), (3, H - 1), (3, H + 1), (3, M),                                            # differ in the low word only
             (H, 5), (H + 1, 5), (M, 5),                                                        # ... (with (3, 5)) in the high word only
             (3, 5), (3, 5), (M, M), (0, 0), (H + 1, 5)]                                        # repeats
    return [(v, 1) for v in valid] + [((3, 5), 0), ((M, M), 2), ((3, 6), 0), ((4, 5), 2), ((H, H), 3)]


def _two_word_run():
    """320 keys under ONE high word above 2^63, their low words from 1000 up across 2^63, neighbours under the high words next to it;
    neither (0, 0) nor (2^64 - 1, 2^64 - 1)"""
    run = [(H + 7, 1000 + i * (M // 330)) for i in range(320)]
    win = [(key, 1) for i, key in enumerate(run) for _ in range(i % 3 + 1)]
    win += [((H + 6, lo), 1) for lo in (3, H, M)] + [((H + 8, lo), 1) for lo in (0, 1, H + 5)] + [((2, lo), 1) for lo in (H - 1, H, 77, 77)]
    win += [((H + 7, 999), 0), (run[5], 0), (run[300], 2), ((1, 1), 0)]
    return win


def _windows(pairs, w):
    keys = [key for key, _ in pairs]
    return _as_array(keys, w), np.array([f for _, f in pairs], np.uint8)


ONE_WORD = {"edges": _one_word_edges(), "inner": _one_word_inner(), "many": _one_word_many(),
            "all_invalid": [(5, 0), (H, 2), (0, 0), (M, 2)], "single": [(H, 1), (H, 3), (H, 0), (4, 0), (H, 1)]}
TWO_WORD = {"edges": _two_word_edges(), "run": _two_word_run(),
            "all_invalid": [((3, 5), 0), ((M, M), 2), ((0, 0), 0)], "single": [((H, H - 1), 1), ((H, H - 1), 1), ((H, H), 0), ((0, 0), 2)]}
CASES = [(1, name) for name in ONE_WORD] + [(2, name) for name in TWO_WORD]


def _case(w, name):
    return _windows((ONE_WORD if w == 1 else TWO_WORD)[name], w)


# ---------------------------------------------------------------- table_of
def test_the_inputs_hold_what_they_are_there_for():
    for w, cases in ((1, ONE_WORD), (2, TWO_WORD)):
        valid = {key for name in ("edges", "many", "run") for key, f in cases.get(name, ()) if f & 1}
        invalid = {key for name in ("edges", "many", "run") for key, f in cases.get(name, ()) if not f & 1}
        assert valid & invalid and invalid - valid                    # invalid windows with the word of a valid one, and with a word of none
        words = [x for key in valid for x in ((key,) if w == 1 else key)]
        assert {0, M, H - 1, H} <= set(words) and any(x < H for x in words) and any(x > H for x in words)
        assert all(len(pairs) <= 2000 for pairs in cases.values())
        assert any(len(pairs) > len({key for key, _ in pairs}) for pairs in cases.values())   # repeated keys
    keys = {key for key, f in TWO_WORD["edges"] if f & 1}
    assert any(a[0] == b[0] and a[1] != b[1] for a in keys for b in keys)     # two-word keys that differ in the low word only
    assert any(a[0] != b[0] and a[1] == b[1] for a in keys for b in keys)     # ... in the high word only
    # orders that a signed or a low-word-first comparison gets wrong
    assert any(a[0] < H <= b[0] for a in keys for b in keys) and any(a[0] == b[0] and a[1] < H <= b[1] for a in keys for b in keys)
    assert any(a[0] < b[0] and a[1] > b[1] for a in keys for b in keys)
    assert len({hi for (hi, _), f in TWO_WORD["run"] if f & 1 and hi == H + 7}) == 1
    assert len({lo for (hi, lo), f in TWO_WORD["run"] if f & 1 and hi == H + 7}) >= 300


@pytest.mark.parametrize("w,name", CASES)
def test_table_of(w, name):
    canon, flags = _case(w, name)
    keys, counts = _brute_table(canon, flags)
    tk, tc = count_np.table_of(canon, flags)
    assert tk.dtype == np.uint64 and tc.dtype == np.uint64
    assert tk.shape == ((len(keys),) if w == 1 else (len(keys), 2)) and tc.shape == (len(keys),)
    assert _keys_of(tk) == keys
    assert tc.tolist() == counts
    if name == "all_invalid":
        assert len(keys) == 0
    if name == "single":
        assert len(keys) == 1 and counts[0] > 1
    # the order of the windows does not matter
    back = count_np.table_of(canon[::-1], flags[::-1])
    assert back[0].tobytes() == tk.tobytes() and back[1].tobytes() == tc.tobytes()


# ---------------------------------------------------------------- host_lookup
def _queries(keys, w):
    """every key, its neighbours by one in each word, the ends of each word's range and of every run of equal high words"""
    if w == 1:
        q = set(keys) | {key + d for key in keys for d in (-1, 1)} | {0, 1, H - 1, H, M - 1, M}
        return sorted(x for x in q if 0 <= x <= M)
    q = set(keys) | {(0, 0), (0, M), (M, 0), (M, M), (H, H)}
    for hi, lo in keys:
        q |= {(hi, lo - 1), (hi, lo + 1), (hi - 1, lo), (hi + 1, lo), (hi, 0), (hi, M), (hi, lo ^ H)}
    return sorted(x for x in q if 0 <= x[0] <= M and 0 <= x[1] <= M)


@pytest.mark.parametrize("w,name", CASES)
def test_host_lookup(w, name):
    keys, counts = _brute_table(*_case(w, name))
    tk, tc = _as_array(keys, w), np.array(counts, np.uint64)
    queries = _queries(keys, w) if keys else _queries([5] if w == 1 else [(3, 5)], w)
    queries = queries + queries[::-3] + keys[:1] * 4                           # (not sorted, with repeats; a hit under every flag)
    q = _as_array(queries, w)
    qflags = (np.arange(len(queries)) % 4).astype(np.uint8)                    # 0 and 2: not valid, whatever the other bits say
    assert count_np.host_lookup(tk, tc, q).tolist() == _brute_lookup(keys, counts, queries)
    assert count_np.host_lookup(tk, tc, q, qflags).tolist() == _brute_lookup(keys, counts, queries, qflags.tolist())
    assert count_np.host_lookup(tk, None, q).tolist() == _brute_lookup(keys, None, queries)                   # membership: 1 / 0
    assert count_np.host_lookup(tk, None, q, qflags).tolist() == _brute_lookup(keys, None, queries, qflags.tolist())
    out = count_np.host_lookup(tk, tc, q[:0], qflags[:0])                      # no query
    assert out.shape == (0,) and out.dtype == np.uint64
    if not keys:                                                               # an empty table: every answer 0
        assert len(q) > 0 and not count_np.host_lookup(tk, tc, q, qflags).any()
        return
    # of the queries: hits, the first and the last key, misses between keys, hits that the flags clear
    hit = [x in set(keys) for x in queries]
    assert keys[0] in queries and keys[-1] in queries and any(hit)
    assert any(h and not f & 1 for h, f in zip(hit, qflags.tolist())) and any(h and f & 1 for h, f in zip(hit, qflags.tolist()))
    if len(keys) > 1:
        assert any(keys[0] < x < keys[-1] and not h for x, h in zip(queries, hit))
    if name in ("inner", "run", "single"):                                     # (tables that hold neither the least nor the greatest key)
        assert any(x < keys[0] for x in queries) and any(x > keys[-1] for x in queries)
    if w == 2:
        # a high word the table holds, the low word below, between and above the low words of that run
        runs = collections.defaultdict(list)
        for hi, lo in keys:
            runs[hi].append(lo)
        miss = [x for x, h in zip(queries, hit) if not h and x[0] in runs]
        assert any(lo < min(runs[hi]) for hi, lo in miss) and any(lo > max(runs[hi]) for hi, lo in miss)
        if name in ("edges", "run"):
            assert any(min(runs[hi]) < lo < max(runs[hi]) for hi, lo in miss)
        if name == "run":
            assert len(runs[H + 7]) >= 300                                     # more than a couple of bisection steps


def test_host_lookup_counts_past_bit_63():
    """the answer is the table's count, whatever its size"""
    tk = np.array([[7, 1], [H, 1], [0, 2]], np.uint64)
    tc = np.array([M, H, 1], np.uint64)
    q = np.array([[H, 1], [7, 1], [0, 2], [1, 2]], np.uint64)
    assert count_np.host_lookup(tk, tc, q).tolist() == [H, M, 1, 0]
    assert count_np.host_lookup(np.array([0, 7, H], np.uint64), tc, np.array([H, 7, 0, 1], np.uint64)).tolist() == [1, H, M, 0]


# ---------------------------------------------------------------- the read batches
def test_words():
    assert [count_np.words(k) for k in (1, 31, 33, 64)] == [1, 1, 2, 2]


def test_orc_windows_takes_the_oracle_call_of_the_width():
    class Orc:
        def canonical_windows(self, host, n, L, k, offsets=None):
            return None, None, [1, 2, 3], [1, 0, 1]

        def canonical_windows2(self, host, n, L, k, offsets=None):
            return None, None, [[1, 2], [3, 4]], [1, 0]

    for k, shape in ((31, (3,)), (33, (2, 2))):
        canon, flags = count_np.orc_windows(Orc(), None, 1, 40, k)
        assert canon.shape == shape and canon.dtype == np.uint64 and flags.dtype == np.uint8 and len(flags) == shape[0]


def test_random_reads():
    a = count_np.random_reads(np.random.default_rng(3), 5000)
    assert a.dtype == np.uint8 and a.shape == (5000,) and set(a.tolist()) == set(b"ACGT")
    assert a.tobytes() == count_np.random_reads(np.random.default_rng(3), 5000).tobytes()
    assert a.tobytes() != count_np.random_reads(np.random.default_rng(4), 5000).tobytes()
    assert count_np.random_reads(np.random.default_rng(3), 0).shape == (0,)


@pytest.mark.parametrize("share", (0.0, 0.1, 1.0))
def test_dirty(share):
    n, L = 400, 37
    host = count_np.random_reads(np.random.default_rng(5), n * L)
    before = host.copy()
    h = count_np.dirty(host, np.random.default_rng(6), share, n, L)
    assert host.tobytes() == before.tobytes()                                  # a copy: the input is left alone
    assert h.tobytes() == count_np.dirty(host, np.random.default_rng(6), share, n, L).tobytes()
    changed = (h != host).reshape(n, L)
    chosen = np.random.default_rng(6).random(n) < share                        # the first draw: which reads
    assert (changed.sum(axis=1) == chosen).all()                               # one byte of every chosen read, none of any other
    rows, cols = np.nonzero(changed)
    want = np.where(rows % 3 != 0, ord("N"), ord(">"))
    assert (h.reshape(n, L)[rows, cols] == want).all()
    if share == 0.1:
        assert 0 < len(rows) < n and len(set(want.tolist())) == 2 and len(set(cols.tolist())) > 10


def test_two_batches():
    n, L = 301, 50
    a, b = count_np.two_batches(np.random.default_rng(7), n, L)
    a2, b2 = count_np.two_batches(np.random.default_rng(7), n, L)
    assert a.tobytes() == a2.tobytes() and b.tobytes() == b2.tobytes()
    A, B = a.reshape(n, L), b.reshape(n, L)
    assert (B[::2] == A[::2]).all()                                            # every second read of B is A's
    assert not (B[1::2] == A[1::2]).all(axis=1).any()                          # and no other
    # A is the first draw of the stream, B's own reads the second
    rng = np.random.default_rng(7)
    assert a.tobytes() == count_np.random_reads(rng, n * L).tobytes()
    assert (B[1::2] == count_np.random_reads(rng, n * L).reshape(n, L)[1::2]).all()
