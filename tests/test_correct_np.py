"""The host reference of kmx_count_correct_reads(2) (tests/correct_np.py) pinned on strings, without a GPU: what the rule of
include/kmx.h says about an isolated substitution, the read's two ends, two errors close together, two fixing bases, N bytes, lower
case, solid_min == 0 and an empty table -- and the rolling implementation against one that spells every window afresh.  One
end-to-end case on the reference alone: reads with 1 % substitutions against their own count table."""
import numpy as np
import pytest

from tests.correct_np import (brute_correct, canonical_of, correct_reads, count_kmers, dict_count, revcomp_bytes, table_arrays, windows_of,
                              word_of)

K = 11


def _genome(seed, n):
    return np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", np.uint8), n).astype(np.uint8)


def _table(seqs, k, count=5):
    t = {}
    for s in seqs:
        for w in range(len(s) - k + 1):
            t[canonical_of(bytes(s[w:w + k]), k)] = count
    return t


def _other(c, step=1):
    return b"ACGT"[(b"ACGT".index(c & 0xDF) + step) % 4]


def _run(read, table, k=K, solid_min=3, min_cover=1):
    read = np.frombuffer(bytes(read), np.uint8)
    out, rows = correct_reads(read, 1, len(read), k, dict_count(table), solid_min, min_cover)
    assert (bytes(out), tuple(int(x) for x in rows[0])) == brute_correct(read, k, dict_count(table), solid_min, min_cover)
    return bytes(out), tuple(int(x) for x in rows[0])


@pytest.fixture(scope="module")
def g():
    genome = _genome(11, 400)
    return genome, _table([genome], K)


def test_words():
    assert word_of("ACGT", 4) == 0 | 1 << 2 | 2 << 4 | 3 << 6
    assert canonical_of("ACGT", 4) == word_of("ACGT", 4)                      # its own reverse complement
    assert canonical_of("TTTT", 4) == 0
    fw, rc, valid = windows_of(np.frombuffer(b"ACGTNacg", np.uint8), 3)
    assert valid.tolist() == [True, True, False, False, False, True]
    assert fw[0] == word_of("ACG", 3) and rc[0] == word_of("CGT", 3) and fw[5] == word_of("ACG", 3)


def test_isolated_substitution_is_restored(g):
    genome, table = g
    clean = bytes(genome[100:180])
    read = bytearray(clean)
    read[40] = _other(read[40])
    out, row = _run(read, table)
    assert out == clean and row == (K, 1, 1, 0)
    assert _run(clean, table) == (clean, (0, 0, 0, 0))


def test_read_ends_need_min_cover_1(g):
    genome, table = g
    clean = bytes(genome[100:180])
    for p in (0, len(clean) - 1):
        read = bytearray(clean)
        read[p] = _other(read[p])
        assert _run(read, table, min_cover=1) == (clean, (1, 1, 1, 0))
        assert _run(read, table, min_cover=2) == (bytes(read), (1, 0, 0, 0))


def test_two_errors_closer_than_k_are_left_and_k_apart_restored(g):
    genome, table = g
    clean = bytes(genome[100:180])
    near = bytearray(clean)
    near[30] = _other(near[30])
    near[30 + K - 1] = _other(near[30 + K - 1])
    out, row = _run(near, table)
    assert out == bytes(near) and row[1] >= 2 and row[2:] == (0, 0)           # candidates, nothing fixes
    far = bytearray(clean)
    far[30] = _other(far[30])
    far[30 + K] = _other(far[30 + K])
    out, row = _run(far, table)
    # (the K - 1 bases between the two see weak windows only -- the left error's up to its own window, the right one's from there --
    # so they are candidates as well, and nothing fixes them)
    assert out == clean and row == (2 * K, K + 1, 2, 0)


def test_two_fixing_bases_are_ambiguous(g):
    genome, _ = g
    variant = genome.copy()
    variant[140] = _other(variant[140])
    table = _table([genome, variant], K)
    read = bytearray(genome[100:180])
    read[40] = _other(read[40], 2)                                            # neither the genome's base nor the variant's
    out, row = _run(read, table)
    assert out == bytes(read) and row == (K, 1, 0, 1)


def test_n_is_never_replaced_and_its_windows_do_not_cover(g):
    genome, table = g
    clean = bytearray(genome[100:180])
    clean[43] = ord("N")
    read = bytearray(clean)
    read[40] = _other(read[40])
    # the windows that cover base 40 and hold no N: 30 .. 32
    out, row = _run(read, table, min_cover=3)
    assert out == bytes(clean) and row == (3, 1, 1, 0)
    out, row = _run(read, table, min_cover=4)
    assert out == bytes(read) and row == (3, 0, 0, 0)
    # an N no window of the table explains stays an N
    alone = bytearray(genome[100:180])
    alone[20] = ord("N")
    assert _run(alone, table)[0] == bytes(alone)


def test_lowercase_stays_lowercase(g):
    genome, table = g
    clean = bytes(genome[100:180]).lower()
    read = bytearray(clean)
    read[40] = _other(read[40]) | 0x20
    out, row = _run(read, table)
    assert out == clean and row == (K, 1, 1, 0)
    mixed = bytearray(bytes(genome[100:180]))
    mixed[40] = _other(mixed[40]) | 0x20                                      # a lowercase error among uppercase bases
    want = bytearray(genome[100:180])
    want[40] |= 0x20
    assert _run(mixed, table)[0] == bytes(want)


def test_solid_min_0_and_empty_table_give_the_input_back(g):
    genome, table = g
    read = bytearray(genome[100:180])
    read[40] = _other(read[40])
    read[60] = ord("N")
    assert _run(read, table, solid_min=0) == (bytes(read), (0, 0, 0, 0))
    out, row = _run(read, {}, solid_min=1)
    n_valid = 80 - K + 1 - K
    assert out == bytes(read) and row == (n_valid, 79, 0, 0)                  # every base but the N is a candidate; nothing fixes
    # membership: a key with count 0 is still a member; with counts it reads as absent
    zero = {key: 0 for key in table}
    out, _ = correct_reads(np.frombuffer(bytes(read), np.uint8), 1, 80, K, dict_count(zero, membership=True), 1, 1)
    assert bytes(out)[40] == genome[140] and correct_reads(np.frombuffer(bytes(read), np.uint8), 1, 80, K, dict_count(zero), 1, 1)[1][0, 2] == 0


def test_reads_without_a_window_are_copied_through():
    host = np.frombuffer(b"ACGTACGTAC", np.uint8)
    out, rows = correct_reads(host, 2, 5, 6, dict_count({}), 1, 1)
    assert (out == host).all() and (rows == 0).all()
    offsets = np.array([2, 2, 5, 10], np.uint64)                              # an empty read, a short one, one of 5 bases
    out, rows = correct_reads(host, 3, 0, 5, dict_count({}), 1, 1, offsets=offsets)
    assert (out == host).all() and rows.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [1, 5, 0, 0]]


@pytest.mark.parametrize("k", (1, 2, 3, 8, 33))
def test_rolling_reference_against_the_spelled_one(k):
    """dense tables at small k: ambiguous positions and wrong repairs happen, and both implementations agree on all of them"""
    rng = np.random.default_rng(500 + k)
    genome = _genome(600 + k, 300)
    table = {key: 5 for key in count_kmers(genome, 1, len(genome), k)}
    for key in list(table)[::9]:
        table[key] = 1
    seen = np.zeros(4, np.int64)
    for _ in range(12):
        L = int(rng.integers(max(k - 1, 1), k + 70))
        a = int(rng.integers(0, len(genome) - L))
        read = genome[a:a + L].copy()
        for p in np.nonzero(rng.random(L) < 0.05)[0]:
            read[p] = _other(read[p], int(rng.integers(1, 4)))
        if rng.random() < 0.3:
            read[int(rng.integers(0, L))] = ord("N")
        read[rng.random(L) < 0.2] |= 0x20
        read[read == (ord("N") | 0x20)] = ord("N")
        for mc in (1, min(2, k), k):
            out, rows = correct_reads(read, 1, L, k, dict_count(table), 2, mc)
            assert (bytes(out), tuple(int(x) for x in rows[0])) == brute_correct(read, k, dict_count(table), 2, mc), (k, L, mc)
            seen += rows[0].astype(np.int64)
    assert seen[1] > 0
    if k in (2, 3):
        assert seen[3] > 0, seen                                              # AMBIGUOUS occurs where the table is dense
    if k == 8:
        assert seen[2] > 0, seen                                              # ... and CORRECTED beside it


def test_table_arrays_order():
    t = {5: 1, (1 << 64) + 2: 3, 7: 2, (1 << 65): 9}
    tk, tc = table_arrays(t, 40)
    assert tk.tolist() == [[5, 0], [7, 0], [2, 1], [0, 2]] and tc.tolist() == [1, 2, 3, 9]
    tk, tc = table_arrays({9: 1, 3: 4}, 31)
    assert tk.tolist() == [3, 9] and tc.tolist() == [4, 1]


@pytest.mark.parametrize("k,L,share", ((15, 100, 0.5), (31, 100, 0.5), (47, 150, 1 / 3)))
def test_end_to_end_on_reads_against_their_own_table(k, L, share):
    """random genome of 3 000 bases, 1 200 reads from both strands, 1 % substitutions, an N in 5 % of the reads, table = the counts
    of the reads themselves, solid_min = 3: no base that agrees with the genome is changed, and at least `share` of the planted
    errors are restored (a CPU model of the rule gave 78 % at k = 15, 59 % at k = 31, 44 % at k = 47 on 150-base reads)"""
    rng = np.random.default_rng(2024)
    genome = _genome(2025, 3000)
    n = 1200
    truth = np.zeros((n, L), np.uint8)
    for r in range(n):
        a = int(rng.integers(0, len(genome) - L + 1))
        s = genome[a:a + L]
        truth[r] = revcomp_bytes(s) if rng.random() < 0.5 else s
    reads = truth.copy()
    err = rng.random((n, L)) < 0.01
    step = rng.integers(1, 4, (n, L))
    for r, p in zip(*np.nonzero(err)):
        reads[r, p] = _other(truth[r, p], int(step[r, p]))
    for r in np.nonzero(rng.random(n) < 0.05)[0]:
        p = int(rng.integers(0, L))
        reads[r, p] = ord("N")
        err[r, p] = False
    host = reads.reshape(-1)
    table = count_kmers(host, n, L, k)
    out, rows = correct_reads(host, n, L, k, dict_count(table), 3, 1)
    out = out.reshape(n, L)
    changed = out != reads
    assert int(rows[:, 2].sum()) == int(changed.sum())
    assert not (changed & ~err).any(), "a base that agreed with the genome was changed"
    restored = int((changed & err & (out == truth)).sum())
    broken = int((changed & (out != truth)).sum())
    planted = int(err.sum())
    print(f"k={k}: planted {planted}, restored {restored} ({restored / planted:.0%}), changed to a wrong base {broken}")
    assert broken == 0
    assert restored >= share * planted, (restored, planted)
