"""tests/color_np.py, the host reference of the coloured-table calls, pinned three ways without a GPU: on strings written out by hand,
against a second implementation (numpy bit unpacking and B.T @ B for the matrix; one key set per colour and windows spelled from
the strings for the rows), and on the identities that follow from the rule of include/kmx.h.  ColorMatrix.jaccard / containment of
kmers_amd.api are checked here on host tensors."""
import numpy as np
import pytest

from tests.color_np import (RC_ALL, RC_ANY, RC_BEST, RC_N_HIT, RC_N_SWITCH, RC_N_UNIQUE, RC_N_VALID, RC_THRESH, color_dict, color_matrix,
                            color_matrix_fast, interesting, read_colors, window_masks)
from tests.correct_np import canonical_of, count_kmers, dict_count, revcomp_bytes
from tests.count_np import random_reads


def _arr(s):
    return np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), np.uint8)


# ---------------------------------------------------------------- by hand
# Three genomes of 22 bases that share the 12 bases S: 18 windows each at k = 5, the 8 windows inside S in all three, the 10 that
# touch a private base (the four across the junction among them) in one.
K = 5
S = "ACGGTCATTGCA"
GENOMES = ["GGAGCTAAGC" + S, "TTCCGATAGA" + S, S + "CCTGAAGTAC"]


def _hand_table():
    return color_dict([count_kmers(_arr(g), 1, len(g), K) for g in GENOMES])


def test_by_hand_table_and_matrix():
    table = _hand_table()
    assert len(table) == 38 and sorted(table.values()).count(7) == 8
    for g, bit in zip(GENOMES, (1, 2, 4)):
        assert sum(1 for m in table.values() if m == bit) == 10
    assert all(table[canonical_of(S[i:i + K], K)] == 7 for i in range(8))
    matrix, spectrum = color_matrix(table.values(), 3)
    assert matrix.tolist() == [[18, 8, 8], [8, 18, 8], [8, 8, 18]] and spectrum.tolist() == [0, 30, 0, 8]
    # two colours only: the third genome's private k-mers have no colour left -- bin 0 -- and the shared ones have two
    matrix, spectrum = color_matrix(table.values(), 2)
    assert matrix.tolist() == [[18, 8], [8, 18]] and spectrum.tolist() == [10, 20, 8]


@pytest.mark.parametrize("read, row, hits", [
    # inside the shared part: four windows, all three colours in each
    ("GGTCATTG", (4, 4, 0, 7, 7, 7, (4 << 32) | 0, 0), (4, 4, 4)),
    # private to genome 1
    ("CCGATAGA", (4, 4, 4, 2, 2, 2, (4 << 32) | 1, 0), (0, 4, 0)),
    # genome 0 across its junction into S: six windows hold a private base (colour 0 alone), the last two lie in S: one switch;
    # colour 0 is in all 8 windows, colours 1 and 2 in 2 of 8 -- below one half
    ("CTAAGCACGGTC", (8, 8, 6, 1, 7, 1, (8 << 32) | 0, 1), (8, 2, 2)),
    # an N: only the last window is valid, genome 2's junction "GCACC"
    ("TCATNGCACC", (1, 1, 1, 4, 4, 4, (1 << 32) | 2, 0), (0, 0, 1)),
    # nothing of it in any genome
    ("GTACGTAC", (4, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0)),
    # shorter than k
    ("ACGG", (0, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0)),
])
def test_by_hand_reads(read, row, hits):
    table = _hand_table()
    # (the other strand gives the same row: the windows come in reverse order; revcomp_bytes spells ACGT only, so not for the N)
    for s in (_arr(read), _arr(read.lower())) + (() if "N" in read else (revcomp_bytes(_arr(read)),)):
        rows, h = read_colors(s, 1, len(s), K, dict_count(table), 3, (1, 2))
        assert tuple(int(x) for x in rows[0]) == row and tuple(int(x) for x in h[0]) == hits


def test_by_hand_masked_and_thresholds():
    table = _hand_table()
    read = _arr("CTAAGCACGGTC")
    mask_of = dict_count(table)
    # one colour: the windows are all hits still, with the one colour; nothing switches
    rows, h = read_colors(read, 1, len(read), K, mask_of, 1, (1, 2))
    assert [int(x) for x in rows[0]] == [8, 8, 8, 1, 1, 1, 8 << 32, 0] and h.tolist() == [[8]]
    # the private read of genome 1 under one colour: valid windows, no hit
    rows, _ = read_colors(_arr("CCGATAGA"), 1, 8, K, mask_of, 1, (1, 2))
    assert [int(x) for x in rows[0]] == [4, 0, 0, 0, 0, 0, 0, 0]
    for thr, want in (((0, 1), 7), ((1, 4), 7), ((1, 2), 1), ((2, 3), 1), ((1, 1), 1)):
        rows, _ = read_colors(read, 1, len(read), K, mask_of, 3, thr)
        assert int(rows[0, RC_THRESH]) == want, thr
    # a switch needs two neighbouring hit windows: an absent window between them separates them
    table2 = dict(table)
    del table2[canonical_of("CACGG", K)]          # the read's last window with colour 0 alone
    rows, _ = read_colors(read, 1, len(read), K, dict_count(table2), 3, (1, 2))
    assert int(rows[0, RC_N_HIT]) == 7 and int(rows[0, RC_N_SWITCH]) == 0
    # two reads: the last window of the first (colour 0) and the first of the second (all three) are no pair
    two = np.concatenate([_arr("GGAGCTAAGC"), _arr("ACGGTCATTG")])
    rows, _ = read_colors(two, 2, 10, K, mask_of, 3, (1, 2))
    assert rows[:, RC_N_SWITCH].tolist() == [0, 0] and rows[:, RC_ALL].tolist() == [1, 7]


# ---------------------------------------------------------------- a second implementation
def _samples(rng, k, n_samples, size=900):
    """sample tables cut from overlapping stretches of one genome, either strand, plus a private stretch each"""
    genome = random_reads(rng, size)
    samples, seqs = [], []
    for i in range(n_samples):
        a = int(rng.integers(0, size // 2))
        b = a + int(rng.integers(size // 8, size // 2))
        s = np.concatenate([genome[a:b], random_reads(rng, 2 * k)])
        if i % 2:
            s = revcomp_bytes(s).copy()
        seqs.append(s)
        samples.append(count_kmers(s, 1, len(s), k))
    return genome, seqs, samples


def _reads(rng, genome, seqs, L, n):
    out = []
    for r in range(n):
        kind = r % 5
        if kind == 0:
            a = int(rng.integers(0, len(genome) - L + 1))
            s = genome[a:a + L].copy()
        elif kind == 1:
            q = seqs[r % len(seqs)]
            a = int(rng.integers(0, max(len(q) - L, 0) + 1))
            s = np.resize(q[a:a + L], L).copy()
        elif kind == 2:                              # a chimera of two samples
            q, p = seqs[r % len(seqs)], seqs[(r + 1) % len(seqs)]
            s = np.concatenate([q[-(L // 2):], p[:L - L // 2]])
            s = np.resize(s, L).copy()
        elif kind == 3:
            s = random_reads(rng, L)
        else:
            a = int(rng.integers(0, len(genome) - L + 1))
            s = genome[a:a + L].copy()
            s[int(rng.integers(0, L))] = ord("N")
            s[rng.random(L) < 0.3] |= 0x20
        out.append(s)
    return np.concatenate(out)


def _second_rows(host, n, L, k, samples, n_colors, thr):
    """per colour a key set and the windows spelled from the string: presence[c][w], and everything from that array"""
    rows, hits = [], []
    sets = [set(s) for s in samples[:n_colors]]
    for r in range(n):
        read = bytes(host[r * L:(r + 1) * L])
        nw = max(len(read) - k + 1, 0)
        valid = [all(c in b"ACGTacgt" for c in read[w:w + k]) for w in range(nw)]
        P = np.zeros((n_colors, nw), bool)
        for w in range(nw):
            if valid[w]:
                key = canonical_of(read[w:w + k], k)
                for c in range(n_colors):
                    P[c, w] = key in sets[c]
        hit = P.any(axis=0) if nw else np.zeros(0, bool)
        h = P.sum(axis=1)
        nv = int(sum(valid))
        all_ = sum(1 << c for c in range(n_colors) if hit.any() and P[c, hit].all())
        any_ = sum(1 << c for c in range(n_colors) if h[c] > 0)
        thresh = sum(1 << c for c in range(n_colors) if h[c] > 0 and h[c] * thr[1] >= thr[0] * nv)
        best = (int(h.max()) << 32) | int(np.argmax(h)) if hit.any() else 0
        sw = sum(1 for w in range(nw - 1) if hit[w] and hit[w + 1] and (P[:, w] != P[:, w + 1]).any())
        uniq = int((hit & (P.sum(axis=0) == 1)).sum()) if nw else 0
        rows.append([nv, int(hit.sum()), uniq, all_, any_, thresh, best, sw])
        hits.append([int(x) for x in h])
    return np.array(rows, np.uint64).reshape(n, 8), np.array(hits, np.uint32).reshape(n, n_colors)


@pytest.mark.parametrize("k, n_samples, n_colors", [(11, 5, 5), (15, 5, 5), (15, 5, 3), (31, 4, 4), (47, 5, 2)])
def test_rows_against_a_second_implementation(k, n_samples, n_colors):
    rng = np.random.default_rng(700 + k + n_colors)
    genome, seqs, samples = _samples(rng, k, n_samples)
    table = color_dict(samples)
    n, L = 40, k + 70
    host = _reads(rng, genome, seqs, L, n)
    seen = {}
    for thr in ((0, 1), (1, 2), (2, 3), (1, 1)):
        rows, hits = read_colors(host, n, L, k, dict_count(table), n_colors, thr)
        rows2, hits2 = _second_rows(host, n, L, k, samples, n_colors, thr)
        assert (rows == rows2).all(), (thr, np.nonzero((rows != rows2).any(axis=1))[0][:5])
        assert (hits == hits2).all()
        for key, v in interesting(rows).items():
            seen[key] = seen.get(key, False) or v
    assert all(seen.values()), seen


@pytest.mark.parametrize("n_colors", (1, 2, 7, 8, 9, 33, 64))
def test_matrix_against_bit_unpacking(n_colors):
    rng = np.random.default_rng(800 + n_colors)
    masks = rng.integers(0, 2**64, 500, dtype=np.uint64)
    masks[::7] &= np.uint64(0x8000000000000001)
    masks[::11] = 0
    B = ((masks[:, None] >> np.arange(n_colors, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int64)
    matrix, spectrum = color_matrix(masks.tolist(), n_colors)
    assert (matrix.astype(np.int64) == B.T @ B).all()
    assert (spectrum.astype(np.int64) == np.bincount(B.sum(axis=1), minlength=n_colors + 1)).all()
    fast = color_matrix_fast(masks, n_colors)
    assert (fast[0] == matrix).all() and (fast[1] == spectrum).all() and fast[0].dtype == np.uint64
    # the identities: the diagonal is the sizes, the spectrum counts every entry once, and its first moment is the trace
    assert (np.diagonal(matrix).astype(np.int64) == B.sum(axis=0)).all()
    assert int(spectrum.sum()) == len(masks)
    assert sum(j * int(x) for j, x in enumerate(spectrum)) == int(np.trace(matrix))


# ---------------------------------------------------------------- identities
@pytest.mark.parametrize("k", (13, 33))
def test_identities(k):
    rng = np.random.default_rng(900 + k)
    genome, seqs, samples = _samples(rng, k, 6)
    table = color_dict(samples)
    n, L, nc = 50, k + 80, 6
    host = _reads(rng, genome, seqs, L, n)
    mask_of = dict_count(table)
    rows, hits = read_colors(host, n, L, k, mask_of, nc, (1, 2))
    r = rows.astype(object)
    assert all(int(a) & ~int(b) == 0 for a, b in zip(r[:, RC_ALL], r[:, RC_ANY]))
    assert (rows[:, RC_N_UNIQUE] <= rows[:, RC_N_HIT]).all() and (rows[:, RC_N_HIT] <= rows[:, RC_N_VALID]).all()
    any_rows, _ = read_colors(host, n, L, k, mask_of, nc, (0, 1))
    assert (any_rows[:, RC_THRESH] == rows[:, RC_ANY]).all()
    full, _ = read_colors(host, n, L, k, mask_of, nc, (1, 1))
    every = rows[:, RC_N_HIT] == rows[:, RC_N_VALID]
    assert every.any() and (~every).any()
    assert (full[every, RC_THRESH] == rows[every, RC_ALL]).all() and (full[~every, RC_THRESH] == 0).all()
    for i in range(n):
        _, masks = window_masks(host[i * L:(i + 1) * L], k, mask_of, nc)
        assert int(hits[i].sum()) == sum(bin(m).count("1") for m in masks)
    assert ((rows[:, RC_BEST] >> np.uint64(32)) == hits.max(axis=1)).all()
    assert all(interesting(rows).values())


# ---------------------------------------------------------------- ColorMatrix on host tensors
def test_color_matrix_measures_on_host_tensors():
    import torch

    from kmers_amd.api import ColorMatrix

    table = _hand_table()
    matrix, spectrum = color_matrix(table.values(), 3)
    m = ColorMatrix(torch.from_numpy(matrix.astype(np.int64)), torch.from_numpy(spectrum.astype(np.int64)))
    assert m.sizes.tolist() == [18, 18, 18]
    j, c = m.jaccard(), m.containment()
    assert j.dtype == torch.float64 and c.dtype == torch.float64 and j.shape == (3, 3) and c.shape == (3, 3)
    assert torch.equal(j, torch.tensor([[1.0, 8 / 28, 8 / 28], [8 / 28, 1.0, 8 / 28], [8 / 28, 8 / 28, 1.0]], dtype=torch.float64))
    assert torch.equal(c, torch.tensor([[1.0, 8 / 18, 8 / 18], [8 / 18, 1.0, 8 / 18], [8 / 18, 8 / 18, 1.0]], dtype=torch.float64))
    # containment is not symmetric, and an empty sample gives 0 everywhere, as _ratio does
    m = ColorMatrix(torch.tensor([[4, 2, 0], [2, 10, 0], [0, 0, 0]]))
    assert m.spectrum is None
    assert m.containment().tolist() == [[1.0, 0.5, 0.0], [0.2, 1.0, 0.0], [0.0, 0.0, 0.0]]
    assert m.jaccard().tolist() == [[1.0, 2 / 12, 0.0], [2 / 12, 1.0, 0.0], [0.0, 0.0, 0.0]]
