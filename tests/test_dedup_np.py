"""The host reference of kmx_reads_dedup (tests/dedup_np.py) against the contract's known answers and against a plain dictionary
dedup of canonical strings.  CPU only."""
import random

import numpy as np
import pytest

from tests import dedup_np as D


def test_known_answers():
    assert D.H(D.codes(b"")) == 0
    assert D.H(D.codes(b"A")) == 0xFDFDC5956C0F97B4
    assert D.H(D.codes(b"ACGTN")) == 0x63CB9B87BB1D059B
    assert D.H(D.codes(b"ACGTTGCAAC")) == 0x1F145D7BE7DA15F5
    assert D.H(D.rc(D.codes(b"ACGTTGCAAC"))) == 0x80BFCD5CD92DDA4A
    assert D.H(D.rc(D.codes(b"ACGT"))) == D.H(D.codes(b"ACGT"))


def test_rc_is_the_reverse_complement():
    assert D.rc(D.codes(b"AACGN")) == D.codes(b"NCGTT")
    assert D.codes(D.revcomp_bytes(b"AaCgTNx")) == D.rc(D.codes(b"AaCgTNx"))


def test_hash_ignores_case_and_takes_other_bytes_as_one_letter():
    assert D.H(D.codes(b"acgtTGCAac")) == D.H(D.codes(b"ACGTTGCAAC"))
    assert D.H(D.codes(b"ACNGT")) == D.H(D.codes(b"AC.GT")) == D.H(D.codes(b"ACxGT"))
    assert D.H(D.codes(b"ACNGT")) != D.H(D.codes(b"ACAGT"))


def test_hash_does_not_depend_on_where_the_read_lies():
    # the reference sees a read as a sequence: the same bytes cut out of a buffer at every shift are the same read
    read = bytes(random.Random(5).choice(b"ACGTN") for _ in range(41))
    want = D.H(D.codes(read))
    for shift in range(4):
        buf = np.frombuffer(b"." * shift + read + b"..", np.uint8)
        assert D.H(D.codes(buf[shift:shift + len(read)].tobytes())) == want
    # and the length is part of it: a prefix, or a read padded with the pad code's letter, is another read
    assert D.H(D.codes(read[:-1])) != want


def _batch(rng, n, strand_copies):
    """reads of mixed lengths with N, exact copies, copies in the other case, other-strand copies and near misses"""
    base = [bytes(rng.choice(b"ACGT" if rng.random() < 0.9 else b"N") for _ in range(rng.choice([0, 1, 3, 4, 5, 30, 31, 64, 65]))) for _ in range(n)]
    out = []
    for r in base:
        out.append(r)
        pick = rng.random()
        if pick < 0.3:
            out.append(r.lower())
        elif pick < 0.5 and strand_copies:
            out.append(D.revcomp_bytes(r))
        elif pick < 0.7 and r:
            i = rng.randrange(len(r))
            out.append(r[:i] + (b"A" if r[i:i + 1] != b"A" else b"C") + r[i + 1:])
        elif pick < 0.8 and r:
            out.append(r[:-1])
    rng.shuffle(out)
    return out


def _distinct_contents_have_distinct_keys(reads, mates, strand):
    rows, _, _ = D.dedup(reads, mates, strand)
    by_key = {}
    for r in range(len(reads)):
        by_key.setdefault(int(rows[r, D.HASH]), set()).add(D.canonical_string(reads[r], None if mates is None else mates[r], strand))
    return all(len(v) == 1 for v in by_key.values())


@pytest.mark.parametrize("strand", [False, True])
def test_singles_equal_a_dictionary_dedup(strand):
    reads = _batch(random.Random(11), 400, strand)
    assert _distinct_contents_have_distinct_keys(reads, None, strand)
    rows, keep, summary = D.dedup(reads, None, strand)
    assert np.array_equal(keep, D.dict_dedup(reads, None, strand))
    assert int(summary[D.S_COLLISIONS]) == 0 and int(summary[D.S_KEPT]) + int(summary[D.S_DROPPED]) == len(reads)
    assert int(rows[:, D.COUNT].sum()) == len(reads)


@pytest.mark.parametrize("strand", [False, True])
def test_pairs_equal_a_dictionary_dedup(strand):
    rng = random.Random(12)
    pool = _batch(rng, 60, False)
    reads, mates = [], []
    for _ in range(500):
        a, b = rng.choice(pool), rng.choice(pool)
        reads.append(a)
        mates.append(b)
        if rng.random() < 0.3:   # the same fragment from the other strand: the mates exchanged
            reads.append(b)
            mates.append(a)
    assert _distinct_contents_have_distinct_keys(reads, mates, strand)
    _, keep, summary = D.dedup(reads, mates, strand)
    assert np.array_equal(keep, D.dict_dedup(reads, mates, strand))
    assert int(summary[D.S_COLLISIONS]) == 0


@pytest.mark.parametrize("strand", [False, True])
@pytest.mark.parametrize("pairs", [False, True])
def test_few_hash_bits_never_drop_a_read_without_an_equal(strand, pairs):
    rng = random.Random(13)
    reads = _batch(rng, 300, strand)
    mates = [rng.choice(reads[:20]) for _ in reads] if pairs else None
    rows, keep, summary = D.dedup(reads, mates, strand, hash_bits=4)
    n = len(reads)
    assert int(summary[D.S_KEPT]) + int(summary[D.S_DROPPED]) == n
    assert int(summary[D.S_COLLISIONS]) > 0
    canon = [D.canonical_string(reads[r], None if mates is None else mates[r], strand) for r in range(n)]
    for r in range(n):
        if not keep[r]:
            rep = int(rows[r, D.REP])
            assert rep != r and keep[rep] and canon[rep] == canon[r]
    # an item without an equal is kept
    once = {c for c in canon if canon.count(c) == 1}
    assert all(keep[r] for r in range(n) if canon[r] in once)


def test_score_picks_the_head_and_ties_go_to_the_smaller_index():
    reads = [b"ACGTA", b"ACGTA", b"ACGTA", b"TTTT", b"ACGTA"]
    rows, keep, summary = D.dedup(reads, score=[1, 7, 7, 0, 2**40])
    assert list(keep) == [0, 0, 0, 1, 1] and int(rows[0, D.REP]) == 4 and int(rows[4, D.COUNT]) == 4
    rows, keep, _ = D.dedup(reads, score=[1, 7, 7, 0, 3])
    assert list(keep) == [0, 1, 0, 1, 0] and int(rows[2, D.REP]) == 1
    # scores saturate at 2^32 - 1: above it they tie
    _, keep, _ = D.dedup(reads, score=[2**32 - 1, 0, 0, 0, 2**40])
    assert list(keep) == [1, 0, 0, 1, 0]
    assert list(summary) == [2, 3, 4, 0]
