"""kmx_reads_dedup on the GPU (kmx_reads_dedup.hip) and what the Python layer builds on it (Context.reads_dedup,
reads_drop_duplicates).

Every comparison is equality, word for word, of the rows, the keep bytes and the summary with the host reference tests/dedup_np.py
(pinned against the contract's known answers and a dictionary dedup in tests/test_dedup_np.py): there is no tolerance anywhere.  The
raw call goes through `run`, which hands the ABI rows and keep bytes with sentinels on both sides, looks at them afterwards and
checks that the bases are what they were."""
import ctypes as C

import numpy as np
import pytest

from tests import dedup_np as D
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import u64
from tests.reads_dev import SENT, SENT_WORD, dev_bytes, dev_words, ptr, ragged

pytestmark = pytest.mark.gpu

OK, E_ARG, E_NOMEM = 0, 1, 6
GB, GW = 32, 8                                # sentinel bytes / words on either side of an output
STRAND = 1
RQ_WORDS = 8
LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025, 5000]


def seq(rng, n, p_n=0.0):
    s = rng.choice(np.frombuffer(b"ACGT", np.uint8), n).astype(np.uint8)
    if p_n:
        s[rng.random(n) < p_n] = ord("N")
    return s.tobytes()


def other_letter(b):
    return b"C" if b in b"Aa" else b"A"


def family(rng, L, shorter=True):
    """a read of L bases (an N in it from 3 bases on) with a copy, a copy with one substitution at the first, the middle and the last
    base, a copy one base shorter, a lower-case copy (equal) and a copy with another non-ACGT byte for every N (equal)"""
    r = bytearray(seq(rng, L, 0.03))
    if L >= 3:
        r[L // 3] = ord("N")
    r = bytes(r)
    out = [r, r]
    for i in sorted({0, L // 2, L - 1}) if L else []:
        out.append(r[:i] + other_letter(r[i:i + 1]) + r[i + 1:])
    if shorter and L:
        out.append(r[:-1])
    out += [r.lower(), r.replace(b"N", b".")]
    return out


def shuffled(rng, reads):
    return [reads[i] for i in rng.permutation(len(reads))]


class Guarded:
    """an output with sentinels on both sides"""

    def __init__(self, ctx, n, words):
        import torch

        self.g, self.n, self.words = (GW if words else GB), n, words
        self.buf = torch.full((2 * self.g + n,), SENT_WORD if words else SENT, dtype=torch.int64 if words else torch.uint8, device=ctx.device)
        self.sent = np.uint64(SENT_WORD & D.M64) if words else np.uint8(SENT)

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + self.g * (8 if self.words else 1))

    def host(self):
        h = self.buf.cpu().numpy()
        return h.view(np.uint64) if self.words else h

    def payload(self):
        """the n elements, after checking that nothing around them was written"""
        h = self.host()
        assert (h[:self.g] == self.sent).all() and (h[self.g + self.n:] == self.sent).all(), "written outside the output"
        return h[self.g:self.g + self.n]

    def untouched(self):
        return bool((self.host() == self.sent).all())


class Batch:
    """a list of reads on the device: uniform reads of `uniform` bases, or ragged with `first` bytes before the batch; `shift`: where
    d_bases lies on the dword grid"""

    def __init__(self, ctx, reads, uniform=None, first=5, shift=0):
        from kmers_amd._lib import Reads

        n = len(reads)
        if uniform is not None:
            assert all(len(r) == uniform for r in reads)
            self.host, off, self.read_len = np.frombuffer(b"".join(reads), np.uint8), None, uniform
        else:
            self.host, off = ragged(reads, first)
            self.read_len = max([len(r) for r in reads], default=0)
        self.dev = dev_bytes(ctx, self.host, shift)
        self.off = dev_words(ctx, off)
        self.reads = Reads(self.dev.data_ptr() if n else None, n, self.read_len, self.off.data_ptr() if off is not None else None)

    def unchanged(self):
        return len(self.host) == 0 or bool((self.dev.cpu().numpy()[:len(self.host)] == self.host).all())


def run(ctx, reads, mates=None, strand=False, score=None, stride=1, hash_bits=64, lay1=None, lay2=None, want=None):
    """kmx_reads_dedup through the raw ABI into guarded outputs, everything compared with the reference -> (rows, keep, summary)"""
    n = len(reads)
    if want is None:
        want = D.dedup(reads, mates, strand, score, hash_bits)
    w_rows, w_keep, w_sum = want
    b1 = Batch(ctx, reads, **(lay1 or {}))
    b2 = Batch(ctx, mates, **(lay2 or {})) if mates is not None else None
    d_score = None
    if score is not None:
        wide = np.full(max(n * stride, 1), 0x77, np.uint64)
        wide[:n * stride:stride] = np.asarray(score, np.uint64)
        d_score = dev_words(ctx, wide)
    g_rows, g_keep = Guarded(ctx, D.WORDS * n, True), Guarded(ctx, n, False)
    summ = (C.c_uint64 * 4)(77, 77, 77, 77)
    st = ctx.lib.kmx_reads_dedup(ctx._h, C.byref(b1.reads), C.byref(b2.reads) if b2 else None, STRAND if strand else 0, hash_bits, ptr(d_score),
                                 stride, g_rows.ptr(), g_keep.ptr(), summ)
    assert st == OK, ctx.lib.kmx_last_error(ctx._h)
    got = g_rows.payload().reshape(n, D.WORDS)
    bad = np.nonzero((got != w_rows).any(axis=1))[0]
    assert len(bad) == 0, ("rows", len(bad), int(bad[0]), [hex(v) for v in got[bad[0]].tolist()], [hex(v) for v in w_rows[bad[0]].tolist()])
    assert (g_keep.payload() == w_keep).all()
    assert list(summ) == [int(v) for v in w_sum], (list(summ), w_sum)
    assert b1.unchanged() and (b2 is None or b2.unchanged())
    return want


def canon(reads, mates, strand, r):
    return D.canonical_string(reads[r], None if mates is None else mates[r], strand)


def dropped_equal_their_rep(reads, mates, strand, rows, keep):
    for r in np.nonzero(keep == 0)[0]:
        rep = int(rows[r, D.REP])
        assert rep != r and keep[rep] and canon(reads, mates, strand, rep) == canon(reads, mates, strand, int(r))


# ---------------------------------------------------------------- lengths and layouts
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_ragged_lengths_at_every_alignment(ctx, shift):
    rng = np.random.default_rng(100 + shift)
    reads = shuffled(rng, [r for L in LENGTHS for r in family(rng, L)])
    rows, keep, summary = run(ctx, reads, lay1=dict(first=7, shift=shift))
    # per family: the copy, the lower-case copy and the other-byte copy go, the substitutions and the shorter read stay
    assert int(summary[D.S_COLLISIONS]) == 0 and int(summary[D.S_DROPPED]) >= 3 * len(LENGTHS)
    dropped_equal_their_rep(reads, None, False, rows, keep)


@pytest.mark.parametrize("L,shift", [(5, 0), (5, 1), (5, 3), (150, 0), (150, 2), (150, 3)])
def test_uniform_reads(ctx, L, shift):
    rng = np.random.default_rng(200 + L + shift)
    reads = shuffled(rng, [r for _ in range(40) for r in family(rng, L, shorter=False)])
    rows, keep, summary = run(ctx, reads, lay1=dict(uniform=L, shift=shift))
    assert int(summary[D.S_DROPPED]) >= 3 * 40
    dropped_equal_their_rep(reads, None, False, rows, keep)


# ---------------------------------------------------------------- the other strand
PALINDROMES = [b"ACGT", b"AATT" * 4, b"GAATTC", b"caTG", b"TA"]


@pytest.mark.parametrize("strand", [False, True])
@pytest.mark.parametrize("shift", [0, 1])
def test_reverse_complement_copies(ctx, strand, shift):
    rng = np.random.default_rng(300 + shift)
    originals = [seq(rng, L, 0.02) for L in (1, 3, 5, 7, 8, 9, 63, 64, 65, 150, 151, 257, 1025)]
    half = seq(rng, 33)
    palindromes = PALINDROMES + [half + D.revcomp_bytes(half)]
    assert all(D.rc(D.codes(p)) == D.codes(p) for p in palindromes)
    firsts = originals + palindromes   # (no original has the length of a palindrome or of another: no two of them are equal)
    # odd and even lengths back to back: an original and its copy lie at different places of the dword grid
    reads = firsts + [b"GGAGGAGGAGG"] + [D.revcomp_bytes(r) for r in firsts]
    rows, keep, _ = run(ctx, reads, strand=strand, lay1=dict(first=3, shift=shift))
    n0 = len(firsts)
    for i, r in enumerate(firsts):
        c = n0 + 1 + i
        if D.rc(D.codes(r)) == D.codes(r):   # the copy IS the original: it goes with or without the flag, and not as flipped
            assert keep[c] == 0 and int(rows[c, D.REP]) == i and not (int(rows[c, D.FLAGS]) & D.F_FLIPPED)
        elif strand:
            assert keep[c] == 0 and int(rows[c, D.REP]) == i and (int(rows[c, D.FLAGS]) & D.F_FLIPPED)
        else:
            assert keep[c] == 1


# ---------------------------------------------------------------- pairs
@pytest.mark.parametrize("strand", [False, True])
@pytest.mark.parametrize("swap", [False, True])
def test_pairs_in_two_layouts(ctx, strand, swap):
    rng = np.random.default_rng(400)
    L = 50
    m1, m2 = [], []

    def add(a, b):
        m1.append(a)
        m2.append(b)

    for L2 in (50, 50, 50, 0, 1, 30, 77, 300):
        a, b = seq(rng, L, 0.02), seq(rng, L2, 0.02)
        add(a, b)
        add(a.lower(), b)                               # equal
        add(a[:10] + other_letter(a[10:11]) + a[11:], b)   # mate 1 differs
        if L2:
            add(a, b[:-1] + other_letter(b[-1:]))       # mate 2 differs
            add(a, b[:-1])                              # mate 2 shorter
        if L2 == L:
            add(b, a)                                   # exchanged: the other strand of the fragment
            add(b.lower(), a)
    add(m1[0], m1[0])                                   # a pair of equal mates: F_a == F_b
    add(m1[0], m1[0])
    order = rng.permutation(len(m1))
    m1, m2 = [m1[i] for i in order], [m2[i] for i in order]
    lay_u, lay_r = dict(uniform=L, shift=1), dict(first=9, shift=2)
    if swap:
        rows, keep, _ = run(ctx, m2, m1, strand=strand, lay1=lay_r, lay2=lay_u)
        dropped_equal_their_rep(m2, m1, strand, rows, keep)
    else:
        rows, keep, _ = run(ctx, m1, m2, strand=strand, lay1=lay_u, lay2=lay_r)
        dropped_equal_their_rep(m1, m2, strand, rows, keep)
    flipped = int(np.count_nonzero(rows[:, D.FLAGS] & np.uint64(D.F_FLIPPED)))
    assert (flipped > 0) == strand


# ---------------------------------------------------------------- score
def test_best_score_survives_and_ties_go_to_the_smaller_index(ctx):
    rng = np.random.default_rng(500)
    a, b, c = seq(rng, 150), seq(rng, 150), seq(rng, 31)
    reads = [a, b, a, c, a, b, c, c, a.lower()]
    score = [3, 9, 8, 2**33, 8, 9, 2**32 - 1, 5, 1]
    rows, keep, _ = run(ctx, reads, score=score, stride=RQ_WORDS)
    # a: the first of the two 8s (index 2); b: a tie of 9s, index 1; c: 2^33 saturates and ties with 2^32 - 1, index 3
    assert list(keep) == [0, 1, 1, 1, 0, 0, 0, 0, 0]
    assert [int(v) for v in rows[:, D.REP]] == [2, 1, 2, 3, 2, 1, 3, 3, 2]
    run(ctx, reads, score=[0] * len(reads), stride=1, want=D.dedup(reads))   # all equal: the first occurrence, as without a score


# ---------------------------------------------------------------- collisions
def collision_batch(rng, n):
    base = [seq(rng, int(rng.integers(0, 40)), 0.03) for _ in range(n // 2)]
    half = seq(rng, 6)
    base += PALINDROMES + [half + D.revcomp_bytes(half)]
    reads = list(base)
    while len(reads) < n:
        r = base[int(rng.integers(len(base)))]
        pick = rng.random()
        reads.append(r if pick < 0.4 else D.revcomp_bytes(r) if pick < 0.8 else r.lower())
    return shuffled(rng, reads[:n])


@pytest.mark.parametrize("strand", [False, True])
@pytest.mark.parametrize("hash_bits", [1, 4, 8])
def test_few_hash_bits_collide_and_stay_exact(ctx, hash_bits, strand):
    rng = np.random.default_rng(600 + hash_bits)
    reads = collision_batch(rng, 3000)
    rows, keep, summary = run(ctx, reads, strand=strand, hash_bits=hash_bits, lay1=dict(first=1, shift=3))
    assert int(summary[D.S_COLLISIONS]) > 0
    assert int(rows[:, D.HASH].max()) < (1 << hash_bits)
    dropped_equal_their_rep(reads, None, strand, rows, keep)
    if strand:   # the orientation is ambiguous (F_a == F_b) for some item that is dropped as flipped, and for some dropped as it is
        flipped = (rows[:, D.FLAGS] & np.uint64(D.F_FLIPPED)) != 0
        assert flipped.any() and ((keep == 0) & ~flipped).any()


@pytest.mark.parametrize("hash_bits", [1, 4])
def test_few_hash_bits_on_pairs(ctx, hash_bits):
    rng = np.random.default_rng(650)
    pool = [seq(rng, int(rng.integers(0, 30)), 0.03) for _ in range(40)]
    m1 = [pool[int(i)] for i in rng.integers(0, 40, 3000)]
    m2 = [pool[int(i)] for i in rng.integers(0, 40, 3000)]
    rows, keep, summary = run(ctx, m1, m2, strand=True, hash_bits=hash_bits)
    assert int(summary[D.S_COLLISIONS]) > 0
    dropped_equal_their_rep(m1, m2, True, rows, keep)


# ---------------------------------------------------------------- one large class, more items than the grid has waves
def test_a_class_larger_than_a_leaf_among_many_reads(ctx):
    rng = np.random.default_rng(700)
    n_class, n_other = 20000, 50000
    others = rng.choice(np.frombuffer(b"ACGT", np.uint8), (n_other, 24)).astype(np.uint8)
    reads = [b"GATTA"] * n_class + [row.tobytes() for row in others]
    reads = shuffled(rng, reads)
    rows, keep, summary = run(ctx, reads, lay1=dict(first=2, shift=1))
    assert int(summary[D.S_LARGEST]) == n_class
    head = reads.index(b"GATTA")
    assert int(rows[head, D.COUNT]) == n_class and keep[head] == 1


# ---------------------------------------------------------------- other properties
def small_batch(seed=800):
    rng = np.random.default_rng(seed)
    return shuffled(rng, [r for L in (0, 5, 64, 150, 301) for r in family(rng, L)])


def test_repeated_calls_give_identical_bytes(ctx):
    reads = collision_batch(np.random.default_rng(810), 3000)
    want = D.dedup(reads, None, True, None, 6)
    for _ in range(2):
        run(ctx, reads, strand=True, hash_bits=6, want=want)


def test_second_context_and_borrowed_stream(ctx):
    import torch

    from kmers_amd.api import Context

    reads = small_batch()
    want = D.dedup(reads, None, True)
    stream = torch.cuda.Stream(device=ctx.device)
    other = Context(ctx.device, stream=stream)
    try:
        with torch.cuda.stream(stream):   # (the test's own tensors are made and read on the stream the call runs on)
            run(other, reads, strand=True, want=want)
            d = other.reads_dedup(*batch_args(other, reads), strand=True)
            assert (u64(d.rows) == want[0]).all() and (d.keep.cpu().numpy() == want[1]).all()
    finally:
        other.close()
    run(ctx, reads, strand=True, want=want)


def batch_args(ctx, reads, first=0):
    """(bases, n_reads, read_len, offsets) of a ragged batch for the Python layer"""
    host, off = ragged(reads, first)
    return ctx.to_device(host), len(reads), max([len(r) for r in reads], default=0), ctx.to_device(off)


def test_no_reads(ctx):
    from kmers_amd._lib import Reads

    g_rows = Guarded(ctx, 0, True)
    summ = (C.c_uint64 * 4)(77, 77, 77, 77)
    r = Reads(None, 0, 150, None)
    assert ctx.lib.kmx_reads_dedup(ctx._h, C.byref(r), None, 0, 64, None, 0, g_rows.ptr(), None, summ) == OK
    assert list(summ) == [0, 0, 0, 0] and g_rows.untouched()
    assert ctx.lib.kmx_reads_dedup(ctx._h, C.byref(r), None, 0, 65, None, 0, g_rows.ptr(), None, summ) == E_ARG   # (still checked)
    d = ctx.reads_dedup(ctx.empty(1, __import__("torch").uint8), 0, 0)
    assert (d.kept, d.dropped, d.largest, d.collisions) == (0, 0, 0, 0) and d.rows.shape == (0, 4) and d.keep.numel() == 0


def test_bad_arguments(ctx):
    from kmers_amd._lib import Reads

    reads = small_batch()
    n = len(reads)
    b = Batch(ctx, reads)
    g_rows, g_keep = Guarded(ctx, D.WORDS * n, True), Guarded(ctx, n, False)
    score = dev_words(ctx, np.zeros(n, np.uint64))
    summ = (C.c_uint64 * 4)()
    fewer = Reads(b.reads.d_bases, n - 1, b.reads.read_len, b.reads.d_offsets)
    huge = Reads(b.reads.d_bases, 1 << 32, b.reads.read_len, b.reads.d_offsets)
    f = ctx.lib.kmx_reads_dedup
    h, r = ctx._h, C.byref(b.reads)
    assert f(h, r, C.byref(fewer), 0, 64, None, 0, g_rows.ptr(), g_keep.ptr(), summ) == E_ARG    # mates of another size
    assert f(h, r, None, 0, 0, None, 0, g_rows.ptr(), g_keep.ptr(), summ) == E_ARG                # hash_bits
    assert f(h, r, None, 0, 65, None, 0, g_rows.ptr(), g_keep.ptr(), summ) == E_ARG
    assert f(h, r, None, 2, 64, None, 0, g_rows.ptr(), g_keep.ptr(), summ) == E_ARG               # an unknown flag
    assert f(h, r, None, 0, 64, ptr(score), 0, g_rows.ptr(), g_keep.ptr(), summ) == E_ARG         # a score without a stride
    assert f(None, r, None, 0, 64, None, 0, g_rows.ptr(), g_keep.ptr(), summ) == E_ARG
    assert f(h, None, None, 0, 64, None, 0, g_rows.ptr(), g_keep.ptr(), summ) == E_ARG
    assert f(h, r, None, 0, 64, None, 0, None, g_keep.ptr(), summ) == E_ARG
    assert f(h, r, None, 0, 64, None, 0, g_rows.ptr(), g_keep.ptr(), None) == E_ARG
    assert f(h, C.byref(huge), None, 0, 64, None, 0, g_rows.ptr(), g_keep.ptr(), summ) == E_ARG   # the index shares a word with the score
    assert g_rows.untouched() and g_keep.untouched()
    assert f(h, r, None, 0, 64, None, 0, g_rows.ptr(), None, summ) == OK                          # (the keep bytes are optional)
    assert (g_rows.payload().reshape(n, D.WORDS) == D.dedup(reads)[0]).all() and g_keep.untouched()


def test_work_buffer_cap(ctx):
    reads = small_batch()
    n = len(reads)
    b = Batch(ctx, reads)
    g_rows, g_keep = Guarded(ctx, D.WORDS * n, True), Guarded(ctx, n, False)
    summ = (C.c_uint64 * 4)(77, 77, 77, 77)
    call = lambda: ctx.lib.kmx_reads_dedup(ctx._h, C.byref(b.reads), None, 0, 64, None, 0, g_rows.ptr(), g_keep.ptr(), summ)  # noqa: E731
    try:
        ctx.set_work_buffer_limit(1024)
        assert call() == E_NOMEM and g_rows.untouched() and g_keep.untouched() and list(summ) == [0, 0, 0, 0]
    finally:
        ctx.set_work_buffer_limit(0)
    assert call() == OK
    assert (g_rows.payload().reshape(n, D.WORDS) == D.dedup(reads)[0]).all()


# ---------------------------------------------------------------- end to end
def test_drop_duplicates_carries_the_quality_bytes(ctx):
    rng = np.random.default_rng(900)
    reads = shuffled(rng, [r for L in (0, 1, 5, 64, 150, 257) for r in family(rng, L)])
    quals = [rng.integers(33, 74, len(r)).astype(np.uint8).tobytes() for r in reads]
    want_rows, want_keep, _ = D.dedup(reads)
    bases, n, L, off = batch_args(ctx, reads, first=3)
    dq = ctx.to_device(ragged(quals, 3)[0])
    out = ctx.reads_drop_duplicates(bases, n, L, offsets=off, quals=dq)
    kept = [r for r in range(n) if want_keep[r]]
    assert out.reads.n_reads == out.quals.n_reads == len(kept) and out.mates is None and out.mate_quals is None
    assert (out.reads.offsets.cpu().numpy() == out.quals.offsets.cpu().numpy()).all()
    assert out.reads.bases.cpu().numpy().tobytes() == b"".join(reads[r] for r in kept)
    assert out.quals.bases.cpu().numpy().tobytes() == b"".join(quals[r] for r in kept)
    assert out.reads.index.cpu().tolist() == kept
    assert (u64(out.duplicates.rows) == want_rows).all()
    hist = out.duplicates.histogram().cpu().tolist()
    counts = want_rows[:, D.COUNT].astype(np.int64)
    assert hist == np.bincount(counts[counts > 0], minlength=out.duplicates.largest + 1).tolist() and hist[0] == 0


def test_drop_duplicate_pairs_keeps_the_mates_in_step(ctx):
    rng = np.random.default_rng(910)
    frags = [(seq(rng, 40), seq(rng, int(rng.integers(20, 60)))) for _ in range(30)]
    picks = [frags[int(i)] for i in rng.integers(0, 30, 100)]
    m1 = [p[0] for p in picks]
    m2 = [p[1] for p in picks]
    want_keep = D.dedup(m1, m2)[1]
    b1 = ctx.to_device(np.frombuffer(b"".join(m1), np.uint8))
    b2, n, L2, off2 = batch_args(ctx, m2)
    out = ctx.reads_drop_duplicates(b1, n, 40, mates=(b2, L2, off2))
    kept = [r for r in range(n) if want_keep[r]]
    assert out.reads.index.cpu().tolist() == kept == out.mates.index.cpu().tolist()
    assert out.reads.bases.cpu().numpy().tobytes() == b"".join(m1[r] for r in kept)
    assert out.mates.bases.cpu().numpy().tobytes() == b"".join(m2[r] for r in kept)


def test_fragments_sequenced_twice_count_once(ctx):
    """error-free fragments, each sequenced from both strands, merged and deduplicated with strand=True: the k-mer counts of the
    result are those of the fragments taken once"""
    import torch

    rng = np.random.default_rng(920)
    L, k = 100, 21
    frags = [seq(rng, int(rng.integers(110, 171))) for _ in range(200)]
    m1, m2 = [], []
    for f in frags:
        for strand_of in (f, D.revcomp_bytes(f)):
            m1.append(strand_of[:L])
            m2.append(D.revcomp_bytes(strand_of)[:L])
    order = rng.permutation(len(m1))
    m1, m2 = [m1[i] for i in order], [m2[i] for i in order]
    b1 = ctx.to_device(np.frombuffer(b"".join(m1), np.uint8))
    b2 = ctx.to_device(np.frombuffer(b"".join(m2), np.uint8))
    merged = ctx.reads_merge_pairs(b1, b2, len(m1), L, L).merged
    assert merged.n_reads == 2 * len(frags)
    out = ctx.reads_drop_duplicates(merged.bases, merged.n_reads, merged.max_len(), offsets=merged.offsets, strand=True)
    assert out.reads.n_reads == len(frags) and out.duplicates.dropped == len(frags) and out.duplicates.largest == 2
    got = ctx.count_canonical(out.reads.bases, out.reads.n_reads, out.reads.max_len(), k, offsets=out.reads.offsets)
    fb, fn, fl, fo = batch_args(ctx, frags)
    want = ctx.count_canonical(fb, fn, fl, k, offsets=fo)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
