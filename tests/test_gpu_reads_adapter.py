"""kmx_reads_adapter on the GPU (kmx_reads_adapter.hip) and what the Python layer builds on it (Context.reads_adapter,
reads_trim_adapters).

Every comparison is equality of every row word with the host reference tests/adapter_np.py (pinned against brute force in
tests/test_adapter_np.py): there is no tolerance anywhere.  The raw call goes through `run`, which hands the ABI a d_rows with
sentinel words on both sides and looks at them afterwards."""
import ctypes as C

import numpy as np
import pytest

from tests import adapter_np as A
from tests import reads_np
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import u64
from tests.reads_dev import SENT_WORD, dev_bytes, dev_words, ptr, ragged

pytestmark = pytest.mark.gpu

OK, E_ARG = 0, 1
GW = 8                            # sentinel words on either side of d_rows
BASE_ALPHA = np.frombuffer(b"ACGTACGTACGTACGTacgtN", np.uint8)
TRUSEQ = b"AGATCGGAAGAGC"
# lengths 1, 13, 33, 63 and 64 among them; wildcards and lower case
EIGHT = [b"AGATCGGAAGAGC", b"T", b"CTGTCTCTTATACACATCTNNgactgcATCGGAt", b"TGGAATTCTCGGGTGCCAAGG", b"acgGtNcatGGatcaNNagg".ljust(63, b"c"),
         (b"GATTACA" * 10)[:64], b"CTGTCTCTTATACACATCT", b"nnGGT"]


def _adapters_c(adapters):
    blob = b"".join(adapters)
    return (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(blob or b"\0"), (C.c_uint32 * max(len(adapters), 1))(*[len(a) for a in adapters])


def random_reads(rng, lens, adapters, share=0.6):
    """random reads of the given lengths; into `share` of them an adapter is planted at a random position (it may hang over the end),
    sometimes with a substitution or two"""
    out = []
    for L in lens:
        read = bytearray(rng.choice(BASE_ALPHA, L).astype(np.uint8).tobytes())
        if L and rng.random() < share:
            ad = bytearray(adapters[int(rng.integers(0, len(adapters)))].replace(b"N", b"A").replace(b"n", b"g"))
            for _ in range(int(rng.integers(0, 3))):
                ad[int(rng.integers(0, len(ad)))] = ord("ACGT"[int(rng.integers(0, 4))])
            p = int(rng.integers(0, L))
            read[p:p + len(ad)] = ad
            del read[L:]
        out.append(bytes(read))
    return out


def run(ctx, bases, n, read_len, off, adapters, min_overlap=3, err=(1, 10), bshift=0, want=None):
    """kmx_reads_adapter through the raw ABI into a guarded d_rows -> rows uint64[n, 4], compared with the reference `want`
    (computed here unless given)"""
    import torch
    from kmers_amd._lib import Reads

    if want is None:
        want = A.reads_adapter_np(bases, n, read_len, adapters, min_overlap, err[0], err[1], off)
    d_b = dev_bytes(ctx, bases, bshift)
    d_off = dev_words(ctx, off)
    rbuf = torch.full((2 * GW + A.RA_WORDS * n,), SENT_WORD, dtype=torch.int64, device=ctx.device)
    reads = Reads(d_b.data_ptr() if n else None, n, read_len, d_off.data_ptr() if off is not None else None)
    blob, lens = _adapters_c(adapters)
    st = ctx.lib.kmx_reads_adapter(ctx._h, C.byref(reads), blob, lens, len(adapters), min_overlap, err[0], err[1], ptr(rbuf[GW:]))
    assert st == OK, ctx.lib.kmx_last_error(ctx._h)
    ctx.synchronize()
    got = u64(rbuf)
    assert (got[:GW] == np.uint64(SENT_WORD & A.M64)).all() and (got[GW + A.RA_WORDS * n:] == np.uint64(SENT_WORD & A.M64)).all()
    got = got[GW:GW + A.RA_WORDS * n].reshape(n, A.RA_WORDS)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
    return got


def keep_of(rows):
    return (rows[:, A.RA_KEEP] >> np.uint64(32)).astype(np.int64).tolist()


@pytest.mark.parametrize("adapters", [[TRUSEQ], EIGHT], ids=["one", "eight"])
@pytest.mark.parametrize("min_overlap,err", [(3, (1, 10)), (1, (0, 1)), (7, (1, 4))])
def test_read_lengths(ctx, adapters, min_overlap, err):
    """every length at which the walk changes: none, below and at min_overlap, one plane word, the word's edge, two and three words and
    their edges, four words, 1 000 bases, 70 000 bases (1 094 steps); offsets[0] > 0; N and lower case in the reads"""
    rng = np.random.default_rng(21 + min_overlap)
    lens = [0, 1, min_overlap - 1, min_overlap, 63, 64, 65, 127, 128, 129, 150, 191, 192, 193, 250, 1000, 70000, 2, 0, 150]
    reads = random_reads(rng, lens, adapters)
    bases, off = ragged(reads, first=5)
    rows = run(ctx, bases, len(lens), 0, off, adapters, min_overlap, err, bshift=3)
    assert rows[:, A.RA_BASES].tolist() == lens
    assert rows[:, A.RA_HIT].any() and not rows[:, A.RA_HIT].all()


def test_adapter_lengths(ctx):
    """adapters of 1, 13, 33, 63 and 64 bases, each alone, planted whole and hanging over the end"""
    rng = np.random.default_rng(22)
    for ad in (b"G", TRUSEQ, EIGHT[2], EIGHT[4], EIGHT[5]):
        lens = [0, 1, 20, 64, 65, 100, 128, 150, 200]
        reads = random_reads(rng, lens, [ad], share=0.8)
        bases, off = ragged(reads)
        rows = run(ctx, bases, len(lens), 0, off, [ad], min(3, len(ad)), (1, 8), bshift=1)
        assert rows[:, A.RA_HIT].any()


def test_planted_positions_and_boundaries(ctx):
    """reads of '.' (a byte that matches nothing) with one adapter planted: the expected position is known without the reference"""
    ad = TRUSEQ   # 13 bases: floor(13 / 10) = 1 mismatch allowed
    bg = lambda n: b"." * n   # noqa: E731
    reads, want = [], []

    def case(read, keep):
        reads.append(read)
        want.append(len(read) if keep is None else keep)

    case(ad + bg(30), 0)                       # p = 0: an adapter dimer, nothing is kept
    case(bg(1) + ad + bg(30), 1)               # p = 1
    for edge in (64, 128, 192):                # across each 64-base boundary, every split of the adapter
        for p in range(edge - 12, edge + 1):
            case(bg(p) + ad + bg(40), p)
    case(bg(100) + ad + bg(150), 100)          # wholly inside, bases behind it
    case(bg(147) + ad[:3], 147)                # hanging over the end by exactly min_overlap ...
    case(bg(148) + ad[:2], None)               # ... and by one less
    case(bg(61) + ad[:3], 61)                  # (the same at a word's edge)
    case(bg(62) + ad[:2], None)
    one = ad[:5] + b"T" + ad[6:]               # one substitution: at the bound
    two = one[:9] + b"T" + one[10:]            # two: above it
    case(bg(20) + one + bg(20), 20)
    case(bg(20) + two + bg(20), None)
    case(bg(20) + ad[:4] + b"." + ad[5:] + bg(9), 20)              # an invalid byte inside the overlap counts as a mismatch
    case(bg(20) + ad[:4] + b".." + ad[6:] + bg(9), None)
    case(bg(20) + ad.lower() + bg(9), 20)                          # lower case in the read
    bases, off = ragged(reads, first=2)
    rows = run(ctx, bases, len(reads), 0, off, [ad], 3, (1, 10), bshift=2)
    assert keep_of(rows) == want
    # a 33-base adapter at 1 / 10: floor(33 / 10) = 3 mismatches hit, 4 do not
    long = b"CTGTCTCTTATACACATCTCCGAGCCCACGAGA"
    assert len(long) == 33

    def subst(seq, at):
        s = bytearray(seq)
        for i in at:
            s[i] = ord("A") if s[i] != ord("A") else ord("C")
        return bytes(s)

    reads = [bg(70) + subst(long, (0, 9, 32)) + bg(5), bg(70) + subst(long, (0, 9, 20, 32)) + bg(5)]
    bases, off = ragged(reads)
    rows = run(ctx, bases, 2, 0, off, [long], 3, (1, 10))
    assert keep_of(rows) == [70, 108] and int(rows[0, A.RA_HIT]) == 1 | (33 << 16) | (3 << 32) and int(rows[1, A.RA_HIT]) == 0


def test_which_adapter_wins(ctx):
    bg = lambda n: b"." * n   # noqa: E731
    a0, a1, a2, a3 = b"ACGTTGCAAGGCT", b"TTTTTTTTTTGG", b"CCCCCCCCAACC", b"GGATCCGGATAGCT"
    # an earlier hit of adapter 3 against a later hit of adapter 0: the position decides, both bits are in HITS
    reads = [bg(10) + a3 + bg(10) + a0 + bg(10), bg(10) + a0 + bg(10) + a3 + bg(10)]
    bases, off = ragged(reads)
    rows = run(ctx, bases, 2, 0, off, [a0, a1, a2, a3], 5, (0, 1))
    assert keep_of(rows) == [10, 10]
    assert [int(w) & 0xFFFF for w in rows[:, A.RA_HIT]] == [4, 1] and rows[:, A.RA_HITS].tolist() == [0b1001, 0b1001]
    # two adapters hitting at one p: the smaller index, whichever way round they are given
    short, wild = a0[:8], a0[:4] + b"NNnn" + a0[8:]
    reads = [bg(70) + a0 + bg(7)]
    bases, off = ragged(reads)
    for ads in ([a0, short, wild], [wild, a0, short], [short, wild, a0]):
        rows = run(ctx, bases, 1, 0, off, ads, 5, (0, 1))
        n0 = len(ads[0])
        assert int(rows[0, A.RA_HIT]) == 1 | (n0 << 16) and keep_of(rows) == [70] and int(rows[0, A.RA_HITS]) == 0b111


def test_alignments_and_empty_reads(ctx):
    """d_bases at byte shifts 0..15; a ragged batch with offsets[0] > 0 and empty reads: one reference"""
    rng = np.random.default_rng(23)
    lens = [0, 3, 70, 1, 150, 0, 0, 257, 5, 4, 2, 101, 64, 0]
    reads = random_reads(rng, lens, EIGHT)
    bases, off = ragged(reads, first=7)
    want = A.reads_adapter_np(bases, len(lens), 0, EIGHT, 3, 1, 10, off)
    for bshift in range(16):
        run(ctx, bases, len(lens), 0, off, EIGHT, 3, (1, 10), bshift=bshift, want=want)
    # a descending offsets pair counts as an empty read
    bad_off = off.copy()
    bad_off[3] = off[5]
    run(ctx, bases, len(lens), 0, bad_off, EIGHT, 3, (1, 10), bshift=1)


def test_uniform_reads(ctx):
    """the uniform layout (d_offsets NULL), a length that is no multiple of four"""
    rng = np.random.default_rng(24)
    n, L = 41, 101
    reads = random_reads(rng, [L] * n, [TRUSEQ, EIGHT[6]])
    bases, _ = ragged(reads)
    rows = run(ctx, bases, n, L, None, [TRUSEQ, EIGHT[6]], 3, (1, 10), bshift=5)
    assert 0 < np.count_nonzero(rows[:, A.RA_HIT]) < n
    run(ctx, bases, 0, L, None, [TRUSEQ])                  # no reads: a no-op
    run(ctx, np.zeros(0, np.uint8), 5, 0, None, [TRUSEQ])  # uniform reads of no bases: rows of zeros


def test_more_reads_than_the_grid_has_waves(ctx):
    """a wave takes a second and a third read: three stretches of the rows against the reference"""
    rng = np.random.default_rng(25)
    n, L = 3 * 32768 + 11, 9
    bases = rng.choice(np.frombuffer(b"ACGT", np.uint8), n * L).astype(np.uint8)
    rows = u64(ctx.reads_adapter(ctx.to_device(bases), n, L, "ACG", min_overlap=2, max_error=(0, 1)))
    assert (rows[:, A.RA_BASES] == L).all()
    for lo in (0, 32768 - 20, n - 40):
        want = A.reads_adapter_np(bases[lo * L:(lo + 40) * L], 40, L, [b"ACG"], 2, 0, 1)
        assert (rows[lo:lo + 40] == want).all()


def test_repeatable(ctx):
    rng = np.random.default_rng(26)
    lens = [150, 0, 1, 149, 151, 300, 2]
    bases, off = ragged(random_reads(rng, lens, EIGHT), first=1)
    a = run(ctx, bases, len(lens), 0, off, EIGHT, bshift=3)
    b = run(ctx, bases, len(lens), 0, off, EIGHT, bshift=3)
    assert a.tobytes() == b.tobytes()


def test_argument_errors(ctx):
    import torch
    from kmers_amd._lib import Reads

    bases = ctx.to_device(np.full(64, ord("A"), np.uint8))
    rows = torch.zeros(4 * 4, dtype=torch.int64, device=ctx.device)
    reads = Reads(bases.data_ptr(), 4, 16, None)
    f = ctx.lib.kmx_reads_adapter

    def call(r=reads, ads=(TRUSEQ,), n_ad=None, lens=None, min_overlap=3, num=1, den=10, rw=rows, h=ctx._h):
        blob, ln = _adapters_c(list(ads))
        if lens is not None:
            ln = (C.c_uint32 * len(lens))(*lens)
        return f(h, C.byref(r) if r is not None else None, blob, ln, len(ads) if n_ad is None else n_ad, min_overlap, num, den, ptr(rw))

    assert call() == OK
    assert call(min_overlap=0) == E_ARG and call(den=0) == E_ARG and call(num=11) == E_ARG and call(num=10) == OK
    assert call(h=None) == E_ARG and call(r=None) == E_ARG and call(rw=None) == E_ARG
    assert call(n_ad=0) == E_ARG and call(ads=[b"ACGT"] * 9) == E_ARG and call(ads=[b"ACGT"] * 8) == OK
    assert call(lens=[0]) == E_ARG and call(ads=[b"A" * 65]) == E_ARG and call(ads=[b"A" * 64]) == OK
    assert call(ads=[b"ACGU"]) == E_ARG and call(ads=[b"AC-T"]) == E_ARG and call(ads=[b"ACGT", b"AC.T"]) == E_ARG
    assert call(ads=[b"acgtNn"]) == OK
    assert f(ctx._h, C.byref(reads), None, (C.c_uint32 * 1)(4), 1, 3, 1, 10, ptr(rows)) == E_ARG
    assert f(ctx._h, C.byref(reads), (C.c_uint8 * 4)(65, 67, 71, 84), None, 1, 3, 1, 10, ptr(rows)) == E_ARG
    assert call(r=Reads(None, 0, 16, None)) == OK                  # no reads: a no-op ...
    assert call(r=Reads(None, 0, 16, None), ads=[b"AC.T"]) == E_ARG  # ... whose arguments are still checked
    ctx.synchronize()


@pytest.mark.parametrize("min_len", [0, 20])
def test_reads_trim_adapters(ctx, min_len):
    from kmers_amd.api import ADAPTERS

    rng = np.random.default_rng(27)
    lens = rng.integers(0, 200, 200).tolist()
    ads = [a.encode() for a in ADAPTERS.values()]
    assert ads[0] == TRUSEQ and len(ads) == 3
    bases, off = ragged(random_reads(rng, lens, ads), first=3)
    quals = np.concatenate([np.full(3, 0xFF, np.uint8), rng.integers(33, 74, len(bases) - 3).astype(np.uint8)])
    n = len(lens)
    d_off = ctx.to_device(off)
    b, q, rows = ctx.reads_trim_adapters(ctx.to_device(bases), n, max(lens), list(ADAPTERS.values()), offsets=d_off, quals=ctx.to_device(quals),
                                         min_len=min_len)
    want = A.reads_adapter_np(bases, n, 0, ads, 3, 1, 10, off)
    assert (u64(rows) == want).all()
    for batch, src in ((b, bases), (q, quals)):
        out, o, idx = reads_np.select_np(src, n, 0, off, span=want[:, A.RA_KEEP], span_k=0, min_len=min_len)
        assert batch.n_reads == len(idx) and (min_len == 0 or 0 < len(idx) < n)
        assert (u64(batch.offsets) == o).all() and batch.bases.cpu().numpy().tobytes() == out.tobytes()
    assert (u64(b.offsets) == u64(q.offsets)).all() and (u64(b.index) == idx).all()
    assert 0 < b.n_bases < sum(lens)
    b2, q2, _ = ctx.reads_trim_adapters(ctx.to_device(bases), n, max(lens), ADAPTERS["truseq"], offsets=d_off)
    assert q2 is None and b2.n_reads == n
