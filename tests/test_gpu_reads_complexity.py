"""kmx_reads_complexity on the GPU (kmx_reads_complexity.hip) and what the Python layer builds on it (Context.reads_complexity,
reads_trim_poly, reads_complexity_filter, gc_content, dust_score).

Every comparison is equality of every row word and every masked byte with the host reference tests/complexity_np.py (pinned
against brute force in tests/test_complexity_np.py): there is no tolerance anywhere.  The raw call goes through `run`, which hands
the ABI a d_masked with sentinel bytes before, behind and between the reads and a d_rows with sentinel words around it, and looks
at all of them afterwards.  The planted cases also state what they expect without the reference."""
import ctypes as C

import numpy as np
import pytest

from tests import complexity_np as X
from tests import reads_np
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import u64
from tests.quality_np import bounds
from tests.reads_dev import SENT, SENT_WORD, dev_bytes, dev_words, ptr, ragged

pytestmark = pytest.mark.gpu

OK, E_ARG = 0, 1
GUARD = 64
GW = 8                            # sentinel words on either side of d_rows
BASE_ALPHA = np.frombuffer(b"ACGTACGTACGTACGTacgtN", np.uint8)
DEFAULTS = (4, 0, 10, 1, 10, 2, 122)   # tail_bases, head_bases, min_len, err_num, err_den, penalty, dust_max
A_, C_, G_, T_ = 1, 2, 3, 4            # bit index + 1, the high half of RX_TAIL / RX_HEAD


def random_reads(rng, lens):
    """random reads over ACGTacgtN of the given lengths; most get a tail, a head or a repeat planted (with a few errors)"""
    out = []
    for i, L in enumerate(lens):
        read = bytearray(rng.choice(BASE_ALPHA, L).astype(np.uint8).tobytes())
        kind, x = i % 5, b"GgATCGt"[int(rng.integers(0, 7))]
        if kind in (1, 4) and L:
            t = int(rng.integers(1, min(L, 150) + 1))
            read[L - t:] = bytes([x]) * t
        if kind in (2, 4) and L:
            h = int(rng.integers(1, min(L, 150) + 1))
            read[:h] = bytes([x ^ 0x20]) * h
        if kind == 3 and L >= 8:
            unit = [b"A", b"CA", b"ACG", b"ttg"][int(rng.integers(0, 4))]
            n = int(rng.integers(8, min(L, 300) + 1))
            p = int(rng.integers(0, L - n + 1))
            read[p:p + n] = (unit * (n // len(unit) + 1))[:n]
        for _ in range(L // 40):           # a few errors, some of them invalid bytes
            read[int(rng.integers(0, L))] = b"ACGTN"[int(rng.integers(0, 5))]
        out.append(bytes(read))
    return out


def run(ctx, bases, n, read_len, off, params=DEFAULTS, bshift=0, mshift=0, want=None, inplace=False, mask=True, rows=True):
    """kmx_reads_complexity through the raw ABI into guarded buffers -> (masked bytes of the whole layout, rows uint64[n, 8]), both
    compared with the reference `want` = (rows, masked) (computed here unless given)"""
    import torch
    from kmers_amd._lib import Reads

    if want is None:
        want = X.reads_complexity_np(bases, n, read_len, *params, offsets=off)
    d_b = dev_bytes(ctx, bases, bshift)
    d_off = dev_words(ctx, off)
    total = len(bases)
    mbuf = torch.full((GUARD + mshift + total + GUARD,), SENT, dtype=torch.uint8, device=ctx.device)
    d_m = d_b if inplace else mbuf[GUARD + mshift:GUARD + mshift + max(total, 1)]
    rbuf = torch.full((2 * GW + X.RX_WORDS * n,), SENT_WORD, dtype=torch.int64, device=ctx.device)
    d_r = rbuf[GW:]
    reads = Reads(d_b.data_ptr() if n else None, n, read_len, d_off.data_ptr() if off is not None else None)
    st = ctx.lib.kmx_reads_complexity(ctx._h, C.byref(reads), *params, ptr(d_m) if mask else None, ptr(d_r) if rows else None)
    assert st == OK, ctx.lib.kmx_last_error(ctx._h)
    ctx.synchronize()
    got_rows = u64(rbuf)
    assert (got_rows[:GW] == np.uint64(SENT_WORD & X.M64)).all() and (got_rows[GW + X.RX_WORDS * n:] == np.uint64(SENT_WORD & X.M64)).all()
    got_rows = got_rows[GW:GW + X.RX_WORDS * n].reshape(n, X.RX_WORDS)
    if rows:
        bad = np.nonzero((got_rows != want[0]).any(axis=1))[0]
        assert len(bad) == 0, (int(bad[0]), got_rows[bad[0]].tolist(), want[0][bad[0]].tolist())
    else:
        assert (got_rows == np.uint64(SENT_WORD & X.M64)).all()
    # the bytes of the reads are the reference's, every other byte of the buffer is as it was
    inside = np.zeros(total, bool)
    for a, L in bounds(n, read_len, off):
        inside[a:a + L] = True
    if inplace:
        got = d_b.cpu().numpy()[:total]
        expect = np.where(inside, want[1], bases)
    else:
        whole = mbuf.cpu().numpy()
        assert (whole[:GUARD + mshift] == SENT).all() and (whole[GUARD + mshift + total:] == SENT).all()
        got = whole[GUARD + mshift:GUARD + mshift + total]
        expect = np.where(inside, want[1], SENT).astype(np.uint8) if mask else np.full(total, SENT, np.uint8)
    bad = np.nonzero(got != expect)[0]
    assert len(bad) == 0, (int(bad[0]), int(got[bad[0]]), int(expect[bad[0]]))
    return got, got_rows


LENGTHS = [0, 1, 2, 3, 9, 10, 31, 32, 33, 63, 64, 65, 66, 95, 96, 97, 127, 128, 129, 150, 191, 192, 193, 250, 1000, 70000]


@pytest.mark.parametrize("masks", [(4, 0), (15, 15), (1, 8), (0, 0)], ids=["G", "all", "A-T", "none"])
@pytest.mark.parametrize("rate,penalty", [((1, 10), 2), ((0, 1), 0), ((1, 4), 255)], ids=["tenth", "exact", "quarter"])
def test_read_lengths(ctx, masks, rate, penalty):
    """every length at which the poly walks and the windows change: none, below three bases, below and at min_len (10), the edges of
    the first, second, third and fourth window and of the 64-base steps, 1 000 bases, 70 000 bases (1 094 steps, 2 187 windows).
    Ragged with offsets[0] > 0 at each byte alignment of d_bases and, independently, of d_masked; then uniform batches of 150 and of
    37 bases.  N and lower case in the reads."""
    rng = np.random.default_rng(31 + 7 * masks[0] + penalty)
    params = (masks[0], masks[1], 10, rate[0], rate[1], penalty, 122)
    reads = random_reads(rng, LENGTHS)
    bases, off = ragged(reads, first=5)
    want = X.reads_complexity_np(bases, len(reads), 0, *params, offsets=off)
    assert want[0][:, X.RX_BASES].tolist() == LENGTHS and int((want[0][:, X.RX_DUST] >> np.uint64(32)).sum()) > 0
    if masks[0]:
        assert want[0][:, X.RX_TAIL].any() and not want[0][1:, X.RX_TAIL].all()
    for bshift in range(4):
        for mshift in range(4):
            run(ctx, bases, len(reads), 0, off, params, bshift=bshift, mshift=mshift, want=want)
    for L, n in ((150, 23), (37, 41)):
        ubases, _ = ragged(random_reads(rng, [L] * n))
        run(ctx, ubases, n, L, None, params, bshift=1, mshift=2)


def de_bruijn_64():
    """the 64 letters of a de Bruijn sequence over ACGT of order 3: read round and round, any 62 triplets in a row are all different,
    so a window of it has S = 0"""
    seq, a = [], [0] * 12

    def db(t, p):
        if t > 3:
            if 3 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    assert len(seq) == 64
    return bytes(b"ACGT"[i] for i in seq)


def test_planted_cases(ctx):
    """reads of '.' (a byte that matches nothing) with tails, heads and repeats planted: what is expected is written down here,
    without the reference (which `run` checks as well)"""
    bg = lambda n: b"." * n   # noqa: E731
    cases = {}   # params -> [(read, {word: value}, masked or None)]

    def case(read, words, masked=None, params=DEFAULTS):
        cases.setdefault(params, []).append((read, words, masked))

    def keep(start, length):
        return start | (length << 32)

    # a G run of exactly min_len at the end, and of one less
    case(bg(40) + b"G" * 10, {X.RX_TAIL: 10 | (G_ << 32), X.RX_KEEP: keep(0, 40), X.RX_GT: 10, X.RX_DIFF: 0 | (9 << 32)})
    case(bg(40) + b"G" * 9, {X.RX_TAIL: 0, X.RX_KEEP: keep(0, 49)})
    # a tail across the 64th and the 128th base from the end, at every split, behind 0 .. 3 and 30 other bytes
    for t in list(range(58, 71)) + list(range(122, 135)):
        for p in (0, 1, 2, 3, 30):
            case(bg(p) + b"G" * t, {X.RX_TAIL: t | (G_ << 32), X.RX_KEEP: keep(0, p) if p else 0}, params=(4, 0, 10, 1, 10, 2, 1891))
    # ... and a head across the 64th and 128th base
    for h in (63, 64, 65, 127, 128, 129):
        case(b"t" * h + bg(7), {X.RX_HEAD: h | (T_ << 32), X.RX_KEEP: keep(h, 7)}, params=(0, 8, 10, 1, 10, 2, 1891))
    # mismatches exactly at the rate bound (2 in 20 at a tenth) and one above it; at penalty 0 the longest qualifying suffix wins
    case(bg(30) + b"GTT" + b"G" * 17, {X.RX_TAIL: 20 | (G_ << 32), X.RX_KEEP: keep(0, 30)}, params=(4, 0, 10, 1, 10, 0, 1891))
    case(bg(30) + b"GTTT" + b"G" * 16, {X.RX_TAIL: 16 | (G_ << 32), X.RX_KEEP: keep(0, 34)}, params=(4, 0, 10, 1, 10, 0, 1891))
    # (at penalty 2 the 17 clean bases score 17 against 20 - 3 * 2 = 14)
    case(bg(30) + b"GTT" + b"G" * 17, {X.RX_TAIL: 17 | (G_ << 32), X.RX_KEEP: keep(0, 33)}, params=(4, 0, 10, 1, 10, 2, 1891))
    # an invalid byte inside the tail counts as a mismatch: one in 12 passes a tenth, two do not
    case(bg(5) + b"GGGGG.GGGGGG", {X.RX_TAIL: 12 | (G_ << 32)}, params=(4, 0, 10, 1, 10, 0, 1891))
    case(bg(5) + b"GGGGG..GGGGG", {X.RX_TAIL: 0, X.RX_KEEP: keep(0, 17)}, params=(4, 0, 10, 1, 10, 0, 1891))
    # a whole-read homopolymer keeps nothing
    case(b"A" * 50, {X.RX_TAIL: 50 | (A_ << 32), X.RX_KEEP: 0, X.RX_AC: 50, X.RX_DIFF: 0 | (49 << 32)}, params=(15, 0, 10, 1, 10, 2, 1891))
    # a head and a tail that meet, that overlap, and that leave one base
    both = (4, 8, 10, 0, 1, 2, 1891)
    case(b"T" * 12 + b"G" * 12, {X.RX_TAIL: 12 | (G_ << 32), X.RX_HEAD: 12 | (T_ << 32), X.RX_KEEP: 0}, params=both)
    case(b"T" * 12 + b"C" + b"G" * 12, {X.RX_KEEP: keep(12, 1)}, params=both)
    case(b"A" * 30, {X.RX_TAIL: 30 | (A_ << 32), X.RX_HEAD: 30 | (A_ << 32), X.RX_KEEP: 0}, params=(1, 1, 10, 0, 1, 2, 1891))
    # two letters tying at a score of 10 (rate 1 / 1, penalty 0): G with 20 bases of which 10 are A, A with its 10: the longer
    tie = (15, 0, 5, 1, 1, 0, 1891)
    case(b"CCCCC" + b"G" * 10 + b"A" * 10, {X.RX_TAIL: 20 | (G_ << 32), X.RX_KEEP: keep(0, 5)}, params=tie)
    case(b"CCCCC" + b"A" * 10 + b"G" * 10, {X.RX_TAIL: 20 | (A_ << 32), X.RX_KEEP: keep(0, 5)}, params=tie)
    # an equal score at two lengths (penalty 1: ten G score 10, "GT" in front of them 12 - 2 = 10): the longer
    case(b"TTTTGTGGGGGGGGGG", {X.RX_TAIL: 12 | (G_ << 32), X.RX_KEEP: keep(0, 4)}, params=(4, 0, 5, 1, 2, 1, 1891))
    # a lower-case tail
    case(bg(20) + b"g" * 15, {X.RX_TAIL: 15 | (G_ << 32), X.RX_KEEP: keep(0, 20), X.RX_GT: 15})
    # a full window of one letter: S = 1891, masked
    case(b"A" * 64, {X.RX_DUST: 1891 | (1 << 32), X.RX_AC: 64}, b"N" * 64)
    case(b"A" * 64, {X.RX_DUST: 1891}, b"A" * 64, params=(4, 0, 10, 1, 10, 2, 1891))
    # (AC)n: S = 930
    case(b"AC" * 32, {X.RX_DUST: 930 | (1 << 32), X.RX_AC: 32 | (32 << 32), X.RX_DIFF: 63 | (63 << 32)}, b"N" * 64, params=(4, 0, 10, 1, 10, 2, 929))
    case(b"AC" * 32, {X.RX_DUST: 930}, b"AC" * 32, params=(4, 0, 10, 1, 10, 2, 930))
    case((b"ACG" * 22)[:64], {X.RX_DUST: 610 | (1 << 32)}, b"N" * 64)
    # a window holding an N: 29 + 30 counted triplets of one spelling
    case(b"A" * 31 + b"N" + b"A" * 32, {X.RX_DUST: 59 * 58 // 2 | (1 << 32), X.RX_AC: 63, X.RX_DIFF: 0 | (61 << 32)}, b"N" * 64)
    # L = 65: two windows, the second [32, 65) with one new base and 31 triplets (S = 465)
    case(b"A" * 65, {X.RX_DUST: 1891 | (2 << 32)}, b"N" * 65)
    case(b"A" * 65, {X.RX_DUST: 1891 | (1 << 32)}, b"N" * 64 + b"A", params=(4, 0, 10, 1, 10, 2, 1000))
    case(b"C" * 32 + b"A" * 33, {X.RX_DUST: (30 * 29 // 2 + 30 * 29 // 2) | (1 << 32)}, b"N" * 64 + b"A", params=(4, 0, 10, 1, 10, 2, 500))
    # 40 bases of one letter at [50, 90) inside 160 bases without a repeated triplet: windows 1 ([32, 96), 38 triplets) and 2 ([64, 128),
    # 24 triplets) are DUSTY, window 0 (12 triplets: 66 and a few) and window 3 are not: the blocks [32, 128) turn to N
    quiet = de_bruijn_64() * 3
    planted = quiet[:50] + b"A" * 40 + quiet[90:160]
    assert planted[49:50] != b"A" and planted[90:91] != b"A"
    planted_at = len(cases[DEFAULTS])
    case(planted, {}, planted[:32] + b"N" * 96 + planted[128:])
    case(quiet[:128], {X.RX_DUST: 0, X.RX_AC: 32 | (32 << 32), X.RX_GT: 32 | (32 << 32)}, quiet[:128])
    got = {}
    for params, group in cases.items():
        reads = [c[0] for c in group]
        bases, off = ragged(reads, first=2)
        masked, rows = got[params] = run(ctx, bases, len(reads), 0, off, params, bshift=2, mshift=1)
        for r, (read, words, want_m) in enumerate(group):
            assert int(rows[r, X.RX_BASES]) == len(read)
            for w, v in words.items():
                assert int(rows[r, w]) == v, (params, r, read, w, int(rows[r, w]), v)
            if want_m is not None:
                assert masked[int(off[r]):int(off[r + 1])].tobytes() == want_m, (params, r, read)
    dust = int(got[DEFAULTS][1][planted_at, X.RX_DUST])   # two DUSTY windows; the larger holds 38 triplets of A and little else
    assert dust >> 32 == 2 and 38 * 37 // 2 <= (dust & 0xFFFFFFFF) < 38 * 37 // 2 + 40


def test_alignments_and_empty_reads(ctx):
    """d_bases at byte shifts 0..15 crossed with d_masked at 0..3; empty reads; a descending offsets pair counts as an empty read"""
    rng = np.random.default_rng(33)
    lens = [0, 3, 70, 1, 150, 0, 0, 257, 5, 4, 2, 101, 64, 0]
    params = (15, 15, 4, 1, 8, 1, 60)
    bases, off = ragged(random_reads(rng, lens), first=7)
    want = X.reads_complexity_np(bases, len(lens), 0, *params, offsets=off)
    for bshift in range(16):
        run(ctx, bases, len(lens), 0, off, params, bshift=bshift, mshift=(bshift * 3 + 1) % 4, want=want)
    bad_off = off.copy()
    bad_off[3] = off[5]
    run(ctx, bases, len(lens), 0, bad_off, params, bshift=1, mshift=3)
    run(ctx, bases, 0, 101, None, params)                   # no reads: a no-op
    run(ctx, np.zeros(0, np.uint8), 5, 0, None, params)     # uniform reads of no bases: rows of zeros


def test_more_reads_than_the_grid_has_waves(ctx):
    """70 000 ragged reads of 0 to 40 bases (more where the device's capped grid covers more than half of that in one sweep): a wave
    takes a second and a third read.  Every row and every masked byte is checked; the reads are drawn from 1 500 different ones, so
    the reference is computed once for each"""
    import torch

    rng = np.random.default_rng(34)
    sweep = torch.cuda.get_device_properties(ctx.device).multi_processor_count * 8 * 4 * 4   # the reads of one capped grid
    n = max(70000, 2 * sweep + 4463)
    pool = random_reads(rng, rng.integers(0, 41, 1500).tolist())
    params = (15, 1, 5, 1, 5, 2, 40)
    pbases, poff = ragged(pool)
    prow, pmasked = X.reads_complexity_np(pbases, len(pool), 0, *params, offsets=poff)
    pick = rng.integers(0, len(pool), n)
    pick[[0, sweep - 1, sweep, n - 1]] = [3, 4, 8, 9]
    plen = np.diff(poff.astype(np.int64))
    off = np.concatenate([[0], np.cumsum(plen[pick])]).astype(np.uint64) + np.uint64(3)
    at = np.repeat(poff[pick].astype(np.int64) - off[:-1].astype(np.int64), plen[pick]) + np.arange(3, int(off[-1]))   # the source byte of every byte
    bases = np.concatenate([np.full(3, ord("."), np.uint8), pbases[at]])
    want = (prow[pick], np.concatenate([np.full(3, ord("."), np.uint8), pmasked[at]]))
    assert want[0][:, X.RX_TAIL].any() and int((want[0][:, X.RX_DUST] >> np.uint64(32)).sum()) > 0
    run(ctx, bases, n, 0, off, params, bshift=1, mshift=3, want=want)


def test_in_place_and_repeatable(ctx):
    import torch
    from kmers_amd.api import Context

    rng = np.random.default_rng(35)
    lens = [150, 0, 1, 149, 151, 300, 2, 64, 65]
    params = (15, 15, 10, 1, 10, 2, 122)
    bases, off = ragged(random_reads(rng, lens), first=1)
    n = len(lens)
    a = run(ctx, bases, n, 0, off, params, bshift=3, mshift=1)
    b = run(ctx, bases, n, 0, off, params, bshift=3, mshift=1)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and int((a[1][:, X.RX_DUST] >> np.uint64(32)).sum()) > 0
    c = run(ctx, bases, n, 0, off, params, bshift=3, inplace=True)
    assert (c[0][1:] == a[0][1:]).all() and c[1].tobytes() == a[1].tobytes()
    run(ctx, bases, n, 0, off, params, rows=False)           # the mask alone
    run(ctx, bases, n, 0, off, params, mask=False)           # the rows alone
    run(ctx, bases, n, 0, off, params, inplace=True, rows=False)
    # a second stream and a fresh context give the same rows and bytes
    torch.cuda.synchronize()
    for other in (Context(stream=torch.cuda.Stream()), Context()):
        masked, rows = other.reads_complexity(other.to_device(bases), n, max(lens), "ACGT", "ACGT", offsets=other.to_device(off))
        other.synchronize()
        assert u64(rows).tobytes() == a[1].tobytes() and masked.cpu().numpy()[1:].tobytes() == a[0][1:].tobytes()
        other.close()


def test_argument_errors(ctx):
    import torch
    from kmers_amd._lib import Reads

    bases = ctx.to_device(np.full(64 + 16, ord("A"), np.uint8))
    rbuf = torch.full((2 * GW + 8 * 4,), SENT_WORD, dtype=torch.int64, device=ctx.device)
    mbuf = torch.full((GUARD + 64 + GUARD,), SENT, dtype=torch.uint8, device=ctx.device)
    rows, out = rbuf[GW:], mbuf[GUARD:]
    reads = Reads(bases.data_ptr(), 4, 16, None)
    f = ctx.lib.kmx_reads_complexity

    def call(r=reads, tail=4, head=0, min_len=10, num=1, den=10, penalty=2, dust_max=122, m=out, rw=rows, h=ctx._h):
        return f(h, C.byref(r) if r is not None else None, tail, head, min_len, num, den, penalty, dust_max, ptr(m), ptr(rw))

    assert call(tail=16) == E_ARG and call(head=16) == E_ARG and call(tail=15, head=15, dust_max=2**32 - 1) == OK
    assert call(den=0) == E_ARG and call(num=11) == E_ARG and call(num=10) == OK
    assert call(min_len=0) == E_ARG and call(min_len=0, tail=0, head=1) == E_ARG
    assert call(penalty=256) == E_ARG
    assert call(h=None) == E_ARG and call(r=None) == E_ARG and call(m=None, rw=None) == E_ARG
    assert call(m=bases[1:]) == E_ARG                # an overlap with the bases that is not in place
    off = ctx.to_device(np.array([0, 10, 10, 30, 64], np.uint64))
    rag = Reads(bases.data_ptr(), 4, 0, off.data_ptr())
    assert call(r=rag, m=bases[8:]) == E_ARG
    none = Reads(None, 0, 16, None)
    assert call(r=none, tail=16) == E_ARG and call(r=none, den=0) == E_ARG and call(r=none, m=None, rw=None) == E_ARG
    ctx.synchronize()
    # not one of the refused calls, nor the one that ran with a dust_max no window exceeds, touched a byte it should not
    assert (u64(rbuf)[:GW] == np.uint64(SENT_WORD & X.M64)).all() and (u64(rbuf)[GW + 32:] == np.uint64(SENT_WORD & X.M64)).all()
    whole = mbuf.cpu().numpy()
    assert (whole[:GUARD] == SENT).all() and (whole[GUARD + 64:] == SENT).all() and (whole[GUARD:GUARD + 64] == ord("A")).all()
    assert (bases.cpu().numpy() == ord("A")).all()
    assert call(r=none) == OK                                    # no reads: a no-op
    assert call(min_len=0, tail=0) == OK                         # min_len is not looked at without a letter
    assert call(m=None) == OK and call(rw=None) == OK
    assert call(m=bases) == OK and call(r=rag) == OK and call(r=rag, m=bases) == OK   # in place
    ctx.synchronize()


@pytest.mark.parametrize("min_len_out", [0, 20])
def test_reads_trim_poly(ctx, min_len_out):
    rng = np.random.default_rng(36)
    lens = rng.integers(0, 200, 200).tolist()
    bases, off = ragged(random_reads(rng, lens), first=3)
    quals = np.concatenate([np.full(3, 0xFF, np.uint8), rng.integers(33, 74, len(bases) - 3).astype(np.uint8)])
    n = len(lens)
    d_off = ctx.to_device(off)
    b, q, rows = ctx.reads_trim_poly(ctx.to_device(bases), n, max(lens), tail="GA", head="t", offsets=d_off, quals=ctx.to_device(quals),
                                     min_len_out=min_len_out)
    want = X.reads_complexity_np(bases, n, 0, 5, 8, 10, 1, 10, 2, 1891, off)[0]
    assert (u64(rows) == want).all() and want[:, X.RX_TAIL].any() and want[:, X.RX_HEAD].any()
    start, length = X.keep_span(want)
    for batch, src in ((b, bases), (q, quals)):
        out, o, idx = reads_np.select_np(src, n, 0, off, span=want[:, X.RX_KEEP], span_k=0, min_len=min_len_out)
        assert batch.n_reads == len(idx) and (min_len_out == 0 or 0 < len(idx) < n)
        assert (u64(batch.offsets) == o).all() and batch.bases.cpu().numpy().tobytes() == out.tobytes()
    host = b"".join(bytes(bases[int(off[r]) + int(start[r]):int(off[r]) + int(start[r]) + int(length[r])]) for r in range(n)
                    if length[r] >= min_len_out)
    assert b.bases.cpu().numpy().tobytes() == host
    assert (u64(b.offsets) == u64(q.offsets)).all() and (u64(b.index) == idx).all() and 0 < b.n_bases < sum(lens)
    b2, q2, _ = ctx.reads_trim_poly(ctx.to_device(bases), n, max(lens), offsets=d_off)
    assert q2 is None and b2.n_reads == n


@pytest.mark.parametrize("trim", [True, False])
def test_reads_complexity_filter(ctx, trim):
    from kmers_amd.api import dust_score, gc_content

    rng = np.random.default_rng(37)
    lens = rng.integers(0, 200, 240).tolist()
    bases, off = ragged(random_reads(rng, lens), first=3)
    quals = np.concatenate([np.full(3, 0xFF, np.uint8), rng.integers(33, 74, len(bases) - 3).astype(np.uint8)])
    n = len(lens)
    d_off = ctx.to_device(off)
    b, q, rows = ctx.reads_complexity_filter(ctx.to_device(bases), n, max(lens), tail="G", head="A", offsets=d_off, min_diff=(3, 10), max_dust=200,
                                             trim=trim, quals=ctx.to_device(quals), min_len_out=15)
    want = X.reads_complexity_np(bases, n, 0, 4, 1, 10, 1, 10, 2, 122, off)[0]
    assert (u64(rows) == want).all()
    D = (want[:, X.RX_DIFF] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    P = (want[:, X.RX_DIFF] >> np.uint64(32)).astype(np.int64)
    S = (want[:, X.RX_DUST] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    keep = (D * 10 >= 3 * P) & (S <= 200)
    assert 0 < keep.sum() < n and ((D * 10 >= 3 * P) != keep).any() and ((S <= 200) != keep).any()
    for batch, src in ((b, bases), (q, quals)):
        out, o, idx = reads_np.select_np(src, n, 0, off, keep=keep, span=want[:, X.RX_KEEP] if trim else None, span_k=0, min_len=15)
        assert batch.n_reads == len(idx) and 0 < len(idx) < n
        assert (u64(batch.offsets) == o).all() and batch.bases.cpu().numpy().tobytes() == out.tobytes()
    assert (u64(b.offsets) == u64(q.offsets)).all() and (u64(b.index) == idx).all()
    # (the two helpers are float64 quotients of exact integers: the device's division need not round as numpy's does, and one ulp of a
    # value below 32 is 4e-15)
    assert np.allclose(gc_content(rows).cpu().numpy(), X.gc_content_np(want), rtol=0, atol=1e-12)
    assert np.allclose(dust_score(rows).cpu().numpy(), S / 61.0, rtol=0, atol=1e-12)


def test_masked_batch_counts_like_the_host_masked_reads(ctx):
    """count_canonical of the device's masked batch equals count_canonical of the reads the reference masked, at k = 21"""
    rng = np.random.default_rng(38)
    lens = rng.integers(0, 260, 300).tolist() + [600]
    bases, off = ragged(random_reads(rng, lens))
    n, k = len(lens), 21
    d_off = ctx.to_device(off)
    masked, rows = ctx.reads_complexity(ctx.to_device(bases), n, max(lens), offsets=d_off)
    want_rows, want_masked = X.reads_complexity_np(bases, n, 0, *DEFAULTS, offsets=off)
    assert 0 < (want_masked != bases).sum() and (u64(rows) == want_rows).all()
    got = ctx.count_canonical(masked, n, max(lens), k, offsets=d_off)
    ref = ctx.count_canonical(ctx.to_device(want_masked), n, max(lens), k, offsets=d_off)
    plain = ctx.count_canonical(ctx.to_device(bases), n, max(lens), k, offsets=d_off)
    assert u64(got[0]).tobytes() == u64(ref[0]).tobytes() and u64(got[1]).tobytes() == u64(ref[1]).tobytes()
    assert 0 < len(u64(got[0])) < len(u64(plain[0]))
