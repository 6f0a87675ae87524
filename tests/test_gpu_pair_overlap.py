"""kmx_reads_pair_overlap on the GPU (kmx_reads_adapter.hip) and what the Python layer builds on it (Context.reads_pair_overlap,
reads_trim_pairs).

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
ACGT = np.frombuffer(b"ACGT", np.uint8)
JUNK = np.frombuffer(b"ACGTacgtN", np.uint8)


def seq(rng, n, alpha=ACGT):
    return rng.choice(alpha, n).astype(np.uint8).tobytes()


def mutate(rng, s, k):
    """k substitutions at distinct positions"""
    s = bytearray(s)
    for i in rng.choice(len(s), k, replace=False):
        s[i] = ord("ACGT"[("ACGT".index(chr(s[i]).upper()) + 1 + int(rng.integers(0, 3))) % 4])
    return bytes(s)


def mates(rng, L1, L2, insert, mism=0):
    """both mates of a fragment of `insert` bases, read-through junk behind a short fragment; `mism` substitutions in mate 2"""
    frag = seq(rng, insert)
    m1 = (frag + seq(rng, L1, JUNK))[:L1]
    m2 = (A.revcomp(frag) + seq(rng, L2, JUNK))[:L2]
    if mism:
        m2 = mutate(rng, m2[:min(L2, insert)], mism) + m2[min(L2, insert):]
    return m1, m2


def run(ctx, b1, b2, n, len1=0, len2=0, off1=None, off2=None, min_overlap=30, max_mism=5, err=(1, 5), shift1=0, shift2=0, want=None):
    """kmx_reads_pair_overlap through the raw ABI into a guarded d_rows -> rows uint64[n, 4], compared with the reference"""
    import torch
    from kmers_amd._lib import Reads

    if want is None:
        want = A.reads_pair_overlap_np(b1, b2, n, len1, len2, off1, off2, min_overlap, max_mism, err[0], err[1])
    d1, d2 = dev_bytes(ctx, b1, shift1), dev_bytes(ctx, b2, shift2)
    d_o1 = dev_words(ctx, off1)
    d_o2 = dev_words(ctx, off2)
    rbuf = torch.full((2 * GW + A.RP_WORDS * n,), SENT_WORD, dtype=torch.int64, device=ctx.device)
    r1 = Reads(d1.data_ptr() if n else None, n, len1, d_o1.data_ptr() if off1 is not None else None)
    r2 = Reads(d2.data_ptr() if n else None, n, len2, d_o2.data_ptr() if off2 is not None else None)
    st = ctx.lib.kmx_reads_pair_overlap(ctx._h, C.byref(r1), C.byref(r2), min_overlap, max_mism, err[0], err[1], ptr(rbuf[GW:]))
    assert st == OK, ctx.lib.kmx_last_error(ctx._h)
    ctx.synchronize()
    got = u64(rbuf)
    assert (got[:GW] == np.uint64(SENT_WORD & A.M64)).all() and (got[GW + A.RP_WORDS * n:] == np.uint64(SENT_WORD & A.M64)).all()
    got = got[GW:GW + A.RP_WORDS * n].reshape(n, A.RP_WORDS)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
    return got


@pytest.mark.parametrize("L1,L2", [(0, 0), (1, 1), (64, 64), (65, 63), (100, 150), (150, 100), (150, 150), (250, 250), (1024, 1024), (1025, 100)])
def test_length_pairs_and_planted_inserts(ctx, L1, L2):
    """uniform mates of every length pair, inserts planted from 1 to L1 + L2 - min_overlap: d takes both signs, the overlap every
    length from min_overlap up; mate 1 uniform, mate 2 the same reads as a ragged batch at another alignment"""
    rng = np.random.default_rng(31 + L1 + L2)
    min_overlap = 1 if L1 <= 1 else 20
    top = max(L1 + L2 - min_overlap, 1)
    inserts = sorted(set([1, 2, min_overlap, max(min(L1, L2) - 1, 1), max(min(L1, L2), 1), max(L1, L2, 1), max(L1, L2) + 1, top - 1 or 1, top]
                         + rng.integers(1, top + 1, 6).tolist()))
    pairs = [mates(rng, L1, L2, i, mism=int(rng.integers(0, 3)) if i > 8 else 0) for i in inserts]
    pairs.append((seq(rng, L1, JUNK), seq(rng, L2, JUNK)))   # unrelated mates
    n = len(pairs)
    b1 = np.frombuffer(b"".join(p[0] for p in pairs), np.uint8)
    b2, off2 = ragged([p[1] for p in pairs], first=3)
    rows = run(ctx, b1, b2, n, L1, 0, None, off2, min_overlap=min_overlap, max_mism=4, err=(1, 5), shift1=1, shift2=2)
    found = rows[:, A.RP_INSERT].astype(np.int64)
    if L1 == 0 or L1 > A.RP_MAX_LEN:
        assert not rows[:, :2].any()                        # no bases; the cap: no hit by definition
        assert (rows[:, A.RP_KEEP1] >> np.uint64(32) == L1).all() and (rows[:, A.RP_KEEP2] >> np.uint64(32) == L2).all()
    else:
        assert np.count_nonzero(found) >= (3 if L1 >= 64 else 1)
        d = found[found > 0] - L2
        assert L1 < 64 or ((d < 0).any() and (d > 0).any())


def test_homopolymers_every_shift_hits(ctx):
    """the longest overlap wins, of equal ones the largest d"""
    cases = [(150, 100), (100, 150), (150, 150), (64, 64), (65, 200), (1024, 1000)]
    m1s = [b"A" * a for a, _ in cases]
    m2s = [b"t" * b for _, b in cases]
    b1, o1 = ragged(m1s)
    b2, o2 = ragged(m2s, first=1)
    rows = run(ctx, b1, b2, len(cases), 0, 0, o1, o2, min_overlap=10, max_mism=0, err=(0, 1))
    for r, (a, b) in enumerate(cases):
        # n = min(a, b) for d in [0, a - b] (a >= b: the largest is a - b, I = a) or d in [a - b, 0] (a < b: the largest is 0, I = b)
        ins = max(a, b)
        assert rows[r].tolist() == [ins, min(a, b), min(a, ins) << 32, min(b, ins) << 32], (a, b)


def test_thresholds_at_their_boundaries(ctx):
    rng = np.random.default_rng(32)
    frag = seq(rng, 100)
    rc = A.revcomp(frag)
    m2 = {k: mutate(rng, rc, k) for k in (4, 5, 6)}
    b1 = np.frombuffer(frag, np.uint8)

    def ins(m, **kw):
        return int(run(ctx, b1, np.frombuffer(m2[m], np.uint8), 1, 100, 100, **kw)[0, A.RP_INSERT])

    # max_mism, the rate out of the way
    assert ins(5, max_mism=5, err=(1, 1)) == 100 and ins(6, max_mism=5, err=(1, 1)) == 0 and ins(4, max_mism=5, err=(1, 1)) == 100
    # the rate, max_mism out of the way: m * 20 <= 1 * 100 holds for m = 5 and not for m = 6
    assert ins(5, max_mism=50, err=(1, 20)) == 100 and ins(6, max_mism=50, err=(1, 20)) == 0
    # min_overlap at the overlap's length and one above it
    assert ins(4, min_overlap=100) == 100 and ins(4, min_overlap=101) == 0
    r = run(ctx, b1, np.frombuffer(m2[5], np.uint8), 1, 100, 100, max_mism=5)
    assert r[0].tolist() == [100, 100 | (5 << 32), 100 << 32, 100 << 32]


def test_invalid_bytes_inside_the_overlap(ctx):
    """N matches nothing, not even N: each one costs a mismatch"""
    rng = np.random.default_rng(33)
    frag = seq(rng, 120)
    rc = bytearray(A.revcomp(frag))
    m1 = bytearray(frag)
    m1[10], m1[70] = ord("N"), ord("n")
    rc[119 - 10], rc[5] = ord("N"), ord(".")          # the first opposite the N of mate 1: one mismatch, not two, and not a match
    b1, b2 = np.frombuffer(bytes(m1), np.uint8), np.frombuffer(bytes(rc), np.uint8)
    r = run(ctx, b1, b2, 1, 120, 120, max_mism=3)
    assert r[0].tolist() == [120, 120 | (3 << 32), 120 << 32, 120 << 32]
    assert not run(ctx, b1, b2, 1, 120, 120, max_mism=2)[0, :2].any()
    # lower case matches upper case
    r = run(ctx, np.frombuffer(frag.lower(), np.uint8), np.frombuffer(A.revcomp(frag), np.uint8), 1, 120, 120, max_mism=0)
    assert int(r[0, A.RP_INSERT]) == 120 and int(r[0, A.RP_OVERLAP]) == 120


def test_ragged_mates_with_their_own_offsets_and_alignments(ctx):
    rng = np.random.default_rng(34)
    shape = [(150, 150, 90), (0, 40, 5), (40, 0, 5), (151, 149, 200), (100, 100, 100), (1, 1, 1), (250, 101, 180), (64, 128, 70), (150, 150, 299),
             (1024, 300, 500), (1025, 1025, 800), (33, 31, 12), (150, 150, 35)]
    pairs = [mates(rng, a, b, i, mism=1 if i > 30 else 0) for a, b, i in shape]
    b1, o1 = ragged([p[0] for p in pairs], first=6)
    b2, o2 = ragged([p[1] for p in pairs], first=1)
    kw = dict(min_overlap=12, max_mism=3, err=(1, 8))
    want = A.reads_pair_overlap_np(b1, b2, len(pairs), 0, 0, o1, o2, 12, 3, 1, 8)
    assert np.count_nonzero(want[:, A.RP_INSERT]) >= 7
    for s1 in range(4):
        for s2 in (0, 1, 2, 3, 7, 13):
            run(ctx, b1, b2, len(pairs), 0, 0, o1, o2, shift1=s1, shift2=s2, want=want, **kw)
    # a descending offsets pair counts as an empty mate
    bad = o2.copy()
    bad[1] = o2[3]
    run(ctx, b1, b2, len(pairs), 0, 0, o1, bad, **kw)


def test_more_pairs_than_the_grid_has_waves_and_repeatable(ctx):
    rng = np.random.default_rng(35)
    n, L = 3 * 32768 + 5, 12
    frag = rng.choice(ACGT, (n, L)).astype(np.uint8)
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    m2 = comp[frag[:, ::-1]].copy()
    m2[1::2] = rng.choice(ACGT, m2[1::2].shape)              # every other pair: unrelated mates
    b1, b2 = frag.reshape(-1), m2.reshape(-1)
    d1, d2 = ctx.to_device(b1), ctx.to_device(b2)
    rows = u64(ctx.reads_pair_overlap(d1, d2, n, L, L, min_overlap=10, max_mism=0, max_error=(0, 1)))
    again = u64(ctx.reads_pair_overlap(d1, d2, n, L, L, min_overlap=10, max_mism=0, max_error=(0, 1)))
    assert rows.tobytes() == again.tobytes()
    assert (rows[0::2, A.RP_INSERT] == L).all()
    for lo in (0, 32768 - 20, n - 40):
        want = A.reads_pair_overlap_np(b1[lo * L:(lo + 40) * L], b2[lo * L:(lo + 40) * L], 40, L, L, None, None, 10, 0, 0, 1)
        assert (rows[lo:lo + 40] == want).all()


def test_argument_errors(ctx):
    import torch
    from kmers_amd._lib import Reads

    bases = ctx.to_device(np.full(64, ord("A"), np.uint8))
    rows = torch.zeros(4 * 4, dtype=torch.int64, device=ctx.device)
    r4, r3 = Reads(bases.data_ptr(), 4, 16, None), Reads(bases.data_ptr(), 3, 16, None)
    f = ctx.lib.kmx_reads_pair_overlap

    def call(a=r4, b=r4, min_overlap=5, max_mism=2, num=1, den=5, rw=rows, h=ctx._h):
        return f(h, C.byref(a) if a is not None else None, C.byref(b) if b is not None else None, min_overlap, max_mism, num, den, ptr(rw))

    assert call() == OK
    assert call(b=r3) == E_ARG and call(a=r3) == E_ARG and call(a=r3, b=r3) == OK      # the two batches differ in n_reads
    assert call(min_overlap=0) == E_ARG and call(den=0) == E_ARG and call(num=6) == E_ARG and call(num=5) == OK
    assert call(h=None) == E_ARG and call(a=None) == E_ARG and call(b=None) == E_ARG and call(rw=None) == E_ARG
    assert call(b=Reads(None, 4, 16, None)) == E_ARG                                  # reads without a d_bases
    none = Reads(None, 0, 16, None)
    assert call(a=none, b=none) == OK and call(a=none, b=none, den=0) == E_ARG         # no reads: a no-op, its arguments still checked
    ctx.synchronize()


@pytest.mark.parametrize("min_len", [0, 50])
def test_reads_trim_pairs_keeps_the_mates_in_step(ctx, min_len):
    rng = np.random.default_rng(36)
    n = 120
    shape = [(int(rng.integers(60, 151)), int(rng.integers(60, 151)), int(rng.integers(20, 400))) for _ in range(n)]
    pairs = [mates(rng, a, b, i, mism=int(rng.integers(0, 3))) for a, b, i in shape]
    b1, o1 = ragged([p[0] for p in pairs], first=2)
    b2, o2 = ragged([p[1] for p in pairs])
    got1, got2, rows = ctx.reads_trim_pairs(ctx.to_device(b1), ctx.to_device(b2), n, 150, 150, ctx.to_device(o1), ctx.to_device(o2), min_len=min_len)
    want = A.reads_pair_overlap_np(b1, b2, n, 0, 0, o1, o2, 30, 5, 1, 5)
    assert (u64(rows) == want).all()
    keep = ((want[:, A.RP_KEEP1] >> np.uint64(32)) >= min_len) & ((want[:, A.RP_KEEP2] >> np.uint64(32)) >= min_len)
    assert (min_len == 0 and keep.all()) or 0 < keep.sum() < n
    for batch, src, off, col in ((got1, b1, o1, A.RP_KEEP1), (got2, b2, o2, A.RP_KEEP2)):
        out, o, idx = reads_np.select_np(src, n, 0, off, keep=keep, span=want[:, col], span_k=0)
        assert batch.n_reads == len(idx) == int(keep.sum())
        assert (u64(batch.offsets) == o).all() and batch.bases.cpu().numpy().tobytes() == out.tobytes() and (u64(batch.index) == idx).all()
    assert (u64(got1.index) == u64(got2.index)).all()
    assert got1.n_bases < int(o1[-1] - o1[0])             # something was trimmed
