"""kmx_reads_pair_merge on the GPU (kmx_reads_merge.hip) and what the Python layer builds on it (Context.reads_pair_merge,
reads_merge_pairs).

Every comparison is equality of every output byte, offset word and row word with the host reference tests/merge_np.py (pinned
against a literal loop in tests/test_merge_np.py): there is no tolerance anywhere.  The raw call goes through `run`, which hands the
ABI four outputs with sentinels on both sides -- bytes around the bases and the quality bytes, words around the offsets and the
rows -- and looks at them afterwards."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import adapter_np as A
from tests import merge_np as M
from tests import reads_np
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import u64
from tests.reads_dev import SENT, SENT_WORD, dev_bytes, dev_words, ptr, ragged

pytestmark = pytest.mark.gpu

OK, E_ARG, E_NOMEM = 0, 1, 6
GB, GW = 32, 8                                # sentinel bytes / words on either side of an output
ACGT = np.frombuffer(b"ACGT", np.uint8)
JUNK = np.frombuffer(b"ACGTacgtN", np.uint8)


def seq(rng, n, alpha=ACGT):
    return rng.choice(alpha, n).astype(np.uint8).tobytes()


def quals_like(rng, bases, phred=33):
    """a quality byte per byte of the batch, some below phred"""
    return rng.integers(phred - 2, phred + 43, len(bases)).astype(np.uint8)


def mates(rng, L1, L2, insert, dirty=0):
    """both mates of a fragment of `insert` bases, read-through junk behind a short fragment; `dirty` bytes of either mate replaced
    by another letter, another case, N or '.': mismatches and invalid bytes inside the overlap"""
    frag = seq(rng, max(insert, 0))
    m1 = bytearray((frag + seq(rng, L1, JUNK))[:L1])
    m2 = bytearray((M.revcomp(frag) + seq(rng, L2, JUNK))[:L2])
    for m in (m1, m2):
        for i in (rng.choice(len(m), min(dirty, len(m)), replace=False) if len(m) else []):
            m[i] = int(rng.choice(np.frombuffer(b"ACGTacgtNn.", np.uint8)))
    return bytes(m1), bytes(m2)


class Guarded:
    """an output with sentinels on both sides: `n` elements at `shift` elements past the front sentinels"""

    def __init__(self, ctx, n, words, shift=0):
        import torch

        self.g, self.n, self.shift = (GW if words else GB), n, shift
        self.buf = torch.full((2 * self.g + shift + n,), SENT_WORD if words else SENT, dtype=torch.int64 if words else torch.uint8, device=ctx.device)
        self.sent = np.uint64(SENT_WORD & M.M64) if words else np.uint8(SENT)
        self.words = words

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + (self.g + self.shift) * (8 if self.words else 1))

    def host(self):
        h = self.buf.cpu().numpy()
        return h.view(np.uint64) if self.words else h

    def payload(self):
        """the n elements, after checking that nothing around them was written"""
        h, a = self.host(), self.g + self.shift
        assert (h[:a] == self.sent).all() and (h[a + self.n:] == self.sent).all(), "written outside the output"
        return h[a:a + self.n]

    def untouched(self):
        return bool((self.host() == self.sent).all())


def run(ctx, b1, b2, n, len1, len2, insert, off1=None, off2=None, q1=None, q2=None, phred=33, cap=41, in_shifts=(0, 0, 0, 0), out_shifts=(0, 0),
        rows=True, out_quals=True, want=None):
    """kmx_reads_pair_merge through the raw ABI into guarded outputs, everything compared with the reference -> the rows"""
    from kmers_amd._lib import Reads

    if want is None:
        want = M.reads_pair_merge_np(b1, b2, n, len1, len2, insert, q1, q2, off1, off2, phred, cap)
    w_bases, w_quals, w_off, w_rows = want
    nb = len(w_bases)
    d1, d2 = dev_bytes(ctx, b1, in_shifts[0]), dev_bytes(ctx, b2, in_shifts[1])
    dq1 = dev_bytes(ctx, q1, in_shifts[2]) if q1 is not None else None
    dq2 = dev_bytes(ctx, q2, in_shifts[3]) if q2 is not None else None
    d_o1, d_o2, d_ins = dev_words(ctx, off1), dev_words(ctx, off2), dev_words(ctx, np.asarray(insert).astype(np.uint64))
    r1 = Reads(d1.data_ptr() if n else None, n, len1, d_o1.data_ptr() if off1 is not None else None)
    r2 = Reads(d2.data_ptr() if n else None, n, len2, d_o2.data_ptr() if off2 is not None else None)
    g_b, g_o = Guarded(ctx, nb, False, out_shifts[0]), Guarded(ctx, n + 1, True)
    g_q = Guarded(ctx, nb, False, out_shifts[1]) if q1 is not None and out_quals else None
    g_r = Guarded(ctx, M.RM_WORDS * n, True) if rows else None
    nm, nbases = C.c_uint64(77), C.c_uint64(77)
    st = ctx.lib.kmx_reads_pair_merge(ctx._h, C.byref(r1), C.byref(r2), ptr(dq1), ptr(dq2), ptr(d_ins), 1, phred, cap, g_b.ptr(),
                                      g_q.ptr() if g_q else None, g_o.ptr(), g_r.ptr() if g_r else None, nb, C.byref(nm), C.byref(nbases))
    assert st == OK, ctx.lib.kmx_last_error(ctx._h)
    assert nbases.value == nb and nm.value == int(np.count_nonzero(w_rows[:, M.RM_LEN]))
    got_off = g_o.payload()
    assert (got_off == w_off).all(), (got_off[:8], w_off[:8])
    got = g_b.payload()
    bad = np.nonzero(got != w_bases)[0]
    assert len(bad) == 0, ("bases", int(bad[0]), int(np.searchsorted(w_off, bad[0], side="right")) - 1, got[bad[0]], w_bases[bad[0]])
    if g_q:
        got = g_q.payload()
        bad = np.nonzero(got != w_quals)[0]
        assert len(bad) == 0, ("quals", int(bad[0]), int(np.searchsorted(w_off, bad[0], side="right")) - 1, got[bad[0]], w_quals[bad[0]])
    if g_r:
        got = g_r.payload().reshape(n, M.RM_WORDS)
        bad = np.nonzero((got != w_rows).any(axis=1))[0]
        assert len(bad) == 0, ("rows", int(bad[0]), got[bad[0]].tolist(), w_rows[bad[0]].tolist())
    return w_rows


LENGTH_PAIRS = [(1, 1), (64, 64), (65, 63), (100, 150), (150, 100), (150, 150), (250, 250), (1024, 1024), (1025, 100), (0, 40)]


@pytest.mark.parametrize("L1,L2", LENGTH_PAIRS)
def test_length_pairs_and_inserts_at_every_boundary(ctx, L1, L2):
    """mate 1 uniform, mate 2 the same reads as a ragged batch at another alignment; the inserts sit on both sides of every boundary
    (1, the shorter mate, the longer mate, L1 + L2), the mates carry mismatches, N and lower case inside the overlap"""
    rng = np.random.default_rng(51 + L1 + 3 * L2)
    lo, hi = min(L1, L2), max(L1, L2)
    inserts = sorted(set(i for i in [1, 2, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, L1 + L2 - 1, L1 + L2] + rng.integers(1, L1 + L2 + 1, 5).tolist()
                         if i >= 0))
    pairs = [mates(rng, L1, L2, i, dirty=min(6, i // 4)) for i in inserts]
    n = len(pairs)
    b1 = np.frombuffer(b"".join(p[0] for p in pairs), np.uint8)
    b2, off2 = ragged([p[1] for p in pairs], first=3)
    q1, q2 = quals_like(rng, b1), quals_like(rng, b2)
    rows = run(ctx, b1, b2, n, L1, 0, np.array(inserts, np.uint64), None, off2, q1, q2, in_shifts=(1, 2, 3, 0), out_shifts=(1, 1))
    merged = rows[:, M.RM_LEN] != 0
    if 1 <= L1 <= M.RP_MAX_LEN and L2 >= 1:
        assert merged.tolist() == [0 < i < L1 + L2 for i in inserts]
        if L1 >= 64:
            assert (rows[:, M.RM_OVERLAP] >> np.uint64(32)).any() and (rows[:, M.RM_INVALID] != 0).any()   # DIS and invalid bytes occur
    else:
        assert not rows.any()


def test_insert_words_by_stride_from_the_overlap_rows_and_garbage_words(ctx):
    from kmers_amd._lib import Reads

    rng = np.random.default_rng(52)
    shape = [(150, 150, 90), (150, 150, 210), (100, 150, 120), (150, 100, 249), (80, 80, 400), (64, 64, 64), (40, 0, 30), (150, 150, 31)]
    pairs = [mates(rng, a, b, i, dirty=1) for a, b, i in shape]
    n = len(pairs)
    (b1, o1), (b2, o2) = ragged([p[0] for p in pairs], first=1), ragged([p[1] for p in pairs])
    q1, q2 = quals_like(rng, b1), quals_like(rng, b2)
    d1, d2, dq1, dq2 = (ctx.to_device(x) for x in (b1, b2, q1, q2))
    d_o1, d_o2 = ctx.to_device(o1), ctx.to_device(o2)
    ov = ctx.reads_pair_overlap(d1, d2, n, 0, 0, d_o1, d_o2, min_overlap=20, max_mism=8)
    insert = u64(ov)[:, A.RP_INSERT].copy()
    assert np.count_nonzero(insert) >= 5 and (insert == 0).any()
    want = M.reads_pair_merge_np(b1, b2, n, 0, 0, insert, q1, q2, o1, o2)
    # the raw call with (rows + KMX_RP_INSERT, KMX_RP_WORDS): no array in between
    g_b, g_q, g_o, g_r = Guarded(ctx, len(want[0]), False), Guarded(ctx, len(want[0]), False), Guarded(ctx, n + 1, True), Guarded(ctx, 4 * n, True)
    r1, r2 = Reads(d1.data_ptr(), n, 0, d_o1.data_ptr()), Reads(d2.data_ptr(), n, 0, d_o2.data_ptr())
    nm, nb = C.c_uint64(0), C.c_uint64(0)
    st = ctx.lib.kmx_reads_pair_merge(ctx._h, C.byref(r1), C.byref(r2), ptr(dq1), ptr(dq2), C.c_void_p(ov.data_ptr() + 8 * A.RP_INSERT), A.RP_WORDS, 33, 41,
                                      g_b.ptr(), g_q.ptr(), g_o.ptr(), g_r.ptr(), len(want[0]), C.byref(nm), C.byref(nb))
    assert st == OK, ctx.lib.kmx_last_error(ctx._h)
    assert g_b.payload().tobytes() == want[0].tobytes() and g_q.payload().tobytes() == want[1].tobytes()
    assert (g_o.payload() == want[2]).all() and (g_r.payload().reshape(n, 4) == want[3]).all()
    # the Python layer takes the column view as it is
    b, q, rows = ctx.reads_pair_merge(d1, d2, n, 0, 0, ov[:, A.RP_INSERT], dq1, dq2, d_o1, d_o2)
    assert b.bases.cpu().numpy().tobytes() == want[0].tobytes() and q.bases.cpu().numpy().tobytes() == want[1].tobytes()
    assert (u64(b.offsets) == want[2]).all() and (u64(q.offsets) == want[2]).all() and (u64(rows) == want[3]).all() and b.n_reads == n
    # a plain array with garbage words: each gives one defined answer
    garbage = np.array([0, M.M64, 1 << 63, 1 << 32 | 5, 160, 2**31, 64, 299], np.uint64)
    rows = run(ctx, b1, b2, n, 0, 0, garbage, o1, o2, q1, q2)
    assert (rows[:, M.RM_LEN] != 0).tolist() == [False, False, False, False, False, False, False, True]


def _ragged_case(rng):
    shape = [(150, 150, 90), (0, 40, 5), (40, 0, 5), (151, 149, 200), (100, 100, 100), (1, 1, 1), (250, 101, 180), (64, 128, 70), (150, 150, 299),
             (1024, 300, 500), (1025, 1025, 800), (33, 31, 12), (150, 150, 35), (5, 9, 13), (7, 7, 3), (150, 150, 300)]
    pairs = [mates(rng, a, b, i, dirty=2) for a, b, i in shape]
    (b1, o1), (b2, o2) = ragged([p[0] for p in pairs], first=6), ragged([p[1] for p in pairs], first=1)
    return b1, o1, b2, o2, np.array([i for _, _, i in shape], np.uint64), len(shape)


def test_every_input_alignment_of_the_four_buffers(ctx):
    rng = np.random.default_rng(53)
    b1, o1, b2, o2, insert, n = _ragged_case(rng)
    q1, q2 = quals_like(rng, b1), quals_like(rng, b2)
    want = M.reads_pair_merge_np(b1, b2, n, 0, 0, insert, q1, q2, o1, o2)
    assert np.count_nonzero(want[3][:, M.RM_LEN]) >= 10
    for shifts in itertools.product(range(4), repeat=4):
        run(ctx, b1, b2, n, 0, 0, insert, o1, o2, q1, q2, in_shifts=shifts, want=want)
    # a descending offsets pair counts as an empty mate
    bad = o2.copy()
    bad[1] = o2[3]
    run(ctx, b1, b2, n, 0, 0, insert, o1, bad, q1, q2)


def test_every_output_alignment_of_bases_and_quality_bytes(ctx):
    rng = np.random.default_rng(54)
    b1, o1, b2, o2, insert, n = _ragged_case(rng)
    q1, q2 = quals_like(rng, b1), quals_like(rng, b2)
    want = M.reads_pair_merge_np(b1, b2, n, 0, 0, insert, q1, q2, o1, o2)
    assert len(set((want[2] % np.uint64(4)).tolist())) == 4           # the ragged output itself puts reads at every alignment
    for sb, sq in itertools.product((0, 1, 2, 3, 7, 13), repeat=2):
        run(ctx, b1, b2, n, 0, 0, insert, o1, o2, q1, q2, in_shifts=(1, 0, 2, 3), out_shifts=(sb, sq), want=want)
    run(ctx, b1, b2, n, 0, 0, insert, o1, o2, q1, q2, out_quals=False, want=want)   # the quality bytes decide, none are written


def test_without_quality_bytes_mate_1_wins(ctx):
    rng = np.random.default_rng(55)
    b1, o1, b2, o2, insert, n = _ragged_case(rng)
    for sb in (0, 3):
        rows = run(ctx, b1, b2, n, 0, 0, insert, o1, o2, out_shifts=(sb, 0), in_shifts=(2, 1, 0, 0))
    assert (rows[:, M.RM_OVERLAP] >> np.uint64(32)).any()
    assert not (rows[:, M.RM_TAKEN] & np.uint64(0xFFFFFFFF)).any()
    assert ((rows[:, M.RM_TAKEN] >> np.uint64(32)) == (rows[:, M.RM_OVERLAP] >> np.uint64(32))).all()   # every DIS is a tie


@pytest.mark.parametrize("phred,cap", [(33, 0), (33, 41), (33, 255 - 33), (64, 255 - 64), (0, 255)])
def test_q_cap_and_phred_base(ctx, phred, cap):
    rng = np.random.default_rng(56)
    b1, o1, b2, o2, insert, n = _ragged_case(rng)
    q1, q2 = rng.integers(0, 256, len(b1)).astype(np.uint8), rng.integers(0, 256, len(b2)).astype(np.uint8)   # every byte value
    run(ctx, b1, b2, n, 0, 0, insert, o1, o2, q1, q2, phred=phred, cap=cap, out_shifts=(2, 2))


def test_count_only_and_max_bases(ctx):
    from kmers_amd._lib import Reads

    rng = np.random.default_rng(57)
    b1, o1, b2, o2, insert, n = _ragged_case(rng)
    q1, q2 = quals_like(rng, b1), quals_like(rng, b2)
    w_bases, w_quals, w_off, w_rows = M.reads_pair_merge_np(b1, b2, n, 0, 0, insert, q1, q2, o1, o2)
    nb_want, nm_want = len(w_bases), int(np.count_nonzero(w_rows[:, M.RM_LEN]))
    d1, d2, dq1, dq2 = (dev_bytes(ctx, x, s) for x, s in ((b1, 1), (b2, 2), (q1, 3), (q2, 0)))
    d_o1, d_o2, d_ins = dev_words(ctx, o1), dev_words(ctx, o2), dev_words(ctx, insert)
    r1, r2 = Reads(d1.data_ptr(), n, 0, d_o1.data_ptr()), Reads(d2.data_ptr(), n, 0, d_o2.data_ptr())

    def call(g_b, g_q, g_o, g_r, max_bases):
        nm, nb = C.c_uint64(77), C.c_uint64(77)
        st = ctx.lib.kmx_reads_pair_merge(ctx._h, C.byref(r1), C.byref(r2), ptr(dq1), ptr(dq2), ptr(d_ins), 1, 33, 41, g_b.ptr() if g_b else None,
                                          g_q.ptr() if g_q else None, g_o.ptr() if g_o else None, g_r.ptr() if g_r else None, max_bases, C.byref(nm),
                                          C.byref(nb))
        return st, nm.value, nb.value

    # count only, without and with rows
    assert call(None, None, None, None, 0) == (OK, nm_want, nb_want)
    g_r = Guarded(ctx, 4 * n, True)
    assert call(None, None, None, g_r, 0) == (OK, nm_want, nb_want)
    assert (g_r.payload().reshape(n, 4) == w_rows).all()
    # one byte short: the counts, and nothing of the batch written (sentinels and payload alike)
    g_b, g_q, g_o = Guarded(ctx, nb_want, False), Guarded(ctx, nb_want, False), Guarded(ctx, n + 1, True)
    assert call(g_b, g_q, g_o, None, nb_want - 1) == (E_NOMEM, nm_want, nb_want)
    assert g_b.untouched() and g_q.untouched() and g_o.untouched()
    # exact
    assert call(g_b, g_q, g_o, None, nb_want) == (OK, nm_want, nb_want)
    assert g_b.payload().tobytes() == w_bases.tobytes() and g_q.payload().tobytes() == w_quals.tobytes() and (g_o.payload() == w_off).all()


def test_working_set_at_the_work_buffer_cap_and_one_below(ctx):
    """kmx.h states it: 16 bytes per 2 048 pairs and six words, in units of 256 bytes"""
    from kmers_amd._lib import Reads

    n, L = 2 * 2048 * 8 + 1, 4                       # 17 blocks of pairs: 8 * (2 * 17 + 6) = 320 bytes, 512 laid out
    bases = ctx.to_device(np.full(n * L, ord("A"), np.uint8))
    insert = ctx.to_device(np.full(n, 5, np.uint64))
    r = Reads(bases.data_ptr(), n, L, None)
    g_r = Guarded(ctx, 4 * n, True)
    nm, nb = C.c_uint64(77), C.c_uint64(77)
    call = lambda: ctx.lib.kmx_reads_pair_merge(ctx._h, C.byref(r), C.byref(r), None, None, ptr(insert), 1, 33, 41, None, None, None, g_r.ptr(), 0,  # noqa: E731
                                                C.byref(nm), C.byref(nb))
    try:
        ctx.set_work_buffer_limit(511)
        assert call() == E_NOMEM and (nm.value, nb.value) == (0, 0) and g_r.untouched()
        ctx.set_work_buffer_limit(512)
        assert call() == OK and (nm.value, nb.value) == (n, 5 * n)
    finally:
        ctx.set_work_buffer_limit(0)
    assert (g_r.payload().reshape(n, 4) == np.array([5, 3 | 3 << 32, 3 << 32, 0], np.uint64)).all()   # TTTT over AAAA: three positions, all DIS, all tied


def test_more_pairs_than_the_grid_has_waves_and_repeatable(ctx):
    rng = np.random.default_rng(58)
    n, L = 3 * 32768 + 5, 12
    frag = rng.choice(JUNK, (n, L)).astype(np.uint8)
    m2 = rng.choice(JUNK, (n, L)).astype(np.uint8)
    insert = rng.integers(1, 2 * L, n).astype(np.uint64)
    insert[1::2] = rng.choice(np.array([0, 2 * L, 2 * L + 3, 1 << 40], np.uint64), len(insert[1::2]))   # every other pair: not merged
    b1, b2 = frag.reshape(-1), m2.reshape(-1)
    q1, q2 = quals_like(rng, b1), quals_like(rng, b2)
    d1, d2, dq1, dq2, d_ins = (ctx.to_device(x) for x in (b1, b2, q1, q2, insert))
    b, q, rows = ctx.reads_pair_merge(d1, d2, n, L, L, d_ins, dq1, dq2)
    b_again, q_again, rows_again = ctx.reads_pair_merge(d1, d2, n, L, L, d_ins, dq1, dq2)
    got_b, got_q, got_off, got_rows = b.bases.cpu().numpy(), q.bases.cpu().numpy(), u64(b.offsets), u64(rows)
    assert got_b.tobytes() == b_again.bases.cpu().numpy().tobytes() and got_q.tobytes() == q_again.bases.cpu().numpy().tobytes()
    assert got_off.tobytes() == u64(b_again.offsets).tobytes() and got_rows.tobytes() == u64(rows_again).tobytes()
    assert (got_rows[0::2, M.RM_LEN] == insert[0::2]).all() and not got_rows[1::2].any()
    assert got_off[0] == 0 and (np.diff(got_off.astype(np.int64)) == got_rows[:, M.RM_LEN].astype(np.int64)).all() and got_off[-1] == len(got_b)
    for lo in (0, 32768 - 20, n - 40):
        s = slice(lo * L, (lo + 40) * L)
        w_bases, w_quals, w_off, w_rows = M.reads_pair_merge_np(b1[s], b2[s], 40, L, L, insert[lo:lo + 40], q1[s], q2[s])
        a, e = int(got_off[lo]), int(got_off[lo + 40])
        assert (got_rows[lo:lo + 40] == w_rows).all() and (got_off[lo:lo + 41] - got_off[lo] == w_off).all()
        assert got_b[a:e].tobytes() == w_bases.tobytes() and got_q[a:e].tobytes() == w_quals.tobytes()


def test_argument_errors(ctx):
    import torch
    from kmers_amd._lib import Reads

    bases = ctx.to_device(np.full(64, ord("A"), np.uint8))
    quals = ctx.to_device(np.full(64, ord("I"), np.uint8))
    insert = ctx.to_device(np.full(4, 20, np.uint64))
    out_b, out_q = torch.zeros(128, dtype=torch.uint8, device=ctx.device), torch.zeros(128, dtype=torch.uint8, device=ctx.device)
    out_o, rows = torch.zeros(5, dtype=torch.int64, device=ctx.device), torch.zeros(16, dtype=torch.int64, device=ctx.device)
    r4, r3 = Reads(bases.data_ptr(), 4, 16, None), Reads(bases.data_ptr(), 3, 16, None)
    nm, nb = C.c_uint64(0), C.c_uint64(0)
    f = ctx.lib.kmx_reads_pair_merge
    U = object()   # "use the default"

    def call(a=r4, b=r4, q1=quals, q2=quals, ins=insert, stride=1, phred=33, cap=41, ob=out_b, oq=out_q, oo=out_o, rw=rows, max_bases=128, h=U,
             hm=U, hb=U):
        return f(ctx._h if h is U else h, C.byref(a) if a is not None else None, C.byref(b) if b is not None else None, ptr(q1), ptr(q2), ptr(ins), stride,
                 phred, cap, ptr(ob), ptr(oq), ptr(oo), ptr(rw), max_bases, C.byref(nm) if hm is U else hm, C.byref(nb) if hb is U else hb)

    assert call() == OK and (nm.value, nb.value) == (4, 80)
    assert call(b=r3) == E_ARG and call(a=r3) == E_ARG and call(a=r3, b=r3) == OK           # the two batches differ in n_reads
    assert call(stride=0) == E_ARG and call(ins=None) == E_ARG
    assert call(q1=None) == E_ARG and call(q2=None) == E_ARG                                # exactly one of the two
    assert call(q1=None, q2=None) == E_ARG and call(q1=None, q2=None, oq=None) == OK        # d_out_quals without input qualities
    assert call(ob=None) == E_ARG and call(oo=None) == E_ARG                                # exactly one of bases / offsets
    assert call(ob=None, oo=None) == E_ARG and call(ob=None, oo=None, oq=None) == OK        # count only: d_out_quals NULL as well
    assert call(oq=None) == OK and call(rw=None) == OK
    assert call(phred=215, cap=41) == E_ARG and call(phred=214, cap=41) == OK and call(phred=0, cap=256) == E_ARG
    assert call(h=None) == E_ARG and call(a=None) == E_ARG and call(b=None) == E_ARG and call(hm=None) == E_ARG and call(hb=None) == E_ARG
    assert call(b=Reads(None, 4, 16, None)) == E_ARG                                        # reads without a d_bases
    assert call(max_bases=79) == E_NOMEM and (nm.value, nb.value) == (4, 80)
    # outputs that overlap the inputs
    assert call(ob=bases) == E_ARG and call(oq=quals) == E_ARG and call(rw=insert) == E_ARG and call(ob=quals) == E_ARG
    off = ctx.to_device(np.arange(0, 80, 16, dtype=np.uint64))
    assert call(a=Reads(bases.data_ptr(), 4, 0, off.data_ptr()), oo=off) == E_ARG
    none = Reads(None, 0, 16, None)
    assert call(a=none, b=none) == OK and (nm.value, nb.value) == (0, 0)                    # no pairs: a no-op ...
    assert call(a=none, b=none, phred=250) == E_ARG and call(a=none, b=none, q1=None) == E_ARG   # ... its arguments still checked
    ctx.synchronize()


def test_reads_merge_pairs_partitions_the_pairs(ctx):
    rng = np.random.default_rng(59)
    n = 120
    shape = [(int(rng.integers(60, 151)), int(rng.integers(60, 151)), int(rng.integers(20, 400))) for _ in range(n)]
    pairs = [mates(rng, a, b, i, dirty=int(rng.integers(0, 3))) for a, b, i in shape]
    (b1, o1), (b2, o2) = ragged([p[0] for p in pairs], first=2), ragged([p[1] for p in pairs])
    q1, q2 = quals_like(rng, b1), quals_like(rng, b2)
    got = ctx.reads_merge_pairs(ctx.to_device(b1), ctx.to_device(b2), n, 150, 150, ctx.to_device(q1), ctx.to_device(q2), ctx.to_device(o1),
                                ctx.to_device(o2))
    w_ov = A.reads_pair_overlap_np(b1, b2, n, 0, 0, o1, o2, 30, 5, 1, 5)
    w_bases, w_quals, w_off, w_rows = M.reads_pair_merge_np(b1, b2, n, 0, 0, w_ov[:, A.RP_INSERT], q1, q2, o1, o2)
    assert (u64(got.overlap_rows) == w_ov).all() and (u64(got.merge_rows) == w_rows).all()
    keep = w_rows[:, M.RM_LEN] != 0
    assert 20 < keep.sum() < n - 20

    def same(batch, src, off, kp, index=True):
        out, o, idx = reads_np.select_np(src, n, 0, off, keep=kp)
        assert batch.n_reads == len(idx) and (u64(batch.offsets) == o).all() and batch.bases.cpu().numpy().tobytes() == out.tobytes()
        assert not index or (u64(batch.index) == idx).all()

    same(got.merged, w_bases, w_off, keep)
    same(got.merged_quals, w_quals, w_off, keep, index=False)
    same(got.unmerged1, b1, o1, ~keep)
    same(got.unmerged2, b2, o2, ~keep)
    same(got.unmerged1_quals, q1, o1, ~keep, index=False)
    same(got.unmerged2_quals, q2, o2, ~keep, index=False)
    both = np.sort(np.concatenate([u64(got.merged.index), u64(got.unmerged1.index)]))
    assert (both == np.arange(n)).all() and (u64(got.unmerged1.index) == u64(got.unmerged2.index)).all()
    assert (u64(got.merged.offsets) == u64(got.merged_quals.offsets)).all()


def test_merged_error_free_fragments_count_as_the_fragments(ctx):
    """what merging is for: the k-mers of the merged reads are the k-mers of the fragments, each once -- those across the junction
    included, those of the overlap not twice"""
    rng = np.random.default_rng(60)
    n, L1, L2, k = 200, 150, 140, 31
    frags = [seq(rng, int(rng.integers(40, L1 + L2 - 30))) for _ in range(n)]
    m1 = [(f + seq(rng, L1))[:L1] for f in frags]
    m2 = [(M.revcomp(f) + seq(rng, L2))[:L2] for f in frags]
    b1, b2 = np.frombuffer(b"".join(m1), np.uint8), np.frombuffer(b"".join(m2), np.uint8)
    got = ctx.reads_merge_pairs(ctx.to_device(b1), ctx.to_device(b2), n, L1, L2)
    assert got.merged.n_reads == n and got.unmerged1.n_reads == 0 and got.merged_quals is None
    fb, fo = ragged(frags)
    assert got.merged.bases.cpu().numpy().tobytes() == fb.tobytes() and (u64(got.merged.offsets) == fo).all()
    kmers, counts = ctx.count_canonical(got.merged.bases, n, got.merged.max_len(), k, offsets=got.merged.offsets)
    w_kmers, w_counts = ctx.count_canonical(ctx.to_device(fb), n, max(len(f) for f in frags), k, offsets=ctx.to_device(fo))
    assert kmers.numel() > 0 and u64(kmers).tobytes() == u64(w_kmers).tobytes() and u64(counts).tobytes() == u64(w_counts).tobytes()
