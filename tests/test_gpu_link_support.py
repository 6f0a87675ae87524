"""Read support of the unitig links on the GPU: kmx_count_link_support and kmx_count_adjacency_cut (kmx_count_link_support.hip), and
what the Python layer builds on them (Context.count_link_support, count_cut_links, count_prune_links(2), LinkSupport).

Every comparison is u64 (or byte) equality of whole arrays with the sequential host reference tests/link_support_np.py (pinned against
Python strings in tests/test_link_support_np.py).  Both calls read index arrays only, so the reference is run over the very arrays the
device call was given -- the segments, unitigs and links the existing, separately tested calls made on the device -- and, for the
garbage cases, over arrays built on the host.  No test needs a tolerance.  Every family asserts of its own input that it holds what it
is there for."""
import numpy as np
import pytest

from tests import link_np, link_support_np
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import random_reads, u64
from tests.test_gpu_read_paths import COMP, _ragged, _rc
from tests.test_gpu_unitig_links import Linked

pytestmark = pytest.mark.gpu

E_ARG = 1
POISON = -0x5A5A5A5A5A5A5A5B
GUARD = 32


def dev(ctx, a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(ctx.device)


class Threaded:
    """a table (the k-mers of `table_seqs`) with its graph, and a batch of reads threaded through it: all made on the device by the
    calls the other test files cover, with host copies of what the two new calls read"""

    def __init__(self, ctx, k, table_seqs, reads, min_count=1):
        two = k > 32
        self.ctx, self.k, self.two = ctx, k, two
        bases, offsets = _ragged(table_seqs)
        d_k, d_c = (ctx.count_canonical2 if two else ctx.count_canonical)(ctx.to_device(bases), len(offsets) - 1, 0, k, offsets=ctx.to_device(offsets))
        self.x = Linked(ctx, k, d_k, d_c, min_count)
        self.links = self.x.links()
        self.lo, self.tg = u64(self.links.offsets), u64(self.links.targets)
        self.set_reads(reads)

    def set_reads(self, reads):
        ctx, x = self.ctx, self.x
        rb, ro = _ragged(reads)
        self.reads, self.d_bases, self.d_roff, self.n_reads = reads, ctx.to_device(rb), ctx.to_device(ro), len(reads)
        paths = ctx.count_read_paths2 if self.two else ctx.count_read_paths
        self.paths = paths(self.d_bases, self.n_reads, 0, self.k, x.d_k, x.unitigs, place=x.d_place, offsets=self.d_roff)
        self.segs = u64(self.paths.segments).reshape(-1, 4)
        self._want = None

    def want(self):
        if self._want is None:
            self._want = link_support_np.link_support_np(self.segs, self.x.uoff, self.lo, self.tg)
        return self._want

    def support(self, out=None):
        return self.ctx.count_link_support(self.paths, self.x.unitigs, self.links, out=out)


def check(t, twice=False):
    """the device's support and summary against the reference's, every word; -> (support, summary) on the host"""
    want, want_summary = t.want()
    got = t.support()
    assert np.array_equal(u64(got.support), want), (t.k, "support")
    assert np.array_equal(u64(got.summary), want_summary), (t.k, u64(got.summary), want_summary)
    assert (got.junctions, got.crossed, got.unlinked) == tuple(int(v) for v in want_summary)
    if twice:                                                            # accumulated into: exactly twice, and the same bytes again
        again = t.support(out=got)
        assert again is got
        assert np.array_equal(u64(got.support), 2 * want) and np.array_equal(u64(got.summary), 2 * want_summary)
    return want, want_summary


# ---------------------------------------------------------------- the main case
_MAIN = {}


def _main_input():
    """a genome of 20 000 bases with three copied repeats; five pieces of it with a substitution no read has (their k-mers are in the
    table, the links into them are walked by nobody); 2 000 reads of 30 .. 150 bases, both strands, 1 % substitutions, some with an N"""
    rng = np.random.default_rng(7100)
    g = random_reads(rng, 20_000)
    for src, dst, n in ((1000, 9000, 300), (3000, 15_000, 120), (5000, 17_500, 60)):
        g[dst:dst + n] = g[src:src + n]
    pieces = []
    for at in (2100, 6100, 11_100, 13_100, 19_100):
        p = g[at - 80:at + 80].copy()
        p[80] = COMP[p[80]]
        pieces.append(p)
    reads = []
    for i in range(2000):
        L = int(rng.integers(30, 151))
        a = int(rng.integers(0, len(g) - L + 1))
        r = g[a:a + L].copy()
        flip = rng.random(L) < 0.01
        r[flip] = COMP[r[flip]]
        if i % 37 == 0:
            r[L // 3] = ord("N")
        reads.append(_rc(r) if i % 2 else r)
    return g, pieces, reads


def _main(ctx, k):
    if k not in _MAIN or _MAIN[k].ctx is not ctx:
        g, pieces, reads = _main_input()
        _MAIN[k] = Threaded(ctx, k, reads + [g] + pieces, reads)
    return _MAIN[k]


@pytest.mark.parametrize("k", (21, 33))
def test_main_case(ctx, k):
    """case 1, and the same once through the two-word calls"""
    t = _main(ctx, k)
    assert t.paths.n_segments > 2000 and t.links.n_links > 100
    support, summary = check(t, twice=True)
    assert int(summary[2]) == 0 and int(summary[0]) == int(summary[1]) > 1000     # unlinked == 0
    assert (support == 0).any() and (support > 1).any()
    pairs = link_np.link_pairs(t.lo, t.tg)
    by_pair = dict(zip(pairs, support.tolist()))
    assert all(by_pair[(b ^ 1, a ^ 1)] == s for (a, b), s in by_pair.items())      # odd k: a link and its mirror carry the same number


# ---------------------------------------------------------------- one long read over a dense graph
def test_one_read_that_owns_hundreds_of_segments(ctx):
    """case 2: a read of 3 000 bases over its own graph at k = 5 -- 512 canonical 5-mers, nearly every node a fork, nearly every
    window a segment of its own -- so junctions straddle every wave and block boundary and the read takes the long-read route; a
    second read of one window ends the batch with a segment that has no junction"""
    rng = np.random.default_rng(7200)
    long_read = random_reads(rng, 3000)
    t = Threaded(ctx, 5, [long_read], [long_read, long_read[40:45].copy()])
    po = u64(t.paths.offsets)
    assert int(po[1]) - int(po[0]) > 600 and int(po[2]) - int(po[1]) == 1
    support, summary = check(t, twice=True)
    assert int(summary[2]) == 0 and int(summary[1]) > 600
    # n_segments 0 and 1: no pair, nothing is added
    from kmers_amd.api import ReadPaths

    for n in (0, 1):
        got = ctx.count_link_support(ReadPaths(t.paths.offsets, t.paths.segments[:n], 5), t.x.unitigs, t.links)
        assert not u64(got.support).any() and not u64(got.summary).any()
    # the first two segments alone: one pair
    got = ctx.count_link_support(ReadPaths(t.paths.offsets, t.paths.segments[:2], 5), t.x.unitigs, t.links)
    want, want_summary = link_support_np.link_support_np(t.segs[:2], t.x.uoff, t.lo, t.tg)
    assert np.array_equal(u64(got.support), want) and np.array_equal(u64(got.summary), want_summary) and int(want_summary[0]) == 1


# ---------------------------------------------------------------- contention
def test_five_thousand_reads_on_one_link(ctx):
    """case 3: 5 000 copies of a read that crosses one link: exactly 5 000 on the link and on its mirror, nothing anywhere else"""
    rng = np.random.default_rng(7300)
    k = 21
    g = random_reads(rng, 300)
    v = g.copy()
    v[200] = COMP[v[200]]
    read = g[150:215].copy()                                             # windows 150 .. 194: out of the left arm into one branch
    t = Threaded(ctx, k, [g, v], [read] * 5000)
    assert t.paths.n_segments == 10_000
    support, summary = check(t)
    assert summary.tolist() == [5000, 5000, 0]
    hot = np.nonzero(support)[0]
    assert len(hot) == 2 and support[hot].tolist() == [5000, 5000]
    pairs = link_np.link_pairs(t.lo, t.tg)
    (a, b), (c, d) = pairs[int(hot[0])], pairs[int(hot[1])]
    assert (c, d) == (b ^ 1, a ^ 1)


# ---------------------------------------------------------------- circle, hairpin, even k, garbage
def test_circle_and_hairpin(ctx):
    """case 4: the self-link across the written start of a circular unitig, and the link of a unitig to its own mirror"""
    rng = np.random.default_rng(7400)
    k, m = 31, 300
    circle = random_reads(rng, m)
    four = np.concatenate([circle] * 4)
    laps = [four[a:a + 2 * m + m // 2 + k - 1] for a in (3, m // 4, m // 2)]
    t = Threaded(ctx, k, [np.concatenate([circle, circle[:k - 1]])], laps + [_rc(x) for x in laps] + [circle])
    assert t.x.U == 1 and int(t.x.unitigs.circular[0]) == 1
    support, summary = check(t, twice=True)
    assert link_np.link_pairs(t.lo, t.tg) == [(0, 0), (1, 1)]
    assert int(summary[2]) == 0 and support[0] == support[1] and 12 <= int(support[0]) <= 19   # two or three passages per read of laps

    k = 21
    stem = random_reads(rng, 60)
    hp = np.concatenate([stem, _rc(stem)])
    t = Threaded(ctx, k, [hp], [hp, hp, _rc(hp), hp[k:-k].copy(), stem])
    assert t.x.U == 1
    support, summary = check(t)
    assert link_np.link_pairs(t.lo, t.tg) == [(0, 1)] or link_np.link_pairs(t.lo, t.tg) == [(1, 0)]
    assert support.tolist() == [4] and summary.tolist() == [4, 4, 0]               # its own mirror: once per crossing


def test_even_k_on_a_dense_table(ctx):
    """case 4: k = 6 over most of the 2 080 canonical 6-mers, palindromes among them: the rule as written"""
    rng = np.random.default_rng(7500)
    s = random_reads(rng, 3000)
    t = Threaded(ctx, 6, [s], [s, _rc(s), s[100:400].copy()])
    assert t.x.palindromic_unitigs()
    support, summary = check(t, twice=True)
    assert int(summary[1]) > 1000


@pytest.mark.parametrize("n_segments", (300, 70_001))
def test_garbage_inputs_give_the_defined_result(ctx, n_segments):
    """case 4: unitig indices beyond U, targets beyond 2 U, link and unitig offsets that do not ascend, lists longer than four, lengths
    of zero: every index is compared with its bound before it is used, so the call returns the reference's defined result and writes
    nothing outside support and summary (guard words behind both)"""
    import torch

    from kmers_amd.api import _ptr

    rng = np.random.default_rng(7600 + n_segments)
    n_unitigs = 6
    offsets = np.cumsum(rng.integers(0, 5, n_unitigs + 1)).astype(np.uint64)
    offsets[[2, 4]] = offsets[[4, 2]]                                    # (they descend somewhere)
    lo = np.concatenate([[0], np.cumsum(rng.integers(0, 5, 2 * n_unitigs))]).astype(np.uint64)
    n_links = int(lo[-1])
    lo[[4, 11]] = (2**63, n_links + 5)                                   # (not ascending; beyond the links)
    tg = rng.integers(0, 2 * n_unitigs + 4, n_links).astype(np.uint64)
    size = np.maximum(np.diff(offsets.astype(np.int64)), 0)
    u = rng.integers(0, n_unitigs + 2, n_segments)
    d = rng.integers(0, 2, n_segments)
    m = size[np.minimum(u, n_unitigs - 1)]
    fits = rng.random(n_segments) < 0.8                                  # a segment that spans its unitig ends on the exit and starts on the entry
    length = np.where(fits, m, rng.integers(0, 4, n_segments))
    q = np.where(fits, np.where(d == 0, 0, np.maximum(m - 1, 0)), rng.integers(0, 6, n_segments))
    gap = rng.integers(0, 6, n_segments) == 0
    start = np.concatenate([[0], np.cumsum(length + gap)[:-1]]) % 2**32
    segs = np.zeros((n_segments, 4), np.uint64)
    segs[:, 0] = np.sort(rng.integers(0, max(n_segments // 50, 2), n_segments))
    segs[:, 1] = (length.astype(np.uint64) << np.uint64(32)) | start.astype(np.uint64)
    segs[:, 2] = u
    segs[:, 3] = (q.astype(np.uint64) << np.uint64(1)) | d.astype(np.uint64)
    segs[::97, 2] = 2**64 - 1
    want, want_summary = link_support_np.link_support_np(segs, offsets, lo, tg)
    assert int(want_summary[1]) > 0 and int(want_summary[2]) > 0 and (want > 0).any()
    d_support = torch.full((n_links + GUARD,), POISON, dtype=torch.int64, device=ctx.device)
    d_summary = torch.full((3 + GUARD,), POISON, dtype=torch.int64, device=ctx.device)
    d_support[:n_links] = 0
    d_summary[:3] = 0
    d_segs, d_off, d_lo, d_tg = dev(ctx, segs), dev(ctx, offsets), dev(ctx, lo), dev(ctx, tg)
    st = ctx.lib.kmx_count_link_support(ctx._h, _ptr(d_segs), n_segments, _ptr(d_off), n_unitigs, _ptr(d_lo), _ptr(d_tg), n_links, _ptr(d_support),
                                        _ptr(d_summary))
    ctx.synchronize()
    assert st == 0
    got, got_summary = u64(d_support), u64(d_summary)
    assert np.array_equal(got[:n_links], want) and np.array_equal(got_summary[:3], want_summary)
    poison = np.uint64(POISON & (2**64 - 1))
    assert (got[n_links:] == poison).all() and (got_summary[3:] == poison).all()
    # argument errors: nothing is launched
    assert ctx.lib.kmx_count_link_support(None, _ptr(d_segs), n_segments, _ptr(d_off), n_unitigs, _ptr(d_lo), _ptr(d_tg), n_links, _ptr(d_support),
                                          _ptr(d_summary)) == E_ARG
    assert ctx.lib.kmx_count_link_support(ctx._h, _ptr(d_segs), n_segments, _ptr(d_off), n_unitigs, _ptr(d_lo), _ptr(d_tg), n_links, _ptr(d_support),
                                          None) == E_ARG
    assert ctx.lib.kmx_count_link_support(ctx._h, None, n_segments, _ptr(d_off), n_unitigs, _ptr(d_lo), _ptr(d_tg), n_links, _ptr(d_support),
                                          _ptr(d_summary)) == E_ARG


# ---------------------------------------------------------------- identity with the counter at k + 1
def test_support_is_the_count_of_the_link_at_k_plus_one(ctx):
    """case 5: every link's 22-mer, spelled from the unitigs' sequences, counted in the same reads by count_canonical at k = 22 and
    looked up: the count is the support, on every link"""
    k = 21
    t = _main(ctx, k)
    support, _ = t.want()
    seq = t.x.unitigs.sequences().cpu().numpy()
    uoff = t.x.uoff.astype(np.int64)
    word = lambda u: seq[uoff[u] + u * (k - 1):uoff[u + 1] + (u + 1) * (k - 1)]
    oriented = lambda t_: word(t_ >> 1) if t_ & 1 == 0 else _rc(word(t_ >> 1))
    pairs = link_np.link_pairs(t.lo, t.tg)
    mers = np.concatenate([np.concatenate([oriented(a)[-k:], oriented(b)[k - 1:k]]) for a, b in pairs]).astype(np.uint8)
    assert len(mers) == (k + 1) * len(pairs)
    d_k22, d_c22 = ctx.count_canonical(t.d_bases, t.n_reads, 0, k + 1, offsets=t.d_roff)
    w = ctx.canonical_windows(ctx.to_device(mers), len(pairs), k + 1, k + 1, want=("canon", "flags"))
    assert int(w["flags"].min()) & 1
    counts = u64(ctx.count_lookup(d_k22, d_c22, k + 1, w["canon"]))
    assert np.array_equal(counts, support)


# ---------------------------------------------------------------- the cut
def _cut_raw(ctx, x, links, d_cut, d_out, edges=None):
    from kmers_amd.api import _ptr

    st = ctx.lib.kmx_count_adjacency_cut(ctx._h, _ptr(x.adj[0] if edges is None else edges), _ptr(x.adj[1]), _ptr(x.adj[2]), x.n, _ptr(x.unitigs.nodes),
                                         _ptr(x.unitigs.offsets), x.U, _ptr(x.d_place), _ptr(links.offsets), links.n_links, _ptr(d_cut), _ptr(d_out))
    ctx.synchronize()
    return st


def _check_cut(ctx, t, mask):
    x = t.x
    want = link_support_np.adjacency_cut_np(x.edges, x.flips, x.nbr, x.n, x.nodes, x.uoff, x.place, t.lo, mask)
    edges, flips, nbr = ctx.count_cut_links(x.unitigs, t.links, x.adj, x.n, dev(ctx, mask), place=x.d_place)
    assert flips is x.adj[1] and np.array_equal(edges.cpu().numpy(), want), t.k
    assert np.array_equal(x.adj[0].cpu().numpy(), x.edges)               # the input is not written
    return want


def test_cut_three_masks(ctx):
    """case 6: random, all, none -- every byte"""
    t = _main(ctx, 21)
    rng = np.random.default_rng(7700)
    n_links = t.links.n_links
    some = _check_cut(ctx, t, (rng.random(n_links) < 0.3).astype(np.uint8))
    every = _check_cut(ctx, t, np.full(n_links, 7, np.uint8))           # (any non-zero byte cuts)
    none = _check_cut(ctx, t, np.zeros(n_links, np.uint8))
    assert np.array_equal(none, t.x.edges) and not np.array_equal(some, t.x.edges)
    bits = lambda a: int(np.unpackbits(a).sum())
    assert bits(t.x.edges) - bits(every) == n_links                       # a bit per link slot


def test_cut_one_node_unitigs_sharing_a_dword(ctx):
    """case 6: dense k = 5 -- one-node unitigs cut on both sides (the two nibbles of one byte, cleared by two lanes) and neighbouring
    entries in one dword; an output that does not begin on a dword; guard bytes around it"""
    import torch

    rng = np.random.default_rng(7800)
    s = random_reads(rng, 3000)
    t = Threaded(ctx, 5, [s], [s[:50].copy()])
    x = t.x
    sizes = np.diff(x.uoff.astype(np.int64))
    deg = np.diff(t.lo.astype(np.int64)).reshape(-1, 2)
    assert ((sizes == 1) & (deg[:, 0] > 0) & (deg[:, 1] > 0)).sum() > 50
    n_links = t.links.n_links
    for mask in ((rng.random(n_links) < 0.5).astype(np.uint8), np.ones(n_links, np.uint8)):
        want = _check_cut(ctx, t, mask)
        buf = torch.full((x.n + 2 * GUARD + 1,), 0xA5, dtype=torch.uint8, device=ctx.device)
        out = buf[GUARD + 1:GUARD + 1 + x.n]                              # (an odd address)
        assert _cut_raw(ctx, x, t.links, dev(ctx, mask), out) == 0
        got = buf.cpu().numpy()
        assert np.array_equal(got[GUARD + 1:GUARD + 1 + x.n], want)
        assert (got[:GUARD + 1] == 0xA5).all() and (got[GUARD + 1 + x.n:] == 0xA5).all()
    # an output that is, or overlaps, the input: E_ARG, nothing written
    d_cut = dev(ctx, np.ones(n_links, np.uint8))
    both = torch.cat([x.adj[0], x.adj[0]])
    assert _cut_raw(ctx, x, t.links, d_cut, x.adj[0]) == E_ARG
    assert _cut_raw(ctx, x, t.links, d_cut, both[x.n // 2:x.n // 2 + x.n], edges=both[:x.n]) == E_ARG
    assert np.array_equal(x.adj[0].cpu().numpy(), x.edges)


def test_prune_links(ctx):
    """case 6: count_prune_links on the main case.  The links cut are the reference's; the graph does not grow; and with the reads
    threaded through the new graph nothing is unlinked and every link left is walked (only support-0 links went, and support belongs
    to the pair of nodes).  No crossing is lost: where the cut turns a fork into a plain path the two unitigs become one, the two
    segments of a read that crossed there become one, and that junction is no junction any more -- so the crossed total falls by
    exactly the number of segments that merged, and by nothing else."""
    t = _main(ctx, 21)
    x = t.x
    support, summary = t.want()
    adj, un, links, first, n_cut = ctx.count_prune_links(t.d_bases, t.n_reads, 0, 21, x.d_k, x.d_c, offsets=t.d_roff)
    assert np.array_equal(u64(first.support), support) and np.array_equal(u64(first.summary), summary)
    mask = link_support_np.unsupported_np(support)
    assert n_cut == int(mask.sum()) > 0
    assert np.array_equal(adj[0].cpu().numpy(), link_support_np.adjacency_cut_np(x.edges, x.flips, x.nbr, x.n, x.nodes, x.uoff, x.place, t.lo, mask))
    assert un.n_unitigs <= x.U and links.n_links <= t.links.n_links - n_cut
    paths = ctx.count_read_paths(t.d_bases, t.n_reads, 0, 21, x.d_k, un, offsets=t.d_roff)
    again = ctx.count_link_support(paths, un, links)
    want2, want_summary2 = link_support_np.link_support_np(u64(paths.segments).reshape(-1, 4), u64(un.offsets), u64(links.offsets), u64(links.targets))
    assert np.array_equal(u64(again.support), want2) and np.array_equal(u64(again.summary), want_summary2)
    assert again.unlinked == 0 and (want2 >= 1).all()
    assert int(summary[1]) - again.crossed == t.paths.n_segments - paths.n_segments
    # min_support = 3 cuts more, and what is left is walked three times at least
    adj3, un3, links3, _, n_cut3 = ctx.count_prune_links(t.d_bases, t.n_reads, 0, 21, x.d_k, x.d_c, min_support=3, offsets=t.d_roff)
    assert n_cut3 == int(link_support_np.unsupported_np(support, 3).sum()) > n_cut
    paths3 = ctx.count_read_paths(t.d_bases, t.n_reads, 0, 21, x.d_k, un3, offsets=t.d_roff)
    assert (u64(ctx.count_link_support(paths3, un3, links3).support) >= 3).all()


def test_gfa_with_support(ctx):
    """Unitigs.write_gfa: without support byte for byte what it was; with it, RC:i:<n> on every L line"""
    import io

    rng = np.random.default_rng(7300)
    g = random_reads(rng, 300)
    v = g.copy()
    v[200] = COMP[v[200]]
    t = Threaded(ctx, 21, [g, v], [g, _rc(g), g[150:215].copy()])
    plain, tagged = io.StringIO(), io.StringIO()
    t.x.unitigs.write_gfa(plain, t.links)
    t.x.unitigs.write_gfa(tagged, t.links, t.support())
    a, b = plain.getvalue().splitlines(), tagged.getvalue().splitlines()
    assert len(a) == len(b) and any(ln.startswith("L") for ln in a)
    for x, y in zip(a, b):
        if x.startswith("L"):
            head, _, n = y.rpartition("\tRC:i:")
            assert head == x and n in ("0", "2", "3")                    # the variant's branch: nobody; the genome's: both strands (+ the piece)
        else:
            assert x == y
