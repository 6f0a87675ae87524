"""Cleaning the compacted graph on the GPU: kmx_count_unitig_clean (kmx_count_clean.hip) and what the Python layer builds on it
(Context.count_unitig_clean, Context.count_simplify(2), Unitigs.mean_counts).

Every comparison is equality of the keep and reason bytes with the sequential host reference tests/clean_np.py (pinned against
expectations built from strings in tests/test_clean_np.py).  The reference is fed the host copies of what the device made -- unitigs
and links, each compared with its own reference in the tests of its own layer.  The string cases are tests/test_clean_np.py's, the
dense and hairpin tables tests/test_gpu_count_unitigs.py's, rebuilt here through tests/test_gpu_unitig_links.Linked.  Every family
asserts of its own input that it holds what it is there for."""
import numpy as np
import pytest

from tests import clean_np
from tests.count_np import ctx  # noqa: F401  (the fixture, found by name in this module)
from tests.count_np import random_reads, u64
from tests.test_clean_np import cases, expected, table, tips_formula
from tests.test_gpu_count_graph import _dense_reads
from tests.test_gpu_count_unitigs import _dense8_reads, _hairpin_reads, _table
from tests.test_gpu_read_paths import _ragged
from tests.test_gpu_unitig_links import Linked

pytestmark = pytest.mark.gpu

POISON = 0xA5
E_ARG = 1
STRING_KS = (15, 31, 33, 47)
OFF = dict(tip_max_nodes=0, tip_num=0, tip_den=1, bubble_max_nodes=0, bubble_max_diff=0, island_max_nodes=0)


def rule_sets(k):
    """name -> (Context.count_unitig_clean's keyword arguments, the six integers of the C call)"""
    kws = {"defaults": {}, "topological": dict(tip_ratio=None), "half, islands": dict(tip_ratio=(1, 2), island_max_nodes=k)}
    return {name: (kw, clean_np.rule_of(k, **kw)) for name, kw in kws.items()}


class Cleaned:
    """a Linked table with its links on the device and the host copies the reference reads"""

    def __init__(self, x):
        self.x, self.ctx, self.k, self.U = x, x.ctx, x.k, x.U
        self.links = x.links()
        self.circ, self.sums = x.unitigs.circular.cpu().numpy(), u64(x.unitigs.count_sums)
        self.lo, self.tg = u64(self.links.offsets), u64(self.links.targets)
        self._want = {}

    def want(self, rule):
        key = tuple(sorted(rule.items()))
        if key not in self._want:
            self._want[key] = clean_np.clean_np(self.x.uoff, self.circ, self.sums, self.lo, self.tg, **rule)
        return self._want[key]

    def check(self, kw, rule):
        keep, reason = self.ctx.count_unitig_clean(self.x.unitigs, self.links, **kw)
        want_keep, want_reason = self.want(rule)
        assert keep.dtype == reason.dtype and keep.numel() == reason.numel() == self.U
        assert np.array_equal(reason.cpu().numpy(), want_reason), (self.k, kw, "reason")
        assert np.array_equal(keep.cpu().numpy(), want_keep), (self.k, kw, "keep")
        return want_reason


_CLEANED = {}


def _cleaned(ctx, key, make):
    if key not in _CLEANED or _CLEANED[key].ctx is not ctx:
        _CLEANED[key] = Cleaned(make())
    return _CLEANED[key]


def _count(ctx, k, seqs):
    """[(sequence, times)] counted on the device"""
    bases, offsets = _ragged([np.frombuffer(s.encode(), np.uint8) for s, times in seqs for _ in range(times)])
    return (ctx.count_canonical if k <= 31 else ctx.count_canonical2)(ctx.to_device(bases), len(offsets) - 1, 0, k, offsets=ctx.to_device(offsets))


# ---------------------------------------------------------------- the string cases, every layer on the device
@pytest.mark.parametrize("name", ("backbone", "swapped", "fork", "fork topological", "fork tie"))
@pytest.mark.parametrize("k", STRING_KS)
def test_string_cases(ctx, k, name):
    seqs, kw, want, first = cases(k)[name]
    d_k, d_c = _count(ctx, k, seqs)
    tk, tc = table(seqs, k)
    assert np.array_equal(u64(d_k).reshape(tk.shape), tk) and np.array_equal(u64(d_c), tc)
    c = Cleaned(Linked(ctx, k, d_k, d_c))
    reason = c.check(kw, clean_np.rule_of(k, **kw))
    assert {name_: int((reason == code).sum()) for name_, code in (("tips", 1), ("bubbles", 2), ("islands", 3))} == first
    gk, gc, log = (ctx.count_simplify if k <= 31 else ctx.count_simplify2)(d_k, d_c, k, **kw)
    if want is None:                                                         # the tie: what the host's rounds leave
        wk, wc, want_log = clean_np.simplify_np(tk, tc, k, **clean_np.rule_of(k, **kw))
        branches = np.nonzero(tips_formula(c.x.uoff, c.circ, c.lo, k))[0]
        assert len(branches) == 2 and np.nonzero(reason)[0].tolist() == [branches.max()]   # of two equal dead ends the larger index goes
    else:
        wk, wc, want_log = expected(seqs, want, first, k)
    assert np.array_equal(u64(gk).reshape(wk.shape), wk) and np.array_equal(u64(gc), wc)
    assert log == want_log


@pytest.mark.parametrize("k", (15, 47))
def test_simplify_rounds_and_min_count(ctx, k):
    """rounds=1 stops after the first round; entries below min_count leave in the first round, with or without a unitig to drop"""
    seqs, kw, want, first = cases(k)["backbone"]
    once = "".join("ACGT"[i] for i in np.random.default_rng(9950 + k).integers(0, 4, k + 30))
    d_k, d_c = _count(ctx, k, seqs + [(once, 1)])                            # a sequence seen once: below min_count = 2
    simplify = ctx.count_simplify if k <= 31 else ctx.count_simplify2
    tk, tc = u64(d_k), u64(d_c)
    wk, wc, want_log = clean_np.simplify_np(tk, tc, k, min_count=2, **clean_np.rule_of(k))
    gk, gc, log = simplify(d_k, d_c, k, min_count=2)
    assert np.array_equal(u64(gk), wk) and np.array_equal(u64(gc), wc) and log == want_log
    assert int((tc < 2).sum()) > 0 and (wc >= 2).all() and len(log) == 2
    gk1, gc1, log1 = simplify(d_k, d_c, k, min_count=2, rounds=1)
    assert log1 == want_log[:1] and np.array_equal(u64(gk1), wk)
    assert simplify(gk, gc, k, rounds=0)[2] == []


# ---------------------------------------------------------------- dense graphs, palindromes, hairpins, self-links
WIDE = dict(tip_max_nodes=1000, bubble_max_nodes=1000, bubble_max_diff=1000, island_max_nodes=1000)


@pytest.mark.parametrize("k", (4, 5, 6, 8))
def test_dense_graph(ctx, k):
    """degrees up to four, self-links, hairpins and (even k) palindromic one-node unitigs: against the reference only"""
    t = _table(ctx, _dense_reads if k < 8 else _dense8_reads, k)
    deg_max, dropped = 0, 0
    for min_count in (1, 2):
        c = _cleaned(ctx, ("dense", k, min_count), lambda: Linked(ctx, k, t.d_k, t.d_c, min_count))
        deg_max = max(deg_max, int(np.diff(c.lo.astype(np.int64)).max()))
        for kw in ({}, dict(WIDE), dict(WIDE, tip_ratio=(1, 2)), dict(WIDE, tip_ratio=None), dict(tip_max_nodes=2, bubble_max_nodes=0)):
            dropped += int((c.check(kw, clean_np.rule_of(k, **kw)) != 0).sum())
    assert deg_max == 4 and (dropped > 0 or k <= 5)                          # (at k <= 5 nearly every k-mer occurs: no dead end, no bubble)


@pytest.mark.parametrize("k", (6, 8))
def test_hairpins(ctx, k):
    t = _table(ctx, _hairpin_reads, k)
    c = _cleaned(ctx, ("hairpin", k), lambda: Linked(ctx, k, t.d_k, t.d_c))
    assert c.U == 2
    for kw in ({}, dict(WIDE), dict(WIDE, tip_ratio=None)):
        c.check(kw, clean_np.rule_of(k, **kw))


# ---------------------------------------------------------------- past one block
_BIG_TABLES = {}
# the reference's drops on this input, measured on the CPU: k = 31 (85 554 entries, 3 802 unitigs) 891 tips and 116 bubbles with the
# defaults, 1 073 tips topologically, 603 at ratio 1/2; k = 47 (85 998 entries, 3 073 unitigs) 1 077 tips and 9 bubbles, 1 587, 471.
# The floors: 500 tips and 50 bubbles for every set at k = 31, about half of the measured counts at k = 47.
FLOORS = {31: {"defaults": (500, 50), "topological": (500, 50), "half, islands": (500, 50)},
          47: {"defaults": (500, 4), "topological": (750, 4), "half, islands": (230, 4)}}


def _big(ctx, k):
    """2400 reads of 100 bases over a sequence of 48 000, 1.2 % of the bases substituted (tests/test_gpu_unitig_links.py's input)"""
    def make():
        rng = np.random.default_rng(9100 + k)
        genome = random_reads(rng, 48_000)
        n, L = 2400, 100
        starts = rng.integers(0, len(genome) - L + 1, n)
        starts[:480] = np.arange(480) * 100            # every base is covered
        reads = genome[starts[:, None] + np.arange(L)[None, :]].reshape(-1).copy()
        sub = np.nonzero(rng.random(len(reads)) < 0.012)[0]
        reads[sub] = random_reads(rng, len(sub))
        return (ctx.count_canonical if k <= 31 else ctx.count_canonical2)(ctx.to_device(reads), n, L, k)

    if k not in _BIG_TABLES or _BIG_TABLES[k][0] is not ctx:
        _BIG_TABLES[k] = (ctx,) + tuple(make())
    _, d_k, d_c = _BIG_TABLES[k]
    return _cleaned(ctx, ("big", k), lambda: Linked(ctx, k, d_k, d_c))


@pytest.mark.parametrize("rules", ("defaults", "topological", "half, islands"))
@pytest.mark.parametrize("k", (31, 47))
def test_more_unitigs_than_one_block(ctx, k, rules):
    c = _big(ctx, k)
    assert c.x.n > 70_000 and c.U > 3000                                     # a dozen blocks of 256 lanes
    kw, rule = rule_sets(k)[rules]
    reason = c.check(kw, rule)
    tips, bubbles = int((reason == clean_np.CLEAN_TIP).sum()), int((reason == clean_np.CLEAN_BUBBLE).sum())
    assert tips >= FLOORS[k][rules][0] and bubbles >= FLOORS[k][rules][1], (k, rules, tips, bubbles)
    assert (reason[:256] != 0).any() and (reason[256:] != 0).any()           # drops on both sides of the first block's boundary


@pytest.mark.parametrize("k", (31, 47))
def test_topological_setting_is_the_tips_mask(ctx, k):
    import torch

    c = _big(ctx, k)
    for max_nodes in (k, 5):
        keep, reason = c.ctx.count_unitig_clean(c.x.unitigs, c.links, tip_max_nodes=max_nodes, tip_ratio=None, bubble_max_nodes=0)
        tips = c.x.unitigs.tips(c.links, max_nodes)
        assert int(tips.sum()) > 100
        assert torch.equal(keep.to(torch.bool), ~tips) and torch.equal(reason == clean_np.CLEAN_TIP, tips)


def test_mean_counts(ctx):
    c = _big(ctx, 31)
    want = c.sums.astype(np.float64) / np.diff(c.x.uoff.astype(np.int64))
    assert np.array_equal(c.x.unitigs.mean_counts.cpu().numpy(), want) and want.max() > 2.0


def test_more_unitigs_than_one_sweep_of_the_grid(ctx):
    """The launcher caps its grid at 4096 blocks of 256 lanes, so a lane takes unitig u, u + 2^20, ...: the graph of the backbone case
    (a tip, two bubbles) laid out 2^20 / U + 1 times over, every copy's indices shifted by its place.  LOSES breaks ties by index, and
    a shift moves both sides alike, so every copy has the answer of the first."""
    import torch

    k = 31
    d_k, d_c = _count(ctx, k, cases(k)["backbone"][0])
    c = Cleaned(Linked(ctx, k, d_k, d_c))
    rule = clean_np.rule_of(k, island_max_nodes=1000)
    _, reason1 = c.want(rule)
    assert sorted(set(reason1.tolist())) == [0, 1, 2]
    U, L = c.U, len(c.tg)
    copies = (1 << 20) // U + 2
    n = copies * U
    assert n > 4096 * 256
    lengths = np.tile(np.diff(c.x.uoff.astype(np.int64)), copies)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    lo = (np.tile(c.lo[:-1].astype(np.int64), copies) + np.repeat(np.arange(copies) * L, 2 * U))
    lo = np.concatenate([lo, [copies * L]])
    tg = np.tile(c.tg.astype(np.int64), copies) + np.repeat(np.arange(copies) * 2 * U, L)
    from kmers_amd.api import UnitigLinks, Unitigs

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)
    un = Unitigs(None, dev(offsets), dev(np.tile(c.circ, copies)), dev(np.tile(c.sums.view(np.int64), copies)), n, k)
    keep, reason = ctx.count_unitig_clean(un, UnitigLinks(dev(lo), dev(tg)), island_max_nodes=1000)
    want = torch.from_numpy(np.tile(reason1, copies)).to(ctx.device)
    assert torch.equal(reason, want) and torch.equal(keep, (want == 0).to(torch.uint8))


# ---------------------------------------------------------------- inconsistent inputs
def _raw(ctx, a, rule, n_unitigs, n_links, keep, reason, handle="ctx"):
    """the C call as it is -> status; `a` maps the five input arrays' names to tensors or None"""
    from kmers_amd.api import _ptr

    return ctx.lib.kmx_count_unitig_clean(ctx._h if handle == "ctx" else handle, _ptr(a["offsets"]), _ptr(a["circular"]), _ptr(a["sums"]), n_unitigs,
                                          _ptr(a["link_offsets"]), _ptr(a["links"]), n_links, rule["tip_max_nodes"], rule["tip_num"], rule["tip_den"],
                                          rule["bubble_max_nodes"], rule["bubble_max_diff"], rule["island_max_nodes"], _ptr(keep), _ptr(reason))


@pytest.mark.parametrize("U", (300, 20_001))
def test_inconsistent_inputs(ctx, U):
    """random bytes in every array, exactly sized: include/kmx.h defines the result, every index is checked before it is used, and
    nothing behind byte U of either output is written"""
    import torch

    rng = np.random.default_rng(9700 + U)
    n_links = 3 * U
    # link offsets: mostly ascending in steps of 0 .. 4 with the right total, some words random (beyond the array, descending, wide)
    lo = np.concatenate([[0], np.cumsum(rng.integers(0, 4, 2 * U))]).astype(np.uint64)
    lo = np.minimum(lo, np.uint64(n_links))
    wild = rng.random(2 * U + 1) < 0.05
    lo[wild] = rng.integers(0, 2**64, int(wild.sum()), dtype=np.uint64)
    near = wild & (rng.random(2 * U + 1) < 0.5)
    lo[near] = rng.integers(0, n_links + 9, int(near.sum())).astype(np.uint64)
    tg = rng.integers(0, 2 * U, n_links).astype(np.uint64)
    wild = rng.random(n_links) < 0.03
    tg[wild] = rng.integers(0, 2**64, int(wild.sum()), dtype=np.uint64)
    tg[wild & (rng.random(n_links) < 0.5)] = np.uint64(2 * U)                # the first word that names no oriented unitig
    offsets = np.concatenate([[0], np.cumsum(rng.integers(1, 40, U))]).astype(np.uint64)
    wild = rng.random(U + 1) < 0.03
    offsets[wild] = rng.integers(0, 2**64, int(wild.sum()), dtype=np.uint64)
    circ = (rng.integers(0, 256, U) * (rng.random(U) < 0.1)).astype(np.uint8)
    sums = rng.integers(0, 2**64, U, dtype=np.uint64)
    small = rng.random(U) < 0.7
    sums[small] = rng.integers(0, 50, int(small.sum())).astype(np.uint64)    # (many equal means: the ties by index)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else a).to(ctx.device)
    a = {"offsets": dev(offsets), "circular": dev(circ), "sums": dev(sums), "link_offsets": dev(lo), "links": dev(tg)}
    seen = set()
    for rule in (dict(tip_max_nodes=30, tip_num=1, tip_den=1, bubble_max_nodes=30, bubble_max_diff=8, island_max_nodes=20),
                 dict(tip_max_nodes=2**64 - 1, tip_num=65535, tip_den=65535, bubble_max_nodes=2**64 - 1, bubble_max_diff=2**64 - 1,
                      island_max_nodes=2**64 - 1),
                 dict(tip_max_nodes=25, tip_num=1, tip_den=3, bubble_max_nodes=0, bubble_max_diff=0, island_max_nodes=0)):
        want_keep, want_reason = clean_np.clean_np(offsets, circ, sums, lo, tg, **rule)
        buf = torch.full((2, U + 64), POISON, dtype=torch.uint8, device=ctx.device)
        assert _raw(ctx, a, rule, U, n_links, buf[0], buf[1]) == 0
        got = buf.cpu().numpy()
        assert np.array_equal(got[1, :U], want_reason) and np.array_equal(got[0, :U], want_keep)
        assert (got[:, U:] == POISON).all()
        seen |= set(want_reason.tolist())
    assert {0, 1, 3} <= seen                                                 # (random words close no bubble: the next test plants them)


def test_bubbles_of_random_links(ctx):
    """random bytes rarely close a bubble: here simple bubbles are planted into otherwise random links, then single words of some are
    broken, so that every condition of the bubble rule decides somewhere"""
    import torch

    rng = np.random.default_rng(9800)
    B = 600                                                                  # bubbles: unitigs 4 b .. 4 b + 3 = s, u, y, x
    U = 4 * B
    lists = [[] for _ in range(2 * U)]
    for b in range(B):
        s, u, y, x = (2 * (4 * b + j) + int(rng.integers(0, 2)) for j in range(4))
        lists[s] = [u, y] if rng.random() < 0.5 else [y, u]
        lists[u], lists[y] = [x], [x]
        lists[x ^ 1] = [u ^ 1, y ^ 1] if rng.random() < 0.5 else [y ^ 1, u ^ 1]
        lists[u ^ 1], lists[y ^ 1] = [s ^ 1], [s ^ 1]
    lo = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    tg = np.array([t for l in lists for t in l], np.uint64)
    broken = rng.random(len(tg)) < 0.04
    tg[broken] = rng.integers(0, 2 * U, int(broken.sum())).astype(np.uint64)
    lengths = rng.integers(1, 12, U)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    circ = (rng.random(U) < 0.03).astype(np.uint8)
    sums = (lengths * rng.integers(1, 4, U)).astype(np.uint64)               # means 1, 2, 3: ties by index
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else a).to(ctx.device)
    a = {"offsets": dev(offsets), "circular": dev(circ), "sums": dev(sums), "link_offsets": dev(lo), "links": dev(tg)}
    for rule, floor in ((dict(OFF, bubble_max_nodes=11, bubble_max_diff=11), B // 4), (dict(OFF, bubble_max_nodes=8, bubble_max_diff=2), B // 20)):
        want_keep, want_reason = clean_np.clean_np(offsets, circ, sums, lo, tg, **rule)
        buf = torch.full((2, U), POISON, dtype=torch.uint8, device=ctx.device)
        assert _raw(ctx, a, rule, U, len(tg), buf[0], buf[1]) == 0
        assert np.array_equal(buf[1].cpu().numpy(), want_reason) and np.array_equal(buf[0].cpu().numpy(), want_keep)
        popped = int((want_reason == clean_np.CLEAN_BUBBLE).sum())
        assert floor < popped < B - floor                                    # many close; the broken, the circular, the long ones do not


# ---------------------------------------------------------------- the order, past 64 and past 128 bits
def order_cases():
    """a fork written as arrays (tests/test_clean_np.py's): a stem of 10 nodes and two dead ends of M and M - 1 nodes with sums near
    2^64, so that S m c needs 104 to 142 bits -> [(offsets, sums, (num, den), the highest 64-bit limb in which the two sides of
    '1 LOSES to 2' differ, None if they are equal)]"""
    out = []
    for M in (2**40, 2**62):
        offsets = np.array([0, 10, 10 + M, 10 + 2 * M - 1], np.uint64)
        pairs = [(2**64 - 2, 2**64 - 1), (2**64 - 1, 2**64 - 2**24 - 1), (2 * M, 2 * (M - 1)), (2**64 - 1, 2**63 + 12345), (3 * 2**61, 3 * 2**61 + 1),
                 (2**64 - 2**20, 2**64 - 2**20)]
        for s1, s2 in pairs:
            for num, den in ((1, 1), (65535, 65535), (3, 7), (65534, 65535)):
                l, r = s1 * (M - 1) * den, s2 * M * num
                limb = None if l == r else max(i for i in range(3) if (l >> 64 * i) & (2**64 - 1) != (r >> 64 * i) & (2**64 - 1))
                out.append((offsets, np.array([100, s1, s2], np.uint64), (num, den), limb))
    return out


def test_order_past_128_bits(ctx):
    """the kernel's three-limb products against Python's integers: ties, differences in the lowest limb only, in the middle, at the top"""
    import torch

    link_offsets = np.array([0, 2, 2, 2, 3, 3, 4], np.uint64)               # 0 -> 2, 0 -> 4; mirror(1) -> mirror(0); mirror(2) -> mirror(0)
    targets = np.array([2, 4, 1, 1], np.uint64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else a).to(ctx.device)
    limbs, losers = set(), set()
    for offsets, sums, (num, den), limb in order_cases():
        rule = dict(OFF, tip_max_nodes=2**64 - 1, tip_num=num, tip_den=den)
        want_keep, want_reason = clean_np.clean_np(offsets, None, sums, link_offsets, targets, **rule)
        a = {"offsets": dev(offsets), "circular": None, "sums": dev(sums), "link_offsets": dev(link_offsets), "links": dev(targets)}
        buf = torch.full((2, 3), POISON, dtype=torch.uint8, device=ctx.device)
        assert _raw(ctx, a, rule, 3, 4, buf[0], buf[1]) == 0
        assert buf[1].cpu().tolist() == want_reason.tolist() and buf[0].cpu().tolist() == want_keep.tolist(), (offsets, sums, num, den)
        assert want_reason[0] == 0                                           # the stem is a dead end without a sibling: it stays
        limbs.add(limb)
        losers.add(tuple(want_reason[1:].tolist()))
    assert limbs == {None, 0, 1, 2}
    assert losers == {(1, 0), (0, 1), (0, 0)}                                # either branch; and at a ratio below 1 neither


# ---------------------------------------------------------------- the call's conventions
def test_conventions(ctx):
    import torch

    c = _big(ctx, 31)
    kw, rule = rule_sets(31)["half, islands"]
    want_keep, want_reason = c.want(rule)
    a = {"offsets": c.x.unitigs.offsets, "circular": c.x.unitigs.circular, "sums": c.x.unitigs.count_sums, "link_offsets": c.links.offsets,
         "links": c.links.targets}
    L = c.links.n_links
    fresh = lambda: torch.full((c.U + 32,), POISON, dtype=torch.uint8, device=ctx.device)
    keep, reason = fresh(), fresh()
    assert _raw(ctx, a, rule, c.U, L, keep, reason) == 0
    assert np.array_equal(keep[:c.U].cpu().numpy(), want_keep) and np.array_equal(reason[:c.U].cpu().numpy(), want_reason)
    assert (keep[c.U:] == POISON).all() and (reason[c.U:] == POISON).all()   # nothing behind byte U
    keep2, reason2 = fresh(), fresh()
    assert _raw(ctx, a, rule, c.U, L, keep2, reason2) == 0 and torch.equal(keep, keep2) and torch.equal(reason, reason2)   # identical bytes
    keep3 = fresh()
    assert _raw(ctx, a, rule, c.U, L, keep3, None) == 0 and torch.equal(keep3, keep)   # no reason asked for
    # no circular flags: none is circular; no sums: every mean is 1
    for missing in ("circular", "sums"):
        b = dict(a, **{missing: None})
        wk, wr = clean_np.clean_np(c.x.uoff, None if missing == "circular" else c.circ, None if missing == "sums" else c.sums, c.lo, c.tg, **rule)
        keep, reason = fresh(), fresh()
        assert _raw(ctx, b, rule, c.U, L, keep, reason) == 0
        assert np.array_equal(reason[:c.U].cpu().numpy(), wr) and np.array_equal(keep[:c.U].cpu().numpy(), wk)
    assert not np.array_equal(clean_np.clean_np(c.x.uoff, c.circ, None, c.lo, c.tg, **rule)[1], want_reason)   # (the sums do decide here)
    # no unitigs: a no-op
    keep, reason = fresh(), fresh()
    none = dict.fromkeys(a)
    assert _raw(ctx, none, rule, 0, 0, keep, reason) == 0 and _raw(ctx, none, rule, 0, 0, None, None) == 0 and _raw(ctx, a, rule, 0, L, keep, reason) == 0
    ctx.synchronize()
    assert (keep == POISON).all() and (reason == POISON).all()


def test_argument_errors(ctx):
    import torch

    c = _big(ctx, 31)
    rule = clean_np.rule_of(31)
    a = {"offsets": c.x.unitigs.offsets, "circular": c.x.unitigs.circular, "sums": c.x.unitigs.count_sums, "link_offsets": c.links.offsets,
         "links": c.links.targets}
    L = c.links.n_links
    keep = torch.full((c.U,), POISON, dtype=torch.uint8, device=ctx.device)
    reason = keep.clone()
    assert _raw(ctx, a, rule, c.U, L, keep, reason, handle=None) == E_ARG    # NULL ctx
    assert _raw(ctx, a, rule, c.U, L, None, reason) == E_ARG                 # NULL d_keep
    for name in ("offsets", "link_offsets", "links"):
        assert _raw(ctx, dict(a, **{name: None}), rule, c.U, L, keep, reason) == E_ARG, name
    assert _raw(ctx, a, rule, 2**40 + 1, L, keep, reason) == E_ARG and _raw(ctx, a, rule, c.U, 2**43 + 1, keep, reason) == E_ARG
    for bad in (dict(tip_num=2, tip_den=1), dict(tip_num=0, tip_den=0), dict(tip_num=1, tip_den=65536), dict(tip_num=65536, tip_den=65536),
                dict(tip_num=70000, tip_den=70001)):
        assert _raw(ctx, a, dict(rule, **bad), c.U, L, keep, reason) == E_ARG, bad
    with pytest.raises(Exception) as e:
        ctx.count_unitig_clean(c.x.unitigs, c.links, tip_ratio=(3, 2))
    assert getattr(e.value, "status", None) == E_ARG
    ctx.synchronize()
    assert (keep == POISON).all() and (reason == POISON).all()               # nothing ran
    assert _raw(ctx, a, dict(rule, tip_max_nodes=0, tip_num=0, tip_den=0), c.U, L, keep, reason) == 0   # no tip rule: its ratio is not looked at
    assert _raw(ctx, dict(a, links=None), rule, c.U, 0, keep, reason) == 0   # no links at all: d_links may be NULL
    assert np.array_equal(reason.cpu().numpy(), clean_np.clean_np(c.x.uoff, c.circ, c.sums, c.lo, c.tg[:0], **rule)[1])


@pytest.mark.parametrize("k", (15, 33))
def test_empty_table(ctx, k):
    import torch

    kmers = torch.zeros((0,) if k <= 31 else (0, 2), dtype=torch.int64, device=ctx.device)
    counts = torch.zeros(0, dtype=torch.int64, device=ctx.device)
    x = Linked(ctx, k, kmers, counts)
    keep, reason = ctx.count_unitig_clean(x.unitigs, x.links())
    assert keep.numel() == 0 and reason.numel() == 0 and x.unitigs.mean_counts.numel() == 0
    gk, gc, log = (ctx.count_simplify if k <= 31 else ctx.count_simplify2)(kmers, counts, k)
    assert gk.numel() == 0 and gc.numel() == 0 and log == []


@pytest.mark.parametrize("k", (2, 15, 31, 33, 64))
def test_one_entry(ctx, k):
    """the all-A k-mer links to itself on both sides: kept whatever the limits; and a table of one unitig with no link is an island"""
    d_k, d_c = (ctx.count_canonical if k <= 31 else ctx.count_canonical2)(ctx.to_device(np.full(k + 3, ord("A"), np.uint8)), 1, k + 3, k)
    c = Cleaned(Linked(ctx, k, d_k, d_c))
    assert c.x.n == 1 and c.U == 1
    assert c.check(dict(WIDE), clean_np.rule_of(k, **WIDE)).tolist() == [0]
    if k >= 15:
        seq = "".join("ACGT"[i] for i in np.random.default_rng(9900 + k).integers(0, 4, k + 9))
        d_k, d_c = _count(ctx, k, [(seq, 1)])
        c = Cleaned(Linked(ctx, k, d_k, d_c))
        assert c.U == 1 and c.x.n == 10
        assert c.check({}, clean_np.rule_of(k)).tolist() == [0]
        assert c.check(dict(island_max_nodes=10), clean_np.rule_of(k, island_max_nodes=10)).tolist() == [3]
        assert c.check(dict(island_max_nodes=9), clean_np.rule_of(k, island_max_nodes=9)).tolist() == [0]
        sk, sc, log = (ctx.count_simplify if k <= 31 else ctx.count_simplify2)(d_k, d_c, k, island_max_nodes=10)
        assert sk.numel() == 0 and log == [dict(tips=0, bubbles=0, islands=1, removed=10)]
