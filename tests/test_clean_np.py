"""The host reference of the cleaning rule (tests/clean_np.py), pinned on the CPU against expectations that are built from strings
alone: what is left of a sequence with a substitution, a spur and a deletion hung on it is the table of the sequence, the stronger
of two alleles survives, of a fork's two dead ends the weaker goes.  Rounds are simulated on the host (clean_np.simplify_np: the
references of every layer, then link_np.select_np).  With it the pieces that need no device: the order LOSES on numbers that need
more than 64 bits, the equivalence of the topological setting with Unitigs.tips, and the torch composition of
tools/bench_unitig_clean.py.  No GPU, no oracle, no library.

The string cases (cases(k)) are shared with tests/test_gpu_unitig_clean.py, which runs them through the device's own layers."""
import numpy as np
import pytest
import torch

from tests import clean_np, link_np
from tests.test_unitig_np import COMP, LETTERS, _canon, _kmers_of, _random_seq, _val

KS = (15, 31)
TIPS_ONLY = dict(bubble_max_nodes=0, island_max_nodes=0)


def table(seqs, k):
    """[(sequence, how often)] -> (keys, counts) as count_canonical(2) would give them"""
    occ = {}
    for s, times in seqs:
        for w in _kmers_of(s, k):
            occ[_val(_canon(w))] = occ.get(_val(_canon(w)), 0) + times
    vals = sorted(occ)
    tk = (np.array(vals, np.uint64) if k <= 31 else np.array([[v & (2**64 - 1), v >> 64] for v in vals], np.uint64).reshape(-1, 2))
    return tk, np.array([occ[v] for v in vals], np.uint64)


def _substitute(s, p):
    return s[:p] + LETTERS[(LETTERS.index(s[p]) + 1) % 4] + s[p + 1:]


def cases(k):
    """name -> (input [(sequence, times)], the rule's arguments, the sequences whose k-mers stay (None: see the test), the unitigs
    the first round drops)"""
    rng = np.random.default_rng(7000 + k)
    main = _random_seq(rng, 600)
    var = _substitute(main, 200)
    snp = var[200 - (k - 1):200 + k]                                         # the 2k - 1 bases around the substituted base
    tail = _random_seq(rng, 5)
    if tail[0] == main[400]:
        tail = COMP[tail[0]] + tail[1:]
    spur = main[400 - (k - 1):400] + tail                                    # five new bases hung on the middle
    dele = main[500 - (k - 1):500] + main[501:501 + k - 1]                   # base 500 left out, spelled over 2k - 2 bases
    stem, a, b = _random_seq(rng, 300), _random_seq(rng, 6), _random_seq(rng, 6)
    if a[0] == b[0]:
        b = COMP[b[0]] + b[1:]
    weak = stem[-(k - 1):] + b
    return {
        "backbone": ([(main, 10), (snp, 3), (spur, 2), (dele, 4)], {}, [(main, 10)], dict(tips=1, bubbles=2, islands=0)),
        "swapped": ([(main, 3), (snp, 10)], {}, [(var, 1)], dict(tips=0, bubbles=1, islands=0)),
        "fork": ([(stem + a, 5), (weak, 2)], TIPS_ONLY, [(stem + a, 5)], dict(tips=1, bubbles=0, islands=0)),
        "fork topological": ([(stem + a, 5), (weak, 2)], dict(TIPS_ONLY, tip_ratio=None), [(stem, 5)], dict(tips=2, bubbles=0, islands=0)),
        "fork tie": ([(stem + a, 2), (weak, 2)], TIPS_ONLY, None, dict(tips=1, bubbles=0, islands=0)),
    }


def key_list(tk):
    return [tuple(r) for r in tk.tolist()] if tk.ndim == 2 else tk.tolist()


def expected(seqs, want, first, k):
    """-> (keys, counts, log): the entries of the input's table whose keys the sequences `want` spell, with the counts they have in
    the input (a variant's outermost windows can spell k-mers of the sequence it hangs on); everything else leaves in the first
    round, which drops the unitigs `first` lists, and a second round removes nothing"""
    tk, tc = table(seqs, k)
    stay = set(key_list(table(want, k)[0]))
    mask = np.array([x in stay for x in key_list(tk)])
    assert int(mask.sum()) == len(stay)                                      # the input holds all of them
    return tk[mask], tc[mask], [dict(first, removed=int((~mask).sum())), dict(tips=0, bubbles=0, islands=0, removed=0)]


def tips_formula(offsets, circular, link_offsets, max_nodes):
    """Unitigs.tips in numpy"""
    deg = np.diff(np.asarray(link_offsets).astype(np.int64)).reshape(-1, 2)
    return (np.asarray(circular) == 0) & (np.diff(np.asarray(offsets).astype(np.int64)) <= max_nodes) & ((deg == 0).sum(1) == 1)


def big_style_reads(rng, genome_len, n, L, share):
    """the reads of test_gpu_unitig_links._big: n reads of L bases over a random sequence, every base covered, a share substituted"""
    from tests.count_np import random_reads

    genome = random_reads(rng, genome_len)
    starts = rng.integers(0, len(genome) - L + 1, n)
    starts[:genome_len // L] = np.arange(genome_len // L) * L
    reads = genome[starts[:, None] + np.arange(L)[None, :]].reshape(-1).copy()
    sub = np.nonzero(rng.random(len(reads)) < share)[0]
    reads[sub] = random_reads(rng, len(sub))
    return reads


def host_table(reads, n, L, k):
    """the count table of a clean uniform batch, on the host (two-word keys as rows (low, high))"""
    from tests.count_np import table_of

    code = np.zeros(256, np.uint64)
    code[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4, dtype=np.uint64)
    c = code[reads].reshape(n, L)
    W = L - k + 1
    fw, rc = np.zeros((2, n, W), np.uint64), np.zeros((2, n, W), np.uint64)
    for i in range(k):
        fw[i // 32] |= c[:, i:i + W] << np.uint64(2 * (i % 32))
        j = k - 1 - i
        rc[j // 32] |= (np.uint64(3) - c[:, i:i + W]) << np.uint64(2 * (j % 32))
    less = (rc[1] < fw[1]) | ((rc[1] == fw[1]) & (rc[0] < fw[0]))
    canon = np.where(less[None], rc, fw).reshape(2, -1)
    canon = canon[0] if k <= 31 else np.ascontiguousarray(canon.T)
    return table_of(canon, np.ones(n * W, np.uint8))


# ---------------------------------------------------------------- the string cases
@pytest.mark.parametrize("name", ("backbone", "swapped", "fork", "fork topological"))
@pytest.mark.parametrize("k", KS)
def test_string_cases(k, name):
    seqs, kw, want, first = cases(k)[name]
    tk, tc = table(seqs, k)
    gk, gc, got_log = clean_np.simplify_np(tk, tc, k, **clean_np.rule_of(k, **kw))
    wk, wc, log = expected(seqs, want, first, k)
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    assert got_log == log


@pytest.mark.parametrize("k", KS)
def test_fork_topological_is_the_tips_formula(k):
    seqs, kw, _, _ = cases(k)["fork topological"]
    tk, tc = table(seqs, k)
    _, _, keep, reason, (out, place, lo, tg) = clean_np.clean_table_np(tk, tc, k, 1, clean_np.rule_of(k, **kw))
    tips = tips_formula(out[1], out[2], lo, k)
    assert tips.sum() == 2 and np.array_equal(reason == clean_np.CLEAN_TIP, tips) and np.array_equal(keep == 0, tips)


@pytest.mark.parametrize("k", KS)
def test_fork_with_equal_coverage_loses_the_larger_index(k):
    seqs, kw, _, first = cases(k)["fork tie"]
    tk, tc = table(seqs, k)
    _, _, keep, reason, (out, place, lo, tg) = clean_np.clean_table_np(tk, tc, k, 1, clean_np.rule_of(k, **kw))
    branches = np.nonzero(tips_formula(out[1], out[2], lo, k))[0]
    assert len(branches) == 2
    assert np.nonzero(reason)[0].tolist() == [branches.max()] and reason[branches.max()] == clean_np.CLEAN_TIP
    log = clean_np.simplify_np(tk, tc, k, **clean_np.rule_of(k, **kw))[2]
    assert log == [dict(first, removed=6), dict(tips=0, bubbles=0, islands=0, removed=0)]


def _small_big(k):
    rng = np.random.default_rng(9100 + k)
    reads = big_style_reads(rng, 6000, 300, 100, 0.012)
    return host_table(reads, 300, 100, k)


_CLEANED = {}


def _cleaned_small_big(k):
    if k not in _CLEANED:
        tk, tc = _small_big(k)
        _CLEANED[k] = link_np.links_of_table_np(tk, tc, k)
    return _CLEANED[k]


@pytest.mark.parametrize("k", KS)
def test_of_a_bubble_exactly_one_branch_goes(k):
    inputs = [table(cases(k)[name][0], k) for name in ("backbone", "swapped")]
    graphs = [link_np.links_of_table_np(tk, tc, k) for tk, tc in inputs] + [_cleaned_small_big(k)]
    seen = 0
    for out, place, lo, tg in graphs:
        link_np.assert_mirror_symmetric(lo, tg)
        keep, reason = clean_np.clean_np(out[1], out[2], out[3], lo, tg, **clean_np.rule_of(k))
        for u in np.nonzero(reason == clean_np.CLEAN_BUBBLE)[0].tolist():
            partner = clean_np.bubble_partner(u, lo, tg)
            assert partner != u and reason[partner] == clean_np.CLEAN_KEEP and keep[partner] == 1
            seen += 1
    assert seen >= 5


@pytest.mark.parametrize("k", KS)
def test_topological_setting_is_the_tips_mask(k):
    out, place, lo, tg = _cleaned_small_big(k)
    for max_nodes in (k, 3):
        keep, reason = clean_np.clean_np(out[1], out[2], out[3], lo, tg, max_nodes, 0, 1, 0, 0, 0)
        tips = tips_formula(out[1], out[2], lo, max_nodes)
        assert np.array_equal(reason == clean_np.CLEAN_TIP, tips) and np.array_equal(keep == 0, tips)
    assert tips_formula(out[1], out[2], lo, k).sum() >= 20


# ---------------------------------------------------------------- the bench tool's torch composition
@pytest.mark.parametrize("rule", ("defaults", "ratio", "topological"))
@pytest.mark.parametrize("k", KS)
def test_bench_composition_equals_the_reference(k, rule):
    from kmers_amd.api import UnitigLinks, Unitigs
    from tools.bench_unitig_clean import clean_composition

    r = {"defaults": clean_np.rule_of(k, island_max_nodes=k), "ratio": clean_np.rule_of(k, tip_ratio=(1, 2), bubble_max_diff=0),
         "topological": clean_np.rule_of(k, tip_ratio=None)}[rule]
    t = lambda a: torch.from_numpy(np.asarray(a).view(np.int64) if np.asarray(a).dtype == np.uint64 else np.asarray(a))
    graphs = [link_np.links_of_table_np(*table(cases(k)[name][0], k), k) for name in ("backbone", "fork tie")] + [_cleaned_small_big(k)]
    dropped = 0
    for out, place, lo, tg in graphs:
        keep, reason = clean_np.clean_np(out[1], out[2], out[3], lo, tg, **r)
        un = Unitigs(t(out[0]), t(out[1]), t(out[2]), t(out[3]), len(out[2]), k)
        got, tie = clean_composition(un, UnitigLinks(t(lo), t(tg)), **r)
        decided = ~tie.numpy()
        assert np.array_equal(got.numpy()[decided], reason[decided])
        dropped += int((reason[decided] != 0).sum())
    assert dropped >= 10


def test_mean_counts_without_sums_are_one():
    from kmers_amd.api import Unitigs

    un = Unitigs(None, torch.tensor([0, 3, 4, 9]), None, None, 3, 15)
    assert un.mean_counts.tolist() == [1.0, 1.0, 1.0] and un.mean_counts.dtype == torch.float64
    un = Unitigs(None, torch.tensor([0, 3, 4, 9]), None, torch.tensor([6, -1, 5]), 3, 15)   # (-1: the u64 2^64 - 1)
    assert un.mean_counts.tolist() == [2.0, 2.0**64, 1.0]


# ---------------------------------------------------------------- the order
def test_loses_needs_more_than_64_bits():
    m = 2**40
    s = 2**64 - 1
    # equal means up to one count in 2^64: the products differ in their lowest bits only
    assert clean_np.loses(s - 1, m, 0, s, m, 1, 1, 1) and not clean_np.loses(s, m, 0, s - 1, m, 1, 1, 1)
    assert clean_np.loses(s - 1, m, 0, s, m, 1, 65535, 65535) and not clean_np.loses(s, m, 1, s - 1, m, 0, 65535, 65535)
    # the same mean written with different lengths: a tie, decided by the index
    assert clean_np.loses(3 * 2**62, 3 * 2**38, 7, 2**62, 2**38, 5, 1, 1) and not clean_np.loses(3 * 2**62, 3 * 2**38, 5, 2**62, 2**38, 7, 1, 1)
    # a product that wraps in 64 and in 128 bits must not: 2^63 * 2^40 * 2 against (2^63 + 1) * 2^40 * 2
    assert clean_np.loses(2**63, m, 0, 2**63 + 1, m, 1, 2, 2) and not clean_np.loses(2**63 + 1, m, 0, 2**63, m, 1, 2, 2)
    # the ratio: half the mean loses at 1/1, does not at 1/2 (equal sides, smaller index), does at 1/2 with the larger index
    assert clean_np.loses(s // 2, m, 0, s - 1, m, 1, 1, 1)
    assert not clean_np.loses(2**63, m, 0, 2**64 - 2**40, m - 1, 1, 1, 2)
    assert not clean_np.loses(2**62, m, 0, 2**63, m, 1, 1, 2) and clean_np.loses(2**62, m, 1, 2**63, m, 0, 1, 2)


def test_order_on_the_arrays():
    """a fork written as arrays, its two dead ends with sums near 2^64 over lengths near 2^40: the products need about 104 bits, and
    in the second case they differ by one"""
    m = 2**40
    offsets = np.array([0, 10, 10 + m, 10 + 2 * m - 1], np.uint64)          # a stem of 10 nodes, branches of 2^40 and 2^40 - 1
    link_offsets = np.array([0, 2, 2, 2, 3, 3, 4], np.uint64)               # 0 -> 2, 0 -> 4; mirror(1) -> mirror(0); mirror(2) -> mirror(0)
    targets = np.array([2, 4, 1, 1], np.uint64)
    for sums, loser in (((100, 2**64 - 2, 2**64 - 1), 1), ((100, 2**64 - 1, 2**64 - 2**24 - 1), 2), ((100, 2 * m, 2 * (m - 1)), 2)):
        keep, reason = clean_np.clean_np(offsets, np.zeros(3, np.uint8), np.array(sums, np.uint64), link_offsets, targets, m, 1, 1, 0, 0, 0)
        assert reason.tolist() == [clean_np.CLEAN_TIP if u == loser else 0 for u in range(3)], (sums, reason)
    keep, reason = clean_np.clean_np(offsets, None, None, link_offsets, targets, m, 1, 1, 0, 0, 0)   # no sums: every mean is 1
    assert reason.tolist() == [0, 0, clean_np.CLEAN_TIP] and keep.tolist() == [1, 1, 0]
