"""What the read-preparation fuzz (tests/test_gpu_reads_fuzz.py) will do, checked without a GPU: the coverage of the default seed set,
read off reads_fuzz_np.plan alone; the non-vacuity of its inputs, read off the reference chain reads_fuzz_np.host_pipeline alone; and
the relations the GPU test states on the device -- mates swapped, pairs permuted, error-free fragments -- on the references."""
import collections

import numpy as np
import pytest

from tests import adapter_np as A
from tests import merge_np as M
from tests import quality_np as Q
from tests import reads_fuzz_np as F
from tests import reads_np

SEEDS = range(F.N_DEFAULT)


@pytest.fixture(scope="module")
def plans():
    return [F.plan(s) for s in SEEDS]


@pytest.fixture(scope="module")
def chains(plans):
    """the reference chain of every default seed, computed once for the tests that read it (none of them writes into it)"""
    return [F.host_pipeline(p) for p in plans]


def test_plan_and_texts_are_pure_functions_of_the_seed():
    assert all(F.plan(s) == F.plan(s) for s in (0, 7, 30))
    for s in (5, 6):
        a, b = F._case_of(F.plan(s)), F._case_of(F.plan(s))
        assert a.texts == b.texts and all(np.array_equal(x, y) for m in range(2) for x, y in zip(a.reads[m] + a.quals[m], b.reads[m] + b.quals[m]))


def test_coverage_of_the_default_seeds(plans):
    layouts = collections.Counter(n for p in plans for n in p.layout_names())
    assert all(layouts[n] >= 4 for n in F.LAYOUTS), layouts
    first = collections.Counter(p.layouts[0].name for p in plans)
    assert all(first[n] >= 1 for n in F.LAYOUTS), first
    assert all(p.stream == ("side" if p.seed % 2 else "default") for p in plans)
    assert {(p.stream, p.length_mode) for p in plans} == {(s, m) for s in ("side", "default") for m in ("one", "mix")}
    assert {p.stream for p in plans if p.has_long} == {"side", "default"}
    assert len(plans) // 5 <= sum(p.has_long for p in plans) <= len(plans) // 3
    sizes = collections.Counter(len(p.adapters) for p in plans)
    assert sizes[1] >= 1 and sizes[8] >= 1 and all(1 <= n <= 8 for n in sizes), sizes
    lens = {len(a) for p in plans for a in p.adapters}
    assert {1, 64} <= lens and max(lens) == 64, lens
    assert all(any(b"N" in a.upper() for a in p.adapters) for p in plans)
    assert {p.phred_base for p in plans} == {33, 64} and {p.trim for p in plans} == {"mott", "run", None}
    assert {(c, t) for p in plans for c, t in zip(p.crlf, p.trail)} == {(c, t) for c in (False, True) for t in (False, True)}
    assert all(1 <= p.ad_min_overlap <= 12 for p in plans) and {p.ad_max_error for p in plans} == set(F.MAX_ERRORS)
    assert {p.layouts[i].uniform for p in plans for i in range(len(p.layouts)) if p.layouts[i].name == "misaligned"} == {False, True}
    for p in plans:
        assert ("uniform" in p.layout_names()) == (p.length_mode == "one") and [l.name for l in p.layouts] == [l.name for l in p.layouts2]
        for l in p.layouts:
            if l.name == "misaligned":
                assert 1 <= l.lead <= 15 and (p.qlead(l) - l.lead) % 4 != 0 and (l.uniform or 1 <= p.first(l) <= F.GUARD_BYTES)
            else:
                assert l.lead == 0 and p.first(l) == 0


def _four_lines(text):
    lines = text.replace(b"\r\n", b"\n").split(b"\n")
    if text.endswith(b"\n"):
        lines.pop()
    assert len(lines) % 4 == 0 and all(h[:1] == b"@" for h in lines[0::4]) and all(x[:1] == b"+" for x in lines[2::4])
    return lines[1::4]


def test_the_texts_are_what_the_plan_says(plans):
    for p in plans:
        c = F.case_of(p)
        assert len(c.frags) == p.n_pairs and 40 <= p.n_pairs <= 302
        for m in range(2):
            text, reads, quals = c.texts[m], c.reads[m], c.quals[m]
            assert len(reads) == len(quals) == p.n_pairs and sum(len(r) for r in reads) <= F.MAX_BASES * 1.1
            assert (b"\r" in text) == p.crlf[m] and text.endswith(b"\n") == p.trail[m] and text.count(b"\r\n") == (text.count(b"\n") if p.crlf[m] else 0)
            assert [bytes(x) for x in _four_lines(text)] == [r.tobytes() for r in reads]
            qb, qo = Q.fastq_quals(text)
            assert np.array_equal(qb, F.ragged(quals)[0]) and np.array_equal(qo, F.ragged(quals)[1])
            lens = np.array([len(r) for r in reads])
            if p.length_mode == "one":
                assert (lens == (p.len1, p.len2)[m]).all() and lens[0] in F.ONE_LENGTHS
            else:
                assert (lens == 0).any() and ((lens >= 1) & (lens <= 3)).any() and lens[(lens <= 260)].max() == p.mix_max
                assert sorted(lens[lens > 260].tolist()) == sorted(x[m] for x in p.long_pairs) and all(1000 <= x <= 1030 for x in lens[lens > 260])
            assert int(lens.max()) == p.longest[m]
            both, q = np.concatenate(reads), np.concatenate(quals)
            assert (both == ord("N")).any() and ((both >= ord("a")) & (both <= ord("t"))).any() and (~F._VALID[both]).any(), p.seed
            assert (q < p.phred_base).any() and np.isin(q, np.frombuffer(b"@>+", np.uint8)).any() and b"\n" not in q.tobytes() + both.tobytes()
            assert any(x[:1] in (b"@", b">", b"+") for x in (y.tobytes() for y in quals))
        if p.has_long:
            L = [(len(a), len(b)) for a, b in zip(*c.reads)]
            assert any(max(x) > A.RP_MAX_LEN for x in L) and any(max(x) == A.RP_MAX_LEN for x in L)
        for h in F.handovers(p, c):
            l = h["layout"]
            assert all((o is None) == l.uniform for o in h["offsets"])
            assert [len(b) for b in h["bufs"]] == [2 * F.GUARD_BYTES + lead + h["nbytes"][i // 2] for i, lead in enumerate(h["leads"])]
            assert l.uniform or all(int(o[0]) == h["first"] for o in h["offsets"])


def test_the_reference_chain_has_structure_in_every_stage(plans, chains):
    """conditions, not measurements: per seed the shares of merged pairs and of adapter hits, over the seed set every flag of
    reads_fuzz_np.structure in three quarters of the seeds, mates over 1 024 bases in every seed that has long mates"""
    seen = collections.Counter()
    for p, H in zip(plans, chains):
        n = p.n_pairs
        merged = int((H["mg_rows"][:, M.RM_LEN] != 0).sum())
        assert 4 * merged >= n and 8 * (n - merged) >= n, (p.seed, merged, n)
        hit = int((H["ad_rows"][:, A.RA_HIT] != 0).sum())
        assert 5 * hit >= n and 5 * (n - hit) >= n, (p.seed, hit, n)
        s = F.structure(p, H)
        assert s["mate_over_1024"] == p.has_long, (p.seed, s)
        if p.has_long:                                    # on both sides of KMX_RP_MAX_LEN: a mate of 1 024 merges, one of 1 025 has no hit
            L1, L2 = np.diff(H["pq1_offsets"].astype(np.int64)), np.diff(H["pq2_offsets"].astype(np.int64))
            got = H["mg_rows"][:, M.RM_LEN] != 0
            assert (got & (np.maximum(L1, L2) == A.RP_MAX_LEN)).any() and not (got & (np.maximum(L1, L2) > A.RP_MAX_LEN)).any(), p.seed
        assert np.array_equal(np.sort(np.concatenate([H["mp_m_index"], H["mp_u1_index"]])), np.arange(n, dtype=np.uint64))
        assert np.array_equal(H["mp_u1_index"], H["mp_u2_index"]) and np.array_equal(H["tp1_index"], H["tp2_index"])
        seen.update(name for name, ok in s.items() if ok)
    need = -(-3 * len(plans) // 4)
    flags = set(F.structure(plans[0], chains[0])) - {"mate_over_1024"}
    assert len(flags) == 17 and all(seen[name] >= need for name in flags), (seen, need)


def test_mates_swapped_on_the_references(plans, chains):
    for p, H in zip(plans, chains):
        n = p.n_pairs
        c1, q1, o1, c2, q2, o2 = H["pq1_bases"], H["pq1_quals"], H["pq1_offsets"], H["pq2_bases"], H["pq2_quals"], H["pq2_offsets"]
        assert np.array_equal(F.overlap_np(p, c2, o2, c1, o1, n), F.swapped_overlap_expect(H["ov_rows"])), p.seed
        expect = F.swapped_merge_expect((H["mg_bases"], H["mg_quals"], H["mg_offsets"], H["mg_rows"]), F.pairs_over_acgtn(c1, o1, c2, o2))
        got = M.reads_pair_merge_np(c2, c1, n, 0, 0, H["ov_rows"][:, A.RP_INSERT], q2, q1, o2, o1, p.phred_base, p.q_cap)
        checked = F.check_swapped_merge(expect, got)
        merged = int((H["mg_rows"][:, M.RM_LEN] != 0).sum())
        assert 2 * checked >= merged > 0, (p.seed, checked, merged)


def test_pairs_permuted_on_the_references(plans, chains):
    for p, H in zip(plans, chains):
        n = p.n_pairs
        perm = F.permutation(p)
        (c1, q1, o1), (c2, q2, o2) = F.permuted(H, perm)
        ov = F.overlap_np(p, c1, o1, c2, o2, n)
        assert np.array_equal(ov, H["ov_rows"][perm]), p.seed
        b, q, off, rows = M.reads_pair_merge_np(c1, c2, n, 0, 0, ov[:, A.RP_INSERT], q1, q2, o1, o2, p.phred_base, p.q_cap)
        assert np.array_equal(rows, H["mg_rows"][perm])
        wb, woff = reads_np.gather_np(H["mg_bases"], n, 0, perm, H["mg_offsets"])
        wq, _ = reads_np.gather_np(H["mg_quals"], n, 0, perm, H["mg_offsets"])
        assert np.array_equal(b, wb) and np.array_equal(off, woff) and np.array_equal(q, wq), p.seed


def test_clean_pairs_merge_into_their_fragments(plans):
    """the pairs the device relation "merged error-free fragments count as the fragments" runs on: there are some in at least three
    quarters of the seeds, and the references merge every one of them into its fragment"""
    some = 0
    for p in plans:
        c = F.case_of(p)
        (b1, o1), (b2, o2), frags = F.clean_pairs(c)
        n = len(frags)
        some += n >= 4
        ov = A.reads_pair_overlap_np(b1, b2, n, 0, 0, o1, o2)
        b, _, off, _ = M.reads_pair_merge_np(b1, b2, n, 0, 0, ov[:, A.RP_INSERT], None, None, o1, o2)
        fb, fo = F.ragged(frags) if n else (b, off)
        assert np.array_equal(b, fb) and np.array_equal(off, fo), p.seed
    assert 4 * some >= 3 * len(plans), some
