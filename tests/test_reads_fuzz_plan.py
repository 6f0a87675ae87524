"""What the read-preparation fuzz (tests/test_gpu_reads_fuzz.py) will do, checked without a GPU: the coverage of the default seed set,
read off reads_fuzz_np.plan alone; the non-vacuity of its inputs, read off the reference chain reads_fuzz_np.host_pipeline alone; and
the relations the GPU test states on the device -- mates swapped, pairs permuted, error-free fragments; for the second library the
dedup of permuted, exchanged and reverse-complemented items, its idempotence and conservation, the mirrored complexity rows and the
FASTA image out of the FASTQ image -- on the references.

Non-vacuity of the second library, checked once on the CPU by breaking a scratch copy of a reference and comparing its chain with the
real one's arrays (no kernel was broken); the default seeds whose FIRST differing stage is the one named:
* the tie order of dedup heads (the last of equal scores instead of the first): dedup_pairs in 41 seeds (all but 20, 26, 27, 30, 32,
  37, 40), dedup_single in 30 and 32, the route pass's reads_dedup in 20, 26, 27, 37, 40;
* FLIPPED never set: dedup_pairs in 0, 2, 7, 9, 10, 15, 18, 19, 20, 23, 28, 31, 35, 38, 40, 42, 43, 46, the route pass in 39 (19 of
  the 24 strand seeds);
* h + t > L for h + t >= L: poly in 38 seeds (all but 2, 9, 21, 22, 27, 34, 39, 40, 45, 46);
* S_j >= dust_max for S_j > dust_max: poly in all 48;
* name_skip not clamped to the name's length: format in 0, 2, 4, 5, 10, 14, 15, 18, 21, 27, 32, 37, 41, 47, the route pass in 26, 33
  (the seeds with name_skip = 3, where the name that is only '@' is shorter than the skip);
* a FASTA record of L % width == 0 bases given one line more: format in 38 seeds (all with fa_width >= 1)."""
import collections

import numpy as np
import pytest

from tests import adapter_np as A
from tests import complexity_np as X
from tests import dedup_np as D
from tests import fastx_out_np as FO
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
    """conditions, not measurements: per seed the shares of merged pairs and of adapter hits, of dropped duplicates, of reads with a
    poly-X end and of reads the complexity filter drops; over the seed set every flag of reads_fuzz_np.structure in three quarters of
    the seeds (of the seeds that can show it: STRUCTURE_WHEN), mates over 1 024 bases in every seed that has long mates"""
    seen, every = collections.Counter(), []
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
        # ---- the second library: what the planting is there for, per seed
        lib = F.library_of(p)
        dropped = int((H["dd_keep"] == 0).sum())
        if p.dd_hash_bits == 64:                          # (fewer bits keep what collides: reads_fuzz_np's docstring)
            assert 10 * dropped >= lib.n and 2 * dropped <= lib.n, (p.seed, dropped, lib.n)
            assert int(H["dd_summary"][D.S_LARGEST]) >= (40 if p.seed % 6 == 2 else 5), (p.seed, H["dd_summary"])
        else:
            assert 2 * dropped <= lib.n and int(H["dd_summary"][D.S_COLLISIONS]) > 0, (p.seed, dropped, H["dd_summary"])
        ns = len(H["ds_index"])
        shortened = int((np.diff(H["xt_offsets"].astype(np.int64)) < np.diff(H["ds_offsets"].astype(np.int64))).sum())
        assert len(H["xt_index"]) == ns and 8 * shortened >= ns and 4 * shortened <= 3 * ns, (p.seed, shortened, ns)
        assert ns - len(H["xf_index"]) >= 2 and 2 * len(H["xf_index"]) >= ns, (p.seed, len(H["xf_index"]), ns)
        seen.update(name for name, ok in s.items() if ok)
        every.append(s)
    need = -(-3 * len(plans) // 4)
    flags = set(every[0]) - {"mate_over_1024"}
    assert len(flags) == 40 and set(F.STRUCTURE_WHEN) <= flags
    assert all(seen[name] >= need for name in flags - set(F.STRUCTURE_WHEN)), (seen, need)
    for name, can in F.STRUCTURE_WHEN.items():            # a flag only some seeds can show: in three quarters of those, four or more of them
        able = [s[name] for p, s in zip(plans, every) if can(p)]
        assert len(able) >= 4 and 4 * sum(able) >= 3 * len(able), (name, sum(able), len(able))


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


# ---------------------------------------------------------------- the second library
def test_coverage_of_the_second_librarys_plan_fields(plans):
    """every value of every new plan field occurs in the default set on both streams"""
    for stream in ("side", "default"):
        ps = [p for p in plans if p.stream == stream]
        assert {p.dd_strand for p in ps} == {False, True} and {p.dd_hash_bits for p in ps} == set(F.DD_HASH_BITS), stream
        assert {p.dd_score for p in ps} == set(F.DD_SCORES) and {(p.px_tail, p.px_head) for p in ps} == set(F.PX_PAIRS), stream
        assert {p.px_tail for p in ps} == {p.px_head for p in ps} == set(F.PX_MASKS) == {0, 4, 15, 9}
        assert {p.px_min_len for p in ps} == set(F.PX_MIN_LENS) == {5, 10, 20} and {p.px_max_error for p in ps} == set(F.PX_MAX_ERRORS)
        assert {p.px_penalty for p in ps} == set(F.PX_PENALTIES) == {0, 2, 255} and {p.dust_max for p in ps} == set(F.DUST_MAXES) == {60, 122, 610, 930}
        assert {p.min_diff for p in ps} == set(F.MIN_DIFFS) and {p.fa_width for p in ps} == set(F.FA_WIDTHS) == {0, 1, 60, 61, 70}
        assert {p.name_skip for p in ps} == set(F.NAME_SKIPS) == {0, 1, 3}
    assert all(p.px_tail or p.px_head for p in plans) and 4 * sum(bool(p.px_tail and p.px_head) for p in plans) >= len(plans)
    assert {p.dd_hash_bits for p in plans if p.dd_score != "none"} == set(F.DD_HASH_BITS) and {p.dd_strand for p in plans if p.dd_hash_bits == 64} == {False, True}
    assert all(p.name_base + 16 > 2**64 > p.name_base for p in plans)


def _run_at(read, end, x):
    """the length of the run of the letter x at an end of a read, the case ignored"""
    r = (read if end == "head" else read[::-1]) & 0xDF
    stop = np.nonzero(r != x)[0]
    return int(stop[0]) if len(stop) else len(r)


def test_the_library_with_copies_is_what_the_plan_says(plans):
    kinds_of_ends = collections.Counter()
    for p in plans:
        c, lib = F.case_of(p), F.library_of(p)
        n, N = p.n_pairs, lib.n
        assert n < N <= 1.4 * n + (40 if p.seed % 6 == 2 else 0), (p.seed, n, N)
        for m in range(2):
            text, reads, quals, names = lib.texts[m], lib.reads[m], lib.quals[m], lib.names[m]
            assert len(reads) == len(quals) == len(names) == N and sum(len(r) for r in reads) <= 1.35 * F.MAX_BASES, (p.seed, m)
            assert (b"\r" in text) == p.crlf[m] and text.endswith(b"\n") == p.trail[m] and text.count(b"\r\n") == (text.count(b"\n") if p.crlf[m] else 0)
            assert [bytes(x) for x in _four_lines(text)] == [r.tobytes() for r in reads]
            qb, qo = Q.fastq_quals(text)
            assert np.array_equal(qb, F.ragged(quals)[0]) and np.array_equal(qo, F.ragged(quals)[1])
            nb, no = FO.fastq_names(text)
            assert nb.tobytes() == b"".join(names) and np.array_equal(np.diff(no.astype(np.int64)), [len(x) for x in names])
            lines = text.replace(b"\r\n", b"\n").split(b"\n")
            assert all(lines[4 * i + 2] == b"+" + (names[i][1:] if i % 5 == 0 else b"") for i in range(N))
            # the names: only '@', 300 bytes and more, the four variants, every residue of the record length
            assert b"@" in names and max(len(x) for x in names) >= 300 and all(x[:1] == b"@" for x in names)
            assert all(any(x.endswith(v) for x in names) for v in (b" >x@y+z", b" +", b"@")), p.seed
            rec = [len(x) - min(p.name_skip, len(x)) + 2 * len(r) + 6 for x, r in zip(names, reads)]
            assert [x % 16 for x in rec[:16]] == list(range(16)) and {x % 4 for x in rec[16:]} == {0, 1, 2, 3}, (p.seed, m)
        # the first library's pairs are all there, in order (a poly-X end apart), and the last one is last
        orig = lib.where("orig")
        assert len(orig) == n and orig[-1] == N - 1 and all(len(lib.reads[0][i]) == len(c.reads[0][j]) for j, i in enumerate(orig))
        assert all(np.array_equal(lib.reads[1][i], c.reads[1][j]) for j, i in enumerate(orig))
        assert all(np.array_equal(lib.reads[0][i], c.reads[0][j]) for j, i in enumerate(orig) if i not in lib.ends)
        new = [i for i in range(N) if lib.kind[i] != "orig"]
        assert min(new) < N // 4 and sum(i < N // 2 for i in new) >= len(new) // 4, (p.seed, "the planted items are not only appended")
        # ---- the copies, by the definition of a duplicate (dedup_np.codes), and the near-copies
        code = lambda i: (D.codes(lib.reads[0][i]), D.codes(lib.reads[1][i]))
        raw = lambda i: (lib.reads[0][i].tobytes(), lib.reads[1][i].tobytes())
        for kind in ("exact", "case", "other", "swapped", "rc") + F.NEAR_KINDS:
            assert lib.where(kind), (p.seed, kind)
        for i in lib.where("exact", "case", "other"):
            assert code(i) == code(lib.src[i]), (p.seed, i)
        assert all(raw(i) == raw(lib.src[i]) for i in lib.where("exact")) and all(raw(i) != raw(lib.src[i]) for i in lib.where("case", "other"))
        for i in lib.where("other"):
            a, b = np.concatenate(lib.reads[0][i:i + 1] + lib.reads[1][i:i + 1]), np.concatenate([lib.reads[0][lib.src[i]], lib.reads[1][lib.src[i]]])
            d = np.nonzero(a != b)[0]
            assert len(d) == 1 and D.codes(a[d])[0] == D.codes(b[d])[0] == 4, (p.seed, i)
        for i in lib.where("swapped"):
            assert code(i) == code(lib.src[i])[::-1] and code(i) != code(lib.src[i])
        for i in lib.where("rc"):
            assert D.codes(lib.reads[0][i]) == D.rc(D.codes(lib.reads[0][lib.src[i]])) and code(i)[1] != code(lib.src[i])[1]
        near = lib.where(*F.NEAR_KINDS)
        assert len(near) >= 4
        for i in near:
            (a1, a2), (b1, b2) = code(i), code(lib.src[i])
            k = lib.kind[i]
            if k == "near_last":
                assert a1 == b1 and a2[:-1] == b2[:-1] and a2[-1] != b2[-1]
            elif k == "near_first":
                assert a2 == b2 and a1[1:] == b1[1:] and a1[0] != b1[0]
            elif k == "near_shorter":
                assert a2 == b2 and a1 == b1[:-1] and len(b1) >= 2
            else:
                assert a1 == b1 and a2 != b2
        classes = collections.Counter(code(i) for i in range(N))
        assert max(classes.values()) >= (40 if p.seed % 6 == 2 else 5), p.seed
        if p.seed % 6 == 2:
            big = max(classes, key=classes.get)
            assert len(big[0]) + len(big[1]) <= 80
        # ---- the poly-X ends: the letters of the plan's masks, runs of min_len - 1, min_len and min_len + 1
        for i, (end, kind, R) in lib.ends.items():
            kinds_of_ends[kind] += 1
            read = lib.reads[0][i]
            x = int((read[0] if end == "head" else read[-1]) & 0xDF)
            assert (p.px_tail if end == "tail" else p.px_head) >> b"ACGT".index(x) & 1, (p.seed, i)
            if kind in ("minus", "exact", "plus"):
                assert _run_at(read, end, x) == R == p.px_min_len + {"minus": -1, "exact": 0, "plus": 1}[kind], (p.seed, i, kind)
        ends = collections.Counter(kind for _, kind, _ in lib.ends.values())
        assert ends["minus"] and ends["exact"] and ends["plus"] and {e for e, _, _ in lib.ends.values()} == \
            {e for e, mask in (("tail", p.px_tail), ("head", p.px_head)) if mask}, (p.seed, ends)
        # ---- the reads that are no copies
        r1 = lambda kind: lib.reads[0][lib.where(kind)[0]]
        assert len(set(r1("homopolymer").tolist())) == 1 and len(set(r1("all_x").tolist())) == 1 and len(r1("empty1")) == 0
        for L in F.LC_LENGTHS:
            assert len(r1(f"ac{L}")) == len(r1(f"acg{L}")) == L and len(set(r1(f"ac{L}").tolist())) == 2 and len(set(r1(f"acg{L}").tolist())) == 3
            assert np.array_equal(r1(f"ac{L}")[2:], r1(f"ac{L}")[:-2]) and np.array_equal(r1(f"acg{L}")[3:], r1(f"acg{L}")[:-3])
        S = X.window_scores(X._LETTER[r1("dusty_mid")])
        assert len(S) == 5 and S[2] > p.dust_max >= max(S[0], S[4]) or p.dust_max == 60, (p.seed, S)
        assert X.window_scores(X._LETTER[r1("homopolymer")]).max() == X.DUST_NEVER and X.window_scores(X._LETTER[r1("ac64")])[0] == 930
        assert X.window_scores(X._LETTER[r1("acg64")])[0] == 610 and len(r1("fa_line")) == (p.fa_width if p.fa_width >= 60 else 60)
        cross = r1("cross")
        assert _run_at(cross, "tail" if p.px_tail else "head", int((cross[-1] if p.px_tail else cross[0]))) >= 40
        assert (len(cross) - 40 < 64 < len(cross)) if p.px_tail else _run_at(cross, "head", int(cross[0])) > 64
        ov = r1("overlap")
        assert len(ov) == 2 * (p.px_min_len + 2)
        # ---- the hand-overs: no uniform one; in the misaligned one three leads that differ mod 4
        hs = F.lib_handovers(p, lib)
        assert [h["name"] for h in hs] == [l.name for l in p.layouts if l.name != "uniform"] and len(hs) == 3
        for h in hs:
            assert [len(b) for b in h["bufs"]] == [2 * F.GUARD_BYTES + lead + h["nbytes"][(0, 0, 1, 1, 2)[i]] for i, lead in enumerate(h["leads"])]
            assert all(int(o[0]) == f for o, f in zip(h["offsets"], (h["first"], h["first"], h["nfirst"])))
            if h["name"] == "misaligned":
                b, q, _, _, nm = h["leads"]
                assert (nm - b) % 4 and (nm - q) % 4 and (q - b) % 4 and h["first"] >= 1 and h["nfirst"] >= 1
            else:
                assert set(h["leads"]) == {0} and h["first"] == h["nfirst"] == 0
    assert all(kinds_of_ends[k] >= len(plans) for k in ("minus", "exact", "plus")) and all(kinds_of_ends[k] >= len(plans) // 2 for k in ("lo", "hi", "pnx"))


def test_the_second_librarys_reference_chain_hangs_together(plans, chains):
    """what the references must agree on among themselves: conservation and idempotence of both dedup stages, dict_dedup where the
    contract makes it the answer, the batches in step, the round trip through the formatted image"""
    for p, H in zip(plans, chains):
        lib = F.library_of(p)
        for pre, reads, mates in (("dd", lib.reads[0], lib.reads[1]), ("ds", F.split(H["dp1_bases"], H["dp1_offsets"]), None)):
            rows, keep, summ = H[pre + "_rows"], H[pre + "_keep"], H[pre + "_summary"]
            F.check_dedup_conserved(rows, keep, summ)
            if p.dd_score == "none" and p.dd_hash_bits == 64:
                assert np.array_equal(keep, D.dict_dedup(reads, mates, p.dd_strand)), (p.seed, pre)
            kept = np.nonzero(keep)[0]
            score = None if p.dd_score == "none" else H["lq_rows"][:, Q.RQ_QSUM][kept if pre == "dd" else H["dp1_index"].astype(np.int64)[kept]]
            _, _, again = F.dedup_np([reads[i] for i in kept], None if mates is None else [mates[i] for i in kept], p, score)
            assert int(again[D.S_DROPPED]) == 0 and int(again[D.S_LARGEST]) == 1, (p.seed, pre, again)
        assert np.array_equal(H["dp1_index"], H["dp2_index"]) and np.array_equal(H["xt_index"], np.arange(len(H["ds_index"]), dtype=np.uint64))
        if p.name_skip == 1:                              # the round trip is the identity on the names too
            assert np.array_equal(H["rp_names"], H["xfn_bases"]) and np.array_equal(H["rp_noffsets"], H["xfn_offsets"])
        nb, no = FO.fastq_names(H["fq_image"].tobytes())
        assert np.array_equal(nb, H["rp_names"]) and np.array_equal(no, H["rp_noffsets"]), p.seed
        assert [bytes(x) for x in _four_lines(H["fq_image"].tobytes())] == [x.tobytes() for x in F.split(H["xf_bases"], H["xf_offsets"])]


def test_dedup_relations_on_the_references(plans):
    for p in plans:
        lib = F.library_of(p)
        r1, r2, n = lib.reads[0], lib.reads[1], lib.n
        # items permuted under a score that is unique per item
        perm = F.dedup_permutation(n, p.seed)
        first = F.dedup_np(r1, r2, p, np.arange(n))[:2]
        F.check_dedup_permuted(first, F.dedup_np([r1[i] for i in perm], [r2[i] for i in perm], p, perm)[:2], perm)
        # every pair's mates exchanged, the strand flag on
        rows, keep, _ = D.dedup(r1, r2, True, None, p.dd_hash_bits)
        got = D.dedup(r2, r1, True, None, p.dd_hash_bits)
        F.check_dedup_exchanged((rows, keep), got[:2])
        other = np.uint64(D.F_OTHER)
        assert ((rows[:, D.FLAGS] ^ got[0][:, D.FLAGS]) & ~other).max() == 0 and ((rows[:, D.FLAGS] ^ got[0][:, D.FLAGS]) & other).any(), p.seed
        # every read reverse-complemented, the strand flag on
        keep1 = D.dedup(r1, None, True, None, p.dd_hash_bits)[1]
        assert np.array_equal(D.dedup([F.rc_read(r) for r in r1], None, True, None, p.dd_hash_bits)[1], keep1), p.seed
        assert p.dd_hash_bits < 64 or (keep1 == 0).sum() >= 5, p.seed


def test_complexity_mirror_on_the_references(plans, chains):
    compared = 0
    for p, H in zip(plans, chains):
        b, o = F.mirror_batch(H["ds_bases"], H["ds_offsets"])
        a = F.mirror_args(p)
        got, _ = X.reads_complexity_np(b, len(o) - 1, 0, a["tail"], a["head"], a["min_len"], *a["max_error"], a["penalty"], p.dust_max, offsets=o)
        compared += F.check_complexity_mirror(H["cx_rows"], got)
    assert compared >= 20 * len(plans)


def test_format_relations_on_the_references(plans, chains):
    for p, H in zip(plans, chains):
        nf = len(H["xf_index"])
        named = dict(names=H["xfn_bases"], name_offsets=H["xfn_offsets"], name_skip=p.name_skip)
        fa0, rec0 = FO.format_np(H["xf_bases"], nf, 0, H["xf_offsets"], fmt=FO.FASTA, line_width=0, **named)
        assert np.array_equal(fa0, F.fasta_of_fastq(H["fq_image"], H["fq_rec"])), p.seed
        assert np.array_equal(rec0, F.record_offsets(p, H, FO.FASTA, 0)) and np.array_equal(H["fq_rec"], F.record_offsets(p, H, FO.FASTQ)), p.seed
        assert np.array_equal(H["fa_rec"], F.record_offsets(p, H, FO.FASTA, p.fa_width)), p.seed
        assert len(H["gq_image"]) == int(H["gq_rec"][-1]) and b"@0\n" in H["gq_image"].tobytes() and H["gq_image"].tobytes().startswith(b"@%d\n" % p.name_base)
