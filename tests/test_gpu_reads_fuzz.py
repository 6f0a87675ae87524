"""Seeded differential fuzz of the read-preparation calls on the GPU (tests/reads_fuzz_np.py decides every case and runs the references;
tests/test_reads_fuzz_plan.py checks the seed set's coverage and non-vacuity on the CPU).

Per seed, on a FRESH Context (on a torch.cuda.Stream() of its own for odd seeds, torch's default stream for even ones):

1. the chain -- parse of both FASTQ images, adapters off mate 1, quality mask / rows / filter, the count table of what is left, both
   mates trimmed by quality in step, the mates' overlap and its trim, the merge (with rows, without, without quality bytes), merged
   and unmerged apart, the merged reads by length class; then, on the seed's SECOND library (reads_fuzz_np.library_of: the pairs with
   planted copies, near-copies, poly-X ends, low-complexity reads and odd names), fastq_records of both images with fastx_names
   between the parses, the pairs deduplicated under a quality score (reads_drop_duplicates, names gathered by its index), mate 1 of
   the survivors deduplicated alone, poly-X ends and DUST (reads_complexity out of place and in place, reads_trim_poly,
   reads_complexity_filter), the count table of the masked batch, the batch as FASTQ, FASTA and FASTQ with generated names
   (fastx_format, write_fastx), and that FASTQ image parsed back on the device -- every stage fed by the previous stage's device
   output, every array compared for u64 or byte equality with the reference chain; the outputs the test allocates itself sit between
   guard words;
2. the warm repeat: the chain once more on the same context, byte-identical, with no further allocation of the work buffer;
3. route equivalence: every reads-form call (adapter, quality, pair overlap, pair merge, select with a span, gather) on the raw parsed
   mates, from host-built hand-overs of every layout of the plan, equal to the reference on the first and byte-identical on the others;
   likewise reads_dedup of the pairs, reads_complexity and fastx_format with names on the second library's raw mates, for its three
   layouts (it has no uniform one) -- in the misaligned one bases, quality bytes and names each at a lead of their own mod 4;
4. relations: mates swapped (overlap and merge), pairs permuted, and the merged error-free pairs of the seed count as their fragments;
   for the second library the dedup of permuted items under a unique score, of pairs with their mates exchanged and of
   reverse-complemented reads under the strand flag, idempotence and conservation of both dedup stages, dict_dedup where there is no
   score and the whole fingerprint, the complexity rows of the mirrored batch, the FASTA image out of the FASTQ image, the record
   offsets out of the record lengths, and for name_skip = 1 the round trip through the image as the identity.

Everything is integer work: no tolerance anywhere.  Results are read the way a user on torch's default stream reads them
(Stream.wait_stream, then .cpu(); no host synchronisation is added).  KMX_READS_FUZZ_N widens the seed set for a one-off sweep.

Three more tests: every stage (and fastx_quals and fastx_names without SAME_TEXT) as the first call a context ever serves, for seeds 5
(side stream, mates of one length) and 6 (default stream, a mix with mates of 1 024 bases and more); two contexts interleaved stage by
stage; and fastq_records of mate 1, mate 2, mate 1 on one context.

Measured on one MI355X in one session: this file 13.2 s for its 87 cases, the file as it was before the second library 8.3 s for its
71 next to it (the 8.6 s of an earlier session), so the 48 seeds, the three route layouts and the planted share stay as they are.
The slowest seed is 0 with 2.6 s, which carries the library start-up; the next one takes 0.33 s, most 0.22 s.  reads_dedup is
synchronous and reads a record back per digit its sort descends, up to all 16 for the class of 40 copies (seed % 6 == 2): where
that dominates a seed it is expected, and at these sizes it does not show (seeds 2, 8, 14, ... are not among the ten slowest).
Coverage of the 48 default seeds (96 .. 208 pairs each): layouts ragged0 48, ragged_bound 48, misaligned 48, uniform 14 -- as the
chain's first layout 16, 14, 15 and 3; streams 24 side and 24 default (7 + 7 in length mode "one", 17 + 17 in "mix"); long mates in
12 seeds, 6 on either stream; adapter-set sizes 1: 4 seeds, 2 to 5: 9 each, 8: 8 seeds; phred base 33 in 30 seeds and 64 in 18;
trim "mott", "run" and None in 16 each.  The second library (134 .. 276 items, 35 .. 88 planted poly-X ends; first layout ragged0 19,
misaligned 15, ragged_bound 14): dd_strand 24 / 24; dd_hash_bits 64: 24, 8: 8, 4: 8, 1: 8; dd_score none, strided, contiguous 16
each; px_tail and px_head 4, 15 and 9 (A and T): 14 each, 0: 6, both non-zero in 36; px_min_len 5, 10, 20 and px_max_error 0, 1/10,
1/4 and px_penalty 0, 2, 255 and min_diff 3/10, 1/2, 1/5 and name_skip 0, 1, 3: 16 each; dust_max 60, 122, 610, 930: 12 each;
fa_width 0, 1, 60, 61: 10 each, 70: 8 -- every value on both streams (tests/test_reads_fuzz_plan.py asserts it).  A one-off sweep of
480 seeds (KMX_READS_FUZZ_N=480, 98 s) passed, the second library's stages included: no seed of either set disagreed with its
reference."""
import os

import numpy as np
import pytest

from tests import reads_fuzz_np as F
from tests.test_gpu_count_fuzz import Run as CountRun, _assert_same, _context, _same

pytestmark = pytest.mark.gpu

N_FUZZ = int(os.environ.get("KMX_READS_FUZZ_N", F.N_DEFAULT))
G = F.GUARD_BYTES


def _lens_max(offsets):
    return int(np.diff(np.asarray(offsets).astype(np.int64)).max(initial=0))


class Run(CountRun):
    """one plan on one context: the stages of the chain as methods that return {name: host array}, the device batches kept between them
    as (bases, quality bytes, n, read_len, offsets).  host(), guarded() and intact() are the count fuzz's."""

    def __init__(self, ctx, p, case):
        import torch

        self.torch, self.ctx, self.p, self.case, self.n = torch, ctx, p, case, p.n_pairs
        self.hands = F.handovers(p, case)
        self._handed = {}
        self.host_texts = [np.concatenate([np.full(G, ord("#"), np.uint8), np.frombuffer(t, np.uint8), np.full(G, ord("#"), np.uint8)]) for t in case.texts]
        self.d_texts = [ctx.to_device(t) for t in self.host_texts]
        self.texts = [d[G:len(d) - G] for d in self.d_texts]
        self.quality_args = dict(min_q=p.min_q, trim_q=p.trim_q, k=p.k, phred=p.phred_base)
        self.overlap_args = dict(min_overlap=p.ov_min_overlap, max_mism=p.ov_max_mism)
        # the second library
        self.lib = F.library_of(p, case)
        self.lib_hands = F.lib_handovers(p, self.lib)
        self._lib_handed = {}
        self.host_lib_texts = [np.concatenate([np.full(G, ord("#"), np.uint8), np.frombuffer(t, np.uint8), np.full(G, ord("#"), np.uint8)])
                               for t in self.lib.texts]
        self.d_lib_texts = [ctx.to_device(t) for t in self.host_lib_texts]
        self.lib_texts = [d[G:len(d) - G] for d in self.d_lib_texts]
        self.dedup_args = dict(strand=p.dd_strand, hash_bits=p.dd_hash_bits)
        self.pre_lq = None
        self.relaid = []

    # ---- plumbing
    def on_stream(self):
        return self.torch.cuda.stream(self.ctx.stream)

    def handed(self, i):
        """the raw mates on the device as layout i hands them over -> (mate 1, mate 2), each (bases, quals, n, read_len, offsets)"""
        if i not in self._handed:
            h = self.hands[i]
            first = h["first"]
            d = [self.ctx.to_device(b) for b in h["bufs"]]
            views = [d[j][G + h["leads"][j] - first:G + h["leads"][j] + h["nbytes"][j // 2]] for j in range(4)]
            assert all((views[j].data_ptr() + first) % 16 == h["leads"][j] % 16 for j in range(4))
            offs = [None if o is None else self.ctx.to_device(o) for o in h["offsets"]]
            self._handed[i] = (d, ((views[0], views[1], self.n, h["layout"].bound, offs[0]), (views[2], views[3], self.n, h["layout2"].bound, offs[1])))
        return self._handed[i][1]

    def batch(self, b, q=None):
        """a ReadBatch (and the one of its quality bytes) as the next call takes it"""
        return (b.bases, None if q is None else q.bases, b.n_reads, b.max_len(), b.offsets)

    def out_of(self, prefix, b, q=None, index=True):
        out = {prefix + "_bases": self.host(b.bases), prefix + "_offsets": self.host(b.offsets)}
        assert b.n_reads == len(out[prefix + "_offsets"]) - 1 and b.n_bases == len(out[prefix + "_bases"])
        if q is not None:
            out[prefix + "_quals"] = self.host(q.bases)
            assert _same(self.host(q.offsets), out[prefix + "_offsets"]), (prefix, "bases and quality bytes went apart")
        if index:
            out[prefix + "_index"] = self.host(b.index)
        return out

    # ---- the stages
    def parse(self):
        out = {}
        self.parsed = {}
        for m in (1, 2):
            bases, quals, n, L, offsets = self.ctx.fastq_reads(self.texts[m - 1])
            uniform = offsets is None
            if uniform:
                offsets = self.ctx.to_device(np.arange(n + 1, dtype=np.uint64) * np.uint64(L))
            out.update({f"p{m}_bases": self.host(bases), f"p{m}_quals": self.host(quals), f"p{m}_offsets": self.host(offsets),
                        f"p{m}_layout": np.array([n, L, uniform], np.uint64)})
            self.parsed[m] = (bases, quals, n, L, offsets, uniform)
        self.relayout()
        return out

    def relayout(self):
        """the device-parsed files as the plan's first layout: what stages 2 and 5 take"""
        torch, p = self.torch, self.p
        self.h, self.relaid = {}, [x for x in self.relaid if x[3] == "library"]
        for m, lay in ((1, p.layouts[0]), (2, p.layouts2[0])):
            bases, quals, n, L, off, uniform = self.parsed[m]
            assert uniform or not lay.uniform
            first = p.first(lay)
            if lay.name == "misaligned":
                views = []
                with self.on_stream():
                    for src, lead in ((bases, lay.lead), (quals, p.qlead(lay))):
                        whole = torch.full((G + lead + src.numel() + G,), ord("#"), dtype=torch.uint8, device=src.device)
                        whole[G + lead:G + lead + src.numel()].copy_(src)
                        views.append(whole[G + lead - first:G + lead + src.numel()])
                        self.relaid.append((whole, G + lead, src, "first"))
                    off = None if lay.uniform else off + first
                self.h[m] = (views[0], views[1], n, lay.bound, off)
            else:
                self.h[m] = (bases, quals, n, lay.bound, None if lay.uniform else off)

    def adapter(self):
        p = self.p
        b, q, n, L, off = self.h[1]
        whole, out = self.guarded(4 * n, np.int64)
        rows = self.ctx.reads_adapter(b, n, L, p.adapters, p.ad_min_overlap, p.ad_max_error, offsets=off, out=out)
        assert self.intact(whole, 4 * n), "reads_adapter wrote outside its output"
        tb, tq, rows2 = self.ctx.reads_trim_adapters(b, n, L, p.adapters, p.ad_min_overlap, p.ad_max_error, offsets=off, quals=q, min_len=p.min_len)
        res = {"ad_rows": self.host(rows), **self.out_of("ta", tb, tq)}
        assert _same(self.host(rows2), res["ad_rows"])
        self.ta = self.batch(tb, tq)
        return res

    def quality(self):
        p = self.p
        b, q, n, L, off = self.ta
        nb = int(b.numel())
        whole, out = self.guarded(nb, np.uint8)
        masked, rows = self.ctx.reads_quality(b, q, n, L, weights="ee", offsets=off, out=out, **self.quality_args)
        assert masked is out and self.intact(whole, nb), "reads_quality wrote outside its output"
        with self.on_stream():
            copy = b.clone()
        in_place, rows_b = self.ctx.reads_quality(copy, q, n, L, weights="ee", offsets=off, out=copy, **self.quality_args)
        res = {"q_masked": self.host(out), "q_rows": self.host(rows)}
        assert in_place is copy and _same(self.host(copy), res["q_masked"]) and _same(self.host(rows_b), res["q_rows"]), "reads_quality in place"
        fb, fq, rows_c = self.ctx.reads_quality_filter(b, q, n, L, offsets=off, max_ee=p.max_ee, min_len=p.min_len, trim=p.trim, **self.quality_args)
        assert _same(self.host(rows_c), res["q_rows"])
        res.update(self.out_of("qf", fb, fq))
        self.qf = self.batch(fb, fq)
        return res

    def count(self):
        b, _, n, L, off = self.qf
        fn = self.ctx.count_canonical2 if self.p.count_k > 32 else self.ctx.count_canonical
        d_k, d_c = fn(b, n, L, self.p.count_k, offsets=off)
        return {"table_k": self.host(d_k), "table_c": self.host(d_c)}

    def pair_quality(self):
        res = {}
        self.pq = {}
        for m, trim in ((1, "mott"), (2, "run")):
            b, q, n, L, off = self.h[m]
            fb, fq, rows = self.ctx.reads_quality_filter(b, q, n, L, offsets=off, max_ee=None, min_len=0, trim=trim, **self.quality_args)
            res.update(self.out_of(f"pq{m}", fb, fq))
            res[f"pq{m}_rows"] = self.host(rows)
            self.pq[m] = self.batch(fb, fq)
        return res

    def pair_args(self, pq=None):
        (b1, q1, n, L1, o1), (b2, q2, _, L2, o2) = pq or (self.pq[1], self.pq[2])
        return (b1, b2, n, L1, L2), (q1, q2), (o1, o2)

    def overlap(self):
        reads, _, offs = self.pair_args()
        n = reads[2]
        whole, out = self.guarded(4 * n, np.int64)
        rows = self.ctx.reads_pair_overlap(*reads, *offs, out=out, **self.overlap_args)
        assert self.intact(whole, 4 * n), "reads_pair_overlap wrote outside its output"
        t1, t2, rows2 = self.ctx.reads_trim_pairs(*reads, *offs, min_len=self.p.min_len, **self.overlap_args)
        res = {"ov_rows": self.host(rows), **self.out_of("tp1", t1), **self.out_of("tp2", t2)}
        assert _same(self.host(rows2), res["ov_rows"])
        self.ov = rows
        return res

    def merge_call(self, reads, quals, offs, insert, rows=True):
        b, q, r = self.ctx.reads_pair_merge(*reads, insert, *quals, *offs, phred_base=self.p.phred_base, q_cap=self.p.q_cap, rows=rows)
        assert b.n_reads == reads[2] and (q is None or _same(self.host(q.offsets), self.host(b.offsets)))
        return b, q, r

    def merge(self):
        from kmers_amd._lib import RP_INSERT

        reads, quals, offs = self.pair_args()
        insert = self.ov[:, RP_INSERT]                     # the strided column, as it is
        b, q, rows = self.merge_call(reads, quals, offs, insert)
        res = {"mg_bases": self.host(b.bases), "mg_quals": self.host(q.bases), "mg_offsets": self.host(b.offsets), "mg_rows": self.host(rows)}
        b2, q2, none = self.merge_call(reads, quals, offs, insert, rows=False)
        assert none is None and _same(self.host(b2.bases), res["mg_bases"]) and _same(self.host(q2.bases), res["mg_quals"]) \
            and _same(self.host(b2.offsets), res["mg_offsets"]), "reads_pair_merge without rows"
        b3, q3, rows3 = self.merge_call(reads, (None, None), offs, insert)
        assert q3 is None
        res.update({"mgn_bases": self.host(b3.bases), "mgn_offsets": self.host(b3.offsets), "mgn_rows": self.host(rows3)})
        self.mg = (b.bases, q.bases, b.n_reads, b.max_len(), b.offsets, rows)
        return res

    def merge_pairs(self):
        reads, quals, offs = self.pair_args()
        mp = self.ctx.reads_merge_pairs(*reads, *quals, *offs, phred_base=self.p.phred_base, q_cap=self.p.q_cap, **self.overlap_args)
        res = {**self.out_of("mp_m", mp.merged, mp.merged_quals), **self.out_of("mp_u1", mp.unmerged1, mp.unmerged1_quals),
               **self.out_of("mp_u2", mp.unmerged2, mp.unmerged2_quals), "mp_ov_rows": self.host(mp.overlap_rows), "mp_mg_rows": self.host(mp.merge_rows)}
        for short, long in (("mp_mq_bases", "mp_m_quals"), ("mp_u1q_bases", "mp_u1_quals"), ("mp_u2q_bases", "mp_u2_quals")):
            res[short] = res.pop(long)
        both = np.sort(np.concatenate([res["mp_m_index"], res["mp_u1_index"]]))
        assert _same(both, np.arange(self.n, dtype=np.uint64)) and _same(res["mp_u1_index"], res["mp_u2_index"]), "not a partition of the pairs"
        return res

    def partition(self):
        from kmers_amd._lib import RM_LEN

        torch = self.torch
        b, _, n, L, off, rows = self.mg
        with self.on_stream():                             # (the labels of reads_fuzz_np.length_labels, out of the device's rows)
            length = rows[:, RM_LEN]
            labels = torch.where(length == 0, torch.full_like(length, -1), (length >= 64).to(torch.int64) + (length >= 256).to(torch.int64))
        g = self.ctx.reads_partition(b, n, L, labels, offsets=off)
        assert g.n_groups == int(g.labels.numel())
        return {**self.out_of("pt", g.batch), "pt_labels": self.host(g.labels), "pt_groups": self.host(g.group_offsets)}

    # ---- the stages of the second library
    def lib_handed(self, i):
        """the second library's raw mates and mate 1's names on the device as its layout i hands them over -> (mate 1, mate 2, names):
        (bases, quals, n, read_len, offsets) twice and (names, name offsets)"""
        if i not in self._lib_handed:
            h, n = self.lib_hands[i], self.lib.n
            firsts = (h["first"],) * 4 + (h["nfirst"],)
            d = [self.ctx.to_device(b) for b in h["bufs"]]
            views = [d[j][G + h["leads"][j] - firsts[j]:G + h["leads"][j] + h["nbytes"][(0, 0, 1, 1, 2)[j]]] for j in range(5)]
            assert all((views[j].data_ptr() + firsts[j]) % 16 == h["leads"][j] % 16 for j in range(5))
            offs = [self.ctx.to_device(o) for o in h["offsets"]]
            self._lib_handed[i] = (d, ((views[0], views[1], n, h["bounds"][0], offs[0]), (views[2], views[3], n, h["bounds"][1], offs[1]),
                                       (views[4], offs[2])))
        return self._lib_handed[i][1]

    def _parsed(self, prefix, got):
        """what fastq_records returned as the arrays of the reference -> ({name: array}, offsets on the device)"""
        bases, quals, n, L, offsets, names, noff = got
        uniform = offsets is None
        if uniform:
            offsets = self.ctx.to_device(np.arange(n + 1, dtype=np.uint64) * np.uint64(L))
        return {prefix + "_bases": self.host(bases), prefix + "_quals": self.host(quals), prefix + "_offsets": self.host(offsets),
                prefix + "_layout": np.array([n, L, uniform], np.uint64), prefix + "_names": self.host(names), prefix + "_noffsets": self.host(noff)}, offsets

    def records(self):
        ctx, p, (t1, t2) = self.ctx, self.p, self.lib_texts
        # mate 2 parsed between mate 1's reads and mate 1's names: the SAME_TEXT shortcut serves the image that was summarised last
        ctx.fastq_reads(t1)
        ctx.fastq_reads(t2)
        between = {}
        if p.seed % 2:
            between[2] = ctx.fastx_names(t2, same_text=True)
        between[1] = ctx.fastx_names(t1, same_text=False)
        if not p.seed % 2:
            between[2] = ctx.fastx_names(t2, same_text=False)
        out, got = {}, {}
        for m in (1, 2):
            got[m] = ctx.fastq_records(self.lib_texts[m - 1])
            res, offsets = self._parsed(f"r{m}", got[m])
            assert _same(self.host(between[m][0]), res[f"r{m}_names"]) and _same(self.host(between[m][1]), res[f"r{m}_noffsets"]), \
                (p.seed, "fastx_names between the parses of the two images", m)
            out.update(res)
            got[m] = got[m][:4] + (offsets,) + got[m][5:]
        # the device-parsed library as its first layout: what dedup_pairs takes
        h = self.lib_hands[0]
        self.relaid = [x for x in self.relaid if x[3] != "library"]
        self.lh = {}
        for m in (1, 2):
            bases, quals, n, _, off, _, _ = got[m]
            if h["name"] == "misaligned":
                views = []
                with self.on_stream():
                    for src, lead in ((bases, h["leads"][2 * m - 2]), (quals, h["leads"][2 * m - 1])):
                        whole = self.torch.full((G + lead + src.numel() + G,), ord("#"), dtype=self.torch.uint8, device=src.device)
                        whole[G + lead:G + lead + src.numel()].copy_(src)
                        views.append(whole[G + lead - h["first"]:G + lead + src.numel()])
                        self.relaid.append((whole, G + lead, src, "library"))
                    off = off + h["first"]
                self.lh[m] = (views[0], views[1], n, h["bounds"][m - 1], off)
            else:
                self.lh[m] = (bases, quals, n, h["bounds"][m - 1], off)
        self.lnames = got[1][5:]
        return out

    def dedup_pairs(self):
        from kmers_amd._lib import RQ_QSUM

        ctx, p = self.ctx, self.p
        (b1, q1, n, L1, o1), (b2, q2, _, L2, o2) = self.lh[1], self.lh[2]
        lq = self.pre_lq if self.pre_lq is not None else ctx.reads_quality(b1, q1, n, L1, offsets=o1, mask=False, **self.quality_args)[1]
        self.score = None
        if p.dd_score != "none":
            self.score = lq[:, RQ_QSUM]                      # the strided column, as it is -- or a contiguous copy of it
            if p.dd_score == "contiguous":
                with self.on_stream():
                    self.score = self.score.contiguous()
            assert self.score.is_contiguous() == (p.dd_score == "contiguous")
        dd = ctx.reads_drop_duplicates(b1, n, L1, offsets=o1, quals=q1, mates=(b2, L2, o2), mate_quals=q2, score=self.score, **self.dedup_args)
        d = dd.duplicates
        names = ctx.reads_gather(self.lnames[0], n, 0, dd.reads.index, offsets=self.lnames[1])
        res = {"lq_rows": self.host(lq), "dd_rows": self.host(d.rows), "dd_keep": self.host(d.keep),
               "dd_summary": np.array([d.kept, d.dropped, d.largest, d.collisions], np.uint64), **self.out_of("dp1", dd.reads, dd.quals),
               **self.out_of("dp2", dd.mates, dd.mate_quals), "dpn_bases": self.host(names.bases), "dpn_offsets": self.host(names.offsets)}
        self.dp, self.dp2, self.dp_index, self.dpn = self.batch(dd.reads, dd.quals), self.batch(dd.mates, dd.mate_quals), dd.reads.index, (names.bases, names.offsets)
        return res

    def single_score(self):
        """the score of the pair stage's survivors: the column gathered by their index"""
        if self.score is None:
            return None
        with self.on_stream():
            return self.score[self.dp_index]

    def dedup_single(self):
        ctx = self.ctx
        b, q, n, L, off = self.dp
        d = ctx.reads_dedup(b, n, L, offsets=off, score=self.single_score(), **self.dedup_args)
        sb = ctx.reads_select(b, n, L, keep=d.keep, offsets=off, index=True)
        sq = ctx.reads_select(q, n, L, keep=d.keep, offsets=off)
        names = ctx.reads_gather(self.dpn[0], n, 0, sb.index, offsets=self.dpn[1])
        res = {"ds_rows": self.host(d.rows), "ds_keep": self.host(d.keep), "ds_summary": np.array([d.kept, d.dropped, d.largest, d.collisions], np.uint64),
               **self.out_of("ds", sb, sq), "dsn_bases": self.host(names.bases), "dsn_offsets": self.host(names.offsets)}
        self.ds, self.dsn = self.batch(sb, sq), (names.bases, names.offsets)
        return res

    def poly(self):
        ctx, p = self.ctx, self.p
        b, q, n, L, off = self.ds
        nb = int(b.numel())
        args = dict(offsets=off, **p.px_args)
        whole, out = self.guarded(nb, np.uint8)
        masked, rows = ctx.reads_complexity(b, n, L, dust_max=p.dust_max, mask=True, out=out, **args)
        assert masked is out and self.intact(whole, nb), "reads_complexity wrote outside its output"
        with self.on_stream():
            copy = b.clone()
        in_place, rows_b = ctx.reads_complexity(copy, n, L, dust_max=p.dust_max, mask=True, out=copy, **args)
        res = {"cx_rows": self.host(rows), "cx_masked": self.host(out)}
        assert in_place is copy and _same(self.host(copy), res["cx_masked"]) and _same(self.host(rows_b), res["cx_rows"]), "reads_complexity in place"
        tb, tq, trows = ctx.reads_trim_poly(b, n, L, quals=q, **args)
        res.update({"xt_rows": self.host(trows), **self.out_of("xt", tb, tq)})
        fb, fq, frows = ctx.reads_complexity_filter(b, n, L, dust_max=p.dust_max, min_diff=p.min_diff, trim=True, quals=q, **args)
        assert _same(self.host(frows), res["cx_rows"])
        names = ctx.reads_gather(self.dsn[0], n, 0, fb.index, offsets=self.dsn[1])
        res.update({**self.out_of("xf", fb, fq), "xfn_bases": self.host(names.bases), "xfn_offsets": self.host(names.offsets)})
        self.cxm, self.xf, self.xfn = out, self.batch(fb, fq), (names.bases, names.offsets)
        return res

    def count_masked(self):
        _, _, n, L, off = self.ds
        fn = self.ctx.count_canonical2 if self.p.count_k > 32 else self.ctx.count_canonical
        d_k, d_c = fn(self.cxm, n, L, self.p.count_k, offsets=off)
        return {"cm_k": self.host(d_k), "cm_c": self.host(d_c)}

    def format(self):
        import io

        from kmers_amd._lib import FASTX_FASTA

        ctx, p = self.ctx, self.p
        b, q, n, L, off = self.xf
        named = dict(names=self.xfn[0], name_offsets=self.xfn[1], name_skip=p.name_skip)
        fq, fq_rec = ctx.fastx_format(b, n, L, offsets=off, quals=q, rec_offsets=True, **named)
        fa, fa_rec = ctx.fastx_format(b, n, L, offsets=off, fmt=FASTX_FASTA, line_width=p.fa_width, rec_offsets=True, **named)
        gq, gq_rec = ctx.fastx_format(b, n, L, offsets=off, name_base=p.name_base, qual_fill=p.qual_fill, rec_offsets=True)
        res = {"fq_image": self.host(fq), "fq_rec": self.host(fq_rec), "fa_image": self.host(fa), "fa_rec": self.host(fa_rec),
               "gq_image": self.host(gq), "gq_rec": self.host(gq_rec)}
        file = io.BytesIO()
        assert ctx.write_fastx(file, b, n, L, offsets=off, quals=q, **named) == len(res["fq_image"]) and file.getvalue() == res["fq_image"].tobytes(), "write_fastx"
        # the FASTA image at width 0 is the FASTQ image without its '+' and quality lines
        fa0 = ctx.fastx_format(b, n, L, offsets=off, fmt=FASTX_FASTA, line_width=0, **named)
        assert _same(self.host(fa0), F.fasta_of_fastq(res["fq_image"], res["fq_rec"])), "the FASTA image out of the FASTQ image"
        self.fq_image = fq
        return res

    def reparse(self):
        return self._parsed("rp", self.ctx.fastq_records(self.fq_image))[0]

    # ---- the route pass
    def routes(self, i):
        """every reads-form call on the raw mates as layout i hands them over -> {name: array}, ad_rows and F.ROUTES"""
        from kmers_amd._lib import RA_KEEP, RP_INSERT

        p = self.p
        first = self.hands[i]["first"]
        pq = self.handed(i)
        b, q, n, L, off = pq[0]
        ad = self.ctx.reads_adapter(b, n, L, p.adapters, p.ad_min_overlap, p.ad_max_error, offsets=off)
        masked, qrows = self.ctx.reads_quality(b, q, n, L, weights="ee", offsets=off, **self.quality_args)
        reads, quals, offs = self.pair_args(pq)
        ov = self.ctx.reads_pair_overlap(*reads, *offs, **self.overlap_args)
        mb, mq, mrows = self.merge_call(reads, quals, offs, ov[:, RP_INSERT])
        sel = self.ctx.reads_select(b, n, L, span=ad[:, RA_KEEP], span_k=0, min_len=p.min_len, offsets=off, index=True)
        gat = self.ctx.reads_gather(b, n, L, self.ctx.to_device(F.gather_index(p, n)), span=ad[:, RA_KEEP], offsets=off)
        return {"ad_rows": self.host(ad), "rt_q_masked": self.host(masked)[first:], "rt_q_rows": self.host(qrows), "rt_ov_rows": self.host(ov),
                "rt_mg_bases": self.host(mb.bases), "rt_mg_quals": self.host(mq.bases), "rt_mg_offsets": self.host(mb.offsets),
                "rt_mg_rows": self.host(mrows), "rt_sel_bases": self.host(sel.bases), "rt_sel_offsets": self.host(sel.offsets),
                "rt_sel_index": self.host(sel.index), "rt_gat_bases": self.host(gat.bases), "rt_gat_offsets": self.host(gat.offsets)}

    def routes2(self, i):
        """reads_dedup of the pairs, reads_complexity and fastx_format of mate 1 on the second library's raw mates as its layout i
        hands them over -> {name: array}, F.ROUTES2"""
        ctx, p = self.ctx, self.p
        h = self.lib_hands[i]
        (b1, q1, n, L1, o1), (b2, _, _, L2, o2), (nm, noff) = self.lib_handed(i)
        d = ctx.reads_dedup(b1, n, L1, offsets=o1, mates=(b2, L2, o2), **self.dedup_args)
        masked, rows = ctx.reads_complexity(b1, n, L1, dust_max=p.dust_max, offsets=o1, **p.px_args)
        image, rec = ctx.fastx_format(b1, n, L1, offsets=o1, quals=q1, names=nm, name_offsets=noff, name_skip=p.name_skip, rec_offsets=True)
        return {"rt2_dd_rows": self.host(d.rows), "rt2_dd_keep": self.host(d.keep),
                "rt2_dd_summary": np.array([d.kept, d.dropped, d.largest, d.collisions], np.uint64), "rt2_cx_rows": self.host(rows),
                "rt2_cx_masked": self.host(masked)[h["first"]:], "rt2_fq_image": self.host(image), "rt2_fq_rec": self.host(rec)}

    # ---- a context that has served no call yet
    def preload(self, H):
        """every device object a stage reads, uploaded from the reference's arrays: copies only, no kernel -- so that the stage called
        next is the first call the context ever serves; the raw mates come as the first layout's host-built hand-over"""
        dev = self.ctx.to_device
        self.h = dict(zip((1, 2), self.handed(0)))
        for name, pre in (("ta", "ta"), ("qf", "qf")):
            setattr(self, name, (dev(H[pre + "_bases"]), dev(H[pre + "_quals"]), len(H[pre + "_offsets"]) - 1, _lens_max(H[pre + "_offsets"]),
                                 dev(H[pre + "_offsets"])))
        self.pq = {m: (dev(H[f"pq{m}_bases"]), dev(H[f"pq{m}_quals"]), self.n, _lens_max(H[f"pq{m}_offsets"]), dev(H[f"pq{m}_offsets"])) for m in (1, 2)}
        self.ov = dev(H["ov_rows"])
        self.mg = (dev(H["mg_bases"]), dev(H["mg_quals"]), self.n, _lens_max(H["mg_offsets"]), dev(H["mg_offsets"]), dev(H["mg_rows"]))
        # the second library: its raw mates as its first layout's host-built hand-over, every later input from the reference's arrays
        from kmers_amd._lib import RQ_QSUM

        def up(pre, names=None):
            n = len(H[pre + "_offsets"]) - 1
            setattr(self, pre if pre[-1] != "1" else pre[:-1], (dev(H[pre + "_bases"]), dev(H[pre + "_quals"]), n, _lens_max(H[pre + "_offsets"]), dev(H[pre + "_offsets"])))
            if names:
                setattr(self, names, (dev(H[names + "_bases"]), dev(H[names + "_offsets"])))

        self.lh = dict(zip((1, 2), self.lib_handed(0)[:2]))
        self.lnames = self.lib_handed(0)[2]
        self.pre_lq = dev(H["lq_rows"])
        self.score = None if self.p.dd_score == "none" else dev(H["lq_rows"][:, RQ_QSUM])
        self.dp_index = dev(H["dp1_index"])
        up("dp1", "dpn")
        up("ds", "dsn")
        up("xf", "xfn")
        self.cxm, self.fq_image = dev(H["cx_masked"]), dev(H["fq_image"])

    def chain(self):
        """a generator over the stages of F.STAGES, in order: (stage, {name: array})"""
        for stage in F.STAGES:
            yield stage, getattr(self, stage)()

    def buffers_intact(self):
        for whole, at, src, _ in self.relaid:
            w, n = self.host(whole), int(src.numel())
            if not ((w[:at] == ord("#")).all() and (w[at + n:] == ord("#")).all() and _same(w[at:at + n], self.host(src))):
                return False
        return all(_same(self.host(d), h) for d, h in zip(self.d_texts + self.d_lib_texts, self.host_texts + self.host_lib_texts)) and \
            all(_same(self.host(d), b) for i, (ds, _) in self._handed.items() for d, b in zip(ds, self.hands[i]["bufs"])) and \
            all(_same(self.host(d), b) for i, (ds, _) in self._lib_handed.items() for d, b in zip(ds, self.lib_hands[i]["bufs"]))


def _want(H, stage):
    return {name: H[name] for name in F.STAGES[stage]}


_CASES = {}


def _case(seed):
    """(plan, case, reference chain) of a seed, computed once for all the tests that need it (none of them writes into it)"""
    if seed not in _CASES:
        p = F.plan(seed)
        case = F.case_of(p)
        _CASES[seed] = (p, case, F.host_pipeline(p, case))
    return _CASES[seed]


def _relations(run, p, case, H, first, seed):
    from kmers_amd._lib import RP_INSERT

    ctx, n = run.ctx, p.n_pairs
    # ---- mates swapped
    (b1, b2, _, L1, L2), (q1, q2), (o1, o2) = run.pair_args()
    sw = (b2, b1, n, L2, L1), (q2, q1), (o2, o1)
    ov = ctx.reads_pair_overlap(*sw[0], *sw[2], **run.overlap_args)
    _assert_same({"rows": run.host(ov)}, {"rows": F.swapped_overlap_expect(first["overlap"]["ov_rows"])}, (seed, "overlap of swapped mates"))
    mg, pq = first["merge"], first["pair_quality"]
    expect = F.swapped_merge_expect((mg["mg_bases"], mg["mg_quals"], mg["mg_offsets"], mg["mg_rows"]),
                                    F.pairs_over_acgtn(pq["pq1_bases"], pq["pq1_offsets"], pq["pq2_bases"], pq["pq2_offsets"]))
    b, q, rows = run.merge_call(*sw, run.ov[:, RP_INSERT])
    checked = F.check_swapped_merge(expect, (run.host(b.bases), run.host(q.bases), run.host(b.offsets), run.host(rows)))
    assert 2 * checked >= int((mg["mg_rows"][:, 0] != 0).sum()), (seed, "swapped merge checked on too few pairs", checked)
    # ---- pairs permuted
    perm = F.permutation(p)
    (c1, cq1, co1), (c2, cq2, co2) = F.permuted(H, perm)
    dev = ctx.to_device
    pm = (dev(c1), dev(c2), n, _lens_max(co1), _lens_max(co2)), (dev(cq1), dev(cq2)), (dev(co1), dev(co2))
    ov = ctx.reads_pair_overlap(*pm[0], *pm[2], **run.overlap_args)
    _assert_same({"rows": run.host(ov)}, {"rows": first["overlap"]["ov_rows"][perm]}, (seed, "overlap of permuted pairs"))
    b, q, rows = run.merge_call(*pm, ov[:, RP_INSERT])
    mb, mq, _, mL, moff, _ = run.mg
    d_perm = dev(perm.astype(np.int64))
    gb, gq = ctx.reads_gather(mb, n, mL, d_perm, offsets=moff), ctx.reads_gather(mq, n, mL, d_perm, offsets=moff)
    _assert_same({"rows": run.host(rows), "bases": run.host(b.bases), "quals": run.host(q.bases), "offsets": run.host(b.offsets)},
                 {"rows": mg["mg_rows"][perm], "bases": run.host(gb.bases), "quals": run.host(gq.bases), "offsets": run.host(gb.offsets)},
                 (seed, "merge of permuted pairs"))
    # ---- the merged error-free pairs count as their fragments
    (f1, fo1), (f2, fo2), frags = F.clean_pairs(case)
    if frags:
        nf = len(frags)
        got = ctx.reads_merge_pairs(dev(f1), dev(f2), nf, _lens_max(fo1), _lens_max(fo2),
                                    offsets1=dev(fo1), offsets2=dev(fo2))
        fb, fo = F.ragged(frags)
        assert got.merged.n_reads == nf and got.unmerged1.n_reads == 0 and got.merged_quals is None
        _assert_same({"bases": run.host(got.merged.bases), "offsets": run.host(got.merged.offsets)}, {"bases": fb, "offsets": fo},
                     (seed, "error-free pairs merge into their fragments"))
        fn = ctx.count_canonical2 if p.count_k > 32 else ctx.count_canonical
        kmers, counts = fn(got.merged.bases, nf, got.merged.max_len(), p.count_k, offsets=got.merged.offsets)
        w_kmers, w_counts = fn(dev(fb), nf, _lens_max(fo), p.count_k, offsets=dev(fo))
        _assert_same({"k": run.host(kmers), "c": run.host(counts)}, {"k": run.host(w_kmers), "c": run.host(w_counts)}, (seed, "the fragments' table"))


def _dedup_host(run, d):
    return run.host(d.rows), run.host(d.keep), np.array([d.kept, d.dropped, d.largest, d.collisions], np.uint64)


def _library_relations(run, p, H, first, seed):
    """the relations of the second library's calls, on the device: reads_fuzz_np states them, tests/test_reads_fuzz_plan.py holds the
    references to them first"""
    from tests import dedup_np as D
    from tests import fastx_out_np as FO

    ctx, lib, dev = run.ctx, run.lib, run.ctx.to_device
    n = lib.n
    pd, sd, px = first["dedup_pairs"], first["dedup_single"], first["poly"]
    # ---- conservation, of both stages
    F.check_dedup_conserved(pd["dd_rows"], pd["dd_keep"], pd["dd_summary"])
    F.check_dedup_conserved(sd["ds_rows"], sd["ds_keep"], sd["ds_summary"])
    if p.dd_score == "none" and p.dd_hash_bits == 64:         # no score, no collisions to speak of: a dictionary of canonical strings is the answer
        assert _same(pd["dd_keep"], D.dict_dedup(lib.reads[0], lib.reads[1], p.dd_strand)), (seed, "dict_dedup of the pairs")
        assert _same(sd["ds_keep"], D.dict_dedup(F.split(pd["dp1_bases"], pd["dp1_offsets"]), None, p.dd_strand)), (seed, "dict_dedup of mate 1")
    # ---- idempotence: the survivors of either stage hold no duplicate
    (b1, _, k, L1, o1), (b2, _, _, L2, o2) = run.dp, run.dp2
    again = ctx.reads_dedup(b1, k, L1, offsets=o1, mates=(b2, L2, o2), score=run.single_score(), **run.dedup_args)
    assert (again.dropped, again.largest) == (0, 1), (seed, "dedup of the surviving pairs", again.dropped, again.largest)
    b, _, k, L, o = run.ds
    with run.on_stream():
        score = None if run.score is None else run.single_score()[dev(sd["ds_index"].astype(np.int64))]
    again = ctx.reads_dedup(b, k, L, offsets=o, score=score, **run.dedup_args)
    assert (again.dropped, again.largest) == (0, 1), (seed, "dedup of the surviving reads", again.dropped, again.largest)
    # ---- items permuted, under a score that is unique per item
    (rb1, _, _, rL1, ro1), (rb2, _, _, rL2, ro2) = run.lh[1], run.lh[2]
    perm = F.dedup_permutation(n, seed)
    base = ctx.reads_dedup(rb1, n, rL1, offsets=ro1, mates=(rb2, rL2, ro2), score=dev(np.arange(n, dtype=np.int64)), **run.dedup_args)
    (pb1, po1), (pb2, po2) = (F.ragged([lib.reads[m][i] for i in perm]) for m in range(2))
    got = ctx.reads_dedup(dev(pb1), n, _lens_max(po1), offsets=dev(po1), mates=(dev(pb2), _lens_max(po2), dev(po2)), score=dev(perm.astype(np.int64)),
                          **run.dedup_args)
    F.check_dedup_permuted(_dedup_host(run, base)[:2], _dedup_host(run, got)[:2], perm)
    # ---- every pair's mates exchanged, the strand flag on
    base = ctx.reads_dedup(rb1, n, rL1, offsets=ro1, mates=(rb2, rL2, ro2), strand=True, hash_bits=p.dd_hash_bits)
    got = ctx.reads_dedup(rb2, n, rL2, offsets=ro2, mates=(rb1, rL1, ro1), strand=True, hash_bits=p.dd_hash_bits)
    want = D.dedup(lib.reads[1], lib.reads[0], True, None, p.dd_hash_bits)[0]
    F.check_dedup_exchanged(_dedup_host(run, base)[:2], _dedup_host(run, got)[:2], want[:, D.FLAGS])
    # ---- every read of mate 1 reverse-complemented, the strand flag on
    base = ctx.reads_dedup(rb1, n, rL1, offsets=ro1, strand=True, hash_bits=p.dd_hash_bits)
    mb, mo = F.mirror_batch(H["r1_bases"], H["r1_offsets"])
    got = ctx.reads_dedup(dev(mb), n, _lens_max(mo), offsets=dev(mo), strand=True, hash_bits=p.dd_hash_bits)
    assert _same(run.host(got.keep), run.host(base.keep)), (seed, "dedup of the reverse-complemented reads")
    # ---- the complexity rows of the mirrored batch
    mb, mo = F.mirror_batch(sd["ds_bases"], sd["ds_offsets"])
    _, rows = ctx.reads_complexity(dev(mb), len(mo) - 1, _lens_max(mo), dust_max=p.dust_max, offsets=dev(mo), mask=False, **F.mirror_args(p))
    F.check_complexity_mirror(px["cx_rows"], run.host(rows))
    # ---- the record offsets are the cumulative record lengths
    fm, lens = first["format"], {"xf_offsets": px["xf_offsets"], "xfn_offsets": px["xfn_offsets"]}
    assert _same(fm["fq_rec"], F.record_offsets(p, lens, FO.FASTQ)) and _same(fm["fa_rec"], F.record_offsets(p, lens, FO.FASTA, p.fa_width)), (seed, "rec_offsets")
    if p.name_skip == 1:                                   # the round trip through the image is the identity
        rp = first["reparse"]
        _assert_same({"bases": rp["rp_bases"], "quals": rp["rp_quals"], "offsets": rp["rp_offsets"], "names": rp["rp_names"], "noffsets": rp["rp_noffsets"]},
                     {"bases": px["xf_bases"], "quals": px["xf_quals"], "offsets": px["xf_offsets"], "names": px["xfn_bases"], "noffsets": px["xfn_offsets"]},
                     (seed, "the round trip through the FASTQ image"))


@pytest.mark.parametrize("seed", range(N_FUZZ))
def test_reads_pipeline(seed):
    p = F.plan(seed)
    case = F.case_of(p)
    H = F.host_pipeline(p, case)
    ctx = _context(p)
    try:
        run = Run(ctx, p, case)
        # 1. the chain against the reference, on a context that has done nothing yet
        first = {}
        for stage, got in run.chain():
            _assert_same(got, _want(H, stage), (seed, stage))
            first[stage] = got
        info = ctx.work_buffer_info()
        # 2. the warm repeat: the same bytes, and a work buffer that no longer grows
        for stage, got in run.chain():
            _assert_same(got, first[stage], (seed, "warm", stage))
        assert ctx.work_buffer_info() == info, (seed, "the warm pass allocated", info, ctx.work_buffer_info())
        # 3. every reads-form call on the raw mates, for every layout of the plan: the first against the reference, the others against it
        route0 = run.routes(0)
        _assert_same(route0, {name: H[name] for name in ("ad_rows",) + F.ROUTES}, (seed, "route", run.hands[0]["layout"].name))
        for i in range(1, len(run.hands)):
            _assert_same(run.routes(i), route0, (seed, "route", run.hands[i]["layout"].name))
        route0 = run.routes2(0)
        _assert_same(route0, {name: H[name] for name in F.ROUTES2}, (seed, "route of the second library", run.lib_hands[0]["name"]))
        for i in range(1, len(run.lib_hands)):
            _assert_same(run.routes2(i), route0, (seed, "route of the second library", run.lib_hands[i]["name"]))
        # 4. the relations
        _relations(run, p, case, H, first, seed)
        _library_relations(run, p, H, first, seed)
        assert run.buffers_intact(), (seed, "a call wrote into its inputs or their guard bytes")
    finally:
        ctx.close()


FRESH_STAGES = list(F.STAGES) + ["parse_quals", "names_not_same_text"]


# seed 5: a side stream, mates of one length; seed 6: torch's default stream, a mix of lengths with mates of 1 024 bases and more
@pytest.mark.parametrize("stage", FRESH_STAGES)
@pytest.mark.parametrize("seed", (5, 6))
def test_first_call_on_a_fresh_context(seed, stage):
    """every stage as the FIRST call a context ever serves: its inputs are the reference's arrays, uploaded (copies, no kernel), so the
    stage meets a work buffer that holds nothing -- the merge plan, the select plan and the parse summaries have to make it themselves"""
    p, case, H = _case(seed)
    assert p.stream == ("side" if seed % 2 else "default") and (p.length_mode, p.has_long) == (("one", False) if seed == 5 else ("mix", True))
    ctx = _context(p)
    try:
        assert ctx.work_buffer_info()[1] == 0, "a context that has served no call holds no work buffer"
        run = Run(ctx, p, case)
        run.preload(H)
        assert ctx.work_buffer_info()[1] == 0, "the uploads went through the work buffer"
        if stage == "parse_quals":
            for m in (1, 2) if seed == 5 else (2, 1):
                quals, qoff = ctx.fastx_quals(run.texts[m - 1], None, same_text=False)
                _assert_same({"quals": run.host(quals), "offsets": run.host(qoff)}, {"quals": H[f"p{m}_quals"], "offsets": H[f"p{m}_offsets"]},
                             (seed, "fresh", stage, m))
        elif stage == "names_not_same_text":
            for m in (1, 2) if seed == 5 else (2, 1):
                names, noff = ctx.fastx_names(run.lib_texts[m - 1], same_text=False)
                _assert_same({"names": run.host(names), "offsets": run.host(noff)}, {"names": H[f"r{m}_names"], "offsets": H[f"r{m}_noffsets"]},
                             (seed, "fresh", stage, m))
        else:
            _assert_same(getattr(run, stage)(), _want(H, stage), (seed, "fresh", stage))
        assert run.buffers_intact()
    finally:
        ctx.close()


def test_two_contexts_interleaved():
    """two contexts on one device from one host thread, one on a side stream and one on torch's default stream: stage i of pipeline A
    alternates with stage i of pipeline B, on different plans -- the SAME_TEXT state, the pinned read-back and the work buffer of the
    one must not leak into the other; both end equal to their references"""
    import torch

    from kmers_amd.api import Context

    (pa, casea, Ha), (pb, caseb, Hb) = _case(5), _case(6)
    ca, cb = Context(stream=torch.cuda.Stream()), Context()
    try:
        a, b = Run(ca, pa, casea), Run(cb, pb, caseb)
        done = 0
        for (sa, ga), (sb, gb) in zip(a.chain(), b.chain()):
            assert sa == sb
            _assert_same(ga, _want(Ha, sa), ("A", sa))
            _assert_same(gb, _want(Hb, sb), ("B", sb))
            done += 1
        assert done == len(F.STAGES) and a.buffers_intact() and b.buffers_intact()
    finally:
        ca.close()
        cb.close()


@pytest.mark.parametrize("seed", (5, 6))
def test_two_images_on_one_context(seed):
    """fastq_records of mate 1, of mate 2, of mate 1 again on one context: the SAME_TEXT shortcut (taken twice per call now: by the quality
    bytes and by the names) is only ever applied to the image that was just summarised"""
    from tests import fastx_out_np as FO

    p, case, H = _case(seed)
    ctx = _context(p)
    try:
        run = Run(ctx, p, case)
        for m in (1, 2, 1):
            bases, quals, n, L, offsets, names, noff = ctx.fastq_records(run.texts[m - 1])
            w_names, w_noff = FO.fastq_names(case.texts[m - 1])
            want = {"bases": H[f"p{m}_bases"], "quals": H[f"p{m}_quals"], "layout": H[f"p{m}_layout"], "names": w_names, "noffsets": w_noff}
            got = {"bases": run.host(bases), "quals": run.host(quals), "layout": np.array([n, L, offsets is None], np.uint64),
                   "names": run.host(names), "noffsets": run.host(noff)}
            if offsets is not None:
                got["offsets"], want["offsets"] = run.host(offsets), H[f"p{m}_offsets"]
            _assert_same(got, want, (seed, "image", m))
        assert run.buffers_intact()
    finally:
        ctx.close()
