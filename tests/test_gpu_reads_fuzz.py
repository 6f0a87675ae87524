"""Seeded differential fuzz of the read-preparation calls on the GPU (tests/reads_fuzz_np.py decides every case and runs the references;
tests/test_reads_fuzz_plan.py checks the seed set's coverage and non-vacuity on the CPU).

Per seed, on a FRESH Context (on a torch.cuda.Stream() of its own for odd seeds, torch's default stream for even ones):

1. the chain -- parse of both FASTQ images, adapters off mate 1, quality mask / rows / filter, the count table of what is left, both
   mates trimmed by quality in step, the mates' overlap and its trim, the merge (with rows, without, without quality bytes), merged
   and unmerged apart, the merged reads by length class -- every stage fed by the previous stage's device output, every array compared
   for u64 or byte equality with the reference chain; the outputs the test allocates itself sit between guard words;
2. the warm repeat: the chain once more on the same context, byte-identical, with no further allocation of the work buffer;
3. route equivalence: every reads-form call (adapter, quality, pair overlap, pair merge, select with a span, gather) on the raw parsed
   mates, from host-built hand-overs of every layout of the plan, equal to the reference on the first and byte-identical on the others;
4. relations: mates swapped (overlap and merge), pairs permuted, and the merged error-free pairs of the seed count as their fragments.

Everything is integer work: no tolerance anywhere.  Results are read the way a user on torch's default stream reads them
(Stream.wait_stream, then .cpu(); no host synchronisation is added).  KMX_READS_FUZZ_N widens the seed set for a one-off sweep.

Three more tests: every stage (and fastx_quals without SAME_TEXT) as the first call a context ever serves, for seeds 5 (side stream,
mates of one length) and 6 (default stream, a mix with mates of 1 024 bases and more); two contexts interleaved stage by stage; and
fastq_reads of mate 1, mate 2, mate 1 on one context.

Measured on one MI355X in one session: this file 8.6 s for its 71 cases (tests/test_gpu_count_fuzz.py next to it: 19.4 s for 83), so
the 48 seeds and the 24 000 bases per mate file stay as they are.  The slowest seed is 0 with 2.2 s, which carries the library
start-up; the next one takes 0.24 s, most 0.15 s.  Coverage of the 48 default seeds (96 .. 208 pairs each): layouts ragged0 48,
ragged_bound 48, misaligned 48, uniform 14 -- as the chain's first layout 16, 14, 15 and 3; streams 24 side and 24 default (7 + 7 in
length mode "one", 17 + 17 in "mix"); long mates in 12 seeds, 6 on either stream; adapter-set sizes 1: 4 seeds, 2 to 5: 9 each,
8: 8 seeds; phred base 33 in 30 seeds and 64 in 18; trim "mott", "run" and None in 16 each.  A one-off sweep of 480 seeds passed."""
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
        self.h, self.relaid = {}, []
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
                        self.relaid.append((whole, G + lead, src))
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

    def chain(self):
        """a generator over the stages of F.STAGES, in order: (stage, {name: array})"""
        for stage in F.STAGES:
            yield stage, getattr(self, stage)()

    def buffers_intact(self):
        for whole, at, src in getattr(self, "relaid", ()):
            w, n = self.host(whole), int(src.numel())
            if not ((w[:at] == ord("#")).all() and (w[at + n:] == ord("#")).all() and _same(w[at:at + n], self.host(src))):
                return False
        return all(_same(self.host(d), h) for d, h in zip(self.d_texts, self.host_texts)) and \
            all(_same(self.host(d), b) for i, (ds, _) in self._handed.items() for d, b in zip(ds, self.hands[i]["bufs"]))


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
        # 4. the relations
        _relations(run, p, case, H, first, seed)
        assert run.buffers_intact(), (seed, "a call wrote into its inputs or their guard bytes")
    finally:
        ctx.close()


FRESH_STAGES = list(F.STAGES) + ["parse_quals"]


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
    """fastq_reads of mate 1, of mate 2, of mate 1 again on one context: the SAME_TEXT shortcut is only ever applied to the image that was
    just summarised"""
    p, case, H = _case(seed)
    ctx = _context(p)
    try:
        run = Run(ctx, p, case)
        for m in (1, 2, 1):
            bases, quals, n, L, offsets = ctx.fastq_reads(run.texts[m - 1])
            want = {"bases": H[f"p{m}_bases"], "quals": H[f"p{m}_quals"], "layout": H[f"p{m}_layout"]}
            got = {"bases": run.host(bases), "quals": run.host(quals), "layout": np.array([n, L, offsets is None], np.uint64)}
            if offsets is not None:
                got["offsets"], want["offsets"] = run.host(offsets), H[f"p{m}_offsets"]
            _assert_same(got, want, (seed, "image", m))
        assert run.buffers_intact()
    finally:
        ctx.close()
