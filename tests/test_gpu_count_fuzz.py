"""Seeded differential fuzz of the whole count-table pipeline on the GPU (tests/count_fuzz_np.py decides every case and runs the
references; tests/test_count_fuzz_plan.py checks the seed set's coverage and non-vacuity on the CPU).

Per seed, on a FRESH Context (on a torch.cuda.Stream() of its own for odd seeds, torch's default stream for even ones):

1. the chain -- table, lookup, read stats, set algebra, adjacency, unitigs, index, links, clean, components, read paths, link support,
   prune, correction, colours, select / gather -- every stage fed by the previous stage's device output, every array compared for u64
   or byte equality with the reference chain; the outputs the test allocates itself sit between guard words;
2. the warm repeat: the chain once more on the same context, byte-identical, with no further allocation of the work buffer;
3. route equivalence: every reads-form call again for every other layout the plan lists, byte-identical to the first layout's;
4. order and strand: the table of the reverse-complemented reads, of permuted reads and the merge of two halves equal the table; link
   support over permuted reads is the same vector, their paths are the paths permuted.

Everything is integer work: no tolerance anywhere.  Results are read the way a user on torch's default stream reads them: the default
stream is told to wait for the context's stream (Stream.wait_stream, the ordering the "Stream discipline" of kmers_amd/api.py asks
of a caller; no host synchronisation), then the tensors and the result classes' properties are evaluated there.

KMX_COUNT_FUZZ_N widens the seed set for a one-off sweep."""
import os

import numpy as np
import pytest

from tests import component_np, link_support_np
from tests import count_fuzz_np as F

pytestmark = pytest.mark.gpu

N_FUZZ = int(os.environ.get("KMX_COUNT_FUZZ_N", F.N_DEFAULT))
POISON = -0x5A5A5A5A5A5A5A5B
GUARD = 16          # elements on either side of an output the test allocates (16 int64 = 128 bytes: the interior stays 16-byte aligned)
READS_FORM = ("table", "lookup_reads", "read_stats", "correct", "read_colors", "read_paths", "select", "prune_links")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool((a == b).all())


def _assert_same(got, want, what):
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    for name in want:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not (g == w).all():
            bad = np.argwhere(g != w)
            raise AssertionError((what, name, f"{len(bad)} of {g.size} differ, first at {bad[0].tolist()}", g[tuple(bad[0])], w[tuple(bad[0])]))


class Handed:
    """the reads on the device as one layout hands them over: the buffer with its guard bytes, the (perhaps misaligned) view of the
    reads in it, and the arguments of a reads-form call"""

    def __init__(self, ctx, layout, buf, lead, nbytes, offsets, n_reads):
        self.layout, self.host_buf, self.n = layout, buf, n_reads
        self.d_buf = ctx.to_device(buf)
        self.bases = self.d_buf[F.GUARD_BYTES + lead:F.GUARD_BYTES + lead + nbytes]
        assert self.bases.data_ptr() % 16 == lead % 16
        self.offsets = None if offsets is None else ctx.to_device(offsets)
        self.args = (self.bases, n_reads, layout.bound)


class Run:
    """one plan on one context: the stages of the chain as methods that return {name: host array}, the device objects kept between
    them"""

    def __init__(self, ctx, p, reads):
        import torch

        self.torch, self.ctx, self.p, self.k, self.reads, self.n = torch, ctx, p, p.k, reads, len(reads)
        self.hands = F.handovers(p, reads)
        self._handed = {}
        self.nbytes = sum(len(r) for r in reads)
        self.n_windows = sum(max(len(r) - p.k + 1, 0) for r in reads)

    # ---- plumbing
    def fn(self, name):
        return getattr(self.ctx, name + "2" if self.p.two else name)

    def handed(self, i):
        if i not in self._handed:
            self._handed[i] = Handed(self.ctx, *self.hands[i], self.n)
        return self._handed[i]

    def host(self, t):
        """a device tensor -- or what a callable computes with torch, a property of a result class for instance -- as a user on the
        default stream reads it: behind the context's stream; int64 words as u64"""
        cur = self.torch.cuda.current_stream(self.ctx.device)
        cur.wait_stream(self.ctx.stream)
        if callable(t):
            t = t()
        a = t.cpu().numpy()
        return a.view(np.uint64) if a.dtype == np.int64 else a

    def guarded(self, n, dtype):
        """-> (whole buffer, the n elements between its guards), poisoned throughout"""
        fill = POISON if dtype == np.int64 else 0xA5
        whole = self.ctx.to_device(np.full(n + 2 * GUARD, fill, dtype))
        return whole, whole[GUARD:GUARD + n]

    def intact(self, whole, n):
        self.torch.cuda.current_stream(self.ctx.device).wait_stream(self.ctx.stream)
        a = whole.cpu().numpy()
        fill = POISON if a.dtype == np.int64 else 0xA5
        return bool((a[:GUARD] == fill).all() and (a[GUARD + n:] == fill).all())

    def upload(self, reads):
        bases, offsets = F.ragged(reads)
        return self.ctx.to_device(bases if len(bases) else np.zeros(16, np.uint8)), len(reads), self.ctx.to_device(offsets)

    def table_of(self, reads):
        d, n, off = self.upload(reads)
        return self.fn("count_canonical")(d, n, 0, self.k, offsets=off)

    # ---- the stages; those that take reads take the layout's index
    def table(self, i=0):
        h = self.handed(i)
        d_k, d_c = self.fn("count_canonical")(*h.args, self.k, offsets=h.offsets)
        if i == 0:
            self.d_k, self.d_c, self.n_entries = d_k, d_c, int(d_c.numel())
        return {"table_k": self.host(d_k), "table_c": self.host(d_c)}

    def lookup_reads(self, i=0):
        h = self.handed(i)
        whole, out = self.guarded(self.n_windows, np.int64)
        got = self.fn("count_lookup_reads")(*h.args, self.k, self.d_k, self.d_c, offsets=h.offsets, out=out)
        assert got is out and self.intact(whole, self.n_windows), "lookup_reads wrote outside its output"
        return {"lookup": self.host(out)}

    def read_stats(self, i=0):
        h = self.handed(i)
        whole, out = self.guarded(8 * self.n, np.int64)
        got = self.fn("count_read_stats")(*h.args, self.k, self.d_k, self.d_c, solid_min=F.SOLID_MIN, offsets=h.offsets, out=out)
        assert self.intact(whole, 8 * self.n), "read_stats wrote outside its output"
        if i == 0:
            self.d_stats = got
        return {"stats": self.host(got)}

    def setop(self):
        from kmers_amd._lib import RULE_MIN

        a, b = F.halves(self.reads)
        (ka, ca), (kb, cb) = self.table_of(a), self.table_of(b)
        out = {}
        for name, (dk, dc) in (("merge", self.fn("count_merge")(ka, ca, kb, cb)), ("inter", self.fn("count_intersect")(ka, ca, kb, cb, RULE_MIN)),
                               ("sub", self.fn("count_subtract")(ka, ca, kb)), ("sym", self.fn("count_symdiff")(ka, ca, kb, cb)),
                               ("csub", self.fn("count_counter_subtract")(ka, ca, kb, cb))):
            out[name + "_k"], out[name + "_c"] = self.host(dk), self.host(dc)
        cmp = self.fn("count_compare")(ka, ca, kb, cb)
        out["compare"] = np.array([getattr(cmp, f) for f in F.COMPARE_FIELDS], np.uint64)
        return out

    def adjacency(self):
        self.adj = self.fn("count_adjacency")(self.d_k, self.d_c, self.k, 1, flips=True, neighbors=True)
        return {"edges": self.host(self.adj[0]), "flips": self.host(self.adj[1]), "nbr": self.host(self.adj[2])}

    def unitigs(self):
        self.un = un = self.fn("count_unitigs")(self.d_k, self.d_c, self.k, 1, adjacency=self.adj)
        out = {"u_nodes": self.host(un.nodes), "u_offsets": self.host(un.offsets), "u_circular": self.host(un.circular), "u_sums": self.host(un.count_sums)}
        assert un.n_unitigs == len(out["u_offsets"]) - 1 and un.n_nodes == len(out["u_nodes"])
        lengths = np.diff(out["u_offsets"].astype(np.int64))
        assert _same(self.host(lambda: un.lengths), lengths.astype(np.uint64)), "Unitigs.lengths"
        assert _same(self.host(lambda: un.mean_counts), out["u_sums"].astype(np.float64) / lengths.astype(np.float64)), "Unitigs.mean_counts"
        return out

    def index(self):
        self.place = self.ctx.count_unitig_index(self.un, self.n_entries)
        return {"place": self.host(self.place)}

    def links(self):
        self.lk = lk = self.ctx.count_unitig_links(self.un, self.adj, self.n_entries, place=self.place)
        out = {"l_offsets": self.host(lk.offsets), "l_targets": self.host(lk.targets)}
        deg = np.diff(out["l_offsets"].astype(np.int64))
        assert lk.n_links == len(out["l_targets"])
        assert _same(self.host(lambda: lk.degrees), deg.reshape(-1, 2).astype(np.uint64)), "UnitigLinks.degrees"
        assert _same(self.host(lambda: lk.sources()), np.repeat(np.arange(len(deg)), deg).astype(np.uint64)), "UnitigLinks.sources"
        return out

    def clean(self):
        self.keep, reason = self.ctx.count_unitig_clean(self.un, self.lk)
        ck, cc = self.fn("count_unitig_select")(self.d_k, self.d_c, self.un, self.keep, place=self.place)
        return {"keep": self.host(self.keep), "reason": self.host(reason), "clean_k": self.host(ck), "clean_c": self.host(cc)}

    def components(self):
        self.comp = comp = self.ctx.count_unitig_components(self.un, self.lk, mask=self.keep)
        out = {"c_labels": self.host(comp.labels), "c_ids": self.host(comp.ids), "c_records": self.host(comp.records),
               "c_n": np.array([comp.n_components], np.uint64)}
        rec = out["c_records"]
        for col, prop in enumerate(("roots", "n_unitigs", "n_nodes", "count_sums")):
            assert _same(self.host(lambda: getattr(comp, prop)), rec[:, col]), ("UnitigComponents", prop)
        assert _same(self.host(lambda: comp.keep(min_nodes=self.k, largest=3)), component_np.keep_np(out["c_ids"], rec, min_nodes=self.k, largest=3)), \
            "UnitigComponents.keep"
        return out

    def read_paths(self, i=0):
        h = self.handed(i)
        paths = self.fn("count_read_paths")(*h.args, self.k, self.d_k, self.un, place=self.place, offsets=h.offsets)
        out = {"p_offsets": self.host(paths.offsets), "p_segments": self.host(paths.segments)}
        if i == 0:
            self.paths = paths
            seg = out["p_segments"]
            assert paths.n_segments == len(seg)
            want = {"read": seg[:, 0], "start": seg[:, 1] & np.uint64(0xFFFFFFFF), "length": seg[:, 1] >> np.uint64(32), "unitig": seg[:, 2],
                    "pos": seg[:, 3] >> np.uint64(1)}
            for name, w in want.items():
                assert _same(self.host(lambda: getattr(paths, name)), w), ("ReadPaths", name)
            assert _same(self.host(lambda: paths.reverse), (seg[:, 3] & np.uint64(1)) != 0), "ReadPaths.reverse"
            U = self.un.n_unitigs
            cov = np.zeros(U, np.int64)
            np.add.at(cov, seg[:, 2].astype(np.int64), want["length"].astype(np.int64))
            assert _same(self.host(lambda: paths.unitig_coverage(U)), cov.astype(np.uint64)), "ReadPaths.unitig_coverage"
            ids = self.host(self.comp.ids).astype(np.int64)[seg[:, 2].astype(np.int64)]
            rcomp = np.full(self.n, np.iinfo(np.int64).max)
            np.minimum.at(rcomp, seg[:, 0].astype(np.int64), np.where(ids >= 0, ids, np.iinfo(np.int64).max))
            rcomp[rcomp == np.iinfo(np.int64).max] = -1
            assert _same(self.host(lambda: paths.read_components(self.comp, self.n)), rcomp.astype(np.uint64)), "ReadPaths.read_components"
        return out

    def link_support(self, paths=None):
        sup = self.ctx.count_link_support(self.paths if paths is None else paths, self.un, self.lk)
        out = {"s_support": self.host(sup.support), "s_summary": self.host(sup.summary)}
        assert (sup.junctions, sup.crossed, sup.unlinked) == tuple(int(x) for x in out["s_summary"])
        assert _same(self.host(lambda: sup.unsupported(1)), link_support_np.unsupported_np(out["s_support"], 1)), "LinkSupport.unsupported"
        return out

    def prune_links(self, i=0):
        h = self.handed(i)
        adj, un, lk, sup, n_cut = self.fn("count_prune_links")(*h.args, self.k, self.d_k, self.d_c, min_support=1, min_count=1, offsets=h.offsets)
        return {"cut_edges": self.host(adj[0]), "n_cut": np.array([n_cut], np.uint64), "pr_nodes": self.host(un.nodes), "pr_offsets": self.host(un.offsets),
                "pr_circular": self.host(un.circular), "pr_sums": self.host(un.count_sums), "pr_l_offsets": self.host(lk.offsets),
                "pr_l_targets": self.host(lk.targets), "pr_support": self.host(sup.support)}

    def correct(self, i=0):
        h = self.handed(i)
        whole, out = self.guarded(self.nbytes, np.uint8)
        got, fixes = self.fn("count_correct_reads")(*h.args, self.k, self.d_k, self.d_c, solid_min=F.SOLID_MIN, min_cover=1, offsets=h.offsets, out=out)
        assert got is out and self.intact(whole, self.nbytes), "correct_reads wrote outside its output"
        return {"corrected": self.host(out), "fixes": self.host(fixes)}

    def colors(self):
        tables = [self.table_of(self.reads[c::F.N_COLORS]) for c in range(F.N_COLORS)]
        self.ct = ct = self.fn("count_color_build")(tables, k=self.k)
        cm = self.ctx.count_color_matrix(ct.colors, F.N_COLORS)
        assert ct.n_colors == F.N_COLORS
        out = {"color_k": self.host(ct.kmers), "color_m": self.host(ct.colors), "cm_shared": self.host(cm.shared), "cm_spectrum": self.host(cm.spectrum)}
        assert _same(self.host(lambda: cm.sizes), np.diagonal(out["cm_shared"])), "ColorMatrix.sizes"
        out.update(self.read_colors(0))
        return out

    def read_colors(self, i=0):
        h = self.handed(i)
        whole, out = self.guarded(8 * self.n, np.int64)
        rows, hits = self.fn("count_read_colors")(*h.args, self.k, self.ct.kmers, self.ct.colors, F.N_COLORS, offsets=h.offsets, hits=True, out=out)
        assert self.intact(whole, 8 * self.n), "read_colors wrote outside its output"
        return {"rc_rows": self.host(rows), "rc_hits": self.host(hits)}

    def select(self, i=0):
        from kmers_amd._lib import RS_SPAN

        h = self.handed(i)
        batch, stats = self.fn("count_select_reads")(*h.args, self.k, self.d_k, self.d_c, solid_min=F.SOLID_MIN, min_median=F.MIN_MEDIAN, offsets=h.offsets)
        out = {"sel_bases": self.host(batch.bases), "sel_offsets": self.host(batch.offsets), "sel_index": self.host(batch.index)}
        assert batch.n_reads == len(out["sel_index"]) and batch.n_bases == len(out["sel_bases"])
        assert batch.max_len() == int(np.diff(out["sel_offsets"].astype(np.int64)).max(initial=0)), "ReadBatch.max_len"
        g = self.ctx.reads_gather(*h.args, self.ctx.to_device(F.gather_index(self.p, self.n)), span=stats[:, RS_SPAN], span_k=self.k, offsets=h.offsets)
        out.update({"gat_bases": self.host(g.bases), "gat_offsets": self.host(g.offsets)})
        return out

    def preload(self, H):
        """every device object a stage reads, uploaded from the reference's arrays: copies only, no kernel -- so that the stage called
        next is the first call the context ever serves, with a work buffer that holds nothing yet"""
        from kmers_amd import api

        dev = self.ctx.to_device
        self.d_k, self.d_c, self.n_entries = dev(H["table_k"]), dev(H["table_c"]), len(H["table_c"])
        self.d_stats = dev(H["stats"])
        self.adj = (dev(H["edges"]), dev(H["flips"]), dev(H["nbr"]))
        self.un = api.Unitigs(dev(H["u_nodes"]), dev(H["u_offsets"]), dev(H["u_circular"]), dev(H["u_sums"]), len(H["u_offsets"]) - 1, self.k, self.d_k,
                              self.ctx)
        self.place = dev(H["place"])
        self.lk = api.UnitigLinks(dev(H["l_offsets"]), dev(H["l_targets"]))
        self.keep = dev(H["keep"])
        self.comp = api.UnitigComponents(dev(H["c_labels"]), dev(H["c_ids"]), dev(H["c_records"]), int(H["c_n"][0]), 0)
        self.paths = api.ReadPaths(dev(H["p_offsets"]), dev(H["p_segments"]), self.k)
        self.ct = api.ColorTable(dev(H["color_k"]), dev(H["color_m"]), F.N_COLORS, self.k)
        self.handed(0)

    # ---- the chain
    def chain(self):
        """a generator over the stages of F.STAGES, in order, on the first layout: (stage, {name: array})"""
        for stage in F.STAGES:
            yield stage, getattr(self, stage)()

    def buffers_intact(self):
        return all(_same(self.host(h.d_buf), h.host_buf) for h in self._handed.values())


def _want(H, stage, got):
    """the reference's arrays of a stage (prune_links also returns the first pass's support: link_support's)"""
    want = {name: H[name] for name in F.STAGES[stage]}
    if stage == "prune_links":
        want["pr_support"] = H["s_support"]
    return want


def _context(p):
    import torch

    from kmers_amd.api import Context

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return Context(stream=torch.cuda.Stream() if p.stream == "side" else None)


def _permuted_paths(first, perm):
    """the paths of first = (p_offsets, p_segments) with the reads in the order perm"""
    po, seg = first["p_offsets"].astype(np.int64), first["p_segments"]
    rows, offs = [], [0]
    for j, r in enumerate(perm):
        s = seg[po[r]:po[r + 1]].copy()
        s[:, 0] = j
        rows.append(s)
        offs.append(offs[-1] + len(s))
    return {"p_offsets": np.array(offs, np.uint64), "p_segments": np.concatenate(rows) if rows else seg[:0]}


@pytest.mark.parametrize("seed", range(N_FUZZ))
def test_count_pipeline(seed):
    p = F.plan(seed)
    reads = F.reads_of(p)
    H = F.host_pipeline(p, reads)
    ctx = _context(p)
    try:
        run = Run(ctx, p, reads)
        # 1. the chain against the reference, on a context that has done nothing yet
        first = {}
        for stage, got in run.chain():
            _assert_same(got, _want(H, stage, got), (seed, stage))
            first[stage] = got
        assert _same(first["setop"]["merge_k"], first["table"]["table_k"]) and _same(first["setop"]["merge_c"], first["table"]["table_c"])
        info = ctx.work_buffer_info()
        # 2. the warm repeat: the same bytes, and a work buffer that no longer grows
        for stage, got in run.chain():
            _assert_same(got, first[stage], (seed, "warm", stage))
        assert ctx.work_buffer_info() == info, (seed, "the warm pass allocated", info, ctx.work_buffer_info())
        # 3. every reads-form call again for every other layout of the plan, on the same table
        for i in range(1, len(run.hands)):
            name = run.hands[i][0].name
            for stage in READS_FORM:
                got = getattr(run, stage)(i)
                want = first["colors" if stage == "read_colors" else stage]
                _assert_same(got, {x: want[x] for x in got}, (seed, "route", name, stage))
        # 4. order and strand
        table = first["table"]
        rng = np.random.default_rng(55_000 + seed)
        perm = rng.permutation(len(reads)).tolist()
        shuffled = [reads[r] for r in perm]
        for what, batch in (("reverse complement", [F.rc_read(r) for r in reads]), ("permutation", shuffled)):
            d_k, d_c = run.table_of(batch)
            _assert_same({"table_k": run.host(d_k), "table_c": run.host(d_c)}, table, (seed, what))
        d, n, off = run.upload(shuffled)
        paths = run.fn("count_read_paths")(d, n, 0, p.k, run.d_k, run.un, place=run.place, offsets=off)
        _assert_same({"p_offsets": run.host(paths.offsets), "p_segments": run.host(paths.segments)}, _permuted_paths(first["read_paths"], perm),
                     (seed, "paths of permuted reads"))
        _assert_same(run.link_support(paths), first["link_support"], (seed, "support over permuted reads"))
        assert run.buffers_intact(), (seed, "a call wrote into the reads or their guard bytes")
    finally:
        ctx.close()


_FRESH = {}


def _fresh_case(seed):
    """(plan, reads, reference chain) of a seed, computed once for all the stages"""
    if seed not in _FRESH:
        p = F.plan(seed)
        reads = F.reads_of(p)
        _FRESH[seed] = (p, reads, F.host_pipeline(p, reads))
    return _FRESH[seed]


# both hand their reads over with a bound above 256 first, so the reads-form calls cut segments into the work buffer before they
# nest: seed 19 on a side stream with two-word keys, seed 22 on the default stream with one-word keys and a mix of lengths
@pytest.mark.parametrize("stage", [s for s in F.STAGES if s != "read_colors"] + ["read_colors"])
@pytest.mark.parametrize("seed", (19, 22))
def test_first_call_on_a_fresh_context(seed, stage):
    """every stage as the FIRST call a context ever serves: its inputs are the reference's arrays, uploaded (copies, no kernel), so the
    stage meets a work buffer that holds nothing and has to grow it itself, nested calls included -- the path a real user hits first
    and the chain above, where every stage follows the earlier ones, does not"""
    p, reads, H = _fresh_case(seed)
    assert p.layouts[0].name == "ragged_long" and p.stream == ("side" if seed % 2 else "default")
    ctx = _context(p)
    try:
        assert ctx.work_buffer_info()[1] == 0, "a context that has served no call holds no work buffer"
        run = Run(ctx, p, reads)
        run.preload(H)
        assert ctx.work_buffer_info()[1] == 0, "the uploads went through the work buffer"
        got = getattr(run, stage)()
        want = _want(H, "colors" if stage == "read_colors" else stage, got)
        _assert_same(got, {x: want[x] for x in got}, (seed, "fresh", stage))
        assert run.buffers_intact()
    finally:
        ctx.close()


def test_two_contexts_interleaved():
    """two contexts on one device from one host thread, one on a side stream and one on torch's default stream: stage i of pipeline A
    alternates with stage i of pipeline B, on different plans; both end equal to their references"""
    import torch

    from kmers_amd.api import Context

    pa, pb = F.plan(5), F.plan(8)
    assert (pa.two, pb.two) == (False, True) and pa.k != pb.k
    ra, rb = F.reads_of(pa), F.reads_of(pb)
    Ha, Hb = F.host_pipeline(pa, ra), F.host_pipeline(pb, rb)
    ca, cb = Context(stream=torch.cuda.Stream()), Context()
    try:
        a, b = Run(ca, pa, ra), Run(cb, pb, rb)
        done = 0
        for (sa, ga), (sb, gb) in zip(a.chain(), b.chain()):
            assert sa == sb
            _assert_same(ga, _want(Ha, sa, ga), ("A", sa))
            _assert_same(gb, _want(Hb, sb, gb), ("B", sb))
            done += 1
        assert done == len(F.STAGES) and a.buffers_intact() and b.buffers_intact()
    finally:
        ca.close()
        cb.close()
