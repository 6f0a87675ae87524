"""The seeded differential fuzz of the whole count-table pipeline, host side: what tests/test_gpu_count_fuzz.py runs on the device and
tests/test_count_fuzz_plan.py checks on the CPU.

* plan(seed): a pure function from the seed to the configuration of one case -- k, the pieces of the genome, the reads' lengths, the
  stream, the layouts the reads may legally be handed over as.  The ONE place where a case is decided: the CPU test enumerates from it
  what the GPU test will do.
* reads_of(plan): the reads themselves, a list of uint8 arrays, built from the plan alone (seeded by plan.seed).
* handovers(plan, reads): per layout of the plan, the host buffer, where the reads start in it, read_len and the offsets to hand over.
* host_pipeline(plan): the existing references end to end, each stage fed by the previous stage's reference output -> a dict of named
  arrays (STAGES lists which names belong to which stage).  No reference is written here: every operation's reference is imported
  from where it lives.

Where the issue's wording leaves a choice, it is made here and said here:

* Uniform layouts need reads of ONE length, so short and empty reads, and the mix of lengths, live in the seeds of length mode "mix";
  a seed of mode "one" has dirty reads (N, lower case, invalid bytes) but no short ones.  The one length is drawn from {36, 100, 150,
  250} among the values of at least 2 k bases, so every read holds a run of windows.
* "Uniform with L > 256" can only be reached by a batch whose reads are ALL of one length above 256.  In the quarter of the seeds
  with long reads, mode "mix" adds a few reads of 300 .. 1 200 bases to the mix; mode "one" makes every read of one length in
  300 .. 420 (at the low end of the range, so that 150 reads stay within the base budget below).
* The number of reads is drawn from 150 .. 600 and then cut to what MAX_BASES allows at the plan's mean length, never below 150: the
  Python references of read_paths, correct and read_colors walk every base several times.

numpy only: the oracle is loaded inside host_pipeline, torch nowhere.
"""
import dataclasses
import functools
import itertools

import numpy as np

from tests import clean_np, color_np, component_np, correct_np, graph_np, link_np, link_support_np, path_np, reads_np, unitig_np
from tests.count_np import host_lookup, orc_windows, table_of

KS1 = (5, 12, 13, 21, 22, 31)
KS2 = (33, 34, 47, 63, 64)
KS = KS1 + KS2
ONE_LENGTHS = (36, 100, 150, 250)
LAYOUTS = ("uniform", "uniform_long", "ragged0", "ragged_tight", "ragged_long", "misaligned")
N_DEFAULT = 48
MAX_BASES = 32_000
GUARD_BYTES = 64
SOLID_MIN = 2
MIN_MEDIAN = 2
N_COLORS = 3

_ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.arange(256, dtype=np.uint8)          # the complement of a byte: ACGT and acgt swap, every other byte is itself
COMP[list(b"ACGTacgt")] = list(b"TGCAtgca")

# which names of host_pipeline's dict belong to which stage (the order of the chain)
STAGES = {
    "table": ("table_k", "table_c"),
    "lookup_reads": ("lookup",),
    "read_stats": ("stats",),
    "setop": ("merge_k", "merge_c", "inter_k", "inter_c", "sub_k", "sub_c", "sym_k", "sym_c", "csub_k", "csub_c", "compare"),
    "adjacency": ("edges", "flips", "nbr"),
    "unitigs": ("u_nodes", "u_offsets", "u_circular", "u_sums"),
    "index": ("place",),
    "links": ("l_offsets", "l_targets"),
    "clean": ("keep", "reason", "clean_k", "clean_c"),
    "components": ("c_labels", "c_ids", "c_records", "c_n"),
    "read_paths": ("p_offsets", "p_segments"),
    "link_support": ("s_support", "s_summary"),
    "prune_links": ("cut_edges", "n_cut", "pr_nodes", "pr_offsets", "pr_circular", "pr_sums", "pr_l_offsets", "pr_l_targets"),
    "correct": ("corrected", "fixes"),
    "colors": ("color_k", "color_m", "cm_shared", "cm_spectrum", "rc_rows", "rc_hits"),
    "select": ("sel_bases", "sel_offsets", "sel_index", "gat_bases", "gat_offsets"),
}


def rc_read(r):
    return COMP[r[::-1]]


@dataclasses.dataclass(frozen=True)
class Layout:
    """one way to hand the reads over: `uniform` = no offsets array; bound = kmx_reads.read_len (the one length of uniform reads, the
    length bound of ragged ones, 0 = none); lead = bytes by which the base pointer is moved off its 16-byte alignment"""
    name: str
    uniform: bool
    bound: int
    lead: int = 0


@dataclasses.dataclass(frozen=True)
class Plan:
    seed: int
    k: int
    stream: str                # "side" (odd seeds) or "default"
    genome_len: int
    pieces: tuple              # (name, parameters...) of everything built into the genome or put next to it
    n_reads: int
    length_mode: str           # "one" or "mix"
    read_len: int              # mode "one": the length of every read; mode "mix": 0
    mix_max: int               # mode "mix": the longest of the mixed lengths (one read has exactly this length); mode "one": 0
    long_lens: tuple           # mode "mix": the lengths, 300 .. 1 200, of the long reads that are added
    sub_rate: float
    dirty_every: int           # one read in so many carries an N, a lower-case stretch or another invalid byte, by turns
    layouts: tuple             # of Layout; the first is the one the chain runs on

    @property
    def two(self):
        return self.k > 32

    @property
    def has_long(self):
        return bool(self.long_lens) or self.read_len > 256

    @property
    def longest(self):
        return max(self.long_lens + (self.mix_max, self.read_len))

    def layout_names(self):
        return tuple(l.name for l in self.layouts)


def _layouts(seed, mode, L, longest, rng):
    lead = int(rng.integers(1, 16))
    if mode == "one":
        if L > 256:
            out = [Layout("uniform_long", True, L), Layout("ragged0", False, 0), Layout("ragged_long", False, L)]
        else:
            out = [Layout("uniform", True, L), Layout("ragged0", False, 0), Layout("ragged_tight", False, L),
                   Layout("ragged_long", False, 257 + int(rng.integers(0, 300)))]
        # (a misaligned base in both forms, by turns)
        out.append(Layout("misaligned", seed % 4 >= 2, L if seed % 4 >= 2 else 0, lead))
    else:
        # (the tight bound is the longest read; above 256 it is a long-read bound, and named so)
        out = [Layout("ragged0", False, 0)]
        if longest > 256:
            out.append(Layout("ragged_long", False, longest))
        else:
            out += [Layout("ragged_tight", False, longest), Layout("ragged_long", False, 300 + int(rng.integers(0, 300)))]
        out.append(Layout("misaligned", False, 0 if seed % 4 >= 2 else longest, lead))
    # the chain runs on a layout that turns with the seed, the others are compared with it
    first = (seed // 3) % len(out)
    return tuple(out[first:] + out[:first])


def plan(seed):
    """seed -> Plan.  k walks KS with the seed (every value comes up again every 11 seeds); long reads come with seed % 8 in (3, 6) --
    a quarter of the seeds, of both parities, so on both streams; the rest is drawn from default_rng(seed)."""
    seed = int(seed)
    rng = np.random.default_rng(77_000 + seed)
    k = KS[seed % len(KS)]
    has_long = seed % 8 in (3, 6)
    if has_long:
        mode = "one" if ((seed // 8) % 2 == 0) == (seed % 8 == 3) else "mix"
    else:
        mode = "one" if rng.random() < 0.5 else "mix"
    if mode == "one":
        if has_long:
            L = int(rng.integers(300, 421))
        else:
            ok = [x for x in ONE_LENGTHS if x >= 2 * k]
            L = int(rng.choice(ok))
        mix_max, long_lens = 0, ()
        mean_len = L
    else:
        L = 0
        mix_max = int(rng.integers(180, 261))
        long_lens = tuple(int(x) for x in rng.integers(300, 1201, int(rng.integers(2, 6)))) if has_long else ()
        mean_len = (k + mix_max) // 2
    genome_len = int(rng.integers(1500, 6001))
    n_reads = max(150, min(int(rng.integers(150, 601)), (MAX_BASES - sum(long_lens)) // mean_len))
    # ---- the pieces: (name, position, size, ...) -- positions are spread so that pieces do not overwrite each other
    slot = itertools.cycle(rng.permutation(np.arange(200, genome_len - 400, 330)).tolist())   # (a short genome reuses slots: pieces
    #                                                                                           then overlap, which is legal)
    pieces = []
    for _ in range(int(rng.integers(1, 4))):
        pieces.append(("repeat", next(slot), next(slot), k + 3 + int(rng.integers(0, 2 * k + 20))))      # src, dst, length > k
    for _ in range(int(rng.integers(1, 4))):
        pieces.append(("variant", next(slot) + int(rng.integers(0, 200)), int(rng.integers(1, 4)), 0.3))   # position, base shift, share
    pieces.append(("hairpin", next(slot), k + 2 + int(rng.integers(0, 30))))                              # position, arm length > k
    pieces.append(("homopolymer", next(slot), k + 2 + int(rng.integers(0, 12)), int(rng.integers(0, 4))))  # position, length > k, base
    for _ in range(int(rng.integers(1, 3))):
        pieces.append(("tip", next(slot) + 150, 2 + int(rng.integers(0, max(k // 2, 2)))))                 # where it leaves the genome, tail
    pieces.append(("graft", next(slot) + 100))                                                             # where a stray contig overlaps
    pieces.append(("circle", 3 * k + 120 + int(rng.integers(0, 200))))                                     # its length
    return Plan(seed, k, "side" if seed % 2 else "default", genome_len, tuple(pieces), n_reads, mode, L, mix_max, long_lens,
                float(rng.uniform(0.005, 0.02)), 17, _layouts(seed, mode, L, max(long_lens + (mix_max, L)), rng))


# ---------------------------------------------------------------- the reads of a plan
def _contigs(p, rng):
    """-> (genome, variants, [(contig, weight, circular, min_reads)]): the genome with its pieces built in, the variants its reads may
    carry, and the contigs next to it -- the tips, the graft and the circle"""
    k = p.k
    g = rng.choice(_ACGT, p.genome_len).astype(np.uint8)
    variants = []
    side = []
    span = max(p.read_len, k + 60)            # what a side contig needs so that a read of the one length fits
    for piece in p.pieces:
        name = piece[0]
        if name == "repeat":
            _, src, dst, n = piece
            g[dst:dst + n] = g[src:src + n]
        elif name == "hairpin":
            _, at, arm = piece
            g[at + arm:at + 2 * arm] = rc_read(g[at:at + arm])
        elif name == "homopolymer":
            _, at, n, base = piece
            g[at:at + n] = _ACGT[base]
    for piece in p.pieces:                     # (after the overwrites: these read the finished genome)
        name = piece[0]
        if name == "variant":
            variants.append(piece[1:])
        elif name == "tip":
            _, at, tail = piece
            at = min(max(at, span), p.genome_len)
            side.append((np.concatenate([g[at - (span - tail):at], rng.choice(_ACGT, tail)]).astype(np.uint8), 0.0, False, 3))
        elif name == "graft":
            at = min(piece[1], p.genome_len - k)
            # a stray contig whose last k - 1 bases are the genome's at `at`: its last k-mer is a second predecessor of the genome's
            # k-mer there, and no read walks from the one into the other -- a link with support 0
            side.append((np.concatenate([rng.choice(_ACGT, span - (k - 1)), g[at:at + k - 1]]).astype(np.uint8), 0.0, False, 3))
        elif name == "circle":
            side.append((rng.choice(_ACGT, piece[1]).astype(np.uint8), piece[1] / p.genome_len, True, 4))
    return g, variants, side


def _draw(rng, contig, circular, L, to_end=False):
    """L bases of a contig (fewer if it is shorter), from a random start; a circle wraps around"""
    n = len(contig)
    if circular:
        a = int(rng.integers(0, n))
        return np.resize(np.roll(contig, -a), L) if L else np.zeros(0, np.uint8)
    L = min(L, n)
    a = n - L if to_end else int(rng.integers(0, n - L + 1))
    return contig[a:a + L].copy()


def _dirty(rng, r, i):
    """an N, a lower-case stretch or another invalid byte, by turns"""
    if len(r) == 0:
        return r
    at = int(rng.integers(0, len(r)))
    if i % 3 == 0:
        r[at] = ord("N")
    elif i % 3 == 1:
        n = int(rng.integers(1, 12))
        r[at:at + n] |= 0x20
    else:
        r[at] = (ord(">"), 0, 0xFF, ord("-"))[(i // 3) % 4]
    return r


def _reads_of(p):
    rng = np.random.default_rng(88_000 + p.seed)
    k = p.k
    g, variants, side = _contigs(p, rng)
    lengths = []
    for i in range(p.n_reads):
        if p.length_mode == "one":
            lengths.append(p.read_len)
        else:
            u = rng.random()
            lengths.append(0 if u < 0.03 else int(rng.integers(1, k)) if u < 0.10 else int(rng.integers(k, p.mix_max + 1)))
    forced = set()                             # reads whose length the plan names: they come from the genome, which holds them
    if p.length_mode == "mix":
        lengths[1] = p.mix_max
        forced.add(1)
        for j, L in enumerate(p.long_lens):
            lengths[(j * 37 + 5) % p.n_reads] = L
            forced.add((j * 37 + 5) % p.n_reads)
    # which contig a read comes from: the side contigs get their minimum first, then by weight
    source = []
    for s, (_, _, _, least) in enumerate(side):
        source += [s] * least
    weights = np.array([1.0] + [w for _, w, _, _ in side])
    weights /= weights.sum()
    source += (rng.choice(len(side) + 1, p.n_reads, p=weights) - 1).tolist()
    order = rng.permutation(p.n_reads)
    reads = [None] * p.n_reads
    n_dirty = 0
    for slot, i in enumerate(order.tolist()):
        s, L = (-1 if i in forced else source[slot]), lengths[i]
        if s < 0:
            a = int(rng.integers(0, len(g) - L + 1))
            r = g[a:a + L].copy()
            for at, shift, share in variants:            # a minority of the reads over a variant carry it
                if a <= at < a + L and rng.random() < share:
                    r[at - a] = _ACGT[(int(np.nonzero(_ACGT == r[at - a])[0][0]) + shift) % 4]
        else:
            contig, _, circular, _ = side[s]
            r = _draw(rng, contig, circular, L, to_end=slot % 2 == 0)   # (every second read of a tip or the graft runs to its end)
        r = np.array(r, np.uint8)
        flip = rng.random(len(r)) < p.sub_rate
        r[flip] = COMP[r[flip]]
        if rng.random() < 0.5:
            r = rc_read(r)
        if (i * 7 + p.seed) % p.dirty_every == 0 and len(r):
            r = _dirty(rng, r, n_dirty)
            n_dirty += 1
        if p.length_mode == "one":
            assert len(r) == p.read_len, (p.seed, len(r), p.read_len)
        reads[i] = np.ascontiguousarray(r)
    return reads


@functools.lru_cache(maxsize=4)
def _reads_cached(seed):
    return _reads_of(plan(seed))


def reads_of(p):
    return [r.copy() for r in _reads_cached(p.seed)]


def ragged(reads):
    offsets = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    return (np.concatenate(reads) if int(offsets[-1]) else np.zeros(0, np.uint8)).astype(np.uint8), offsets


def handovers(p, reads):
    """[(Layout, buffer, lead, n_bytes, offsets or None)]: the reads of a plan as each of its layouts hands them
    over -- `buffer` holds GUARD_BYTES of '#', `lead` more of them, the reads back to back, and GUARD_BYTES of '#' again; the reads'
    bytes are buffer[GUARD_BYTES + lead:][:n_bytes]"""
    bases, offsets = ragged(reads)
    longest = max((len(r) for r in reads), default=0)
    assert longest == p.longest, (p.seed, longest, p.longest)
    out = []
    for l in p.layouts:
        if l.uniform:
            assert all(len(r) == l.bound for r in reads)
        assert l.uniform or l.bound == 0 or l.bound >= longest
        buf = np.concatenate([np.full(GUARD_BYTES + l.lead, ord("#"), np.uint8), bases, np.full(GUARD_BYTES, ord("#"), np.uint8)])
        out.append((l, buf, l.lead, len(bases), None if l.uniform else offsets))
    return out


# ---------------------------------------------------------------- the reference chain
def key_ints(tk):
    lo, hi = graph_np.split(tk)
    return [int(a) | (int(b) << 64) for a, b in zip(lo, hi)]


def windows_of_batch(orc, reads, k):
    from oracle import oracle as _o

    bases, offsets = ragged(reads)
    canon, flags = orc_windows(orc, bases if len(bases) else np.zeros(1, np.uint8), len(reads), 0, k, offsets=offsets)
    wo = _o.win_offsets_for(len(reads), 0, k, offsets)
    return bases, offsets, canon, flags, np.asarray(wo, np.uint64)


def table_of_reads(orc, reads, k):
    _, _, canon, flags, _ = windows_of_batch(orc, reads, k)
    return table_of(canon, flags)


def halves(reads):
    h = len(reads) // 2
    return reads[:h], reads[h:]


def gather_index(p, n_reads):
    """the index reads_gather is given: seeded, with repeats and a few indices outside the batch"""
    rng = np.random.default_rng(99_000 + p.seed)
    idx = rng.integers(0, n_reads, 40).astype(np.int64)
    idx[::7] = n_reads + rng.integers(0, 5, len(idx[::7]))
    return idx


def host_pipeline(p, reads=None):
    """the references end to end -> dict of arrays, keys as STAGES lists them"""
    from kmers_amd._lib import RULE_MIN, RULE_SUM, SETOP_COUNTER_SUBTRACT, SETOP_INTERSECT, SETOP_SUBTRACT, SETOP_SYMDIFF, SETOP_UNION
    from oracle import oracle as orc
    from tests.test_gpu_count_read_stats import _host_stats
    from tests.test_gpu_count_setop import _host_compare, _host_setop

    k = p.k
    reads = reads_of(p) if reads is None else reads
    n = len(reads)
    H = {}
    bases, offsets, canon, flags, wo = windows_of_batch(orc, reads, k)
    tk, tc = table_of(canon, flags)
    H["table_k"], H["table_c"] = tk, tc
    H["lookup"] = host_lookup(tk, tc, canon, flags)
    H["stats"] = _host_stats(H["lookup"], flags, wo, SOLID_MIN)
    # ---- set algebra of the tables of the two halves
    a, b = halves(reads)
    (ka, ca), (kb, cb) = table_of_reads(orc, a, k), table_of_reads(orc, b, k)
    H["merge_k"], H["merge_c"] = _host_setop(SETOP_UNION, RULE_SUM, ka, ca, kb, cb)
    H["inter_k"], H["inter_c"] = _host_setop(SETOP_INTERSECT, RULE_MIN, ka, ca, kb, cb)
    H["sub_k"], H["sub_c"] = _host_setop(SETOP_SUBTRACT, 0, ka, ca, kb, cb)
    H["sym_k"], H["sym_c"] = _host_setop(SETOP_SYMDIFF, 0, ka, ca, kb, cb)
    H["csub_k"], H["csub_c"] = _host_setop(SETOP_COUNTER_SUBTRACT, 0, ka, ca, kb, cb)
    cmp = _host_compare(ka, ca, kb, cb)
    H["compare"] = np.array([cmp[f] for f in COMPARE_FIELDS], np.uint64)
    # ---- the graph
    edges, flips, nbr = graph_np.adjacency_np(tk, tc, k, 1)
    H["edges"], H["flips"], H["nbr"] = edges, flips, nbr
    nodes, uoff, circ, sums = unitig_np.unitigs_np(tk, tc, k, 1, edges, flips, nbr)
    H["u_nodes"], H["u_offsets"], H["u_circular"], H["u_sums"] = nodes, uoff, circ, sums
    place = path_np.place_np(nodes, uoff, len(tc))
    H["place"] = place
    lo, tg = link_np.links_of_unitigs_np(edges, flips, nbr, len(tc), nodes, uoff, place)
    H["l_offsets"], H["l_targets"] = lo, tg
    keep, reason = clean_np.clean_np(uoff, circ, sums, lo, tg, **clean_np.rule_of(k))
    H["keep"], H["reason"] = keep, reason
    H["clean_k"], H["clean_c"] = link_np.select_np(tk, tc, place, uoff, keep)
    labels, ids, rec, c = component_np.components_np(uoff, sums, lo, tg, mask=keep)
    H["c_labels"], H["c_ids"], H["c_records"], H["c_n"] = labels, ids, rec, np.array([c], np.uint64)
    # ---- the reads over the graph
    po, segs = path_np.read_paths_np(canon, flags, wo, tk, place, uoff)
    H["p_offsets"], H["p_segments"] = po, segs
    support, summary = link_support_np.link_support_np(segs, uoff, lo, tg)
    H["s_support"], H["s_summary"] = support, summary
    cut = link_support_np.unsupported_np(support, 1)
    cut_edges = link_support_np.adjacency_cut_np(edges, flips, nbr, len(tc), nodes, uoff, place, lo, cut)
    H["cut_edges"], H["n_cut"] = cut_edges, np.array([int(cut.sum())], np.uint64)
    pn, pof, pc, ps = unitig_np.unitigs_np(tk, tc, k, 1, cut_edges, flips, nbr)
    H["pr_nodes"], H["pr_offsets"], H["pr_circular"], H["pr_sums"] = pn, pof, pc, ps
    H["pr_l_offsets"], H["pr_l_targets"] = link_np.links_of_unitigs_np(cut_edges, flips, nbr, len(tc), pn, pof, path_np.place_np(pn, pof, len(tc)))
    # ---- correction
    table = dict(zip(key_ints(tk), (int(x) for x in tc)))
    H["corrected"], H["fixes"] = correct_np.correct_reads(bases, n, 0, k, correct_np.dict_count(table), SOLID_MIN, 1, offsets=offsets)
    # ---- colours: three samples, the reads by index modulo 3
    samples = [set(key_ints(table_of_reads(orc, reads[c::N_COLORS], k)[0])) for c in range(N_COLORS)]
    cdict = color_np.color_dict(samples)
    H["color_k"], H["color_m"] = correct_np.table_arrays(cdict, k)
    H["cm_shared"], H["cm_spectrum"] = color_np.color_matrix(H["color_m"], N_COLORS)
    H["rc_rows"], H["rc_hits"] = color_np.read_colors(bases, n, 0, k, correct_np.dict_count(cdict), N_COLORS, offsets=offsets)
    # ---- read editing: keep the reads whose median abundance is at least MIN_MEDIAN, clipped to their longest solid run
    stats = H["stats"]
    H["sel_bases"], H["sel_offsets"], H["sel_index"] = reads_np.select_np(bases, n, 0, offsets, keep=stats[:, 6] >= np.uint64(MIN_MEDIAN),
                                                                         span=stats[:, 7], span_k=k, min_len=k)
    H["gat_bases"], H["gat_offsets"] = reads_np.gather_np(bases, n, 0, gather_index(p, n), offsets, span=stats[:, 7], span_k=k)
    assert set(H) == {x for names in STAGES.values() for x in names}
    return H


COMPARE_FIELDS = ("n_both", "n_only_a", "n_only_b", "sum_a", "sum_b", "sum_a_both", "sum_b_both", "sum_min", "sum_max")


def structure(p, H, reads=None):
    """what the non-vacuity test asks of a seed, read off the reference's arrays alone -> dict of bools"""
    reads = reads_of(p) if reads is None else reads
    bases, offsets = ragged(reads)
    nib = lambda x: np.array([bin(v).count("1") for v in range(16)])[x]
    seg_per_read = np.diff(H["p_offsets"].astype(np.int64))
    trimmed = len(H["sel_index"]) < len(reads) or not np.array_equal(
        np.diff(H["sel_offsets"].astype(np.int64)), np.diff(offsets.astype(np.int64))[H["sel_index"].astype(np.int64)])
    return {
        "fork": bool(((nib(H["edges"] & 15) > 1) | (nib(H["edges"] >> 4) > 1)).any()),
        "link": len(H["l_targets"]) > 0,
        "cleaned": bool((H["keep"] == 0).any()),
        "two_components": int(H["c_n"][0]) >= 2,
        "multi_segment_read": bool((seg_per_read >= 2).any()),
        "support_0_and_many": bool((H["s_support"] == 0).any() and (H["s_support"] > 1).any()),
        "corrected": bool((H["fixes"][:, 2] > 0).any()) and not np.array_equal(H["corrected"], bases),
        "selected": bool(trimmed),
    }
