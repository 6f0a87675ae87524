"""Batch API over the libkmx C ABI with torch tensors as device buffers.

torch is plumbing here (device memory, streams, torch.distributed); every computation is a
hand-written HIP kernel behind include/kmx.h.  All functions run on `Context.stream` (by
default torch's current stream of the device at construction) and are asynchronous like any torch CUDA op.

Stream discipline: kmx kernels are enqueued on `Context.stream`.  Every method makes that stream torch's current
stream for its whole body, so the buffers it allocates, the launch and the device-to-host read-back are ordered on ONE
stream -- also when the context was built on a side stream, or is used inside `with torch.cuda.stream(other)`.  Tensors
handed IN by the caller must be ready on `Context.stream` (produced there, or after a `wait_stream`): they are marked
with `record_stream` so the caching allocator does not recycle them under a running kmx kernel.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import math

import numpy as np
import torch

from . import _lib
from ._lib import (CLEAN_BUBBLE, CLEAN_ISLAND, CLEAN_TIP, COMP_COUNT_SUM, COMP_N_NODES, COMP_N_UNITIGS, COMP_ROOT, COMP_WORDS, CR_WORDS, HASH_IDENTITY, HASH_LEX, HASH_NONE, LS_CROSSED, LS_JUNCTIONS, LS_UNLINKED, LS_WORDS, NO_ENTRY, PATH_POS, PATH_READ, PATH_SPAN, PATH_UNITIG, PATH_WORDS, RC_WORDS, REDUCE_SUM_FW, RS_SPAN, RS_WORDS, RULE_LEFT, RULE_MAX, RULE_MIN, RULE_RIGHT, RULE_SUM,
                   SETOP_COUNTER_SUBTRACT, SETOP_INTERSECT, SETOP_SUBTRACT, SETOP_SYMDIFF, SETOP_UNION, KmxError, Reads, Summary, Summary2,
                   TableCompare)

SEED_DEFAULT = 0x6B6D6572735F7631  # "kmers_v1"


def _ptr(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("kmx expects contiguous CUDA tensors")
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(int(t))


def u64_numpy(t: torch.Tensor) -> np.ndarray:
    """int64 CUDA tensor holding u64 words -> numpy uint64 (host)."""
    return t.detach().cpu().numpy().view(np.uint64)


def read_stats_span(stats: torch.Tensor, k: int) -> tuple[torch.Tensor, torch.Tensor]:
    """column RS_SPAN of count_read_stats' rows -> (first_base, end_base), int64 per read: the bases [first_base, end_base) of the
    longest run of solid windows (a run of `len` windows from window `start` covers start .. start + len + k - 1); (0, 0) for a read
    without a solid window.  Works on host and device tensors."""
    word = stats.reshape(-1, RS_WORDS)[:, RS_SPAN]
    start, length = word & 0xFFFFFFFF, (word >> 32) & 0xFFFFFFFF
    return start, torch.where(length > 0, start + length + (int(k) - 1), torch.zeros_like(start))


def _u64_key(v: int) -> int:
    """the int64 that orders like the u64 v (0 <= v < 2^64) once the sign bit is flipped"""
    v = int(v) ^ (1 << 63)
    return v - (1 << 64) if v >= (1 << 63) else v


def _u64_ge(t: torch.Tensor, v: int) -> torch.Tensor:
    """t >= v with the int64 words of t read as u64"""
    return (t ^ (-2**63)) >= _u64_key(v)


def _u64_le(t: torch.Tensor, v: int) -> torch.Tensor:
    return (t ^ (-2**63)) <= _u64_key(v)


def _ratio(num: int, den: int) -> float:
    return num / den if den else 0.0


@dataclasses.dataclass(frozen=True)
class TableComparison:
    """kmx_table_compare on the host: how many keys two count tables share and the sums of their counts (u64 values, sums wrapped
    mod 2^64 as the device adds them), and the similarity measures that follow (0.0 where a denominator is 0)."""
    n_both: int
    n_only_a: int
    n_only_b: int
    sum_a: int
    sum_b: int
    sum_a_both: int
    sum_b_both: int
    sum_min: int
    sum_max: int

    @property
    def jaccard(self) -> float:
        return _ratio(self.n_both, self.n_both + self.n_only_a + self.n_only_b)

    @property
    def containment_a(self) -> float:
        """the share of a's keys that b holds"""
        return _ratio(self.n_both, self.n_both + self.n_only_a)

    @property
    def containment_b(self) -> float:
        return _ratio(self.n_both, self.n_both + self.n_only_b)

    @property
    def weighted_jaccard(self) -> float:
        return _ratio(self.sum_min, self.sum_max)

    @property
    def bray_curtis(self) -> float:
        """the Bray-Curtis dissimilarity 1 - 2 sum_min / (sum_a + sum_b)"""
        return 1.0 - 2.0 * self.sum_min / (self.sum_a + self.sum_b) if self.sum_a + self.sum_b else 0.0


@dataclasses.dataclass(frozen=True)
class ColorTable:
    """A coloured table: the sorted distinct keys of a table (int64[n]; k 33..64: int64[n, 2] = (low, high) words) and, in the place
    of the counts, one u64 bit mask per key (int64[n]) of the samples -- colours 0 .. n_colors - 1, at most 64 -- that hold it.  Every
    call that takes a table (kmers, counts) takes (kmers, colors).  `k` is carried along for the caller (None = not said)."""
    kmers: torch.Tensor
    colors: torch.Tensor
    n_colors: int
    k: int | None = None


@dataclasses.dataclass(frozen=True)
class ColorMatrix:
    """What kmx_count_color_matrix fills -- shared int64[n_colors, n_colors]: the entries that hold colours i and j (symmetric, the
    diagonal = the samples' sizes); spectrum int64[n_colors + 1] or None: the entries with exactly j colours -- and the similarity
    measures that follow, for all pairs at once.  Host or device tensors."""
    shared: torch.Tensor
    spectrum: torch.Tensor | None = None

    @property
    def sizes(self) -> torch.Tensor:
        """int64[n_colors]: the number of entries of each colour"""
        return torch.diagonal(self.shared)

    def _over(self, den: torch.Tensor) -> torch.Tensor:
        num, den = self.shared.to(torch.float64), den.to(torch.float64)
        return torch.where(den > 0, num / den.clamp(min=1.0), torch.zeros_like(num))   # (an empty pair gives 0, as _ratio does)

    def jaccard(self) -> torch.Tensor:
        """float64[n_colors, n_colors]: shared / (size_i + size_j - shared)"""
        sz = self.sizes
        return self._over(sz[:, None] + sz[None, :] - self.shared)

    def containment(self) -> torch.Tensor:
        """float64[n_colors, n_colors]: element [i, j] = the share of sample i's keys that sample j holds"""
        return self._over(self.sizes[:, None].expand_as(self.shared))


_POPCOUNT4 = [bin(v).count("1") for v in range(16)]


@dataclasses.dataclass(frozen=True)
class GraphSummary:
    """The 256 bins of kmx_count_edge_histogram on the host -- bins[b] = entries whose edge byte is b: the low nibble of b holds the
    successor edges (out), the high nibble the predecessor edges (in) -- and the degree statistics that follow from them."""
    bins: tuple

    def _sum(self, pred) -> int:
        return sum(v for b, v in enumerate(self.bins) if pred(_POPCOUNT4[b >> 4], _POPCOUNT4[b & 15]))

    @property
    def n_entries(self) -> int:
        return sum(self.bins)

    @property
    def n_edges(self) -> int:
        """directed edge slots: an edge between two entries is listed by both (a self-loop by both sides of one)"""
        return sum(v * (_POPCOUNT4[b >> 4] + _POPCOUNT4[b & 15]) for b, v in enumerate(self.bins))

    @property
    def n_isolated(self) -> int:
        """entries without an edge (entries that are not present among them)"""
        return self.bins[0]

    @property
    def n_tips(self) -> int:
        """entries with edges on one side only: dead ends"""
        return self._sum(lambda i, o: (i == 0) != (o == 0))

    @property
    def n_branching(self) -> int:
        """entries with more than one edge on a side"""
        return self._sum(lambda i, o: i > 1 or o > 1)

    @property
    def n_interior(self) -> int:
        """entries with exactly one predecessor and one successor"""
        return self._sum(lambda i, o: i == 1 and o == 1)

    @property
    def degrees(self) -> np.ndarray:
        """int64[5, 5]: degrees[i, o] = entries with i predecessor edges and o successor edges"""
        m = np.zeros((5, 5), np.int64)
        for b, v in enumerate(self.bins):
            m[_POPCOUNT4[b >> 4], _POPCOUNT4[b & 15]] += v
        return m


@dataclasses.dataclass
class Unitigs:
    """What kmx_count_unitigs(2) returns: the canonical unitigs of a count table's de Bruijn graph, in order of their head entries.
    nodes int64[n_nodes]: the oriented nodes 2 * entry + o (o = 1: the entry read as its reverse complement), one unitig after
    another; offsets int64[n_unitigs + 1] into nodes; circular uint8[n_unitigs]; count_sums int64[n_unitigs] (the u64 wrapping sums of
    the entries' counts).  `kmers` is the table's key tensor, kept for the sequences."""
    nodes: "torch.Tensor"
    offsets: "torch.Tensor"
    circular: "torch.Tensor"
    count_sums: "torch.Tensor"
    n_unitigs: int
    k: int
    kmers: "torch.Tensor" = dataclasses.field(repr=False, default=None)
    _ctx: "Context" = dataclasses.field(repr=False, default=None)
    _seq: "torch.Tensor" = dataclasses.field(repr=False, default=None)

    @property
    def n_nodes(self) -> int:
        return int(self.nodes.numel())

    @property
    def lengths(self):
        """int64[n_unitigs]: nodes per unitig (its sequence has k - 1 bases more)"""
        return self.offsets[1:] - self.offsets[:-1]

    @property
    def mean_counts(self):
        """float64[n_unitigs]: the mean count per node, count_sums (as u64) / lengths -- for looking at a graph.  Without count_sums
        every mean is 1, as the cleaning rule reads it.  The rule itself (count_unitig_clean) never uses this: it compares integer
        products."""
        if self.count_sums is None:
            return torch.ones(self.n_unitigs, dtype=torch.float64, device=self.offsets.device)
        s = self.count_sums.to(torch.float64)
        s = torch.where(self.count_sums < 0, s + 2.0**64, s)
        return s / self.lengths.to(torch.float64)

    def sequences(self):
        """kmx_count_unitig_sequences(2) -> uint8[n_nodes + n_unitigs * (k - 1)], ASCII ACGT: unitig u starts at byte
        offsets[u] + u * (k - 1) and has lengths[u] + k - 1 bases.  Computed once and kept."""
        if self._seq is None:
            self._seq = self._ctx._unitig_sequences(self)
        return self._seq

    def sequence(self, u: int) -> bytes:
        """the bases of unitig u, on the host"""
        if not 0 <= u < self.n_unitigs:
            raise IndexError(u)
        lo, hi = (int(v) for v in self.offsets[u:u + 2].cpu())
        at = lo + u * (self.k - 1)
        return bytes(self.sequences()[at:at + (hi - lo) + self.k - 1].cpu().numpy())

    def tips(self, links: "UnitigLinks", max_nodes: int, islands: bool = False):
        """bool[n_unitigs], in torch: the unitigs to clip as dead ends -- not circular, at most max_nodes nodes, and exactly one of
        the two sides (2 u, 2 u + 1) without a link.  islands=True: a unitig without a link on either side qualifies too."""
        open_sides = (links.degrees == 0).sum(1)
        loose = (open_sides == 1) | (open_sides == 2) if islands else open_sides == 1
        return (self.circular == 0) & (self.lengths <= int(max_nodes)) & loose

    def write_fasta(self, file, width: int = 60):
        """The unitigs as FASTA, formatted on the device (kmx_fastx_format over sequences()): record u is named u, its bases in
        lines of `width` (0: one line).  `file`: a path or a binary file object -> the bytes written."""
        step = torch.arange(self.n_unitigs + 1, dtype=torch.int64, device=self.offsets.device) * (self.k - 1)
        return self._ctx.write_fastx(file, self.sequences(), self.n_unitigs, 0, offsets=self.offsets + step, fmt=_lib.FASTX_FASTA,
                                     line_width=int(width))

    def write_gfa(self, file, links: "UnitigLinks | None" = None, support: "LinkSupport | None" = None):
        """The compacted graph as GFA 1, written on the host -- for graphs one would look at, not for 1e9 nodes.  `file` is a path
        or a text file object.  H VN:Z:1.0; one S line per unitig u, named u, with LN:i (bases) and KC:i (the sum of its entries'
        counts); with `links`, one L line per link, + / - from the orientation bit and an overlap of (k - 1)M.  A link and its mirror
        image say the same thing and are one line, written from the smaller of (t, t') and (t' ^ 1, t ^ 1); lines are sorted.
        With `support` (count_link_support over these links) every L line ends in RC:i:<n>, the reads that cross the link -- the
        larger of the two numbers where a link and its mirror differ (even k, around a palindromic k-mer)."""
        if isinstance(file, (str, bytes)) or hasattr(file, "__fspath__"):
            with open(file, "w") as f:
                return self.write_gfa(f, links, support)
        k = self.k
        seq = self.sequences().cpu().numpy().tobytes().decode("ascii")
        offs = self.offsets.cpu().tolist()
        sums = u64_numpy(self.count_sums).tolist()
        file.write("H\tVN:Z:1.0\n")
        for u in range(self.n_unitigs):
            s = seq[offs[u] + u * (k - 1):offs[u + 1] + (u + 1) * (k - 1)]
            file.write(f"S\t{u}\t{s}\tLN:i:{len(s)}\tKC:i:{sums[u]}\n")
        if links is not None:
            pairs = {min((t, t2), (t2 ^ 1, t ^ 1)) for t, t2 in zip(links.sources().cpu().tolist(), links.targets.cpu().tolist())}
            rc = {}
            if support is not None:
                for t, t2, c in zip(links.sources().cpu().tolist(), links.targets.cpu().tolist(), u64_numpy(support.support).tolist()):
                    key = min((t, t2), (t2 ^ 1, t ^ 1))
                    rc[key] = max(rc.get(key, 0), c)
            for t, t2 in sorted(pairs):
                tag = f"\tRC:i:{rc[(t, t2)]}" if support is not None else ""
                file.write(f"L\t{t >> 1}\t{'+-'[t & 1]}\t{t2 >> 1}\t{'+-'[t2 & 1]}\t{k - 1}M{tag}\n")


@dataclasses.dataclass
class UnitigLinks:
    """What kmx_count_unitig_links returns: which oriented unitig follows which.  The oriented unitig t = 2 * u + s is unitig u as
    written (s = 0) or its reverse complement (s = 1); offsets int64[2 * n_unitigs + 1]: t owns targets[offsets[t]:offsets[t + 1]], at
    most four; targets int64[n_links]: the oriented unitigs t' that follow, each overlapping t by k - 1 bases."""
    offsets: "torch.Tensor"
    targets: "torch.Tensor"

    @property
    def n_links(self) -> int:
        return int(self.targets.numel())

    @property
    def degrees(self):
        """int64[n_unitigs, 2]: the links leaving unitig u as written (column 0) and leaving its mirror (column 1)"""
        return (self.offsets[1:] - self.offsets[:-1]).view(-1, 2)

    def sources(self):
        """int64[n_links]: the t of every link, in the order of `targets`"""
        deg = self.offsets[1:] - self.offsets[:-1]
        return torch.repeat_interleave(torch.arange(deg.numel(), device=deg.device), deg)


@dataclasses.dataclass
class LinkSupport:
    """What kmx_count_link_support accumulates: support int64[n_links] (u64 words), the junctions of the reads that cross each link
    slot or its mirror -- for paths over the links' own graph, the occurrences in the reads, on either strand, of the (k + 1)-mer
    the link spells -- and summary int64[3] (columns _lib.LS_*): junctions = crossed + unlinked.  Both live on the device; hand the
    object back as `out` to add another batch of reads."""
    support: "torch.Tensor"
    summary: "torch.Tensor"

    @property
    def junctions(self) -> int:
        """pairs of consecutive segments of one read with no gap between them"""
        return int(u64_numpy(self.summary)[LS_JUNCTIONS])

    @property
    def crossed(self) -> int:
        """... that cross a link"""
        return int(u64_numpy(self.summary)[LS_CROSSED])

    @property
    def unlinked(self) -> int:
        """... that cross none: 0 when the paths were made over the graph the links were made of -- a self-check"""
        return int(u64_numpy(self.summary)[LS_UNLINKED])

    def unsupported(self, min_support: int = 1):
        """uint8[n_links] for count_cut_links: 1 where fewer than min_support reads cross the link (as u64).  A link and its mirror
        carry the same support wherever the mirror exists, so the mask removes an edge in both directions."""
        m = int(min_support)
        s = self.support
        below = (s >= 0) & (s < m) if m < 2**63 else (s >= 0) | (s < m - 2**64)
        return below.to(torch.uint8)


@dataclasses.dataclass
class UnitigComponents:
    """What kmx_count_unitig_components returns: the connected components of the compacted graph.  labels int64[U]: the smallest
    unitig index of the unitig's component; ids int64[U]: the component's number, 0 .. n_components - 1 in ascending order of the
    labels (both -1, COMPONENT_NONE, for a unitig the mask left out); records int64[C, 4] (u64 words, columns _lib.COMP_*), None
    with stats=False; rounds: the hook / jump rounds the call ran."""
    labels: "torch.Tensor"
    ids: "torch.Tensor"
    records: "torch.Tensor"
    n_components: int
    rounds: int

    @property
    def roots(self):
        """int64[C]: the label of each component"""
        return self.records[:, COMP_ROOT]

    @property
    def n_unitigs(self):
        """int64[C]: unitigs per component"""
        return self.records[:, COMP_N_UNITIGS]

    @property
    def n_nodes(self):
        """int64[C]: nodes (entries of the table) per component"""
        return self.records[:, COMP_N_NODES]

    @property
    def count_sums(self):
        """int64[C]: the u64 wrapping sum of the count sums of the component's unitigs"""
        return self.records[:, COMP_COUNT_SUM]

    @property
    def mean_counts(self):
        """float64[C]: the mean count per node, count_sums (as u64) / n_nodes, as Unitigs.mean_counts -- for looking at a graph"""
        s = self.count_sums.to(torch.float64)
        s = torch.where(self.count_sums < 0, s + 2.0**64, s)
        return s / self.n_nodes.to(torch.float64)

    def keep(self, min_nodes=0, min_unitigs=0, min_count_sum=0, largest=None):
        """uint8[U] for count_unitig_select(2): 1 iff the unitig's component has at least min_nodes nodes, min_unitigs unitigs and a
        count sum (as u64) of min_count_sum, all of them; largest=n keeps, of those, only the n components with the most nodes,
        ties going to the smaller id.  A unitig the mask left out is 0.  In torch."""
        if self.records is None:
            raise ValueError("keep needs the records: count_unitig_components(..., stats=True)")
        cs = self.count_sums
        big = int(min_count_sum) >= 2**63   # (u64 order on int64 words: a negative word is a sum of 2^63 or more)
        enough = (cs < 0) & (cs >= int(min_count_sum) - 2**64) if big else (cs < 0) | (cs >= int(min_count_sum))
        ok = (self.n_nodes >= int(min_nodes)) & (self.n_unitigs >= int(min_unitigs)) & enough
        if largest is not None:
            order = torch.sort(self.n_nodes, descending=True, stable=True).indices   # (stable: equal sizes stay in order of id)
            top = torch.zeros_like(ok)
            top[order[:max(int(largest), 0)]] = True
            ok = ok & top
        alive = self.ids >= 0
        out = torch.zeros(self.ids.numel(), dtype=torch.uint8, device=self.ids.device)
        out[alive] = ok[self.ids[alive]].to(torch.uint8)
        return out


@dataclasses.dataclass
class ReadPaths:
    """What kmx_count_read_paths(2) returns: the segments of every read over the unitigs, ordered by read, then by start.
    offsets int64[n_reads + 1]: read r owns segments[offsets[r]:offsets[r + 1]]; segments int64[S, 4] (u64 words, columns
    _lib.PATH_*).  A segment is a maximal run of consecutive windows of one read that walk one unitig in one direction: window
    start + t of the read sits at node pos + t of the unitig, or at pos - t when `reverse` is set."""
    offsets: "torch.Tensor"
    segments: "torch.Tensor"
    k: int

    @property
    def n_segments(self) -> int:
        return int(self.segments.shape[0])

    @property
    def read(self):
        return self.segments[:, PATH_READ]

    @property
    def start(self):
        """position of the segment's first window in its read (its bases: start .. start + length + k - 1)"""
        return self.segments[:, PATH_SPAN] & 0xFFFFFFFF

    @property
    def length(self):
        """windows in the segment"""
        return (self.segments[:, PATH_SPAN] >> 32) & 0xFFFFFFFF

    @property
    def unitig(self):
        return self.segments[:, PATH_UNITIG]

    @property
    def pos(self):
        """node of the unitig, counted from its written start, where the segment's first window sits"""
        return (self.segments[:, PATH_POS] >> 1) & 0x7FFFFFFFFFFFFFFF

    @property
    def reverse(self):
        """bool: the read walks the unitig's mirror (positions descend along the read)"""
        return (self.segments[:, PATH_POS] & 1) != 0

    def unitig_coverage(self, n_unitigs: int):
        """int64[n_unitigs]: how many windows of the batch lie on each unitig"""
        cov = torch.zeros(int(n_unitigs), dtype=torch.int64, device=self.segments.device)
        return cov.scatter_add_(0, self.unitig, self.length)

    def components(self, comp: "UnitigComponents"):
        """int64[S]: the component id of every segment's unitig (-1 where the mask of count_unitig_components left the unitig
        out) -- a gather in torch.  Reads in different components share no unitig: the batch splits into independent jobs."""
        return comp.ids[self.unitig]

    def read_components(self, comp: "UnitigComponents", n_reads: int):
        """int64[n_reads]: per read the smallest component id over its segments, -1 for a read without a segment in a component
        (no mapped window, or only unitigs the mask left out) -- a scatter_reduce(amin) in torch.  What Context.reads_partition
        wants as labels: a read whose segments lie in one component goes to that component's group."""
        big = torch.iinfo(torch.int64).max
        ids = self.components(comp)
        out = torch.full((int(n_reads),), big, dtype=torch.int64, device=self.segments.device)
        out.scatter_reduce_(0, self.read, torch.where(ids >= 0, ids, torch.full_like(ids, big)), "amin", include_self=True)
        return torch.where(out == big, torch.full_like(out, -1), out)


def ee_weights(phred: int = 33) -> np.ndarray:
    """The default weight table of reads_quality: 256 words by the RAW quality byte, round(2^32 * 10^(-q / 10)) with
    q = max(byte - phred, 0) -- expected errors as exact integer sums."""
    q = np.maximum(np.arange(256, dtype=np.int64) - int(phred), 0)
    return np.round(2.0**32 * 10.0 ** (-q / 10.0)).astype(np.uint64)


def expected_errors(rows):
    """float64[n_reads]: RQ_WEIGHT of reads_quality's rows (weights "ee") as expected errors; the word is a u64, so the top bit
    is added back"""
    w = rows[:, _lib.RQ_WEIGHT]
    return (w & 0x7FFFFFFFFFFFFFFF).to(torch.float64) / 2.0**32 + (w < 0).to(torch.float64) * 2.0**31


def gc_content(rows):
    """float64[n_reads]: (C + G) / (A + C + G + T) out of reads_complexity's rows; 0 for a read without a valid base"""
    ac, gt = rows[:, _lib.RX_AC], rows[:, _lib.RX_GT]
    cg = (ac >> 32) + (gt & 0xFFFFFFFF)
    total = (ac & 0xFFFFFFFF) + (gt >> 32) + cg
    return cg.to(torch.float64) / total.clamp(min=1).to(torch.float64)


def dust_score(rows):
    """float64[n_reads]: the largest DUST numerator of a read's windows out of reads_complexity's rows, over 61 -- the sdust /
    prinseq score of a full 64-base window (a homopolymer: 31, random bases: about 0.5, sdust's threshold: 2)"""
    return (rows[:, _lib.RX_DUST] & 0xFFFFFFFF).to(torch.float64) / 61.0


def _letters_arg(letters) -> int:
    """"G" -> 4, "ACGT" -> 15, "" -> 0: the base mask of kmx_reads_complexity (an int passes through)"""
    if isinstance(letters, int):
        return letters
    mask = 0
    for ch in letters:
        at = "ACGT".find(ch.upper())
        if at < 0:
            raise ValueError("letters: a string over ACGT")
        mask |= 1 << at
    return mask


# The public Illumina adapter sequences, as the 3' read-through shows them: what reads_adapter / reads_trim_adapters take.
ADAPTERS = {
    "truseq": "AGATCGGAAGAGC",
    "nextera": "CTGTCTCTTATACACATCT",
    "small_rna": "TGGAATTCTCGGGTGCCAAGG",
}


@dataclasses.dataclass
class ReadBatch:
    """A ragged batch of reads on the device, what reads_select / reads_gather write: bases uint8[n_bases], offsets
    int64[n_reads + 1] starting at 0, and -- where asked for -- index int64[n_reads], the source read of every read.  It goes
    straight into any call as (b.bases, b.n_reads, b.max_len(), offsets=b.offsets).  `ctx` is the context that made it (for
    max_len)."""
    bases: "torch.Tensor"
    offsets: "torch.Tensor"
    n_reads: int
    index: "torch.Tensor | None" = None
    ctx: "Context | None" = dataclasses.field(default=None, repr=False, compare=False)

    @property
    def n_bases(self) -> int:
        return int(self.bases.numel())

    def max_len(self) -> int:
        """the longest read (kmx_reads_length_range: one host round trip), the bound kmx_reads.read_len wants; 0 for no reads"""
        if self.n_reads == 0:
            return 0
        return self.ctx.reads_length_range(self.offsets)[1]


@dataclasses.dataclass
class ReadGroups:
    """What reads_partition returns: `batch` holds the reads of every non-negative label, grouped by label ascending and in source
    order within a group (batch.index: the source reads); labels int64[G], the distinct labels; group_offsets int64[G + 1]: group g
    is reads [group_offsets[g], group_offsets[g + 1]) of `batch`."""
    batch: ReadBatch
    labels: "torch.Tensor"
    group_offsets: "torch.Tensor"

    @property
    def n_groups(self) -> int:
        return int(self.labels.numel())


@dataclasses.dataclass
class MergedPairs:
    """What reads_merge_pairs returns.  merged / merged_quals: the consensus reads of the pairs that merged and their quality bytes
    (identical offsets; merged.index: the source pair).  unmerged1 / unmerged2: the mates of the pairs that did not, in step
    (both carry the pair index), unmerged1_quals / unmerged2_quals their quality bytes.  The *_quals are None where no quality
    bytes were given.  overlap_rows int64[n_reads, RP_WORDS] and merge_rows int64[n_reads, RM_WORDS] belong to the SOURCE pairs."""
    merged: ReadBatch
    merged_quals: "ReadBatch | None"
    unmerged1: ReadBatch
    unmerged2: ReadBatch
    unmerged1_quals: "ReadBatch | None"
    unmerged2_quals: "ReadBatch | None"
    overlap_rows: "torch.Tensor"
    merge_rows: "torch.Tensor"


@dataclasses.dataclass
class ReadDuplicates:
    """What reads_dedup returns.  rows int64[n, DD_WORDS] (viewable as u64; include/kmx.h has the words) in source order, keep
    uint8[n] (1 iff kept: what reads_select takes, for both mates of a pair), and the four words of the summary."""
    rows: "torch.Tensor"
    keep: "torch.Tensor"
    kept: int
    dropped: int
    largest: int
    collisions: int

    def histogram(self) -> "torch.Tensor":
        """int64[largest + 1]: entry c is the number of classes of c items (kept items whose COUNT is c); entry 0 is 0"""
        counts = self.rows[:, _lib.DD_COUNT]
        return torch.bincount(counts[counts > 0], minlength=self.largest + 1)


@dataclasses.dataclass
class DeduplicatedReads:
    """What reads_drop_duplicates returns: the kept reads and, where given, their quality bytes (identical offsets), for pairs the
    kept mates in step; every batch of bases carries the index of its source item.  `duplicates` belongs to the SOURCE items."""
    reads: ReadBatch
    quals: "ReadBatch | None"
    mates: "ReadBatch | None"
    mate_quals: "ReadBatch | None"
    duplicates: ReadDuplicates


@dataclasses.dataclass
class Sketch:
    """A counting sketch on the device (kmx_sketch_*): `cells`, uint8[64 << log2_blocks], zero when new; a key's four cells lie in
    block h >> (64 - log2_blocks) of 64 bytes, h its hash under `seed` (kmx.h has the definition).  `ctx` is the context that made
    it (for fill)."""
    cells: "torch.Tensor"
    log2_blocks: int
    seed: int = 0
    ctx: "Context | None" = dataclasses.field(default=None, repr=False, compare=False)

    def fill(self) -> float:
        """the share of non-zero cells (kmx_sketch_stats: one host round trip), what a sketch is sized by"""
        hist = self.ctx.sketch_stats(self)
        return 1.0 - int(hist[0].item()) / int(self.cells.numel())


def _hll_sigma(x: float) -> float:
    if x == 1.0:
        return math.inf
    y, z = 1.0, x
    while True:
        x *= x
        z0 = z
        z += x * y
        y += y
        if z == z0:
            return z


def _hll_tau(x: float) -> float:
    if x == 0.0 or x == 1.0:
        return 0.0
    y, z = 1.0, 1.0 - x
    while True:
        x = math.sqrt(x)
        z0 = z
        y *= 0.5
        z -= (1.0 - x) ** 2 * y
        if z == z0:
            return z / 3.0


def hll_estimate(hist, log2_regs: int) -> float:
    """The number of distinct keys behind HyperLogLog registers, from their 64 bins (kmx_hll_stats; hist[v] = the registers that hold
    v): Ertl's improved estimator as include/kmx.h spells it out, in double precision.  All registers zero gives 0."""
    p = int(log2_regs)
    if not _lib.HLL_MIN_LOG2_REGS <= p <= _lib.HLL_MAX_LOG2_REGS:
        raise ValueError("log2_regs outside 4..24")
    c = [int(v) for v in (hist.tolist() if hasattr(hist, "tolist") else hist)]
    m, q = float(1 << p), 64 - p
    if len(c) < q + 2 or sum(c[:q + 2]) != 1 << p:
        raise ValueError("hll_estimate: the bins 0 .. 65 - log2_regs do not hold 2^log2_regs registers")
    z = m * _hll_tau(1.0 - c[q + 1] / m)
    for j in range(q, 0, -1):
        z = 0.5 * (z + c[j])
    z += m * _hll_sigma(c[0] / m)
    return m * m / (2.0 * math.log(2.0)) / z if z else math.inf   # (every register at the top rank: no upper end)


def hll_sketch_log2_blocks(n_distinct: float, fill: float = 0.25) -> int:
    """The smallest log2_blocks in 0..32 at which a counting sketch that n_distinct keys were added to is at most `fill` full: a key
    marks one of the 16 cells of each row of its block, so the occupancy of a row is 1 - exp(-n / (16 * 2^b)) (at fill = 0.25 about
    14 bytes per distinct key).  32 where even the largest sketch is fuller."""
    if not 0.0 < fill < 1.0:
        raise ValueError("fill outside (0, 1)")
    for b in range(_lib.SKETCH_MAX_LOG2_BLOCKS + 1):
        if 1.0 - math.exp(-float(n_distinct) / (16.0 * float(1 << b))) <= fill:
            return b
    return _lib.SKETCH_MAX_LOG2_BLOCKS


@dataclasses.dataclass
class Hll:
    """HyperLogLog registers on the device (kmx_hll_*): `regs`, uint8[1 << log2_regs], zero when new; a key raises register
    h >> (64 - log2_regs) to the rank of the rest of its hash h under `seed` (kmx.h has the definition).  `ctx` is the context that
    made it."""
    regs: "torch.Tensor"
    log2_regs: int
    seed: int = 0
    ctx: "Context | None" = dataclasses.field(default=None, repr=False, compare=False)

    def histogram(self):
        """kmx_hll_stats -> int64[64] on the device: how many registers hold each value"""
        return self.ctx.hll_stats(self)

    def estimate(self) -> float:
        """the number of distinct keys added (hll_estimate of the histogram: one host round trip)"""
        return hll_estimate(self.histogram().cpu(), self.log2_regs)

    def sketch_log2_blocks(self, fill: float = 0.25) -> int:
        """the log2_blocks of a counting sketch that what was added here fills to at most `fill` (hll_sketch_log2_blocks)"""
        return hll_sketch_log2_blocks(self.estimate(), fill)


@dataclasses.dataclass
class HllComparison:
    """Context.hll_compare: the estimated distinct keys of two samples (a, b), of their union (the bytewise maximum of the registers)
    and, by inclusion-exclusion clipped at 0, of their intersection.  Each carries the estimator's error of about
    1.04 / sqrt(2^log2_regs) of the UNION's size: a small intersection of large samples is mostly noise."""
    a: float
    b: float
    union: float
    intersection: float = dataclasses.field(init=False)

    def __post_init__(self):
        self.intersection = max(self.a + self.b - self.union, 0.0)

    @property
    def jaccard(self) -> float:
        return self.intersection / self.union if self.union else 0.0

    @property
    def containment_a(self) -> float:
        """the share of a's keys that b holds"""
        return min(self.intersection / self.a, 1.0) if self.a else 0.0

    @property
    def containment_b(self) -> float:
        return min(self.intersection / self.b, 1.0) if self.b else 0.0


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")   # the empty block every BGZF file ends with


def bgzf_compress(data, level: int = 6, block_bytes: int = 65280) -> bytes:
    """bytes -> a BGZF file image (host zlib): one raw-DEFLATE gzip member per `block_bytes` of data (65280, what htslib takes, keeps
    every block within 64 KiB at any level), each with the 18-byte 'BC' header, CRC-32 and ISIZE, and the 28-byte EOF marker behind
    them.  What bgzip writes; Context.load_fastx / bgzf_inflate take it back."""
    import zlib

    data = memoryview(bytes(data) if not isinstance(data, (bytes, bytearray, memoryview)) else data).cast("B")
    if not 1 <= block_bytes <= 65280:
        raise ValueError("bgzf_compress: block_bytes in 1..65280")
    out = []
    for i in range(0, len(data), block_bytes):
        piece = data[i:i + block_bytes]
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
        payload = co.compress(piece) + co.flush()
        size = len(payload) + 26
        if size > 65536:
            raise ValueError("bgzf_compress: a block does not fit 64 KiB")
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + (size - 1).to_bytes(2, "little") + payload +
                   zlib.crc32(piece).to_bytes(4, "little") + len(piece).to_bytes(4, "little"))
    out.append(BGZF_EOF)
    return b"".join(out)


@dataclasses.dataclass
class BgzfIndex:
    """kmx_bgzf_index: block b of the image is bytes [block_offsets[b], block_offsets[b+1]) and inflates to bytes
    [text_offsets[b], text_offsets[b+1]) of the text (int64 device tensors of n_blocks + 1 words); trailing: bytes behind the last
    complete block (0 for a sound file); has_eof: the last block is the 28-byte EOF marker."""
    block_offsets: torch.Tensor
    text_offsets: torch.Tensor
    n_blocks: int
    n_text_bytes: int
    trailing: int
    has_eof: bool


def _on_ctx_stream(fn):
    """Run a Context method with Context.stream as torch's current stream (see "Stream discipline" above)."""
    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream == self.stream.cuda_stream:
            return fn(self, *args, **kwargs)
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                a.record_stream(self.stream)
        with torch.cuda.stream(self.stream):
            return fn(self, *args, **kwargs)
    return wrapped


class Context:
    """One kmx_ctx bound to a device and a HIP stream (borrowed from torch)."""

    def __init__(self, device: int | torch.device | None = None, stream: torch.cuda.Stream | None = None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise KmxError(_lib.E_HIP, "no HIP device visible: kmers_amd is GPU-only (no CPU fallback)")
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device if isinstance(device, int) else (device.index or 0))
        with torch.cuda.device(self.device):
            self.stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        h = C.c_void_p()
        st = self.lib.kmx_ctx_create_on_stream(self.device.index, C.c_void_p(self.stream.cuda_stream), C.byref(h))
        _lib.check(self.lib, None, st)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.kmx_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st):
        _lib.check(self.lib, self._h, st)

    def synchronize(self):
        self._ck(self.lib.kmx_ctx_synchronize(self._h))

    def set_work_buffer_limit(self, nbytes: int):
        """cap (bytes; 0 = automatic) on the context's device work buffer: kmx_ctx_set_work_buffer_limit"""
        self._ck(self.lib.kmx_ctx_set_work_buffer_limit(self._h, int(nbytes)))

    def work_buffer_info(self):
        """(bytes held, number of (re)allocations so far): kmx_ctx_work_buffer_info"""
        held, n = C.c_size_t(0), C.c_uint64(0)
        self._ck(self.lib.kmx_ctx_work_buffer_info(self._h, C.byref(held), C.byref(n)))
        return int(held.value), int(n.value)

    # ------------------------------------------------------------- helpers
    @_on_ctx_stream
    def empty(self, n, dtype):
        return torch.empty(int(n), dtype=dtype, device=self.device)

    @_on_ctx_stream
    def to_device(self, a) -> torch.Tensor:
        if isinstance(a, torch.Tensor):
            return a.to(self.device).contiguous()
        if isinstance(a, (bytes, bytearray)):
            a = np.frombuffer(bytes(a), dtype=np.uint8)
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        return torch.from_numpy(a.copy()).to(self.device)

    def _reads(self, bases: torch.Tensor, n_reads: int, read_len: int, offsets: torch.Tensor | None) -> Reads:
        return Reads(_ptr(bases) if bases is not None and bases.numel() else None, int(n_reads), int(read_len),
                     _ptr(offsets))

    # ------------------------------------------------------------ hot path
    @_on_ctx_stream
    def gen_reads(self, nbytes: int, seed: int = SEED_DEFAULT, first_byte: int = 0, out: torch.Tensor | None = None):
        """Deterministic synthetic ACGT stream (kmx_gen_reads)."""
        if out is None:
            out = self.empty(nbytes, torch.uint8)
        self._ck(self.lib.kmx_gen_reads(self._h, seed & (2**64 - 1), first_byte, _ptr(out), int(nbytes)))
        return out

    @_on_ctx_stream
    def canonical_reduce_async(self, bases, n_reads, read_len, k, hasher=HASH_NONE, hasher_k=0, flags=0, offsets=None,
                               out: torch.Tensor | None = None) -> torch.Tensor:
        """kmx_canonical_reduce; returns the device-resident summary (4 x int64 viewable as u64)."""
        if out is None:
            out = self.empty(4, torch.int64)
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(self.lib.kmx_canonical_reduce(self._h, C.byref(r), k, hasher, hasher_k, flags, _ptr(out)))
        return out

    @_on_ctx_stream
    def canonical_reduce(self, bases, n_reads, read_len, k, hasher=HASH_NONE, hasher_k=0, flags=0, offsets=None) -> Summary:
        out = self.canonical_reduce_async(bases, n_reads, read_len, k, hasher, hasher_k, flags, offsets)
        v = u64_numpy(out)
        return Summary(int(v[0]), int(v[1]), int(v[2]), int(v[3]))

    @_on_ctx_stream
    def canonical_reduce_host(self, bases, n_reads, read_len, k, hasher=HASH_NONE, hasher_k=0, flags=0, offsets=None) -> Summary:
        """kmx_canonical_reduce_host: the summary in host memory when the call returns (one launch for clean uniform reads)."""
        out = Summary()
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(self.lib.kmx_canonical_reduce_host(self._h, C.byref(r), k, hasher, hasher_k, flags, C.byref(out)))
        return out

    def win_offsets(self, n_reads, read_len, k, offsets=None) -> np.ndarray:
        if offsets is None:
            w = max(read_len - k + 1, 0)
            return np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(w)
        lens = np.diff(np.asarray(offsets).astype(np.int64))
        return np.concatenate([[0], np.cumsum(np.maximum(lens - k + 1, 0))]).astype(np.uint64)

    @_on_ctx_stream
    def canonical_windows(self, bases, n_reads, read_len, k, offsets=None, host_offsets=None, want=("fw", "rc", "canon", "flags")):
        """kmx_canonical_windows -> dict of device tensors (u64 words as int64, flags uint8)."""
        wo_host = self.win_offsets(n_reads, read_len, k, host_offsets)
        total = int(wo_host[-1])
        d_wo = self.to_device(wo_host) if offsets is not None else None
        outs = {n: (self.empty(total, torch.uint8) if n == "flags" else self.empty(total, torch.int64)) for n in want}
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(self.lib.kmx_canonical_windows(self._h, C.byref(r), _ptr(d_wo), k, _ptr(outs.get("fw")), _ptr(outs.get("rc")),
                                                _ptr(outs.get("canon")), _ptr(outs.get("flags"))))
        return outs

    @_on_ctx_stream
    def count_canonical(self, bases, n_reads, read_len, k, offsets=None, max_distinct=None):
        """kmx_count_canonical -> (kmers, counts): the distinct canonical k-mers of the batch in ascending order and how many
        windows yield each (int64 device tensors holding u64 words, trimmed to the number of distinct k-mers).  Without
        `max_distinct` the buffers are sized to the batch's window count; with it, KmxError (KMX_E_NOMEM) if there are more."""
        if max_distinct is None:
            max_distinct = self._max_windows(n_reads, read_len, k, offsets)
        kmers = self.empty(max(max_distinct, 1), torch.int64)
        counts = self.empty(max(max_distinct, 1), torch.int64)
        nd = C.c_uint64(0)
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(self.lib.kmx_count_canonical(self._h, C.byref(r), k, _ptr(kmers), _ptr(counts), int(max_distinct), C.byref(nd)))
        return kmers[:nd.value], counts[:nd.value]

    @_on_ctx_stream
    def count_merge(self, kmers_a, counts_a, kmers_b, counts_b, max_out=None):
        """kmx_count_merge -> (kmers, counts): the union of two tables of count_canonical, counts of equal k-mers added."""
        na, nb = int(kmers_a.numel()), int(kmers_b.numel())
        if max_out is None:
            max_out = na + nb
        kmers = self.empty(max(max_out, 1), torch.int64)
        counts = self.empty(max(max_out, 1), torch.int64)
        n = C.c_uint64(0)
        self._ck(self.lib.kmx_count_merge(self._h, _ptr(kmers_a) if na else None, _ptr(counts_a) if na else None, na,
                                          _ptr(kmers_b) if nb else None, _ptr(counts_b) if nb else None, nb, _ptr(kmers), _ptr(counts),
                                          int(max_out), C.byref(n)))
        return kmers[:n.value], counts[:n.value]

    def _max_windows(self, n_reads, read_len, k, offsets):
        if offsets is None:
            return int(n_reads) * max(int(read_len) - int(k) + 1, 0)
        lens = offsets[1:] - offsets[:-1]
        return int((lens - int(k) + 1).clamp_(min=0).sum().item()) if int(n_reads) > 0 else 0

    @_on_ctx_stream
    def count_canonical2(self, bases, n_reads, read_len, k, offsets=None, max_distinct=None):
        """kmx_count_canonical2 (k 33..64) -> (kmers, counts): the distinct canonical two-word k-mers of the batch, kmers int64[n, 2] =
        (low word, high word) holding u64 words, ascending as 2k-bit unsigned integers (high word first), and counts int64[n].
        Without `max_distinct` the buffers are sized to the batch's window count; with it, KmxError (KMX_E_NOMEM) if there are more."""
        if max_distinct is None:
            max_distinct = self._max_windows(n_reads, read_len, k, offsets)
        kmers = self.empty(2 * max(max_distinct, 1), torch.int64)
        counts = self.empty(max(max_distinct, 1), torch.int64)
        nd = C.c_uint64(0)
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(self.lib.kmx_count_canonical2(self._h, C.byref(r), k, _ptr(kmers), _ptr(counts), int(max_distinct), C.byref(nd)))
        return kmers[:2 * nd.value].view(-1, 2), counts[:nd.value]

    @_on_ctx_stream
    def count_merge2(self, kmers_a, counts_a, kmers_b, counts_b, max_out=None):
        """kmx_count_merge2 -> (kmers int64[n, 2], counts): the union of two tables of count_canonical2, counts of equal k-mers added."""
        na, nb = int(counts_a.numel()), int(counts_b.numel())
        if max_out is None:
            max_out = na + nb
        kmers_a, kmers_b = kmers_a.contiguous(), kmers_b.contiguous()
        kmers = self.empty(2 * max(max_out, 1), torch.int64)
        counts = self.empty(max(max_out, 1), torch.int64)
        n = C.c_uint64(0)
        self._ck(self.lib.kmx_count_merge2(self._h, _ptr(kmers_a) if na else None, _ptr(counts_a) if na else None, na,
                                           _ptr(kmers_b) if nb else None, _ptr(counts_b) if nb else None, nb, _ptr(kmers), _ptr(counts),
                                           int(max_out), C.byref(n)))
        return kmers[:2 * n.value].view(-1, 2), counts[:n.value]

    # ------------------------------------------------------------ set algebra and comparison of two count tables
    def _setop(self, fn, words, op, kmers_a, counts_a, kmers_b, counts_b, rule, max_out):
        na, nb = int(kmers_a.numel()) // words, int(kmers_b.numel()) // words
        kmers_a, kmers_b = kmers_a.contiguous(), kmers_b.contiguous()
        if max_out is None:
            max_out = min(na, nb) if op == SETOP_INTERSECT else na if op in (SETOP_SUBTRACT, SETOP_COUNTER_SUBTRACT) else na + nb
        ok = self.empty(words * max(max_out, 1), torch.int64)
        oc = self.empty(max(max_out, 1), torch.int64)
        n = C.c_uint64(0)
        self._ck(fn(self._h, int(op), int(rule), _ptr(kmers_a) if na else None, _ptr(counts_a) if counts_a is not None and na else None, na,
                    _ptr(kmers_b) if nb else None, _ptr(counts_b) if counts_b is not None and nb else None, nb, _ptr(ok), _ptr(oc), int(max_out),
                    C.byref(n)))
        ok = ok[:words * n.value]
        return (ok.view(-1, 2) if words == 2 else ok), oc[:n.value]

    @_on_ctx_stream
    def count_setop(self, op, kmers_a, counts_a, kmers_b, counts_b, rule=RULE_SUM, max_out=None):
        """kmx_count_setop -> (kmers, counts): SETOP_INTERSECT / UNION / SUBTRACT / SYMDIFF / COUNTER_SUBTRACT of two count tables, a
        table again.  `rule` (RULE_SUM / MIN / MAX / LEFT / RIGHT) is the count of a key both tables hold, for INTERSECT and UNION;
        the other operations take none (0).  A count tensor the operation never reads may be None (counts_b for SUBTRACT and
        INTERSECT / LEFT, counts_a for INTERSECT / RIGHT).  Without `max_out` the outputs are sized to the operation's own bound."""
        return self._setop(self.lib.kmx_count_setop, 1, op, kmers_a, counts_a, kmers_b, counts_b, rule, max_out)

    @_on_ctx_stream
    def count_setop2(self, op, kmers_a, counts_a, kmers_b, counts_b, rule=RULE_SUM, max_out=None):
        """kmx_count_setop2 (k 33..64): kmers int64[n, 2] = (low, high) words -> (kmers int64[n_out, 2], counts)."""
        return self._setop(self.lib.kmx_count_setop2, 2, op, kmers_a, counts_a, kmers_b, counts_b, rule, max_out)

    def count_intersect(self, kmers_a, counts_a, kmers_b, counts_b, rule=RULE_SUM, max_out=None):
        return self.count_setop(SETOP_INTERSECT, kmers_a, counts_a, kmers_b, counts_b, rule, max_out)

    def count_intersect2(self, kmers_a, counts_a, kmers_b, counts_b, rule=RULE_SUM, max_out=None):
        return self.count_setop2(SETOP_INTERSECT, kmers_a, counts_a, kmers_b, counts_b, rule, max_out)

    def count_union(self, kmers_a, counts_a, kmers_b, counts_b, rule=RULE_SUM, max_out=None):
        return self.count_setop(SETOP_UNION, kmers_a, counts_a, kmers_b, counts_b, rule, max_out)

    def count_union2(self, kmers_a, counts_a, kmers_b, counts_b, rule=RULE_SUM, max_out=None):
        return self.count_setop2(SETOP_UNION, kmers_a, counts_a, kmers_b, counts_b, rule, max_out)

    def count_subtract(self, kmers_a, counts_a, kmers_b, counts_b=None, max_out=None):
        """the entries of a whose key b does not hold (counts_b is not read)"""
        return self.count_setop(SETOP_SUBTRACT, kmers_a, counts_a, kmers_b, counts_b, 0, max_out)

    def count_subtract2(self, kmers_a, counts_a, kmers_b, counts_b=None, max_out=None):
        return self.count_setop2(SETOP_SUBTRACT, kmers_a, counts_a, kmers_b, counts_b, 0, max_out)

    def count_symdiff(self, kmers_a, counts_a, kmers_b, counts_b, max_out=None):
        return self.count_setop(SETOP_SYMDIFF, kmers_a, counts_a, kmers_b, counts_b, 0, max_out)

    def count_symdiff2(self, kmers_a, counts_a, kmers_b, counts_b, max_out=None):
        return self.count_setop2(SETOP_SYMDIFF, kmers_a, counts_a, kmers_b, counts_b, 0, max_out)

    def count_counter_subtract(self, kmers_a, counts_a, kmers_b, counts_b, max_out=None):
        """a's entries with b's counts taken off; a key is dropped where count_a <= count_b"""
        return self.count_setop(SETOP_COUNTER_SUBTRACT, kmers_a, counts_a, kmers_b, counts_b, 0, max_out)

    def count_counter_subtract2(self, kmers_a, counts_a, kmers_b, counts_b, max_out=None):
        return self.count_setop2(SETOP_COUNTER_SUBTRACT, kmers_a, counts_a, kmers_b, counts_b, 0, max_out)

    def _compare(self, fn, words, kmers_a, counts_a, kmers_b, counts_b):
        na, nb = int(kmers_a.numel()) // words, int(kmers_b.numel()) // words
        kmers_a, kmers_b = kmers_a.contiguous(), kmers_b.contiguous()
        rec = TableCompare()
        self._ck(fn(self._h, _ptr(kmers_a) if na else None, _ptr(counts_a) if counts_a is not None and na else None, na,
                    _ptr(kmers_b) if nb else None, _ptr(counts_b) if counts_b is not None and nb else None, nb, C.byref(rec)))
        return TableComparison(*[int(getattr(rec, f)) for f, _ in TableCompare._fields_])

    @_on_ctx_stream
    def count_compare(self, kmers_a, counts_a, kmers_b, counts_b):
        """kmx_count_compare -> TableComparison: keys shared / only in a / only in b and the sums of counts behind Jaccard,
        containment and weighted Jaccard.  Both count tensors None: the key sets alone (the sums are 0)."""
        return self._compare(self.lib.kmx_count_compare, 1, kmers_a, counts_a, kmers_b, counts_b)

    @_on_ctx_stream
    def count_compare2(self, kmers_a, counts_a, kmers_b, counts_b):
        """kmx_count_compare2 (k 33..64): kmers int64[n, 2]."""
        return self._compare(self.lib.kmx_count_compare2, 2, kmers_a, counts_a, kmers_b, counts_b)

    # ------------------------------------------------------------ queries on a count table
    def _lookup(self, fn, words, kmers, counts, k, query, flags, out):
        n = int(kmers.numel()) // words
        nq = int(query.numel()) // words
        kmers, query = kmers.contiguous(), query.contiguous()
        if out is None:
            out = self.empty(nq, torch.int64)
        self._ck(fn(self._h, _ptr(kmers) if n else None, _ptr(counts) if counts is not None and n else None, n, k,
                    _ptr(query) if nq else None, _ptr(flags) if flags is not None and nq else None, nq, _ptr(out) if nq else None))
        return out

    @_on_ctx_stream
    def count_lookup(self, kmers, counts, k, query, flags=None, out=None):
        """kmx_count_lookup -> int64[n_query] (u64 words): the count of every query word in the table (kmers, counts) of
        count_canonical / count_merge / count_filter, 0 where it is absent or its flag lacks KMX_WIN_VALID.  counts=None: membership
        (1 / 0).  `out` may be `query` itself: answers in place."""
        return self._lookup(self.lib.kmx_count_lookup, 1, kmers, counts, k, query, flags, out)

    @_on_ctx_stream
    def count_lookup2(self, kmers, counts, k, query, flags=None, out=None):
        """kmx_count_lookup2 (k 33..64): kmers int64[n, 2], query int64[n_query, 2] = (low, high) words -> int64[n_query]."""
        return self._lookup(self.lib.kmx_count_lookup2, 2, kmers, counts, k, query, flags, out)

    def _lookup_reads(self, fn, words, bases, n_reads, read_len, k, kmers, counts, offsets, win_offsets, out):
        n = int(kmers.numel()) // words
        kmers = kmers.contiguous()
        if offsets is not None and win_offsets is None:
            lens = offsets[1:] - offsets[:-1]
            w = (lens - int(k) + 1).clamp_(min=0)
            w[lens > 0x7FFFFFFF] = 0
            win_offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), torch.cumsum(w, 0)])
        if out is None:
            total = int(win_offsets[-1].item()) if win_offsets is not None else int(n_reads) * max(int(read_len) - int(k) + 1, 0)
            out = self.empty(total, torch.int64)
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(fn(self._h, C.byref(r), _ptr(win_offsets), k, _ptr(kmers) if n else None,
                    _ptr(counts) if counts is not None and n else None, n, _ptr(out) if out.numel() else None))
        return out

    @_on_ctx_stream
    def count_lookup_reads(self, bases, n_reads, read_len, k, kmers, counts, offsets=None, win_offsets=None, out=None):
        """kmx_count_lookup_reads -> int64[windows]: the count, in the table, of the canonical k-mer of every window of the batch, in
        the slot layout of canonical_windows; 0 for a window with an invalid byte.  Ragged reads: `win_offsets` (device, n_reads + 1)
        is made from `offsets` when not given."""
        return self._lookup_reads(self.lib.kmx_count_lookup_reads, 1, bases, n_reads, read_len, k, kmers, counts, offsets, win_offsets, out)

    @_on_ctx_stream
    def count_lookup_reads2(self, bases, n_reads, read_len, k, kmers, counts, offsets=None, win_offsets=None, out=None):
        """kmx_count_lookup_reads2 (k 33..64; kmers int64[n, 2]) -> int64[windows]."""
        return self._lookup_reads(self.lib.kmx_count_lookup_reads2, 2, bases, n_reads, read_len, k, kmers, counts, offsets, win_offsets, out)

    def _read_stats(self, fn, words, bases, n_reads, read_len, k, kmers, counts, solid_min, offsets, out):
        n = int(kmers.numel()) // words if kmers is not None else 0
        if n:
            kmers = kmers.contiguous()
        if out is None:
            out = self.empty(RS_WORDS * int(n_reads), torch.int64)
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(fn(self._h, C.byref(r), k, _ptr(kmers) if n else None, _ptr(counts) if counts is not None and n else None, n,
                    int(solid_min), _ptr(out) if out.numel() else None))
        return out.view(-1, RS_WORDS)

    @_on_ctx_stream
    def count_read_stats(self, bases, n_reads, read_len, k, kmers, counts, solid_min=2, offsets=None, out=None):
        """kmx_count_read_stats -> int64[n_reads, 8] (u64 words, columns _lib.RS_*): per read, over the counts its windows have in
        the table (kmers, counts) -- valid / present / solid (count >= solid_min) windows, min, max, sum, upper median, and the
        longest run of solid windows (column RS_SPAN: read_stats_span decodes it).  counts=None: membership (1 / 0).  Ragged reads
        (`offsets`) need no window offsets.  `out` (int64, 8 * n_reads elements) is overwritten: every row is written."""
        return self._read_stats(self.lib.kmx_count_read_stats, 1, bases, n_reads, read_len, k, kmers, counts, solid_min, offsets, out)

    @_on_ctx_stream
    def count_read_stats2(self, bases, n_reads, read_len, k, kmers, counts, solid_min=2, offsets=None, out=None):
        """kmx_count_read_stats2 (k 33..64; kmers int64[n, 2]) -> int64[n_reads, 8]."""
        return self._read_stats(self.lib.kmx_count_read_stats2, 2, bases, n_reads, read_len, k, kmers, counts, solid_min, offsets, out)

    def _correct_reads(self, fn, words, bases, n_reads, read_len, k, kmers, counts, solid_min, min_cover, offsets, out):
        n = int(kmers.numel()) // words if kmers is not None else 0
        if n:
            kmers = kmers.contiguous()
        if out is None:
            out = bases.clone()   # (the call writes the bytes of the reads only: what lies around them in `bases` is kept)
        fixes = self.empty(CR_WORDS * int(n_reads), torch.int64)
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(fn(self._h, C.byref(r), k, _ptr(kmers) if n else None, _ptr(counts) if counts is not None and n else None, n,
                    int(solid_min), int(min_cover), _ptr(out) if out.numel() else None, _ptr(fixes) if fixes.numel() else None))
        return out, fixes.view(-1, CR_WORDS)

    @_on_ctx_stream
    def count_correct_reads(self, bases, n_reads, read_len, k, kmers, counts, solid_min=2, min_cover=1, offsets=None, out=None):
        """kmx_count_correct_reads -> (corrected uint8 tensor shaped like `bases`, int64[n_reads, 4] (u64 words, columns _lib.CR_*)):
        substitution errors repaired against the table (kmers, counts).  A base that no solid window (count >= solid_min) covers, but
        at least `min_cover` valid ones do, is replaced when exactly one other base makes all of those windows solid; two or three such
        bases leave it as it is (counted in CR_N_AMBIGUOUS).  Decisions are taken against the original bytes, so `out` (uint8, addressed
        as `bases`) must not overlap `bases`; the bytes of the reads are all written -- ragged reads (`offsets`): the bytes
        [offsets[0], offsets[n_reads]) and nothing else; without `out` the result starts as a copy of `bases`.  counts=None: membership."""
        return self._correct_reads(self.lib.kmx_count_correct_reads, 1, bases, n_reads, read_len, k, kmers, counts, solid_min, min_cover, offsets, out)

    @_on_ctx_stream
    def count_correct_reads2(self, bases, n_reads, read_len, k, kmers, counts, solid_min=2, min_cover=1, offsets=None, out=None):
        """kmx_count_correct_reads2 (k 33..64; kmers int64[n, 2]) -> (corrected bases, int64[n_reads, 4])."""
        return self._correct_reads(self.lib.kmx_count_correct_reads2, 2, bases, n_reads, read_len, k, kmers, counts, solid_min, min_cover, offsets, out)

    # ------------------------------------------------------------ coloured tables: more than two samples at once
    def _color_add(self, words, table, kmers_b, color, k):
        taken = table.n_colors if table is not None else 0
        if color is None:
            color = taken
        color = int(color)
        if color >= 64:
            raise ValueError(f"colour {color}: a coloured table holds at most 64 colours (0 .. 63)")
        if color < taken:
            raise ValueError(f"colour {color} may already be set in a table of {taken} colours")
        if k is None and table is not None:
            k = table.k
        kmers_b = kmers_b.contiguous()
        nb = int(kmers_b.numel()) // words
        # (colour 63 is the sign bit of the int64 that holds the u64 mask)
        cb = torch.full((nb,), (1 << color) - (1 << 64 if color == 63 else 0), dtype=torch.int64, device=self.device)
        if table is None:
            return ColorTable(kmers_b.clone(), cb, color + 1, k)
        # (RULE_SUM is OR here: the bit is clear in every mask of the table)
        kmers, colors = self._setop(self.lib.kmx_count_setop2 if words == 2 else self.lib.kmx_count_setop, words, SETOP_UNION, table.kmers,
                                    table.colors, kmers_b, cb, RULE_SUM, None)
        return ColorTable(kmers, colors, color + 1, k)

    @_on_ctx_stream
    def count_color_add(self, table, kmers_b, color=None, k=None):
        """-> ColorTable: the union of the coloured `table` (None: an empty one) with sample b's key set (the sorted distinct keys of a
        table), b's entries getting bit `color` (default: the next free one, table.n_colors).  Built from kmx_count_setop (UNION,
        RULE_SUM) on a filled tensor of 1 << color.  ValueError for a colour at or above 64, or below table.n_colors (that bit may
        already be set).  The result has n_colors = color + 1."""
        return self._color_add(1, table, kmers_b, color, k)

    @_on_ctx_stream
    def count_color_add2(self, table, kmers_b, color=None, k=None):
        """count_color_add for two-word keys (k 33..64): kmers_b int64[n, 2]."""
        return self._color_add(2, table, kmers_b, color, k)

    def count_color_build(self, tables, k=None):
        """-> ColorTable of a list of (kmers, counts) tables, colour i = the list index (the counts are not read: filter each table with
        count_filter first for a presence threshold).  At most 64 tables."""
        table = None
        for kmers, _ in tables:
            table = self.count_color_add(table, kmers, k=k)
        return table

    def count_color_build2(self, tables, k=None):
        table = None
        for kmers, _ in tables:
            table = self.count_color_add2(table, kmers, k=k)
        return table

    @_on_ctx_stream
    def count_color_matrix(self, colors, n_colors, spectrum=True):
        """kmx_count_color_matrix -> ColorMatrix: for all pairs of the n_colors samples, how many entries of the coloured table hold
        both (shared int64[n_colors, n_colors]), and, unless spectrum=False, how many entries hold exactly j colours.  Only the low
        n_colors bits of a mask count.  One call for both key widths (it reads the masks only)."""
        n, nc = int(colors.numel()), int(n_colors)
        shared = self.empty(max(nc, 0) ** 2, torch.int64)
        spec = self.empty(max(nc, 0) + 1, torch.int64) if spectrum else None
        self._ck(self.lib.kmx_count_color_matrix(self._h, _ptr(colors) if n else None, n, nc, _ptr(shared) if shared.numel() else None, _ptr(spec)))
        return ColorMatrix(shared.view(nc, nc), spec)

    def _read_colors(self, fn, words, bases, n_reads, read_len, k, kmers, colors, n_colors, threshold, offsets, hits, out):
        n = int(kmers.numel()) // words if kmers is not None else 0
        if n:
            kmers = kmers.contiguous()
        if out is None:
            out = self.empty(RC_WORDS * int(n_reads), torch.int64)
        h = self.empty(max(int(n_colors), 0) * int(n_reads), torch.int32) if hits else None
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(fn(self._h, C.byref(r), k, _ptr(kmers) if n else None, _ptr(colors) if colors is not None and n else None, n, int(n_colors),
                    int(threshold[0]), int(threshold[1]), _ptr(out) if out.numel() else None, _ptr(h) if h is not None and h.numel() else None))
        return out.view(-1, RC_WORDS), (h.view(int(n_reads), -1) if h is not None else None)

    @_on_ctx_stream
    def count_read_colors(self, bases, n_reads, read_len, k, kmers, colors, n_colors, threshold=(1, 2), offsets=None, hits=False, out=None):
        """kmx_count_read_colors -> (int64[n_reads, 8] (u64 words, columns _lib.RC_*), int32[n_reads, n_colors] or None): per read,
        which samples of the coloured table (kmers, colors) it is compatible with -- valid / hit / single-colour windows, the AND and the
        OR of its hit windows' masks, the colours that at least threshold = (num, den) of its valid windows carry, the best colour with
        its hit count, and how often the mask changes between neighbouring hit windows; with hits=True also the hit windows per
        colour.  Ragged reads (`offsets`) need no window offsets.  `out` (int64, 8 * n_reads elements) is overwritten."""
        return self._read_colors(self.lib.kmx_count_read_colors, 1, bases, n_reads, read_len, k, kmers, colors, n_colors, threshold, offsets, hits, out)

    @_on_ctx_stream
    def count_read_colors2(self, bases, n_reads, read_len, k, kmers, colors, n_colors, threshold=(1, 2), offsets=None, hits=False, out=None):
        """kmx_count_read_colors2 (k 33..64; kmers int64[n, 2]) -> (int64[n_reads, 8], int32[n_reads, n_colors] or None)."""
        return self._read_colors(self.lib.kmx_count_read_colors2, 2, bases, n_reads, read_len, k, kmers, colors, n_colors, threshold, offsets, hits, out)

    @_on_ctx_stream
    def count_spectrum(self, counts, n_bins, out=None):
        """kmx_count_spectrum -> int64[n_bins]: out[min(count, n_bins - 1)] += 1 for every entry; zeroed bins unless handed some
        (they are accumulated into)."""
        if out is None:
            out = torch.zeros(int(n_bins), dtype=torch.int64, device=self.device)
        n = int(counts.numel())
        self._ck(self.lib.kmx_count_spectrum(self._h, _ptr(counts) if n else None, n, int(n_bins), _ptr(out)))
        return out

    def _filter(self, fn, words, kmers, counts, min_count, max_count, max_out):
        n = int(counts.numel())
        kmers = kmers.contiguous()
        if max_out is None:
            max_out = n
        ok = self.empty(words * max(max_out, 1), torch.int64)
        oc = self.empty(max(max_out, 1), torch.int64)
        m = C.c_uint64(0)
        self._ck(fn(self._h, _ptr(kmers) if n else None, _ptr(counts) if n else None, n, int(min_count), int(max_count), _ptr(ok), _ptr(oc),
                    int(max_out), C.byref(m)))
        ok = ok[:words * m.value]
        return (ok.view(-1, 2) if words == 2 else ok), oc[:m.value]

    @_on_ctx_stream
    def count_filter(self, kmers, counts, min_count=1, max_count=2**64 - 1, max_out=None):
        """kmx_count_filter -> (kmers, counts): the entries with min_count <= count <= max_count, order kept (a table again)."""
        return self._filter(self.lib.kmx_count_filter, 1, kmers, counts, min_count, max_count, max_out)

    @_on_ctx_stream
    def count_filter2(self, kmers, counts, min_count=1, max_count=2**64 - 1, max_out=None):
        """kmx_count_filter2 -> (kmers int64[n, 2], counts) for the tables of count_canonical2."""
        return self._filter(self.lib.kmx_count_filter2, 2, kmers, counts, min_count, max_count, max_out)

    # ------------------------------------------------------------ the counting sketch
    @_on_ctx_stream
    def sketch_new(self, log2_blocks, seed=0) -> Sketch:
        """a zeroed sketch of 2^log2_blocks blocks of 64 bytes"""
        if not 0 <= int(log2_blocks) <= _lib.SKETCH_MAX_LOG2_BLOCKS:
            raise ValueError("log2_blocks outside 0..32")
        cells = torch.zeros(_lib.SKETCH_BLOCK_BYTES << int(log2_blocks), dtype=torch.uint8, device=self.device)
        return Sketch(cells, int(log2_blocks), int(seed) & (2**64 - 1), self)

    def _sketch_args(self, sketch):
        return _ptr(sketch.cells), int(sketch.log2_blocks), int(sketch.seed)

    def _sketch_add(self, fn, sketch, bases, n_reads, read_len, k, offsets):
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(fn(self._h, C.byref(r), k, *self._sketch_args(sketch)))
        return sketch

    @_on_ctx_stream
    def sketch_add(self, sketch, bases, n_reads, read_len, k, offsets=None) -> Sketch:
        """kmx_sketch_add: weight 1 for every valid window of the batch, accumulated into `sketch` (returned)."""
        return self._sketch_add(self.lib.kmx_sketch_add, sketch, bases, n_reads, read_len, k, offsets)

    @_on_ctx_stream
    def sketch_add2(self, sketch, bases, n_reads, read_len, k, offsets=None) -> Sketch:
        """kmx_sketch_add2 (k 33..64)."""
        return self._sketch_add(self.lib.kmx_sketch_add2, sketch, bases, n_reads, read_len, k, offsets)

    def _sketch_add_words(self, fn, words, sketch, keys, weights):
        n = int(keys.numel()) // words
        keys = keys.contiguous()
        self._ck(fn(self._h, _ptr(keys) if n else None, _ptr(weights) if weights is not None and n else None, n, *self._sketch_args(sketch)))
        return sketch

    @_on_ctx_stream
    def sketch_add_words(self, sketch, words, weights=None) -> Sketch:
        """kmx_sketch_add_words: the keys as they are (int64 holding u64 words), each with its weight (int64 holding u64, clipped to
        255) or 1: a table with its counts, or the canon array of canonical_windows."""
        return self._sketch_add_words(self.lib.kmx_sketch_add_words, 1, sketch, words, weights)

    @_on_ctx_stream
    def sketch_add_words2(self, sketch, words, weights=None) -> Sketch:
        """kmx_sketch_add_words2: words int64[n, 2] = (low, high)."""
        return self._sketch_add_words(self.lib.kmx_sketch_add_words2, 2, sketch, words, weights)

    def _sketch_lookup(self, fn, words, sketch, keys, out):
        n = int(keys.numel()) // words
        keys = keys.contiguous()
        if out is None:
            out = self.empty(n, torch.uint8)
        self._ck(fn(self._h, _ptr(keys) if n else None, n, *self._sketch_args(sketch), _ptr(out) if n else None))
        return out

    @_on_ctx_stream
    def sketch_lookup(self, sketch, words, out=None):
        """kmx_sketch_lookup -> uint8[n]: the estimate of every key, never below min(255, its true total)."""
        return self._sketch_lookup(self.lib.kmx_sketch_lookup, 1, sketch, words, out)

    @_on_ctx_stream
    def sketch_lookup2(self, sketch, words, out=None):
        """kmx_sketch_lookup2: words int64[n, 2] -> uint8[n]."""
        return self._sketch_lookup(self.lib.kmx_sketch_lookup2, 2, sketch, words, out)

    def _sketch_lookup_reads(self, fn, sketch, bases, n_reads, read_len, k, offsets, win_offsets, out):
        if offsets is not None and win_offsets is None:
            lens = offsets[1:] - offsets[:-1]
            w = (lens - int(k) + 1).clamp_(min=0)
            w[lens > 0x7FFFFFFF] = 0
            win_offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), torch.cumsum(w, 0)])
        if out is None:
            total = int(win_offsets[-1].item()) if win_offsets is not None else int(n_reads) * max(int(read_len) - int(k) + 1, 0)
            out = self.empty(total, torch.uint8)
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(fn(self._h, C.byref(r), _ptr(win_offsets), k, *self._sketch_args(sketch), _ptr(out) if out.numel() else None))
        return out

    @_on_ctx_stream
    def sketch_lookup_reads(self, sketch, bases, n_reads, read_len, k, offsets=None, win_offsets=None, out=None):
        """kmx_sketch_lookup_reads -> uint8[windows]: the estimate of the canonical k-mer of every window of the batch, in the slot
        layout of canonical_windows; 0 for a window with an invalid byte.  Ragged reads: `win_offsets` is made from `offsets` when
        not given."""
        return self._sketch_lookup_reads(self.lib.kmx_sketch_lookup_reads, sketch, bases, n_reads, read_len, k, offsets, win_offsets, out)

    @_on_ctx_stream
    def sketch_lookup_reads2(self, sketch, bases, n_reads, read_len, k, offsets=None, win_offsets=None, out=None):
        """kmx_sketch_lookup_reads2 (k 33..64)."""
        return self._sketch_lookup_reads(self.lib.kmx_sketch_lookup_reads2, sketch, bases, n_reads, read_len, k, offsets, win_offsets, out)

    @_on_ctx_stream
    def sketch_merge(self, a: Sketch, b: Sketch, out: "Sketch | None" = None) -> Sketch:
        """kmx_sketch_merge -> the cellwise saturating sum of two sketches of one size and seed; `out` may be `a` or `b`."""
        if a.log2_blocks != b.log2_blocks or a.seed != b.seed:
            raise ValueError("sketches of different size or seed do not merge")
        if out is None:
            out = Sketch(self.empty(a.cells.numel(), torch.uint8), a.log2_blocks, a.seed, self)
        elif out.log2_blocks != a.log2_blocks or out.seed != a.seed:
            raise ValueError("sketches of different size or seed do not merge")
        self._ck(self.lib.kmx_sketch_merge(self._h, _ptr(a.cells), _ptr(b.cells), a.log2_blocks, _ptr(out.cells)))
        return out

    @_on_ctx_stream
    def sketch_stats(self, sketch: Sketch, out=None):
        """kmx_sketch_stats -> int64[256]: how many cells hold each value; zeroed bins unless handed some (they are accumulated into)."""
        if out is None:
            out = torch.zeros(256, dtype=torch.int64, device=self.device)
        self._ck(self.lib.kmx_sketch_stats(self._h, _ptr(sketch.cells), int(sketch.log2_blocks), _ptr(out)))
        return out

    def _count_min(self, fn, words, sketch, min_est, bases, n_reads, read_len, k, offsets, max_distinct, count_only):
        nd = C.c_uint64(0)
        r = self._reads(bases, n_reads, read_len, offsets)
        if count_only:
            self._ck(fn(self._h, C.byref(r), k, *self._sketch_args(sketch), int(min_est), None, None, 0, C.byref(nd)))
            return int(nd.value)
        if max_distinct is None:
            max_distinct = self._max_windows(n_reads, read_len, k, offsets)
        kmers = self.empty(words * max(max_distinct, 1), torch.int64)
        counts = self.empty(max(max_distinct, 1), torch.int64)
        self._ck(fn(self._h, C.byref(r), k, *self._sketch_args(sketch), int(min_est), _ptr(kmers), _ptr(counts), int(max_distinct), C.byref(nd)))
        kmers = kmers[:words * nd.value]
        return (kmers.view(-1, 2) if words == 2 else kmers), counts[:nd.value]

    @_on_ctx_stream
    def count_canonical_min(self, sketch, min_est, bases, n_reads, read_len, k, offsets=None, max_distinct=None, count_only=False):
        """kmx_count_canonical_min -> (kmers, counts) as count_canonical, of the windows whose estimate in `sketch` is >= min_est
        (0..2^32 - 1; above 255: the empty table).  count_only: the number of distinct k-mers, nothing written."""
        return self._count_min(self.lib.kmx_count_canonical_min, 1, sketch, min_est, bases, n_reads, read_len, k, offsets, max_distinct, count_only)

    @_on_ctx_stream
    def count_canonical_min2(self, sketch, min_est, bases, n_reads, read_len, k, offsets=None, max_distinct=None, count_only=False):
        """kmx_count_canonical_min2 (k 33..64) -> (kmers int64[n, 2], counts)."""
        return self._count_min(self.lib.kmx_count_canonical_min2, 2, sketch, min_est, bases, n_reads, read_len, k, offsets, max_distinct, count_only)

    @staticmethod
    def _batch_args(b):
        if isinstance(b, ReadBatch):
            return b.bases, b.n_reads, b.max_len(), b.offsets
        bases, n_reads, read_len, offsets = b
        return bases, n_reads, read_len, offsets

    def _count_solid(self, words, batches, k, min_count, log2_blocks, seed, tables):
        if not 1 <= int(min_count) <= 255:
            raise ValueError("min_count outside 1..255: a cell of the sketch counts to 255")
        add, count, merge, flt = ((self.sketch_add, self.count_canonical_min, self.count_merge, self.count_filter) if words == 1 else
                                  (self.sketch_add2, self.count_canonical_min2, self.count_merge2, self.count_filter2))
        if log2_blocks is None:   # one more pass: the distinct k-mers of all batches, and the sketch they fill to a quarter
            hll, hll_add = self.hll_new(seed=seed), (self.hll_add if words == 1 else self.hll_add2)
            for b in batches:
                bases, n_reads, read_len, offsets = self._batch_args(b)
                hll_add(hll, bases, n_reads, read_len, k, offsets=offsets)
            log2_blocks = hll.sketch_log2_blocks()
        sketch = self.sketch_new(log2_blocks, seed)
        for b in batches:
            bases, n_reads, read_len, offsets = self._batch_args(b)
            add(sketch, bases, n_reads, read_len, k, offsets=offsets)
        kmers = self.empty(0, torch.int64).view(-1, 2) if words == 2 else self.empty(0, torch.int64)
        counts = self.empty(0, torch.int64)
        for b in batches:
            bases, n_reads, read_len, offsets = self._batch_args(b)
            bk, bc = count(sketch, int(min_count), bases, n_reads, read_len, k, offsets=offsets)
            if tables is not None:
                tables.append(int(bc.numel()))
            kmers, counts = merge(kmers, counts, bk, bc)
        kmers, counts = flt(kmers, counts, int(min_count), 2**64 - 1)
        return kmers, counts, sketch

    def count_solid(self, batches, k, min_count, log2_blocks=None, seed=0, tables=None):
        """The k-mers that occur at least `min_count` (1..255) times in all of `batches` together, counted without ever holding the
        rest: (kmers, counts, sketch).  `batches`: a sequence, iterable twice, of (bases, n_reads, read_len, offsets) or ReadBatch.
        Pass 1 adds every batch to one sketch of 2^log2_blocks blocks; pass 2 counts, per batch, the windows whose estimate reaches
        min_count (count_canonical_min), folds the tables with count_merge and keeps the entries of at least min_count
        (count_filter).  Equal, key for key and count for count, to count_filter of the count of all reads at once -- for any
        sketch size: a small sketch only lets more through.  `tables`, a list: the size of every batch's table is appended.
        log2_blocks = None: one more pass over `batches` first (hll_add into 2^14 registers), and the sketch is the smallest that
        the estimated distinct k-mers fill to at most a quarter (Hll.sketch_log2_blocks)."""
        return self._count_solid(1, batches, k, min_count, log2_blocks, seed, tables)

    def count_solid2(self, batches, k, min_count, log2_blocks=None, seed=0, tables=None):
        """count_solid for k 33..64 (kmers int64[n, 2])."""
        return self._count_solid(2, batches, k, min_count, log2_blocks, seed, tables)

    # ------------------------------------------------------------ the distinct-key estimator
    @_on_ctx_stream
    def hll_new(self, log2_regs=14, seed=0) -> Hll:
        """zeroed HyperLogLog registers, 2^log2_regs bytes (4..24): a relative standard error of about 1.04 / sqrt(2^log2_regs)"""
        if not _lib.HLL_MIN_LOG2_REGS <= int(log2_regs) <= _lib.HLL_MAX_LOG2_REGS:
            raise ValueError("log2_regs outside 4..24")
        regs = torch.zeros(1 << int(log2_regs), dtype=torch.uint8, device=self.device)
        return Hll(regs, int(log2_regs), int(seed) & (2**64 - 1), self)

    def _hll_args(self, hll):
        return _ptr(hll.regs), int(hll.log2_regs), int(hll.seed)

    def _hll_add(self, fn, hll, bases, n_reads, read_len, k, offsets):
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(fn(self._h, C.byref(r), k, *self._hll_args(hll)))
        return hll

    @_on_ctx_stream
    def hll_add(self, hll, bases, n_reads, read_len, k, offsets=None) -> Hll:
        """kmx_hll_add: every valid window of the batch, accumulated into `hll` (returned)."""
        return self._hll_add(self.lib.kmx_hll_add, hll, bases, n_reads, read_len, k, offsets)

    @_on_ctx_stream
    def hll_add2(self, hll, bases, n_reads, read_len, k, offsets=None) -> Hll:
        """kmx_hll_add2 (k 33..64)."""
        return self._hll_add(self.lib.kmx_hll_add2, hll, bases, n_reads, read_len, k, offsets)

    def _hll_add_words(self, fn, words, hll, keys):
        n = int(keys.numel()) // words
        keys = keys.contiguous()
        self._ck(fn(self._h, _ptr(keys) if n else None, n, *self._hll_args(hll)))
        return hll

    @_on_ctx_stream
    def hll_add_words(self, hll, words) -> Hll:
        """kmx_hll_add_words: the keys as they are (int64 holding u64 words): a table's keys, or the canon array of canonical_windows."""
        return self._hll_add_words(self.lib.kmx_hll_add_words, 1, hll, words)

    @_on_ctx_stream
    def hll_add_words2(self, hll, words) -> Hll:
        """kmx_hll_add_words2: words int64[n, 2] = (low, high)."""
        return self._hll_add_words(self.lib.kmx_hll_add_words2, 2, hll, words)

    @_on_ctx_stream
    def hll_merge(self, a: Hll, b: Hll, out: "Hll | None" = None) -> Hll:
        """kmx_hll_merge -> the bytewise maximum of two register arrays of one size and seed, the registers of the union of what they
        saw; `out` may be `a` or `b`."""
        if a.log2_regs != b.log2_regs or a.seed != b.seed:
            raise ValueError("registers of different size or seed do not merge")
        if out is None:
            out = Hll(self.empty(a.regs.numel(), torch.uint8), a.log2_regs, a.seed, self)
        elif out.log2_regs != a.log2_regs or out.seed != a.seed:
            raise ValueError("registers of different size or seed do not merge")
        self._ck(self.lib.kmx_hll_merge(self._h, _ptr(a.regs), _ptr(b.regs), a.log2_regs, _ptr(out.regs)))
        return out

    @_on_ctx_stream
    def hll_stats(self, a: Hll, b: "Hll | None" = None, out=None):
        """kmx_hll_stats -> int64[64]: how many registers of `a` hold each value; with `b` int64[192]: the bins of a, of b and of
        max(a, b).  Zeroed bins unless handed some (they are accumulated into)."""
        if b is not None and (a.log2_regs != b.log2_regs or a.seed != b.seed):
            raise ValueError("registers of different size or seed do not compare")
        if out is None:
            out = torch.zeros(_lib.HLL_BINS * (3 if b is not None else 1), dtype=torch.int64, device=self.device)
        self._ck(self.lib.kmx_hll_stats(self._h, _ptr(a.regs), _ptr(b.regs) if b is not None else None, int(a.log2_regs), _ptr(out)))
        return out

    def hll_compare(self, a: Hll, b: Hll) -> HllComparison:
        """The estimated sizes of two samples, their union and their intersection, with Jaccard index and containment, from one
        kmx_hll_stats over both register arrays (one host round trip)."""
        h = self.hll_stats(a, b).cpu().view(3, _lib.HLL_BINS)
        return HllComparison(*(hll_estimate(h[j], a.log2_regs) for j in range(3)))

    # ------------------------------------------------------------ a count table as a de Bruijn graph
    def _adjacency(self, fn, words, kmers, counts, k, min_count, flips, neighbors):
        n = int(kmers.numel()) // words
        kmers = kmers.contiguous()
        edges = self.empty(n, torch.uint8)
        fl = self.empty(n, torch.uint8) if flips else None
        nb = self.empty(8 * n, torch.int64) if neighbors else None
        self._ck(fn(self._h, _ptr(kmers) if n else None, _ptr(counts) if counts is not None and n else None, n, k, int(min_count),
                    _ptr(edges) if n else None, _ptr(fl) if n else None, _ptr(nb) if n else None))
        out = (edges,) + ((fl,) if flips else ()) + ((nb.view(-1, 8),) if neighbors else ())
        return out if len(out) > 1 else edges

    @_on_ctx_stream
    def count_adjacency(self, kmers, counts, k, min_count=1, flips=False, neighbors=False):
        """kmx_count_adjacency -> edges uint8[n][, flips uint8[n]][, nbr int64[n, 8]]: the table (kmers, counts) as the node set of a de
        Bruijn graph.  Bit c of edges[i] = the successor of entry i that ends in base c is a present entry, bit 4 + c = the predecessor
        that starts with base c is; the same bit of flips[i] = that neighbour is stored as the reverse complement of the word as
        spelled on entry i's strand; nbr[i, e] = its table index, -1 (the u64 KMX_NO_ENTRY) where there is no edge.  An entry is
        present if its count is at least min_count (counts=None: every entry is).  k 2..31."""
        return self._adjacency(self.lib.kmx_count_adjacency, 1, kmers, counts, k, min_count, flips, neighbors)

    @_on_ctx_stream
    def count_adjacency2(self, kmers, counts, k, min_count=1, flips=False, neighbors=False):
        """kmx_count_adjacency2 (k 33..64): kmers int64[n, 2] = (low, high) words."""
        return self._adjacency(self.lib.kmx_count_adjacency2, 2, kmers, counts, k, min_count, flips, neighbors)

    @_on_ctx_stream
    def count_edge_histogram(self, edges, out=None) -> GraphSummary:
        """kmx_count_edge_histogram -> GraphSummary of the 256 bins; `out` (int64[256], device) is accumulated into and summarised."""
        if out is None:
            out = torch.zeros(256, dtype=torch.int64, device=self.device)
        n = int(edges.numel())
        self._ck(self.lib.kmx_count_edge_histogram(self._h, _ptr(edges) if n else None, n, _ptr(out)))
        return GraphSummary(tuple(int(v) for v in u64_numpy(out)))

    @_on_ctx_stream
    def count_unitig_ends(self, edges, flips, nbr):
        """kmx_count_unitig_ends -> uint8[n] from the three outputs of count_adjacency(2): bit 0 = the successor side of the entry ends
        a non-branching path, bit 1 = its predecessor side does (both for an entry without edges)."""
        n = int(edges.numel())
        nbr = nbr.contiguous()
        ends = self.empty(n, torch.uint8)
        self._ck(self.lib.kmx_count_unitig_ends(self._h, _ptr(edges) if n else None, _ptr(flips) if n else None, _ptr(nbr) if n else None, n,
                                                _ptr(ends) if n else None))
        return ends

    def _unitigs(self, words, kmers, counts, k, min_count, adjacency):
        n = int(kmers.numel()) // words
        kmers = kmers.contiguous()
        if adjacency is None:
            adjacency = (self.count_adjacency if words == 1 else self.count_adjacency2)(kmers, counts, k, min_count, flips=True, neighbors=True)
        edges, flips, nbr = adjacency
        nbr = nbr.contiguous()
        nodes, offsets = self.empty(n, torch.int64), self.empty(n + 1, torch.int64)
        circular, sums = self.empty(n, torch.uint8), self.empty(n, torch.int64)
        n_unitigs, n_nodes = C.c_uint64(0), C.c_uint64(0)
        fn = self.lib.kmx_count_unitigs if words == 1 else self.lib.kmx_count_unitigs2
        self._ck(fn(self._h, _ptr(kmers) if n else None, _ptr(counts) if counts is not None and n else None, n, k, int(min_count),
                    _ptr(edges) if n else None, _ptr(flips) if n else None, _ptr(nbr) if n else None, _ptr(nodes) if n else None, _ptr(offsets),
                    _ptr(circular) if n else None, _ptr(sums) if n else None, C.byref(n_unitigs), C.byref(n_nodes)))
        u = int(n_unitigs.value)
        if n == 0:
            offsets.zero_()
        return Unitigs(nodes[:int(n_nodes.value)], offsets[:u + 1], circular[:u], sums[:u], u, k, kmers, self)

    @_on_ctx_stream
    def count_unitigs(self, kmers, counts, k, min_count=1, adjacency=None) -> Unitigs:
        """kmx_count_unitigs -> Unitigs: the maximal non-branching paths of the table's de Bruijn graph as ordered lists of oriented
        nodes (include/kmx.h has the definitions).  adjacency = (edges, flips, nbr) as count_adjacency(..., flips=True,
        neighbors=True) returns them for the same counts and min_count; without it that call is made here.  k 2..31."""
        return self._unitigs(1, kmers, counts, k, min_count, adjacency)

    @_on_ctx_stream
    def count_unitigs2(self, kmers, counts, k, min_count=1, adjacency=None) -> Unitigs:
        """kmx_count_unitigs2 (k 33..64): kmers int64[n, 2] = (low, high) words."""
        return self._unitigs(2, kmers, counts, k, min_count, adjacency)

    @_on_ctx_stream
    def _unitig_sequences(self, u: Unitigs):
        words = 1 if u.kmers.dim() == 1 else 2
        n = int(u.kmers.numel()) // words
        seq = self.empty(u.n_nodes + u.n_unitigs * (u.k - 1), torch.uint8)
        fn = self.lib.kmx_count_unitig_sequences if words == 1 else self.lib.kmx_count_unitig_sequences2
        if u.n_unitigs:
            self._ck(fn(self._h, _ptr(u.kmers), n, u.k, _ptr(u.nodes), _ptr(u.offsets), u.n_unitigs, _ptr(seq)))
        return seq

    # ------------------------------------------------------------ reads threaded through the unitigs
    @_on_ctx_stream
    def count_unitig_index(self, unitigs: Unitigs, n: int):
        """kmx_count_unitig_index -> int64[n] (u64 words): where each of the table's n entries sits in `unitigs` --
        ((p + 1) << 3) | (last << 2) | (first << 1) | o for the entry nodes[p] names, 0 (PLACE_NONE) for an entry in no unitig.  It
        goes into count_lookup(2) / count_lookup_reads(2) as the counts array: 0 = absent or in no unitig."""
        n = int(n)
        place = self.empty(n, torch.int64)
        self._ck(self.lib.kmx_count_unitig_index(self._h, _ptr(unitigs.nodes) if unitigs.n_nodes else None, _ptr(unitigs.offsets), unitigs.n_unitigs, n,
                                                 _ptr(place) if n else None))
        return place

    def _read_paths(self, words, bases, n_reads, read_len, k, kmers, unitigs, place, offsets, max_segments):
        n = int(kmers.numel()) // words if kmers is not None else 0
        if n:
            kmers = kmers.contiguous()
        if place is None:
            place = self.count_unitig_index(unitigs, n)
        fn = self.lib.kmx_count_read_paths if words == 1 else self.lib.kmx_count_read_paths2
        r = self._reads(bases, n_reads, read_len, offsets)
        args = (self._h, C.byref(r), k, _ptr(kmers) if n else None, n, _ptr(place) if n else None, _ptr(unitigs.offsets), unitigs.n_unitigs)
        s = C.c_uint64(0)
        if max_segments is None:   # count, then allocate
            self._ck(fn(*args, None, None, 0, C.byref(s)))
            max_segments = int(s.value)
        po = self.empty(int(n_reads) + 1, torch.int64)
        segs = self.empty(PATH_WORDS * max(int(max_segments), 1), torch.int64)
        self._ck(fn(*args, _ptr(po), _ptr(segs), int(max_segments), C.byref(s)))
        if int(n_reads) == 0:
            po.zero_()
        return ReadPaths(po, segs[:PATH_WORDS * int(s.value)].view(-1, PATH_WORDS), int(k))

    @_on_ctx_stream
    def count_read_paths(self, bases, n_reads, read_len, k, kmers, unitigs: Unitigs, place=None, offsets=None, max_segments=None) -> ReadPaths:
        """kmx_count_read_paths -> ReadPaths: where every read of the batch lies on the unitigs of the table `kmers` -- a 32-byte record
        per maximal run of consecutive windows that walk one unitig in one direction (include/kmx.h has the rule).  `place` is
        count_unitig_index(unitigs, n), made here when not given; `offsets` makes the reads ragged (no window offsets are needed);
        max_segments=None counts first and then allocates, a number gives room for that many (KmxError E_NOMEM above it).  k 2..31."""
        return self._read_paths(1, bases, n_reads, read_len, k, kmers, unitigs, place, offsets, max_segments)

    @_on_ctx_stream
    def count_read_paths2(self, bases, n_reads, read_len, k, kmers, unitigs: Unitigs, place=None, offsets=None, max_segments=None) -> ReadPaths:
        """kmx_count_read_paths2 (k 33..64): kmers int64[n, 2] = (low, high) words."""
        return self._read_paths(2, bases, n_reads, read_len, k, kmers, unitigs, place, offsets, max_segments)

    # ------------------------------------------------------------ the unitigs as a graph
    @_on_ctx_stream
    def count_unitig_links(self, unitigs: Unitigs, adjacency, n: int, place=None, max_links=None) -> UnitigLinks:
        """kmx_count_unitig_links -> UnitigLinks: the links between the oriented unitigs (include/kmx.h has the rule).  adjacency =
        (edges, flips, nbr) as count_adjacency(2)(..., flips=True, neighbors=True) returned them for the table the unitigs were made
        of, n its entry count; `place` is count_unitig_index(unitigs, n), made here when not given.  max_links=None counts first and
        then allocates, a number gives room for that many (KmxError E_NOMEM above it).  One call for both key widths."""
        n = int(n)
        edges, flips, nbr = adjacency
        nbr = nbr.contiguous()
        if place is None:
            place = self.count_unitig_index(unitigs, n)
        u = unitigs.n_unitigs
        args = (self._h, _ptr(edges) if n else None, _ptr(flips) if n else None, _ptr(nbr) if n else None, n,
                _ptr(unitigs.nodes) if unitigs.n_nodes else None, _ptr(unitigs.offsets), u, _ptr(place) if n else None)
        m = C.c_uint64(0)
        if max_links is None:   # count, then allocate
            self._ck(self.lib.kmx_count_unitig_links(*args, None, None, 0, C.byref(m)))
            max_links = int(m.value)
        lo = torch.zeros(2 * u + 1, dtype=torch.int64, device=self.device)
        targets = self.empty(max(int(max_links), 1), torch.int64)
        self._ck(self.lib.kmx_count_unitig_links(*args, _ptr(lo), _ptr(targets), int(max_links), C.byref(m)))
        return UnitigLinks(lo, targets[:int(m.value)])

    def _unitig_select(self, words, kmers, counts, unitigs, keep, place):
        n = int(counts.numel())
        kmers = kmers.contiguous()
        if place is None:
            place = self.count_unitig_index(unitigs, n)
        keep = (keep if keep.dtype == torch.uint8 else keep.to(torch.uint8)).contiguous()
        if keep.numel() != unitigs.n_unitigs:
            raise ValueError("keep holds one byte per unitig")
        ok = self.empty(words * max(n, 1), torch.int64)
        oc = self.empty(max(n, 1), torch.int64)
        m = C.c_uint64(0)
        fn = self.lib.kmx_count_unitig_select if words == 1 else self.lib.kmx_count_unitig_select2
        self._ck(fn(self._h, _ptr(kmers) if n else None, _ptr(counts) if n else None, n, _ptr(place) if n else None, _ptr(unitigs.offsets),
                    unitigs.n_unitigs, _ptr(keep) if unitigs.n_unitigs else None, _ptr(ok), _ptr(oc), n, C.byref(m)))
        ok = ok[:words * m.value]
        return (ok.view(-1, 2) if words == 2 else ok), oc[:m.value]

    @_on_ctx_stream
    def count_unitig_select(self, kmers, counts, unitigs: Unitigs, keep, place=None):
        """kmx_count_unitig_select -> (kmers, counts): the entries of the table that lie in a unitig u with keep[u] set (bool or uint8
        per unitig), order kept -- a table again.  Entries in no unitig are dropped.  `place` as for count_unitig_links."""
        return self._unitig_select(1, kmers, counts, unitigs, keep, place)

    @_on_ctx_stream
    def count_unitig_select2(self, kmers, counts, unitigs: Unitigs, keep, place=None):
        """kmx_count_unitig_select2 -> (kmers int64[n, 2], counts) for the tables of count_canonical2."""
        return self._unitig_select(2, kmers, counts, unitigs, keep, place)

    def _clip_tips(self, words, kmers, counts, k, min_count, max_nodes, rounds, islands):
        one = words == 1
        max_nodes = int(k) if max_nodes is None else int(max_nodes)
        removed = []
        for _ in range(int(rounds)):
            n = int(counts.numel())
            if n == 0:
                break
            adj = (self.count_adjacency if one else self.count_adjacency2)(kmers, counts, k, min_count, flips=True, neighbors=True)
            un = (self.count_unitigs if one else self.count_unitigs2)(kmers, counts, k, min_count, adjacency=adj)
            place = self.count_unitig_index(un, n)
            links = self.count_unitig_links(un, adj, n, place=place)
            keep = ~un.tips(links, max_nodes, islands)
            kmers, counts = (self.count_unitig_select if one else self.count_unitig_select2)(kmers, counts, un, keep, place=place)
            removed.append(n - int(counts.numel()))
            if removed[-1] == 0:
                break
        return kmers, counts, removed

    @_on_ctx_stream
    def count_clip_tips(self, kmers, counts, k, min_count=1, max_nodes=None, rounds=1, islands=False):
        """Tip clipping -> (kmers, counts, removed): the table without the entries of its short dead-end unitigs, and the number of
        entries each round removed.  A round is adjacency -> unitigs -> index -> links -> Unitigs.tips -> select, all on the device;
        it is run `rounds` times, or until a round removes nothing.  max_nodes (default k) is the longest unitig that counts as a
        tip; islands=True also removes short unitigs with no link at all.  Entries below min_count lie in no unitig and leave in the
        first round.  The rule is topological and blunt: it looks at no counts, and a fork whose two branches are BOTH short dead
        ends loses both; count_simplify(2) compares mean counts and pops bubbles as well (count_unitig_clean).  k 2..31."""
        return self._clip_tips(1, kmers, counts, k, min_count, max_nodes, rounds, islands)

    @_on_ctx_stream
    def count_clip_tips2(self, kmers, counts, k, min_count=1, max_nodes=None, rounds=1, islands=False):
        """count_clip_tips for the tables of count_canonical2 (k 33..64)."""
        return self._clip_tips(2, kmers, counts, k, min_count, max_nodes, rounds, islands)

    # ------------------------------------------------------------ cleaning the compacted graph
    @_on_ctx_stream
    def count_unitig_clean(self, unitigs: Unitigs, links: UnitigLinks, tip_max_nodes=None, tip_ratio=(1, 1), bubble_max_nodes=None, bubble_max_diff=4,
                           island_max_nodes=0):
        """kmx_count_unitig_clean -> (keep uint8[U], reason uint8[U]): which unitigs to drop, one kernel over the unitigs and their
        links (include/kmx.h has the rule); `keep` goes into count_unitig_select(2) as it is, reason is CLEAN_KEEP (0), CLEAN_TIP,
        CLEAN_BUBBLE or CLEAN_ISLAND.  A dead end of at most tip_max_nodes nodes (default k) is dropped if its mean count per node
        is below tip_ratio = (num, den) of a sibling's, ties to the smaller index -- (1, 1): the weaker of two; None: every short
        dead end, exactly Unitigs.tips.  Of a simple bubble whose branches have at most bubble_max_nodes nodes (default 2 k: a
        substitution makes branches of k nodes, a short indel somewhat more or fewer) and differ by at most bubble_max_diff nodes
        (default 4), the branch with the lower mean count is dropped.  island_max_nodes > 0 also drops unitigs of at most that many
        nodes with no link at all.  The defaults are choices, not measurements.  One call for both key widths."""
        k = int(unitigs.k)
        num, den = (0, 1) if tip_ratio is None else (int(tip_ratio[0]), int(tip_ratio[1]))
        u = unitigs.n_unitigs
        if links.offsets.numel() != 2 * u + 1:
            raise ValueError("links holds 2 * n_unitigs + 1 offsets")
        keep, reason = self.empty(u, torch.uint8), self.empty(u, torch.uint8)
        self._ck(self.lib.kmx_count_unitig_clean(
            self._h, _ptr(unitigs.offsets), _ptr(unitigs.circular) if unitigs.circular is not None and u else None,
            _ptr(unitigs.count_sums) if unitigs.count_sums is not None and u else None, u, _ptr(links.offsets),
            _ptr(links.targets) if links.n_links else None, links.n_links, k if tip_max_nodes is None else int(tip_max_nodes), num, den,
            2 * k if bubble_max_nodes is None else int(bubble_max_nodes), int(bubble_max_diff), int(island_max_nodes),
            _ptr(keep) if u else None, _ptr(reason) if u else None))
        return keep, reason

    def _simplify(self, words, kmers, counts, k, min_count, rounds, rule):
        one = words == 1
        log = []
        for _ in range(int(rounds)):
            n = int(counts.numel())
            if n == 0:
                break
            adj = (self.count_adjacency if one else self.count_adjacency2)(kmers, counts, k, min_count, flips=True, neighbors=True)
            un = (self.count_unitigs if one else self.count_unitigs2)(kmers, counts, k, min_count, adjacency=adj)
            place = self.count_unitig_index(un, n)
            links = self.count_unitig_links(un, adj, n, place=place)
            keep, reason = self.count_unitig_clean(un, links, **rule)
            kmers, counts = (self.count_unitig_select if one else self.count_unitig_select2)(kmers, counts, un, keep, place=place)
            c = torch.bincount(reason, minlength=4).cpu().tolist()
            log.append({"tips": c[CLEAN_TIP], "bubbles": c[CLEAN_BUBBLE], "islands": c[CLEAN_ISLAND], "removed": n - int(counts.numel())})
            if log[-1]["removed"] == 0:
                break
        return kmers, counts, log

    @_on_ctx_stream
    def count_simplify(self, kmers, counts, k, min_count=1, rounds=4, **rule):
        """Graph simplification -> (kmers, counts, log): the table without the entries of the unitigs count_unitig_clean drops --
        low-coverage dead ends, the weaker branch of every simple bubble and, if asked for, short islands.  A round is adjacency ->
        unitigs -> index -> links -> clean -> select, all on the device; dropping a branch joins the unitigs around it, so rounds
        are run until one removes nothing, `rounds` (default 4, a choice) at the most.  `rule` are count_unitig_clean's keyword
        arguments.  log holds a dict per round: the unitigs dropped as "tips", "bubbles" and "islands", and the entries "removed".
        Entries below min_count lie in no unitig and leave in the first round, as with count_clip_tips.  k 2..31."""
        return self._simplify(1, kmers, counts, k, min_count, rounds, rule)

    @_on_ctx_stream
    def count_simplify2(self, kmers, counts, k, min_count=1, rounds=4, **rule):
        """count_simplify for the tables of count_canonical2 (k 33..64)."""
        return self._simplify(2, kmers, counts, k, min_count, rounds, rule)

    # ------------------------------------------------------------ which unitigs hang together
    @_on_ctx_stream
    def count_unitig_components(self, unitigs: Unitigs, links: UnitigLinks, mask=None, stats=True) -> UnitigComponents:
        """kmx_count_unitig_components -> UnitigComponents: the connected components of the compacted graph (include/kmx.h has the
        rule) -- a label (the smallest unitig index of its component) and an id per unitig, and with stats=True a record per
        component: root, unitigs, nodes, count sum.  `mask` (bool or uint8 per unitig, for instance the keep of count_unitig_clean)
        leaves unitigs out, with their links.  One call for both key widths."""
        u = unitigs.n_unitigs
        if links.offsets.numel() != 2 * u + 1:
            raise ValueError("links holds 2 * n_unitigs + 1 offsets")
        if mask is not None:
            mask = (mask if mask.dtype == torch.uint8 else mask.to(torch.uint8)).contiguous()
            if mask.numel() != u:
                raise ValueError("mask holds one byte per unitig")
        labels, ids = self.empty(u, torch.int64), self.empty(u, torch.int64)
        c, r = C.c_uint64(0), C.c_uint32(0)
        args = (self._h, _ptr(unitigs.offsets), _ptr(unitigs.count_sums) if unitigs.count_sums is not None and u else None, u, _ptr(links.offsets),
                _ptr(links.targets) if links.n_links else None, links.n_links, _ptr(mask) if mask is not None and u else None,
                _ptr(labels) if u else None, _ptr(ids) if u else None)
        self._ck(self.lib.kmx_count_unitig_components(*args, None, 0, C.byref(c), C.byref(r)))
        if not stats:
            return UnitigComponents(labels, ids, None, int(c.value), int(r.value))
        # (the records need C: count, then allocate, as count_unitig_links does)
        rec = self.empty(COMP_WORDS * max(int(c.value), 1), torch.int64)
        self._ck(self.lib.kmx_count_unitig_components(*args, _ptr(rec), int(c.value), C.byref(c), C.byref(r)))
        return UnitigComponents(labels, ids, rec[:COMP_WORDS * int(c.value)].view(-1, COMP_WORDS), int(c.value), int(r.value))

    def _drop_small_components(self, words, kmers, counts, k, min_nodes, min_count):
        one = words == 1
        n = int(counts.numel())
        adj = (self.count_adjacency if one else self.count_adjacency2)(kmers, counts, k, min_count, flips=True, neighbors=True)
        un = (self.count_unitigs if one else self.count_unitigs2)(kmers, counts, k, min_count, adjacency=adj)
        place = self.count_unitig_index(un, n)
        links = self.count_unitig_links(un, adj, n, place=place)
        comp = self.count_unitig_components(un, links)
        kmers, counts = (self.count_unitig_select if one else self.count_unitig_select2)(kmers, counts, un, comp.keep(min_nodes=min_nodes), place=place)
        return kmers, counts, comp

    @_on_ctx_stream
    def count_drop_small_components(self, kmers, counts, k, min_nodes, min_count=1):
        """Component filter -> (kmers, counts, components): the table without the entries of every connected component of fewer than
        min_nodes nodes -- a contaminant, a cluster of errors that forms a graph of its own: what count_simplify(2), whose rules see
        one unitig and its neighbours, keeps -- and the UnitigComponents of the graph BEFORE the cut.  adjacency -> unitigs -> index
        -> links -> components -> keep(min_nodes) -> select, all on the device.  Entries below min_count lie in no unitig and
        leave, as with count_clip_tips.  k 2..31."""
        return self._drop_small_components(1, kmers, counts, k, min_nodes, min_count)

    @_on_ctx_stream
    def count_drop_small_components2(self, kmers, counts, k, min_nodes, min_count=1):
        """count_drop_small_components for the tables of count_canonical2 (k 33..64)."""
        return self._drop_small_components(2, kmers, counts, k, min_nodes, min_count)

    # ------------------------------------------------------------ which links the reads walk
    @_on_ctx_stream
    def count_link_support(self, paths: ReadPaths, unitigs: Unitigs, links: UnitigLinks, out: "LinkSupport | None" = None) -> LinkSupport:
        """kmx_count_link_support -> LinkSupport: per link slot, how many reads of the batch cross it (include/kmx.h has the rule) --
        a pair of consecutive segments of one read, the second beginning one base after the first ends, that leaves the exit node of
        one oriented unitig and enters the entry node of the next; the link and its mirror are both credited.  `paths` as
        count_read_paths(2) returned them for `unitigs`, `links` as count_unitig_links.  `out` (a LinkSupport of the same links) is
        accumulated into: batches of reads stream against one graph.  One call for both key widths; asynchronous."""
        u = unitigs.n_unitigs
        if links.offsets.numel() != 2 * u + 1:
            raise ValueError("links holds 2 * n_unitigs + 1 offsets")
        if out is None:
            out = LinkSupport(torch.zeros(links.n_links, dtype=torch.int64, device=self.device),
                              torch.zeros(LS_WORDS, dtype=torch.int64, device=self.device))
        elif out.support.numel() != links.n_links or out.summary.numel() != LS_WORDS:
            raise ValueError("out holds one word per link and three summary words")
        segs = paths.segments.contiguous()
        s = int(segs.shape[0])
        self._ck(self.lib.kmx_count_link_support(self._h, _ptr(segs) if s else None, s, _ptr(unitigs.offsets), u, _ptr(links.offsets),
                                                 _ptr(links.targets) if links.n_links else None, links.n_links,
                                                 _ptr(out.support) if links.n_links else None, _ptr(out.summary)))
        return out

    @_on_ctx_stream
    def count_cut_links(self, unitigs: Unitigs, links: UnitigLinks, adjacency, n: int, cut, place=None):
        """kmx_count_adjacency_cut -> (edges, flips, nbr): the adjacency with the edge bit of every link slot whose `cut` byte (bool
        or uint8 per link slot, for instance LinkSupport.unsupported()) is set cleared in a copy of the edges; flips and nbr are the
        tensors handed in (a neighbour word behind a cleared bit is never read).  adjacency, n and place as for count_unitig_links,
        which must have made `links` from them.  The result goes into count_unitigs(2)(..., adjacency=) and count_unitig_links: cut,
        then compact again.  A mask that is not closed under the mirror cuts one direction of an edge only, which is legal."""
        n = int(n)
        edges, flips, nbr = adjacency
        nbr = nbr.contiguous()
        u = unitigs.n_unitigs
        if links.offsets.numel() != 2 * u + 1:
            raise ValueError("links holds 2 * n_unitigs + 1 offsets")
        cut = (cut if cut.dtype == torch.uint8 else cut.to(torch.uint8)).contiguous()
        if cut.numel() != links.n_links:
            raise ValueError("cut holds one byte per link slot")
        if place is None:
            place = self.count_unitig_index(unitigs, n)
        out = self.empty(n, torch.uint8)
        self._ck(self.lib.kmx_count_adjacency_cut(self._h, _ptr(edges) if n else None, _ptr(flips) if n else None, _ptr(nbr) if n else None, n,
                                                  _ptr(unitigs.nodes) if unitigs.n_nodes else None, _ptr(unitigs.offsets), u,
                                                  _ptr(place) if n else None, _ptr(links.offsets), links.n_links,
                                                  _ptr(cut) if links.n_links else None, _ptr(out) if n else None))
        return out, flips, nbr

    def _prune_links(self, words, bases, n_reads, read_len, k, kmers, counts, min_support, min_count, offsets):
        one = words == 1
        n = int(counts.numel())
        adj = (self.count_adjacency if one else self.count_adjacency2)(kmers, counts, k, min_count, flips=True, neighbors=True)
        unitigs = self.count_unitigs if one else self.count_unitigs2
        un = unitigs(kmers, counts, k, min_count, adjacency=adj)
        place = self.count_unitig_index(un, n)
        links = self.count_unitig_links(un, adj, n, place=place)
        paths = (self.count_read_paths if one else self.count_read_paths2)(bases, n_reads, read_len, k, kmers, un, place=place, offsets=offsets)
        support = self.count_link_support(paths, un, links)
        cut = support.unsupported(min_support)
        adj = self.count_cut_links(un, links, adj, n, cut, place=place)
        un = unitigs(kmers, counts, k, min_count, adjacency=adj)
        return adj, un, self.count_unitig_links(un, adj, n), support, int(cut.sum())

    @_on_ctx_stream
    def count_prune_links(self, bases, n_reads, read_len, k, kmers, counts, min_support=1, min_count=1, offsets=None):
        """Edge filter -> (adjacency, unitigs, links, support, n_cut): the graph of the table without the links that fewer than
        min_support reads of the batch cross -- two k-mers that overlap by chance, at a repeat boundary or next to an error, with
        no read passing from one to the other.  adjacency -> unitigs -> index -> links -> read paths -> support -> cut, then
        unitigs and links again over the cut adjacency, all on the device.  Returns the cut adjacency (edges, flips, nbr), the
        Unitigs and UnitigLinks made of it, the LinkSupport of the FIRST pass (over the links before the cut) and the number of link
        slots cut.  One pass suffices: support belongs to the pair of nodes a link joins, not to the compaction, so the links that
        remain are links that were counted.  The table is not changed: the cuts live in the adjacency returned here, and
        count_simplify(2), which rebuilds the adjacency from the table, does not see them.  A false join inside a unitig is not a
        link and stays.  k 2..31."""
        return self._prune_links(1, bases, n_reads, read_len, k, kmers, counts, min_support, min_count, offsets)

    @_on_ctx_stream
    def count_prune_links2(self, bases, n_reads, read_len, k, kmers, counts, min_support=1, min_count=1, offsets=None):
        """count_prune_links for the tables of count_canonical2 (k 33..64)."""
        return self._prune_links(2, bases, n_reads, read_len, k, kmers, counts, min_support, min_count, offsets)

    @_on_ctx_stream
    def canonical_reduce2(self, bases, n_reads, read_len, k, with_hash=False, offsets=None) -> Summary2:
        out = self.empty(5, torch.int64)
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(self.lib.kmx_canonical_reduce2(self._h, C.byref(r), k, int(with_hash), _ptr(out)))
        v = u64_numpy(out)
        return Summary2(*[int(x) for x in v])

    @_on_ctx_stream
    def canonical_windows2(self, bases, n_reads, read_len, k, offsets=None, host_offsets=None):
        wo_host = self.win_offsets(n_reads, read_len, k, host_offsets)
        total = int(wo_host[-1])
        d_wo = self.to_device(wo_host) if offsets is not None else None
        outs = {n: self.empty(2 * total, torch.int64) for n in ("fw", "rc", "canon")}
        outs["flags"] = self.empty(total, torch.uint8)
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(self.lib.kmx_canonical_windows2(self._h, C.byref(r), _ptr(d_wo), k, _ptr(outs["fw"]), _ptr(outs["rc"]),
                                                 _ptr(outs["canon"]), _ptr(outs["flags"])))
        return outs

    @_on_ctx_stream
    def histogram(self, bases, n_reads, read_len, k, hasher, hasher_k, log2_buckets, offsets=None,
                  counts: torch.Tensor | None = None) -> torch.Tensor:
        if counts is None:
            counts = torch.zeros(1 << log2_buckets, dtype=torch.int64, device=self.device)
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(self.lib.kmx_histogram(self._h, C.byref(r), k, hasher, hasher_k, log2_buckets, _ptr(counts)))
        return counts

    # ---- the same two passes under std's DefaultHasher (keys 0, 0) / RandomState (its keys): SipHash-1-3 of the canonical word
    @_on_ctx_stream
    def canonical_reduce_sip13(self, bases, n_reads, read_len, k, key0=0, key1=0, flags=0, offsets=None) -> Summary:
        """kmx_canonical_reduce_sip13: xor_hash = xor of SipHash-1-3(key0, key1; canonical word); the rest as canonical_reduce"""
        out = self.empty(4, torch.int64)
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(self.lib.kmx_canonical_reduce_sip13(self._h, C.byref(r), k, key0 & (2**64 - 1), key1 & (2**64 - 1), flags, _ptr(out)))
        v = u64_numpy(out)
        return Summary(int(v[0]), int(v[1]), int(v[2]), int(v[3]))

    @_on_ctx_stream
    def histogram_sip13(self, bases, n_reads, read_len, k, log2_buckets, key0=0, key1=0, offsets=None,
                        counts: torch.Tensor | None = None) -> torch.Tensor:
        """kmx_histogram_sip13: counts (accumulated into) of the bucket of SipHash-1-3(key0, key1; canonical word)"""
        if counts is None:
            counts = torch.zeros(1 << log2_buckets, dtype=torch.int64, device=self.device)
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(self.lib.kmx_histogram_sip13(self._h, C.byref(r), k, key0 & (2**64 - 1), key1 & (2**64 - 1), log2_buckets, _ptr(counts)))
        return counts

    # --------------------------------------------------------- element-wise
    @_on_ctx_stream
    def kmers_from_bytes(self, seqs: torch.Tensor, n: int, k: int) -> torch.Tensor:
        out = self.empty(n, torch.int64)
        bad = C.c_uint64()
        st = self.lib.kmx_kmers_from_bytes(self._h, _ptr(seqs) if n else None, n, k, _ptr(out) if n else None, C.byref(bad))
        if st == _lib.E_INVALID_BASE:
            e = KmxError(st, f"invalid base at byte {bad.value}")
            e.first_bad = bad.value
            raise e
        self._ck(st)
        return out

    @_on_ctx_stream
    def revcomp_words(self, words: torch.Tensor, k: int) -> torch.Tensor:
        out = torch.empty_like(words)
        self._ck(self.lib.kmx_revcomp_words(self._h, _ptr(words), words.numel(), k, _ptr(out)))
        return out

    @_on_ctx_stream
    def canonical_words(self, words: torch.Tensor, k: int):
        canon = torch.empty_like(words)
        isc = self.empty(words.numel(), torch.uint8)
        self._ck(self.lib.kmx_canonical_words(self._h, _ptr(words), words.numel(), k, _ptr(canon), _ptr(isc)))
        return canon, isc

    @_on_ctx_stream
    def hash_words(self, words: torch.Tensor, hasher: int, hasher_k: int) -> torch.Tensor:
        out = torch.empty_like(words)
        self._ck(self.lib.kmx_hash_words(self._h, _ptr(words), words.numel(), hasher, hasher_k, _ptr(out)))
        return out

    @_on_ctx_stream
    def hash_words_sip13(self, words: torch.Tensor, key0: int = 0, key1: int = 0) -> torch.Tensor:
        """hash_one(&DefaultHasher / RandomState, kmer): SipHash-1-3 of each word (kmx_hash_words_sip13)"""
        out = torch.empty_like(words)
        self._ck(self.lib.kmx_hash_words_sip13(self._h, _ptr(words), words.numel(), key0 & (2**64 - 1), key1 & (2**64 - 1), _ptr(out)))
        return out

    @_on_ctx_stream
    def match_words(self, fw, rc, other) -> torch.Tensor:
        out = self.empty(fw.numel(), torch.uint8)
        self._ck(self.lib.kmx_match_words(self._h, _ptr(fw), _ptr(rc), _ptr(other), fw.numel(), _ptr(out)))
        return out

    @_on_ctx_stream
    def ck_shift(self, fw, rc, bases, k, append=True) -> torch.Tensor:
        dropped = self.empty(fw.numel(), torch.uint8)
        fn = self.lib.kmx_ck_append_bases if append else self.lib.kmx_ck_prepend_bases
        self._ck(fn(self._h, _ptr(fw), _ptr(rc), _ptr(bases), fw.numel(), k, _ptr(dropped)))
        return dropped

    @_on_ctx_stream
    def encode_kmers(self, seqs: torch.Tensor, n: int, seq_len: int, enc_byte: int, words_per_kmer: int) -> torch.Tensor:
        out = self.empty(n * words_per_kmer, torch.int64)
        self._ck(self.lib.kmx_encode_kmers(self._h, _ptr(seqs) if seqs.numel() else None, n, seq_len, enc_byte,
                                           words_per_kmer, _ptr(out)))
        return out

    @_on_ctx_stream
    def encode_windows(self, bases, n_reads, read_len, k, enc_byte, words_per_kmer) -> torch.Tensor:
        nwin = max(read_len - k + 1, 0)
        out = self.empty(n_reads * nwin * words_per_kmer, torch.int64)
        r = self._reads(bases, n_reads, read_len, None)
        self._ck(self.lib.kmx_encode_windows(self._h, C.byref(r), k, enc_byte, words_per_kmer, _ptr(out)))
        return out

    @_on_ctx_stream
    def encoding_rev_comp(self, words: torch.Tensor, K: int, enc_byte: int, words_per_kmer: int) -> torch.Tensor:
        out = torch.empty_like(words)
        self._ck(self.lib.kmx_encoding_rev_comp(self._h, _ptr(words), words.numel() // words_per_kmer, K, enc_byte,
                                                words_per_kmer, _ptr(out)))
        return out

    # ---- SeqVector (src/naive_impl/seq_vector.rs): 2-bit packed sequences on the device
    @_on_ctx_stream
    def seqvec_from_bytes(self, data: torch.Tensor, n: int | None = None) -> torch.Tensor:
        """SeqVector::from(&[u8]) (seq_vector.rs:230-242): ceil(n/32) u64 words (as int64 tensor), base i at bits [2i,2i+1]"""
        n = data.numel() if n is None else n
        words = torch.zeros((n + 31) // 32 + 2, dtype=torch.int64, device=self.device)[: (n + 31) // 32]
        return self.seqvec_push_chars(words, 0, data, n)

    @_on_ctx_stream
    def seqvec_push_chars(self, words: torch.Tensor, n_before: int, data: torch.Tensor, n: int | None = None) -> torch.Tensor:
        """SeqVector::push_chars (seq_vector.rs:141-161): append n ASCII bases after the n_before already stored"""
        n = data.numel() if n is None else n
        bad = C.c_uint64()
        st = self.lib.kmx_seqvec_push_chars(self._h, _ptr(words) if words.numel() else None, n_before, _ptr(data) if n else None, n, C.byref(bad))
        if st == _lib.E_INVALID_BASE:
            e = KmxError(st, f"invalid base at byte {bad.value}")
            e.first_bad = bad.value
            raise e
        self._ck(st)
        return words

    @_on_ctx_stream
    def seqvec_to_bytes(self, words: torch.Tensor, n_bases: int) -> torch.Tensor:
        out = self.empty(n_bases, torch.uint8)
        self._ck(self.lib.kmx_seqvec_to_bytes(self._h, _ptr(words) if n_bases else None, n_bases, _ptr(out) if n_bases else None))
        return out

    @_on_ctx_stream
    def seqvec_get_kmers(self, words: torch.Tensor, n_bases: int, pos: torch.Tensor, k: int) -> torch.Tensor:
        out = self.empty(pos.numel(), torch.int64)
        n = pos.numel()
        self._ck(self.lib.kmx_seqvec_get_kmers(self._h, _ptr(words) if n else None, n_bases, _ptr(pos) if n else None, n, k, _ptr(out) if n else None))
        return out

    @_on_ctx_stream
    def seqvec_iter_kmers(self, words: torch.Tensor, n_bases: int, k: int, start: int = 0, end: int | None = None) -> torch.Tensor:
        end = n_bases if end is None else end
        cnt = max(0, end - start - k + 1)
        out = self.empty(cnt, torch.int64)
        self._ck(self.lib.kmx_seqvec_iter_kmers(self._h, _ptr(words), n_bases, start, end, k, _ptr(out) if cnt else None))
        return out

    @_on_ctx_stream
    def seqvec_canonical_reduce(self, words: torch.Tensor, n_reads: int, read_len: int, k: int, hasher: int = 0, hasher_k: int = 0,
                                flags: int = 0, out: torch.Tensor | None = None, sync: bool = True):
        """canonical k-mer scan of the reads stored back to back in a SeqVector (read r = slice [r*L, (r+1)*L))"""
        out = self.empty(4, torch.int64) if out is None else out
        self._ck(self.lib.kmx_seqvec_canonical_reduce(self._h, _ptr(words) if n_reads else None, n_reads, read_len, k, hasher, hasher_k, flags, _ptr(out)))
        if not sync:
            return out
        v = u64_numpy(out)
        return Summary(int(v[0]), int(v[1]), int(v[2]), int(v[3]))

    # ---- minimizers
    @_on_ctx_stream
    def minimizer_words(self, words: torch.Tensor, k: int, width: int, hasher: int, hasher_k: int = 0):
        """Kmer::minimizer_word (kmer.rs:170-192) per k-mer word -> (mmer words int64, offsets int32)"""
        n = words.numel()
        mm, off = self.empty(n, torch.int64), self.empty(n, torch.int32)
        self._ck(self.lib.kmx_minimizer_words(self._h, _ptr(words) if n else None, n, k, width, hasher, hasher_k,
                                              _ptr(mm) if n else None, _ptr(off) if n else None))
        return mm, off

    @_on_ctx_stream
    def seqvec_minimizers(self, words: torch.Tensor, n_reads: int, read_len: int, k: int, w: int, hasher: int, hasher_k: int = 0):
        """SeqVecMinimizerIter over every read slice -> (word int64, pos int32), slot r*(L-k+1)+i"""
        tot = n_reads * max(read_len - k + 1, 0)
        mw, mp = self.empty(tot, torch.int64), self.empty(tot, torch.int32)
        self._ck(self.lib.kmx_seqvec_minimizers(self._h, _ptr(words) if n_reads else None, n_reads, read_len, k, w, hasher, hasher_k,
                                                _ptr(mw) if tot else None, _ptr(mp) if tot else None))
        return mw, mp

    @_on_ctx_stream
    def minimizers(self, bases, n_reads: int, read_len: int, k: int, w: int, hasher: int, hasher_k: int = 0, offsets=None, win_offsets=None,
                   check: bool = True):
        """kmx_minimizers: SeqVecMinimizerIter over every READ (ASCII; uniform, or ragged with offsets + win_offsets) ->
        (word int64, pos int32).  check: ask for the first read with an invalid byte (KmxError KMX_E_INVALID_BASE if there is one)"""
        if offsets is None:
            tot = n_reads * max(read_len - k + 1, 0)
        else:
            tot = int(win_offsets[-1].item()) if n_reads else 0
        mw, mp = self.empty(tot, torch.int64), self.empty(tot, torch.int32)
        r = self._reads(bases, n_reads, read_len, offsets)
        bad = C.c_uint64(0)
        st = self.lib.kmx_minimizers(self._h, C.byref(r), _ptr(win_offsets) if win_offsets is not None else None, k, w, hasher, hasher_k,
                                     _ptr(mw) if tot else None, _ptr(mp) if tot else None, C.byref(bad) if check else None)
        if st == _lib.E_INVALID_BASE:
            e = KmxError(st, f"invalid base in read {bad.value}")
            e.first_bad = bad.value
            raise e
        self._ck(st)
        return mw, mp

    # ---- minimizers under std's DefaultHasher (keys 0, 0) / RandomState (its keys): SipHash-1-3 of each l-mer
    @_on_ctx_stream
    def minimizer_words_sip13(self, words: torch.Tensor, k: int, width: int, key0: int = 0, key1: int = 0):
        """kmx_minimizer_words_sip13 -> (mmer words int64, offsets int32)"""
        n = words.numel()
        mm, off = self.empty(n, torch.int64), self.empty(n, torch.int32)
        self._ck(self.lib.kmx_minimizer_words_sip13(self._h, _ptr(words) if n else None, n, k, width, key0 & (2**64 - 1), key1 & (2**64 - 1),
                                                    _ptr(mm) if n else None, _ptr(off) if n else None))
        return mm, off

    @_on_ctx_stream
    def seqvec_minimizers_sip13(self, words: torch.Tensor, n_reads: int, read_len: int, k: int, w: int, key0: int = 0, key1: int = 0):
        """kmx_seqvec_minimizers_sip13 -> (word int64, pos int32), slot r*(L-k+1)+i"""
        tot = n_reads * max(read_len - k + 1, 0)
        mw, mp = self.empty(tot, torch.int64), self.empty(tot, torch.int32)
        self._ck(self.lib.kmx_seqvec_minimizers_sip13(self._h, _ptr(words) if n_reads else None, n_reads, read_len, k, w, key0 & (2**64 - 1),
                                                      key1 & (2**64 - 1), _ptr(mw) if tot else None, _ptr(mp) if tot else None))
        return mw, mp

    @_on_ctx_stream
    def minimizers_sip13(self, bases, n_reads: int, read_len: int, k: int, w: int, key0: int = 0, key1: int = 0, offsets=None,
                         win_offsets=None, check: bool = True):
        """kmx_minimizers_sip13 -> (word int64, pos int32); check: KmxError (KMX_E_INVALID_BASE, .first_bad = the read) on an invalid byte"""
        if offsets is None:
            tot = n_reads * max(read_len - k + 1, 0)
        else:
            tot = int(win_offsets[-1].item()) if n_reads else 0
        mw, mp = self.empty(tot, torch.int64), self.empty(tot, torch.int32)
        r = self._reads(bases, n_reads, read_len, offsets)
        bad = C.c_uint64(0)
        st = self.lib.kmx_minimizers_sip13(self._h, C.byref(r), _ptr(win_offsets) if win_offsets is not None else None, k, w,
                                           key0 & (2**64 - 1), key1 & (2**64 - 1), _ptr(mw) if tot else None, _ptr(mp) if tot else None,
                                           C.byref(bad) if check else None)
        if st == _lib.E_INVALID_BASE:
            e = KmxError(st, f"invalid base in read {bad.value}")
            e.first_bad = bad.value
            raise e
        self._ck(st)
        return mw, mp

    @_on_ctx_stream
    def fastx_parse(self, text: torch.Tensor, fmt: int = 0, max_reads: int | None = None):
        """kmx_fastx_parse: FASTA/FASTQ file image (uint8, on the device) -> (bases uint8[n_bases], offsets int64[n_reads+1]).
        Two calls: the counts, then the emit into exactly sized buffers.  With `max_reads` (a bound on the number of records the
        caller vouches for): ONE call into buffers sized for the bound; KmxError (KMX_E_NOMEM) if the image holds more records."""
        n = int(text.numel())
        nr, nb = C.c_uint64(0), C.c_uint64(0)
        if max_reads is not None:
            bases = self.empty(max(n, 1), torch.uint8)
            offsets = self.empty(max_reads + 1, torch.int64)
            self._ck(self.lib.kmx_fastx_parse(self._h, _ptr(text) if n else None, n, fmt, _ptr(bases), _ptr(offsets), max_reads, C.byref(nr), C.byref(nb)))
            return bases[:nb.value], offsets[:nr.value + 1]
        self._ck(self.lib.kmx_fastx_parse(self._h, _ptr(text) if n else None, n, fmt, None, None, 0, C.byref(nr), C.byref(nb)))
        bases = self.empty(max(nb.value, 1), torch.uint8)
        offsets = self.empty(nr.value + 1, torch.int64)
        # (KMX_FASTX_SAME_TEXT: the emit reuses the chunk summaries of the counting call just made on the same image)
        self._ck(self.lib.kmx_fastx_parse(self._h, _ptr(text) if n else None, n, fmt | _lib.FASTX_SAME_TEXT, _ptr(bases), _ptr(offsets),
                                          nr.value, C.byref(nr), C.byref(nb)))
        return bases[:nb.value], offsets

    def fastx_reads(self, text: torch.Tensor, fmt: int = 0):
        """file image -> (bases, n_reads, read_len, offsets) the way the scan calls like it best: the uniform layout
        (offsets None, read_len = the length) when every read has the same length, else the ragged layout with the
        longest read as the length bound ("Real FASTQ / FASTA, end to end")"""
        bases, offsets = self.fastx_parse(text, fmt)
        n = int(offsets.numel()) - 1
        mn, mx = self.reads_length_range(offsets)
        if n > 0 and mn == mx:
            return bases, n, mx, None
        return bases, n, mx, offsets

    @_on_ctx_stream
    def fastx_quals(self, text: torch.Tensor, read_offsets: torch.Tensor | None = None, same_text: bool = False):
        """kmx_fastx_parse_quals: FASTQ file image -> (quals uint8[n_bytes], qoffsets int64[n + 1]), the quality lines as fastx_parse
        gives the reads.  Two calls: the counts, then the emit into exactly sized buffers.  same_text=True: the caller vouches that
        the last parse call on this context was on this very image, unchanged (KMX_FASTX_SAME_TEXT: the text is not summarised
        again; fastq_reads does this).  With `read_offsets` (what fastx_parse returned for the image) the lengths
        are compared on the device: ValueError naming the first read whose quality line and sequence line differ in length, or
        the counts where the image ends inside a record."""
        n = int(text.numel())
        nr, nb, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(2**64 - 1)
        tp = _ptr(text) if n else None
        fmt = _lib.FASTX_FASTQ | _lib.FASTX_SAME_TEXT
        self._ck(self.lib.kmx_fastx_parse_quals(self._h, tp, n, fmt if same_text else _lib.FASTX_FASTQ, None, None, 0, None, C.byref(nr),
                                                C.byref(nb), None))
        if read_offsets is not None and int(read_offsets.numel()) - 1 != nr.value:
            raise ValueError(f"fastx_quals: {nr.value} quality lines for {int(read_offsets.numel()) - 1} reads (the image ends inside a record)")
        quals = self.empty(max(nb.value, 1), torch.uint8)
        qoffsets = self.empty(nr.value + 1, torch.int64)
        self._ck(self.lib.kmx_fastx_parse_quals(self._h, tp, n, fmt, _ptr(quals), _ptr(qoffsets), nr.value,
                                                _ptr(read_offsets) if read_offsets is not None else None, C.byref(nr), C.byref(nb),
                                                C.byref(bad) if read_offsets is not None else None))
        if bad.value != 2**64 - 1:
            raise ValueError(f"fastx_quals: read {bad.value}: its quality line and its sequence line differ in length")
        return quals[:nb.value], qoffsets

    def fastq_reads(self, text: torch.Tensor):
        """FASTQ file image -> (bases, quals, n_reads, read_len, offsets): fastx_reads with the quality bytes, laid out as the bases
        are (the same offsets serve both; ValueError where a record's two lines differ in length)"""
        bases, offsets = self.fastx_parse(text, _lib.FASTX_FASTQ)
        quals, _ = self.fastx_quals(text, offsets, same_text=True)
        n = int(offsets.numel()) - 1
        mn, mx = self.reads_length_range(offsets)
        if n > 0 and mn == mx:
            return bases, quals, n, mx, None
        return bases, quals, n, mx, offsets

    @_on_ctx_stream
    def fastx_names(self, text: torch.Tensor, same_text: bool = False):
        """kmx_fastx_parse_names: FASTQ file image -> (names uint8[n_bytes], noffsets int64[n + 1]), line 0 of every record as it
        stands ('@' included; fastx_format skips it with name_skip=1), laid out as fastx_parse gives the reads: a ragged batch that
        reads_gather reorders.  Two calls: the counts, then the emit into exactly sized buffers.  same_text as in fastx_quals."""
        n = int(text.numel())
        nr, nb = C.c_uint64(0), C.c_uint64(0)
        tp = _ptr(text) if n else None
        fmt = _lib.FASTX_FASTQ | _lib.FASTX_SAME_TEXT
        self._ck(self.lib.kmx_fastx_parse_names(self._h, tp, n, fmt if same_text else _lib.FASTX_FASTQ, None, None, 0, C.byref(nr), C.byref(nb)))
        names = self.empty(max(nb.value, 1), torch.uint8)
        noffsets = self.empty(nr.value + 1, torch.int64)
        self._ck(self.lib.kmx_fastx_parse_names(self._h, tp, n, fmt, _ptr(names), _ptr(noffsets), nr.value, C.byref(nr), C.byref(nb)))
        return names[:nb.value], noffsets

    def fastq_records(self, text: torch.Tensor):
        """FASTQ file image -> (bases, quals, n_reads, read_len, offsets, names, name_offsets): fastq_reads plus the record names
        (fastx_names).  ValueError where the image has another number of names than of reads (it ends inside a header line)."""
        bases, quals, n, read_len, offsets = self.fastq_reads(text)
        names, noffsets = self.fastx_names(text, same_text=True)
        if int(noffsets.numel()) - 1 != n:
            raise ValueError(f"fastq_records: {int(noffsets.numel()) - 1} names for {n} reads (the image ends inside a record)")
        return bases, quals, n, read_len, offsets, names, noffsets

    # ------------------------------------------------------------ BGZF-compressed images
    @_on_ctx_stream
    def bgzf_index(self, image: torch.Tensor) -> BgzfIndex:
        """kmx_bgzf_index: a BGZF file image (uint8, on the device) -> BgzfIndex.  Two calls: the counts, then the arrays.  KmxError
        (KMX_E_ARG) for an image that does not begin with a BGZF block header (plain gzip, plain text)."""
        n = int(image.numel())
        info = (C.c_uint64 * 4)()
        ip = _ptr(image) if n else None
        self._ck(self.lib.kmx_bgzf_index(self._h, ip, n, None, None, 0, info))
        nb = int(info[0])
        bo = self.empty(nb + 1, torch.int64)
        to = self.empty(nb + 1, torch.int64)
        self._ck(self.lib.kmx_bgzf_index(self._h, ip, n, _ptr(bo), _ptr(to), nb, info))
        return BgzfIndex(bo, to, nb, int(info[1]), int(info[2]), bool(info[3]))

    @_on_ctx_stream
    def bgzf_inflate(self, image: torch.Tensor, index: "BgzfIndex | None" = None, verify: bool = True, blocks=None) -> torch.Tensor:
        """kmx_bgzf_inflate: a BGZF file image (uint8, on the device) -> its text, a uint8 device tensor (16-byte aligned: fastx_parse
        takes it as it is).  index: what bgzf_index returned for the image (None: made here).  verify=False skips the CRC-32
        comparison.  blocks=(i, j): blocks i..j-1 alone.  ValueError naming the first block that is not sound, and why.  Bytes
        behind the last complete block (index.trailing) are the caller's to judge: load_fastx refuses such a file."""
        if index is None:
            index = self.bgzf_index(image)
        i, j = (0, index.n_blocks) if blocks is None else (int(blocks[0]), int(blocks[1]))
        if not 0 <= i <= j <= index.n_blocks:
            raise ValueError("bgzf_inflate: blocks (i, j) with 0 <= i <= j <= n_blocks")
        if i == j:
            return self.empty(0, torch.uint8)
        span = int(index.text_offsets[j].item()) - int(index.text_offsets[i].item()) if blocks is not None else index.n_text_bytes
        text = self.empty(max(span, 1), torch.uint8)
        status = torch.zeros(j - i, dtype=torch.int32, device=self.device)
        bad = C.c_uint64(2**64 - 1)
        st = self.lib.kmx_bgzf_inflate(self._h, _ptr(image), int(image.numel()), _ptr(index.block_offsets[i:]), _ptr(index.text_offsets[i:]), j - i,
                                       0 if verify else _lib.BGZF_NO_CRC, _ptr(text), span, _ptr(status), C.byref(bad))
        if st == _lib.E_ARG and bad.value != 2**64 - 1:
            why = int(status[bad.value].item())
            raise ValueError(f"bgzf_inflate: block {i + bad.value} is not sound: {_lib.BGZF_ST_NAMES.get(why, why)} (KMX_BGZF_ST {why})")
        self._ck(st)
        return text[:span]

    @_on_ctx_stream
    def bgzf_deflate(self, text: torch.Tensor, block_bytes: int = 65280, stored: bool = False, offsets: bool = False):
        """kmx_bgzf_deflate: a text (uint8, on the device) -> its BGZF image, a uint8 device tensor of its own size (one call
        compresses and writes into a buffer of kmx_bgzf_deflate_bound bytes; a shorter image is copied out of it, so the buffer
        goes when the call returns): one block per `block_bytes` of text (1..65280), dynamic DEFLATE blocks or -- where that is
        not shorter, and throughout with stored=True -- stored ones, the EOF marker last.
        offsets=True -> (image, int64[n_blocks + 1]: where every block starts, the marker included, the image's end last).  The
        bytes depend on the text, block_bytes and stored alone."""
        if not 1 <= int(block_bytes) <= 65280:
            raise ValueError("bgzf_deflate: block_bytes in 1..65280")
        if text.dtype != torch.uint8 or not text.is_cuda:
            raise ValueError("bgzf_deflate: a uint8 CUDA tensor")
        text = text.contiguous()
        n = int(text.numel())
        info = (C.c_uint64 * 4)()
        room = int(self.lib.kmx_bgzf_deflate_bound(n, int(block_bytes)))
        image = self.empty(room, torch.uint8)
        off = self.empty((n + int(block_bytes) - 1) // int(block_bytes) + 2, torch.int64) if offsets else None
        self._ck(self.lib.kmx_bgzf_deflate(self._h, _ptr(text) if n else None, n, int(block_bytes), _lib.BGZF_DEFLATE_STORED if stored else 0,
                                           _ptr(image), room, _ptr(off) if offsets else None, info))
        if int(info[1]) < room:
            image = image[:int(info[1])].clone()
        return (image, off) if offsets else image

    def load_fastx(self, source) -> torch.Tensor:
        """A FASTA / FASTQ file -- a path, or its bytes -- -> its text on the device.  A BGZF image (.fastq.gz as bgzip, htslib and
        samtools write it) is copied compressed and inflated on the device; plain text is copied.  Plain single-member gzip raises
        ValueError: it has no blocks to inflate in parallel.  ctx.fastq_records(ctx.load_fastx(path)) is the whole ingest."""
        if isinstance(source, (bytes, bytearray, memoryview)):
            data = bytes(source)
        else:
            with open(source, "rb") as f:
                data = f.read()
        if data[:2] != b"\x1f\x8b":
            return self.to_device(data) if data else self.empty(0, torch.uint8)
        if not (len(data) >= 18 and data[2:4] == b"\x08\x04" and data[10:16] == b"\x06\0BC\x02\0"):
            raise ValueError("load_fastx: a gzip file that is not BGZF: one DEFLATE stream cannot be inflated in parallel; "
                             "recompress it with bgzip (`gunzip -c f.gz | bgzip > f.bgz.gz`), which writes the blocked form that can")
        image = self.to_device(data)
        index = self.bgzf_index(image)
        if index.trailing:
            raise ValueError(f"load_fastx: {index.trailing} bytes behind the last complete BGZF block (block {index.n_blocks}): a truncated or "
                             "damaged file")
        return self.bgzf_inflate(image, index)

    @_on_ctx_stream
    def fastx_format(self, bases, n_reads, read_len, offsets=None, quals=None, names=None, name_offsets=None, name_skip=1, name_base=0,
                     fmt=_lib.FASTX_FASTQ, line_width=0, qual_fill=ord("I"), rec_offsets=False):
        """kmx_fastx_format -> the batch as a FASTQ (fmt=FASTX_FASTQ) or FASTA (FASTX_FASTA) image, a uint8 device tensor sized
        exactly by a count-only call first; with rec_offsets=True -> (image, int64[n_reads + 1]: where every record starts).
        quals: laid out as the bases are (None: every quality byte is qual_fill).  names / name_offsets: a ragged batch of n_reads
        names, taken from byte name_skip on (1: without the '@' that fastx_names keeps); names None: record r is named
        name_base + r.  line_width: bases per FASTA line (0: one line)."""
        n_reads = int(n_reads)
        if (names is None) != (name_offsets is None):
            raise ValueError("names and name_offsets: both or neither")
        if names is not None and int(name_offsets.numel()) != n_reads + 1:
            raise ValueError("name_offsets: n_reads + 1 words")
        r = self._reads(bases, n_reads, read_len, offsets)
        nm = self._reads(names, n_reads, 0, name_offsets) if names is not None else None
        nb = C.c_uint64(0)
        args = (self._h, C.byref(r), _ptr(quals) if quals is not None and quals.numel() else None, C.byref(nm) if nm is not None else None,
                int(name_skip), int(name_base) & (2**64 - 1), int(fmt), int(line_width), int(qual_fill))
        self._ck(self.lib.kmx_fastx_format(*args, None, None, 0, C.byref(nb)))
        out = self.empty(max(nb.value, 1), torch.uint8)
        off = torch.zeros(n_reads + 1, dtype=torch.int64, device=self.device) if rec_offsets else None
        if n_reads:
            self._ck(self.lib.kmx_fastx_format(*args, _ptr(out), _ptr(off), nb.value, C.byref(nb)))
        return (out[:nb.value], off) if rec_offsets else out[:nb.value]

    def write_fastx(self, file, bases, n_reads, read_len, bgzf_level=None, bgzf_device=False, **kw):
        """fastx_format(bases, n_reads, read_len, **kw), one device-to-host copy, one write -> the bytes written.  `file`: a path
        or a binary file object.  bgzf_level (0..9; None: plain text): the image goes through bgzf_compress (host zlib) first.
        bgzf_device=True: the image is compressed on the device instead (bgzf_deflate) and the one copy is the .gz file; the
        device codes one form, so bgzf_level is None (that form) or 0 (stored blocks) then, and any other level is a ValueError."""
        if bgzf_device and bgzf_level is not None and int(bgzf_level) != 0:
            raise ValueError("write_fastx: bgzf_device=True has no compression levels: bgzf_level None (compressed) or 0 (stored)")
        image = self.fastx_format(bases, n_reads, read_len, **{**kw, "rec_offsets": False})
        if bgzf_device:
            image = self.bgzf_deflate(image, stored=bgzf_level is not None and int(bgzf_level) == 0)
            bgzf_level = None
        image = image.cpu().numpy()
        if bgzf_level is not None:
            image = np.frombuffer(bgzf_compress(memoryview(image), int(bgzf_level)), dtype=np.uint8)
        if isinstance(file, (str, bytes)) or hasattr(file, "__fspath__"):
            with open(file, "wb") as f:
                f.write(memoryview(image))
        else:
            file.write(memoryview(image))
        return int(image.size)

    # ------------------------------------------------------------ quality bytes acted on
    def _weights_arg(self, weights, phred):
        if weights is None:
            return None
        if isinstance(weights, str):
            if weights != "ee":
                raise ValueError('weights: None, "ee" or an int64 tensor of 256 words')
            return self.to_device(ee_weights(phred))
        if weights.dtype != torch.int64 or weights.numel() != 256 or not weights.is_cuda:
            raise ValueError("weights: an int64 CUDA tensor of 256 words, indexed by the raw quality byte")
        return weights.contiguous()

    @_on_ctx_stream
    def reads_quality(self, bases, quals, n_reads, read_len, min_q=0, trim_q=0, k=0, phred=33, weights=None, offsets=None, mask=True, out=None):
        """kmx_reads_quality -> (masked, rows): masked = the bases with every base of q < min_q turned into 'N' (same layout, same
        offsets; None with mask=False; out=bases masks in place), rows int64[n_reads, RQ_WORDS] (viewable as u64; include/kmx.h has
        the words).  weights: None, "ee" (round(2^32 * 10^(-q / 10)): RQ_WEIGHT / 2^32 is the read's expected errors, see
        expected_errors) or an int64 tensor of 256 words indexed by the raw quality byte."""
        n_reads = int(n_reads)
        w = self._weights_arg(weights, int(phred))
        masked = None
        if mask:
            masked = out if out is not None else torch.empty_like(bases)
            if masked.dtype != torch.uint8 or masked.numel() < bases.numel():
                raise ValueError("out: a uint8 tensor as large as bases")
        rows = self.empty(_lib.RQ_WORDS * n_reads, torch.int64)
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(self.lib.kmx_reads_quality(self._h, C.byref(r), _ptr(quals) if quals is not None and quals.numel() else None, int(phred), int(min_q),
                                            int(trim_q), int(k), _ptr(w) if w is not None else None,
                                            _ptr(masked) if masked is not None and masked.numel() else None, _ptr(rows) if n_reads else None))
        return masked, rows.view(-1, _lib.RQ_WORDS)

    @_on_ctx_stream
    def reads_quality_filter(self, bases, quals, n_reads, read_len, min_q=0, trim_q=0, k=0, phred=33, weights=None, offsets=None, max_ee=None,
                             min_len=0, trim="mott"):
        """reads_quality, then reads_select on its rows -> (ReadBatch of the bases, ReadBatch of the quality bytes, rows of the SOURCE
        reads).  trim = "mott" clips every read to its RQ_TRIM span, "run" to its longest run of good bases (RQ_RUN), None keeps it
        whole; max_ee drops the reads whose expected errors (weights "ee" unless a table is given) exceed it; clips shorter than
        min_len are dropped.  The bases that are kept are the MASKED ones.  One keep tensor and one span column (a strided view of
        the rows) go into two reads_select calls, so the two batches have identical offsets."""
        if trim not in ("mott", "run", None):
            raise ValueError('trim: "mott", "run" or None')
        if max_ee is not None and weights is None:
            weights = "ee"
        masked, rows = self.reads_quality(bases, quals, n_reads, read_len, min_q, trim_q, k, phred, weights, offsets)
        keep = None
        if max_ee is not None:
            keep = expected_errors(rows) <= float(max_ee)
        span = None if trim is None else rows[:, _lib.RQ_TRIM if trim == "mott" else _lib.RQ_RUN]
        b = self.reads_select(masked, n_reads, read_len, keep=keep, span=span, span_k=0, min_len=min_len, offsets=offsets, index=True)
        q = self.reads_select(quals, n_reads, read_len, keep=keep, span=span, span_k=0, min_len=min_len, offsets=offsets)
        return b, q, rows

    # ------------------------------------------------------------ adapter read-through
    @staticmethod
    def _adapters_arg(adapters):
        """adapters -> (the bytes back to back, uint32 lengths, count): one adapter as str / bytes, or a sequence of them"""
        if isinstance(adapters, (str, bytes)):
            adapters = [adapters]
        seqs = [a.encode("ascii") if isinstance(a, str) else bytes(a) for a in adapters]
        blob = b"".join(seqs)
        return (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(blob or b"\0"), (C.c_uint32 * max(len(seqs), 1))(*[len(s) for s in seqs]), len(seqs)

    def _rows_arg(self, out, words):
        rows = out if out is not None else self.empty(max(words, 1), torch.int64)
        if rows.dtype != torch.int64 or rows.numel() < words or not rows.is_contiguous():
            raise ValueError(f"out: a contiguous int64 tensor of at least {words} words")
        return rows.view(-1)

    @_on_ctx_stream
    def reads_adapter(self, bases, n_reads, read_len, adapters, min_overlap=3, max_error=(1, 10), offsets=None, out=None):
        """kmx_reads_adapter -> rows int64[n_reads, RA_WORDS] (viewable as u64; include/kmx.h has the words): per read the leftmost
        3' hit of any of `adapters` (str / bytes or a sequence of up to 8, each up to 64 of ACGTacgt and N as a wildcard; see
        ADAPTERS), with an overlap of at least min_overlap bases and at most max_error = (num, den) mismatches per overlapping
        base.  rows[:, RA_KEEP] is the span reads_select takes."""
        n_reads = int(n_reads)
        blob, lens, n_ad = self._adapters_arg(adapters)
        rows = self._rows_arg(out, _lib.RA_WORDS * n_reads)
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(self.lib.kmx_reads_adapter(self._h, C.byref(r), blob, lens, n_ad, int(min_overlap), int(max_error[0]), int(max_error[1]), _ptr(rows)))
        return rows[:_lib.RA_WORDS * n_reads].view(-1, _lib.RA_WORDS)

    @_on_ctx_stream
    def reads_trim_adapters(self, bases, n_reads, read_len, adapters, min_overlap=3, max_error=(1, 10), offsets=None, quals=None, min_len=0):
        """reads_adapter, then reads_select on RA_KEEP -> (ReadBatch of the bases with index, ReadBatch of the quality bytes or None,
        rows of the SOURCE reads): every read cut at its adapter, clips shorter than min_len dropped.  With `quals` (the layout of
        bases) the same span column goes into a second reads_select, so the two batches have identical offsets."""
        rows = self.reads_adapter(bases, n_reads, read_len, adapters, min_overlap, max_error, offsets)
        span = rows[:, _lib.RA_KEEP]
        b = self.reads_select(bases, n_reads, read_len, span=span, span_k=0, min_len=min_len, offsets=offsets, index=True)
        q = None
        if quals is not None:
            q = self.reads_select(quals, n_reads, read_len, span=span, span_k=0, min_len=min_len, offsets=offsets)
        return b, q, rows

    # ------------------------------------------------------------ poly-X ends, composition, low complexity
    @_on_ctx_stream
    def reads_complexity(self, bases, n_reads, read_len, tail="G", head="", min_len=10, max_error=(1, 10), penalty=2, dust_max=122, offsets=None,
                         mask=True, out=None):
        """kmx_reads_complexity -> (masked, rows): masked = the bases with every 64-base window whose DUST numerator exceeds dust_max
        turned into 'N' (same layout, same offsets; None with mask=False; out=bases masks in place), rows int64[n_reads, RX_WORDS]
        (viewable as u64; include/kmx.h has the words).  tail / head: the letters looked for at the 3' / 5' end, a string over ACGT
        ("G": fastp --trim_poly_g, "ACGT": --trim_poly_x, "": none); an end of at least min_len bases with at most max_error =
        (num, den) other bases per base, scored +1 a match and -(penalty) a mismatch.  rows[:, RX_KEEP] is the span reads_select
        takes; gc_content and dust_score read the other words."""
        n_reads = int(n_reads)
        masked = None
        if mask:
            masked = out if out is not None else torch.empty_like(bases)
            if masked.dtype != torch.uint8 or masked.numel() < bases.numel():
                raise ValueError("out: a uint8 tensor as large as bases")
        rows = self.empty(_lib.RX_WORDS * n_reads, torch.int64)
        r = self._reads(bases, n_reads, read_len, offsets)
        self._ck(self.lib.kmx_reads_complexity(self._h, C.byref(r), _letters_arg(tail), _letters_arg(head), int(min_len), int(max_error[0]),
                                               int(max_error[1]), int(penalty), int(dust_max),
                                               _ptr(masked) if masked is not None and masked.numel() else None, _ptr(rows) if n_reads else None))
        return masked, rows.view(-1, _lib.RX_WORDS)

    def _select_pair(self, bases, quals, n_reads, read_len, keep, span, min_len, offsets):
        """one keep tensor and one span column into two reads_select calls: the bases (with index) and the quality bytes or None, with
        identical offsets"""
        b = self.reads_select(bases, n_reads, read_len, keep=keep, span=span, span_k=0, min_len=min_len, offsets=offsets, index=True)
        q = None
        if quals is not None:
            q = self.reads_select(quals, n_reads, read_len, keep=keep, span=span, span_k=0, min_len=min_len, offsets=offsets)
        return b, q

    @_on_ctx_stream
    def reads_trim_poly(self, bases, n_reads, read_len, tail="G", head="", min_len=10, max_error=(1, 10), penalty=2, offsets=None, quals=None,
                        min_len_out=0):
        """reads_complexity, then reads_select on RX_KEEP -> (ReadBatch of the bases with index, ReadBatch of the quality bytes or None,
        rows of the SOURCE reads): every read without its poly-X tail and head, clips shorter than min_len_out dropped.  With `quals`
        (the layout of bases) the same span column goes into a second reads_select, so the two batches have identical offsets."""
        _, rows = self.reads_complexity(bases, n_reads, read_len, tail, head, min_len, max_error, penalty, _lib.RX_DUST_NEVER, offsets, mask=False)
        b, q = self._select_pair(bases, quals, n_reads, read_len, None, rows[:, _lib.RX_KEEP], min_len_out, offsets)
        return b, q, rows

    @_on_ctx_stream
    def reads_complexity_filter(self, bases, n_reads, read_len, tail="G", head="", min_len=10, max_error=(1, 10), penalty=2, dust_max=122,
                                offsets=None, min_diff=(3, 10), max_dust=None, trim=True, quals=None, min_len_out=0):
        """reads_complexity, then reads_select on its rows -> (ReadBatch of the bases with index, ReadBatch of the quality bytes or
        None, rows of the SOURCE reads).  A read is kept iff D * den >= num * P with min_diff = (num, den) -- fastp's complexity of at
        least 30 % by default, None: no such test -- and the largest DUST numerator of its windows is at most max_dust (None: no
        such test); both are exact integer comparisons on the device.  trim=True clips the kept reads to RX_KEEP; clips shorter
        than min_len_out are dropped.  The bases that are kept are the SOURCE bases, not the masked ones."""
        _, rows = self.reads_complexity(bases, n_reads, read_len, tail, head, min_len, max_error, penalty, dust_max, offsets, mask=False)
        keep = None
        if min_diff is not None:
            diff = rows[:, _lib.RX_DIFF]
            keep = (diff & 0xFFFFFFFF) * int(min_diff[1]) >= (diff >> 32) * int(min_diff[0])   # (D, P < 2^31: the words are positive)
        if max_dust is not None:
            low = (rows[:, _lib.RX_DUST] & 0xFFFFFFFF) <= int(max_dust)
            keep = low if keep is None else keep & low
        b, q = self._select_pair(bases, quals, n_reads, read_len, keep, rows[:, _lib.RX_KEEP] if trim else None, min_len_out, offsets)
        return b, q, rows

    @_on_ctx_stream
    def reads_pair_overlap(self, bases1, bases2, n_reads, read_len1, read_len2, offsets1=None, offsets2=None, min_overlap=30, max_mism=5,
                           max_error=(1, 5), out=None):
        """kmx_reads_pair_overlap -> rows int64[n_reads, RP_WORDS]: per mate pair the insert size from the overlap of mate 1 with the
        reverse complement of mate 2 (at least min_overlap bases, at most max_mism mismatches and max_error = (num, den) per
        overlapping base; the longest overlap, of equal ones the longer insert), and the spans that cut the read-through off both
        mates (RP_KEEP1, RP_KEEP2)."""
        n_reads = int(n_reads)
        rows = self._rows_arg(out, _lib.RP_WORDS * n_reads)
        r1 = self._reads(bases1, n_reads, read_len1, offsets1)
        r2 = self._reads(bases2, n_reads, read_len2, offsets2)
        self._ck(self.lib.kmx_reads_pair_overlap(self._h, C.byref(r1), C.byref(r2), int(min_overlap), int(max_mism), int(max_error[0]),
                                                 int(max_error[1]), _ptr(rows)))
        return rows[:_lib.RP_WORDS * n_reads].view(-1, _lib.RP_WORDS)

    @_on_ctx_stream
    def reads_trim_pairs(self, bases1, bases2, n_reads, read_len1, read_len2, offsets1=None, offsets2=None, min_overlap=30, max_mism=5,
                         max_error=(1, 5), min_len=0):
        """reads_pair_overlap, then reads_select on RP_KEEP1 / RP_KEEP2 -> (ReadBatch of mate 1, ReadBatch of mate 2, rows of the
        SOURCE pairs).  A pair is dropped when either clip is shorter than min_len -- one keep tensor, computed from the two span
        words, goes into both calls, so the two batches stay in step (both carry the index of the source pair)."""
        rows = self.reads_pair_overlap(bases1, bases2, n_reads, read_len1, read_len2, offsets1, offsets2, min_overlap, max_mism, max_error)
        keep = ((rows[:, _lib.RP_KEEP1] >> 32) >= int(min_len)) & ((rows[:, _lib.RP_KEEP2] >> 32) >= int(min_len))
        b1 = self.reads_select(bases1, n_reads, read_len1, keep=keep, span=rows[:, _lib.RP_KEEP1], span_k=0, offsets=offsets1, index=True)
        b2 = self.reads_select(bases2, n_reads, read_len2, keep=keep, span=rows[:, _lib.RP_KEEP2], span_k=0, offsets=offsets2, index=True)
        return b1, b2, rows

    # ------------------------------------------------------------ overlapping mates merged into consensus reads
    @_on_ctx_stream
    def reads_pair_merge(self, bases1, bases2, n_reads, read_len1, read_len2, insert, quals1=None, quals2=None, offsets1=None, offsets2=None,
                         phred_base=33, q_cap=41, rows=True):
        """kmx_reads_pair_merge -> (ReadBatch of the merged bases, ReadBatch of their quality bytes or None, rows
        int64[n_reads, RM_WORDS] or None).  Both batches have n_reads reads and identical offsets: read r is the consensus of pair
        r, empty where the pair does not merge.  `insert`: a 1-D int64 tensor of insert sizes, one per pair, with any positive
        element stride -- reads_pair_overlap(...)[:, RP_INSERT] is handed over as it is.  quals1 / quals2 (both or neither): the
        quality bytes, laid out as the bases; without them mate 1 wins every disagreement.  include/kmx.h has the consensus rule
        and the words of a row.  Sizing: a count-only call first, then the write into buffers of exactly that size."""
        n_reads = int(n_reads)
        if (quals1 is None) != (quals2 is None):
            raise ValueError("quals1 and quals2: both or neither")
        ins_t, ins_p, stride = self._span_arg(insert)
        if n_reads and (ins_t is None or ins_t.numel() < n_reads):
            raise ValueError("insert: one word per pair")
        r1 = self._reads(bases1, n_reads, read_len1, offsets1)
        r2 = self._reads(bases2, n_reads, read_len2, offsets2)
        nm, nb = C.c_uint64(0), C.c_uint64(0)
        args = (self._h, C.byref(r1), C.byref(r2), _ptr(quals1), _ptr(quals2), ins_p, max(stride, 1), int(phred_base), int(q_cap))
        self._ck(self.lib.kmx_reads_pair_merge(*args, None, None, None, None, 0, C.byref(nm), C.byref(nb)))
        out = self.empty(max(nb.value, 1), torch.uint8)   # (a pointer also where nothing merges)
        outq = self.empty(max(nb.value, 1), torch.uint8) if quals1 is not None else None
        off = torch.zeros(n_reads + 1, dtype=torch.int64, device=self.device)
        rws = self.empty(_lib.RM_WORDS * n_reads, torch.int64) if rows else None
        if n_reads:
            self._ck(self.lib.kmx_reads_pair_merge(*args, _ptr(out), _ptr(outq), _ptr(off), _ptr(rws), nb.value, C.byref(nm), C.byref(nb)))
        b = ReadBatch(out[:nb.value], off, n_reads, None, self)
        q = ReadBatch(outq[:nb.value], off, n_reads, None, self) if outq is not None else None
        return b, q, rws.view(-1, _lib.RM_WORDS) if rows else None

    @_on_ctx_stream
    def reads_merge_pairs(self, bases1, bases2, n_reads, read_len1, read_len2, quals1=None, quals2=None, offsets1=None, offsets2=None,
                          min_overlap=30, max_mism=5, max_error=(1, 5), phred_base=33, q_cap=41):
        """reads_pair_overlap, reads_pair_merge, then reads_select -> MergedPairs: the merged reads and their quality bytes,
        compacted, with the index of the source pair; the pairs that did not merge as a mate-1 and a mate-2 batch that stay in
        step (with their quality bytes where given, and the pair index); the rows of both calls for the SOURCE pairs.  ONE keep
        tensor, rows[:, RM_LEN] != 0, goes into all the selects (negated for the unmerged mates)."""
        n_reads = int(n_reads)
        overlap_rows = self.reads_pair_overlap(bases1, bases2, n_reads, read_len1, read_len2, offsets1, offsets2, min_overlap, max_mism, max_error)
        m, mq, merge_rows = self.reads_pair_merge(bases1, bases2, n_reads, read_len1, read_len2, overlap_rows[:, _lib.RP_INSERT], quals1, quals2,
                                                  offsets1, offsets2, phred_base, q_cap)
        keep = merge_rows[:, _lib.RM_LEN] != 0
        drop = ~keep
        some = lambda t: t if t.numel() else self.empty(1, torch.uint8)   # (a pointer also where nothing merges)
        merged = self.reads_select(some(m.bases), n_reads, 0, keep=keep, offsets=m.offsets, index=True)
        merged_q = self.reads_select(some(mq.bases), n_reads, 0, keep=keep, offsets=mq.offsets) if mq is not None else None
        un1 = self.reads_select(bases1, n_reads, read_len1, keep=drop, offsets=offsets1, index=True)
        un2 = self.reads_select(bases2, n_reads, read_len2, keep=drop, offsets=offsets2, index=True)
        un1_q = self.reads_select(quals1, n_reads, read_len1, keep=drop, offsets=offsets1) if quals1 is not None else None
        un2_q = self.reads_select(quals2, n_reads, read_len2, keep=drop, offsets=offsets2) if quals2 is not None else None
        return MergedPairs(merged, merged_q, un1, un2, un1_q, un2_q, overlap_rows, merge_rows)

    # ------------------------------------------------------------ duplicate reads and read pairs
    @staticmethod
    def _mates_arg(mates):
        """mates -> (bases, read_len, offsets): a ReadBatch, or a tuple (bases, read_len) / (bases, read_len, offsets)"""
        if isinstance(mates, ReadBatch):
            return mates.bases, mates.max_len(), mates.offsets
        if len(mates) == 2:
            return mates[0], mates[1], None
        return tuple(mates)

    @_on_ctx_stream
    def reads_dedup(self, bases, n_reads, read_len, offsets=None, mates=None, strand=False, score=None, hash_bits=64) -> ReadDuplicates:
        """kmx_reads_dedup -> ReadDuplicates: exact duplicate reads, or mate pairs with `mates` (a ReadBatch, or (bases, read_len) /
        (bases, read_len, offsets) of as many reads), found by a 64-bit fingerprint and verified letter by letter against the
        read they would be dropped for.  Case is ignored and every byte that is not ACGT is one letter.  strand=True: a read's
        reverse complement, or a pair with its mates exchanged, is the same item.  `score`: a 1-D int64 tensor, one word per item
        with any positive element stride (reads_quality(...)[1][:, RQ_QSUM] as it is): the best-scored copy of a class survives,
        ties and no score keep the first.  include/kmx.h has the contract."""
        n_reads = int(n_reads)
        sc_t, sc_p, stride = self._span_arg(score)
        if sc_t is not None and sc_t.numel() < n_reads:
            raise ValueError("score: one word per item")
        r1 = self._reads(bases, n_reads, read_len, offsets)
        r2 = None
        if mates is not None:
            mb, ml, mo = self._mates_arg(mates)
            r2 = self._reads(mb, n_reads, ml, mo)
        rows = self.empty(max(_lib.DD_WORDS * n_reads, 1), torch.int64)   # (a pointer also for no reads)
        keep = self.empty(max(n_reads, 1), torch.uint8)
        summ = (C.c_uint64 * _lib.DD_SUMMARY_WORDS)()
        self._ck(self.lib.kmx_reads_dedup(self._h, C.byref(r1), C.byref(r2) if r2 is not None else None, _lib.DD_STRAND if strand else 0,
                                          int(hash_bits), sc_p, max(stride, 1), _ptr(rows), _ptr(keep), summ))
        return ReadDuplicates(rows[:_lib.DD_WORDS * n_reads].view(-1, _lib.DD_WORDS), keep[:n_reads], int(summ[_lib.DD_S_KEPT]), int(summ[_lib.DD_S_DROPPED]),
                              int(summ[_lib.DD_S_LARGEST]), int(summ[_lib.DD_S_COLLISIONS]))

    @_on_ctx_stream
    def reads_drop_duplicates(self, bases, n_reads, read_len, offsets=None, quals=None, mates=None, mate_quals=None, strand=False, score=None,
                              hash_bits=64) -> DeduplicatedReads:
        """reads_dedup, then reads_select on its keep bytes -> DeduplicatedReads.  ONE keep tensor goes into every select -- the
        bases, the quality bytes (laid out as their bases), and for pairs both mates -- so all the batches stay in step."""
        n_reads = int(n_reads)
        d = self.reads_dedup(bases, n_reads, read_len, offsets, mates, strand, score, hash_bits)
        b = self.reads_select(bases, n_reads, read_len, keep=d.keep, offsets=offsets, index=True)
        q = self.reads_select(quals, n_reads, read_len, keep=d.keep, offsets=offsets) if quals is not None else None
        m = mq = None
        if mates is not None:
            mb, ml, mo = self._mates_arg(mates)
            m = self.reads_select(mb, n_reads, ml, keep=d.keep, offsets=mo, index=True)
            mq = self.reads_select(mate_quals, n_reads, ml, keep=d.keep, offsets=mo) if mate_quals is not None else None
        return DeduplicatedReads(b, q, m, mq, d)

    # ------------------------------------------------------------ a new batch of reads from an old one
    @staticmethod
    def _span_arg(span):
        """span -> (tensor to keep alive, pointer, stride in words).  ONE form: a 1-D int64 tensor of span words, one per source
        read, with any positive element stride -- so a column view such as stats[:, RS_SPAN] of the [n_reads, 8] stats tensor is
        passed as it is, without a copy."""
        if span is None:
            return None, None, 0
        if span.dtype != torch.int64 or span.dim() != 1 or not span.is_cuda:
            raise ValueError("span: a 1-D int64 CUDA tensor of span words (a strided column view is fine)")
        if span.numel() == 0:
            return None, None, 0
        stride = int(span.stride(0)) if span.numel() > 1 else 1
        if stride < 1:
            raise ValueError("span: the element stride must be positive")
        return span, C.c_void_p(span.data_ptr()), stride

    @_on_ctx_stream
    def reads_select(self, bases, n_reads, read_len, keep=None, span=None, span_k=0, min_len=0, offsets=None, index=False) -> ReadBatch:
        """kmx_reads_select -> ReadBatch: the reads with keep[r] != 0 (keep: uint8 or bool per read; None = all), each clipped to its
        span, those whose clip is shorter than min_len dropped, back to back in source order.  `span`: a 1-D int64 tensor of span
        words (start in the low 32 bits, length in the high 32), one per source read; it may be a strided view, so
        stats[:, RS_SPAN] of count_read_stats is handed over without a copy.  span_k = 0: the length counts bases; span_k = k: it
        counts windows of k bases (the packing of RS_SPAN and PATH_SPAN).  index=True also returns the source index of every output
        read.  Sizing: one count-only call first, then the write into buffers of exactly that size (two host round trips, no
        over-allocation)."""
        n_reads = int(n_reads)
        if keep is not None:
            keep = keep.view(torch.uint8) if keep.dtype == torch.bool else keep
            if keep.dtype != torch.uint8 or keep.numel() < n_reads:
                raise ValueError("keep: one uint8 / bool per read")
        span_t, span_p, stride = self._span_arg(span)
        if span_t is not None and span_t.numel() < n_reads:
            raise ValueError("span: one word per read")
        r = self._reads(bases, n_reads, read_len, offsets)
        nr, nb = C.c_uint64(0), C.c_uint64(0)
        args = (self._h, C.byref(r), _ptr(keep) if keep is not None and n_reads else None, span_p, stride, int(span_k), int(min_len))
        self._ck(self.lib.kmx_reads_select(*args, None, None, None, 0, 0, C.byref(nr), C.byref(nb)))
        out = self.empty(max(nb.value, 1), torch.uint8)   # (a pointer also for a batch of empty reads)
        off = torch.zeros(nr.value + 1, dtype=torch.int64, device=self.device)
        idx = self.empty(nr.value, torch.int64) if index else None
        if n_reads:
            self._ck(self.lib.kmx_reads_select(*args, _ptr(out), _ptr(off),
                                               _ptr(idx) if index and nr.value else None, nr.value, nb.value, C.byref(nr), C.byref(nb)))
        return ReadBatch(out[:nb.value], off, int(nr.value), idx, self)

    @_on_ctx_stream
    def reads_gather(self, bases, n_reads, read_len, index, span=None, span_k=0, offsets=None) -> ReadBatch:
        """kmx_reads_gather -> ReadBatch: output read j is the clip of source read index[j] (int64; repeats allowed, an index
        outside [0, n_reads) gives an empty read); `span` / span_k as in reads_select, looked up by the source index.  Sizing: a
        count-only call first, then the write into buffers of exactly that size."""
        index = index.contiguous()
        if index.dtype != torch.int64:
            raise ValueError("index: int64")
        n_index = int(index.numel())
        span_t, span_p, stride = self._span_arg(span)
        if span_t is not None and span_t.numel() < int(n_reads):
            raise ValueError("span: one word per source read")
        r = self._reads(bases, n_reads, read_len, offsets)
        nb = C.c_uint64(0)
        args = (self._h, C.byref(r), _ptr(index) if n_index else None, n_index, span_p, stride, int(span_k))
        self._ck(self.lib.kmx_reads_gather(*args, None, None, 0, C.byref(nb)))
        out = self.empty(max(nb.value, 1), torch.uint8)
        off = torch.zeros(n_index + 1, dtype=torch.int64, device=self.device)
        if n_index:
            self._ck(self.lib.kmx_reads_gather(*args, _ptr(out), _ptr(off), nb.value, C.byref(nb)))
        return ReadBatch(out[:nb.value], off, n_index, index, self)

    @_on_ctx_stream
    def reads_partition(self, bases, n_reads, read_len, labels, offsets=None) -> ReadGroups:
        """The batch split by a label per read (int64[n_reads]; a negative label drops the read) -> ReadGroups: the reads grouped
        by label ascending, source order within a group.  The stable sort of the labels and the group boundaries are torch; the
        copy is ONE kmx_reads_gather over the sorted index.  What ReadPaths.read_components or a colour per read feed."""
        labels = labels.reshape(-1)[:int(n_reads)].to(torch.int64)
        order = torch.sort(labels, stable=True).indices
        order = order[labels[order] >= 0]
        distinct, counts = torch.unique_consecutive(labels[order], return_counts=True)
        group_offsets = torch.zeros(distinct.numel() + 1, dtype=torch.int64, device=labels.device)
        group_offsets[1:] = torch.cumsum(counts, 0)
        batch = self.reads_gather(bases, n_reads, read_len, order, offsets=offsets)
        return ReadGroups(batch, distinct, group_offsets)

    def _select_reads(self, stats_fn, bases, n_reads, read_len, k, kmers, counts, solid_min, min_median, max_median, trim, min_len, offsets):
        stats = stats_fn(bases, n_reads, read_len, k, kmers, counts, solid_min=solid_min, offsets=offsets)
        med = stats[:, _lib.RS_MEDIAN]
        keep = _u64_ge(med, int(min_median)) & _u64_le(med, int(max_median))
        batch = self.reads_select(bases, n_reads, read_len, keep=keep, span=stats[:, RS_SPAN] if trim else None, span_k=int(k) if trim else 0,
                                  min_len=int(k) if min_len is None else int(min_len), offsets=offsets, index=True)
        return batch, stats

    @_on_ctx_stream
    def count_select_reads(self, bases, n_reads, read_len, k, kmers, counts, solid_min=2, min_median=0, max_median=2**64 - 1, trim=True,
                           min_len=None, offsets=None):
        """count_read_stats, then reads_select on its rows -> (ReadBatch with index, stats int64[n_reads, 8]): a read is kept iff
        min_median <= its median abundance (RS_MEDIAN, as u64) <= max_median; with `trim` it is clipped to its longest run of
        solid windows (RS_SPAN, windows of k bases); clips shorter than min_len (default k: one window) are dropped.  The abundance
        cut is the ONE-SHOT, order-independent form of digital normalisation -- every read is judged against the table of the whole
        batch -- not the streaming one, whose table grows with the reads it has kept.  The stats are those of the SOURCE reads.
        Sizing as reads_select: count first, then exactly sized buffers."""
        return self._select_reads(self.count_read_stats, bases, n_reads, read_len, k, kmers, counts, solid_min, min_median, max_median, trim, min_len,
                                  offsets)

    @_on_ctx_stream
    def count_select_reads2(self, bases, n_reads, read_len, k, kmers, counts, solid_min=2, min_median=0, max_median=2**64 - 1, trim=True,
                            min_len=None, offsets=None):
        """count_select_reads for two-word keys (k 33..64; kmers int64[n, 2])."""
        return self._select_reads(self.count_read_stats2, bases, n_reads, read_len, k, kmers, counts, solid_min, min_median, max_median, trim, min_len,
                                  offsets)

    @_on_ctx_stream
    def reads_length_range(self, offsets: torch.Tensor) -> tuple[int, int]:
        """kmx_reads_length_range: (shortest, longest) read of a ragged batch (offsets: int64[n_reads+1] on the device)"""
        n = int(offsets.numel()) - 1
        mn, mx = C.c_uint32(0), C.c_uint32(0)
        self._ck(self.lib.kmx_reads_length_range(self._h, _ptr(offsets) if n > 0 else None, max(n, 0), C.byref(mn), C.byref(mx)))
        return mn.value, mx.value

    @_on_ctx_stream
    def encoding_decode(self, words: torch.Tensor, enc_byte: int, words_per_kmer: int) -> torch.Tensor:
        n = words.numel() // words_per_kmer
        out = self.empty(n * 32 * words_per_kmer, torch.uint8)
        self._ck(self.lib.kmx_encoding_decode(self._h, _ptr(words), n, enc_byte, words_per_kmer, _ptr(out)))
        return out

    # ---- decode / display direction
    @_on_ctx_stream
    def sub_kmer_words(self, words: torch.Tensor, k: int, pos: int, width: int) -> torch.Tensor:
        """Kmer::sub_kmer_word (kmer.rs:156-162) per word"""
        out = torch.empty_like(words)
        n = words.numel()
        self._ck(self.lib.kmx_sub_kmer_words(self._h, _ptr(words) if n else None, n, k, pos, width, _ptr(out) if n else None))
        return out

    @_on_ctx_stream
    def kmers_to_strings(self, words: torch.Tensor, k: int) -> torch.Tensor:
        """String::from(Kmer) (kmer.rs:196-207): uint8[n*k], lower case"""
        n = words.numel()
        out = self.empty(n * k, torch.uint8)
        self._ck(self.lib.kmx_kmers_to_strings(self._h, _ptr(words) if n else None, n, k, _ptr(out) if n * k else None))
        return out

    @_on_ctx_stream
    def bitmers_to_bytes(self, mers: torch.Tensor, length: int) -> torch.Tensor:
        """kmer::bitmer_to_bytes (src/kmer.rs:71-91): uint8[n*len], upper case"""
        n = mers.numel()
        out = self.empty(n * length, torch.uint8)
        self._ck(self.lib.kmx_bitmers_to_bytes(self._h, _ptr(mers) if n else None, n, length, _ptr(out) if n * length else None))
        return out

    # ---- Encoding<P, B> for any utils::Data word type (byte image of [P; B])
    @_on_ctx_stream
    def encode_kmers_p(self, seqs: torch.Tensor, n: int, seq_len: int, enc_byte: int, word_bits: int, words_per_kmer: int) -> torch.Tensor:
        out = self.empty(n * (word_bits // 8) * words_per_kmer, torch.uint8)
        self._ck(self.lib.kmx_encode_kmers_p(self._h, _ptr(seqs) if seqs.numel() else None, n, seq_len, enc_byte, word_bits,
                                             words_per_kmer, _ptr(out) if out.numel() else None))
        return out

    @_on_ctx_stream
    def encoding_rev_comp_p(self, arrays: torch.Tensor, K: int, enc_byte: int, word_bits: int, words_per_kmer: int) -> torch.Tensor:
        out = torch.empty_like(arrays)
        n = arrays.numel() // ((word_bits // 8) * words_per_kmer)
        self._ck(self.lib.kmx_encoding_rev_comp_p(self._h, _ptr(arrays) if n else None, n, K, enc_byte, word_bits, words_per_kmer,
                                                  _ptr(out) if n else None))
        return out

    @_on_ctx_stream
    def encoding_decode_p(self, arrays: torch.Tensor, enc_byte: int, word_bits: int, words_per_kmer: int) -> torch.Tensor:
        n = arrays.numel() // ((word_bits // 8) * words_per_kmer)
        out = self.empty(arrays.numel() * 4, torch.uint8)
        self._ck(self.lib.kmx_encoding_decode_p(self._h, _ptr(arrays) if n else None, n, enc_byte, word_bits, words_per_kmer,
                                                _ptr(out) if n else None))
        return out

    # ---- measurement helper
    @_on_ctx_stream
    def calib_stream_read(self, buf: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """kmx_calib_stream_read: read-only pass over `buf` with the scan's load shape (async; returns the 1-word xor fold)"""
        out = self.empty(1, torch.int64) if out is None else out
        self._ck(self.lib.kmx_calib_stream_read(self._h, _ptr(buf) if buf.numel() else None, buf.numel() * buf.element_size(), _ptr(out)))
        return out


class Comm:
    """kmx_comm: the RCCL communicator behind the C ABI (include/kmx.h, "multi-GPU exchange").  One per Context.

    `exchange_id(id_bytes_or_None) -> bytes` hands rank 0's unique id to the other ranks; with torch.distributed
    initialised the default does it with one broadcast."""

    def __init__(self, ctx: Context, n_ranks: int, rank: int, exchange_id=None):
        self.ctx = ctx
        lib = ctx.lib
        buf = (C.c_uint8 * _lib.COMM_ID_BYTES)()
        # rank 0's status travels WITH the id (one extra byte): if kmx_comm_get_unique_id fails there -- no RCCL on the loader
        # path, say -- every rank learns it from the same broadcast and raises, instead of rank 0 raising alone while the
        # others wait in ncclCommInitRank for a peer that never comes.
        st0 = lib.kmx_comm_get_unique_id(buf) if rank == 0 else 0
        if n_ranks > 1:
            if exchange_id is None:
                exchange_id = self._torch_broadcast
            raw = exchange_id((bytes(buf) + bytes([st0 & 0xFF])) if rank == 0 else None)
            if len(raw) > _lib.COMM_ID_BYTES:
                st0 = raw[_lib.COMM_ID_BYTES]
                raw = raw[:_lib.COMM_ID_BYTES]
            buf = (C.c_uint8 * _lib.COMM_ID_BYTES).from_buffer_copy(raw)
        if st0 != 0:
            raise KmxError(int(st0), "kmx_comm_get_unique_id failed on rank 0 (is librccl.so.1 on the loader path?)")
        h = C.c_void_p()
        ctx._ck(lib.kmx_comm_create(ctx._h, buf, n_ranks, rank, C.byref(h)))
        self._h = h
        self.n_ranks, self.rank = n_ranks, rank

    def _torch_broadcast(self, raw):
        import torch.distributed as dist

        t = torch.zeros(_lib.COMM_ID_BYTES + 1, dtype=torch.uint8)   # the id + rank 0's status byte
        if raw is not None:
            t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).clone()
        if dist.get_backend() == "nccl":
            t = t.to(self.ctx.device)
        dist.broadcast(t, src=0)
        return bytes(t.cpu().numpy().tobytes())

    def close(self):
        if getattr(self, "_h", None):
            self.ctx.lib.kmx_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self) -> int:
        return self.ctx.lib.kmx_comm_size(self._h)

    def histogram_allreduce(self, counts: torch.Tensor) -> torch.Tensor:
        """in-place sum over ranks of the 2^b u64 counters (ncclAllReduce, ncclUint64/ncclSum) on the context's stream"""
        counts.record_stream(self.ctx.stream)
        self.ctx._ck(self.ctx.lib.kmx_histogram_allreduce(self._h, _ptr(counts), counts.numel()))
        return counts

    def summary_allreduce(self, summary: torch.Tensor) -> torch.Tensor:
        """in-place combine of the device-resident 32-byte kmx_summary of every rank"""
        summary.record_stream(self.ctx.stream)
        self.ctx._ck(self.ctx.lib.kmx_summary_allreduce(self._h, _ptr(summary)))
        return summary
