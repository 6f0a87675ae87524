"""The seeded differential fuzz of the read-preparation calls, host side: what tests/test_gpu_reads_fuzz.py runs on the device and
tests/test_reads_fuzz_plan.py checks on the CPU.  The structure is that of tests/count_fuzz_np.py, whose Layout, guard bytes, ragged()
and _dirty() are imported, not copied.

* plan(seed): a pure function from the seed to the configuration of one case -- the two FASTQ images' line ends, the mates' lengths,
  the adapter set, every call's parameters, the stream, the layouts the batches may be handed over as.
* case_of(plan): the two FASTQ texts TOGETHER WITH the reads and quality strings they were built from (the parse reference by
  construction), the fragments the pairs were cut from and which pairs are error-free.
* handovers(plan, case): per layout of the plan, the four host buffers (bases and quality bytes of both mates) with their guard
  bytes, leads, first offset and bounds.
* host_pipeline(plan): the existing references end to end, each stage fed by the previous stage's reference output -> a dict of
  named arrays (STAGES lists which names belong to which stage).  No reference is written here.
* structure(plan, H): what a seed has to get wrong, read off the reference's arrays alone (for the second library: and off its record
  of what was planted where).
* library_of(plan): the seed's second library -- the case's pairs plus planted copies, near-copies, poly-X ends, low-complexity reads
  and odd names -- as two FASTQ images with the reads, quality strings and names they were built from; lib_handovers(plan, library)
  its raw mates and names per layout; library_pipeline its reference chain (dedup_np, complexity_np, fastx_out_np, reads_np and
  quality_np: no reference is written here either), which host_pipeline appends to its dict.

Where the issue's wording leaves a choice, it is made here and said here:

* A uniform batch needs mates of ONE length, so the pairs with mates of 1 000 .. 1 030 bases (seed % 8 in (3, 6): a quarter of the
  seeds, of both parities) always come in length mode "mix"; the other seeds are of mode "one" when seed % 5 is 0 or 3.
* The quality calls use the plan's phred_base as `phred`, so bytes below the base occur for both bases (a space for 33).
* Mate 2 is trimmed to its longest run of GOOD bases before the overlap (stage 5), so it holds no invalid byte when the chain merges:
  a position where NEITHER mate is valid cannot occur there.  The flag merge_none is therefore read off the reference merge of the
  RAW parsed mates (ROUTES: what the route pass runs on every layout and compares with these arrays), where fragments that carry an
  N give both mates one at the same place.
* The overlap's max_mism is drawn from (5, 2, 5, 1, 8): with 0 no pair that merges has a disagreement, and a fifth of the seeds would
  have nothing to get wrong in the consensus rule.
* The route pass hands over the two PARSED mate files (the only batches that can be uniform); the chain hands the device-parsed files
  to its next stage as the plan's first layout.

* The SECOND library of a seed (library_of: "the library with copies") is what the stages records .. reparse run on.  It draws from
  generators of its own (70 000 + and 71 000 + seed), so the first library's plan fields, texts and reference arrays are what they
  were.  Its reads have no one length (a near-copy is a base shorter, the (AC)n reads are 63 .. 97 bases long), so it never comes as
  a uniform batch: lib_handovers hands it over as the plan's ragged and misaligned layouts (a misaligned uniform one as a misaligned
  ragged one) and leaves "uniform" out -- its ragged twin is "ragged_bound".
* The new plan fields are not drawn one by one but SCHEDULED (_scheduled): per block of 48 seeds and per stream every value of a
  field comes equally often, in an order drawn per field, so the default set covers every value on both streams by construction.
  The two poly-X masks are scheduled as a pair that is never (0, 0): a seed without a mask would have nothing to trim.
* The library is at most 1.4 x n_pairs items (1.3 and less from 140 pairs on): 1.25 is not enough for the smallest libraries (96 pairs) to hold every planted
  kind AND one dropped item in ten.  The class of 40 copies (seed % 6 == 2) comes on top of that, as 40 short pairs of 30 bases.
* A duplicate is missed where its key collides with a better ranked item, so with hash_bits of 8, 4 or 1 the call keeps most copies:
  the share of dropped items is a condition of the seeds with hash_bits == 64 only.
* dedup_single and the poly stage need a batch, not keep bytes: dedup_single ends in reads_select on the keep bytes (bases, quality
  bytes) and reads_gather of the names; its score, where the plan has one, is the pair stage's score column gathered by the
  survivors' index (a contiguous tensor either way).
* reads_complexity_filter is called with min_diff from the plan and without max_dust.

numpy only: the oracle is loaded inside host_pipeline, torch nowhere.
"""
import dataclasses
import functools

import numpy as np

from tests import adapter_np as A
from tests import complexity_np as X
from tests import dedup_np as D
from tests import fastx_out_np as FO
from tests import merge_np as M
from tests import quality_np as Q
from tests import reads_np
from tests.count_fuzz_np import COMP, GUARD_BYTES, KS, ONE_LENGTHS, Layout, _dirty, ragged, rc_read
from tests.count_np import orc_windows, table_of
from tests.fastx_cases import QUAL_ALPHA

LAYOUTS = ("uniform", "ragged0", "ragged_bound", "misaligned")
N_DEFAULT = 48
MAX_BASES = 24_000
LONG_AT = ((1024, 1024), (1024, 1001), (1000, 1024))                        # on both sides of KMX_RP_MAX_LEN: these merge ...
LONG_OVER = ((1025, 1000), (1000, 1025), (1030, 1024), (1012, 1029))        # ... these have no hit by definition
MAX_ERRORS = ((1, 10), (1, 5), (3, 10), (0, 1))
GATHER_N = 40

_ACGT = np.frombuffer(b"ACGT", np.uint8)
_VALID = np.zeros(256, bool)
_VALID[list(b"ACGTacgtN")] = True

STAGES = {
    "parse": ("p1_bases", "p1_quals", "p1_offsets", "p1_layout", "p2_bases", "p2_quals", "p2_offsets", "p2_layout"),
    "adapter": ("ad_rows", "ta_bases", "ta_quals", "ta_offsets", "ta_index"),
    "quality": ("q_masked", "q_rows", "qf_bases", "qf_quals", "qf_offsets", "qf_index"),
    "count": ("table_k", "table_c"),
    "pair_quality": ("pq1_bases", "pq1_quals", "pq1_offsets", "pq1_index", "pq1_rows", "pq2_bases", "pq2_quals", "pq2_offsets", "pq2_index",
                     "pq2_rows"),
    "overlap": ("ov_rows", "tp1_bases", "tp1_offsets", "tp1_index", "tp2_bases", "tp2_offsets", "tp2_index"),
    "merge": ("mg_bases", "mg_quals", "mg_offsets", "mg_rows", "mgn_bases", "mgn_offsets", "mgn_rows"),
    "merge_pairs": ("mp_m_bases", "mp_m_offsets", "mp_m_index", "mp_mq_bases", "mp_u1_bases", "mp_u1_offsets", "mp_u1_index", "mp_u2_bases",
                    "mp_u2_offsets", "mp_u2_index", "mp_u1q_bases", "mp_u2q_bases", "mp_ov_rows", "mp_mg_rows"),
    "partition": ("pt_bases", "pt_offsets", "pt_index", "pt_labels", "pt_groups"),
    # ---- the second library
    "records": tuple(f"r{m}_{x}" for m in (1, 2) for x in ("bases", "quals", "offsets", "layout", "names", "noffsets")),
    "dedup_pairs": ("lq_rows", "dd_rows", "dd_keep", "dd_summary", "dp1_bases", "dp1_quals", "dp1_offsets", "dp1_index", "dp2_bases", "dp2_quals",
                    "dp2_offsets", "dp2_index", "dpn_bases", "dpn_offsets"),
    "dedup_single": ("ds_rows", "ds_keep", "ds_summary", "ds_bases", "ds_quals", "ds_offsets", "ds_index", "dsn_bases", "dsn_offsets"),
    "poly": ("cx_rows", "cx_masked", "xt_rows", "xt_bases", "xt_quals", "xt_offsets", "xt_index", "xf_bases", "xf_quals", "xf_offsets", "xf_index",
             "xfn_bases", "xfn_offsets"),
    "count_masked": ("cm_k", "cm_c"),
    "format": ("fq_image", "fq_rec", "fa_image", "fa_rec", "gq_image", "gq_rec"),
    "reparse": ("rp_bases", "rp_quals", "rp_offsets", "rp_layout", "rp_names", "rp_noffsets"),
}
FIRST_LIBRARY = ("parse", "adapter", "quality", "count", "pair_quality", "overlap", "merge", "merge_pairs", "partition")
# the references of the route pass, on the raw parsed mates: adapter rows are ad_rows; these are the rest
ROUTES = ("rt_q_masked", "rt_q_rows", "rt_ov_rows", "rt_mg_bases", "rt_mg_quals", "rt_mg_offsets", "rt_mg_rows", "rt_sel_bases", "rt_sel_offsets",
          "rt_sel_index", "rt_gat_bases", "rt_gat_offsets")
# the route pass of the second library, on its raw mates (mate 1 for the two single-batch calls)
ROUTES2 = ("rt2_dd_rows", "rt2_dd_keep", "rt2_dd_summary", "rt2_cx_rows", "rt2_cx_masked", "rt2_fq_image", "rt2_fq_rec")

DD_HASH_BITS = (64, 64, 64, 8, 4, 1)
DD_SCORES = ("none", "strided", "contiguous")
PX_MASKS = (0, 4, 15, 9)                                                    # none, G, ACGT, A and T
PX_PAIRS = tuple((t, h) for t in PX_MASKS[1:] for h in PX_MASKS[1:]) + tuple((t, 0) for t in PX_MASKS[1:]) + tuple((0, h) for h in PX_MASKS[1:])
PX_MIN_LENS = (5, 10, 20)
PX_MAX_ERRORS = ((0, 1), (1, 10), (1, 4))
PX_PENALTIES = (0, 2, 255)
DUST_MAXES = (60, 122, 610, 930)
MIN_DIFFS = ((3, 10), (1, 2), (1, 5))
FA_WIDTHS = (0, 1, 60, 61, 70)
NAME_SKIPS = (0, 1, 3)
LC_LENGTHS = (63, 64, 65, 96, 97)
NEAR_KINDS = ("near_last", "near_first", "near_shorter", "near_mate2")


@dataclasses.dataclass(frozen=True)
class Plan:
    seed: int
    stream: str                # "side" (odd seeds) or "default"
    n_pairs: int
    length_mode: str           # "one" or "mix"
    len1: int                  # mode "one": the length of every mate 1 (len2: of every mate 2); mode "mix": 0
    len2: int
    mix_max: int               # mode "mix": the longest of the mixed lengths; mode "one": 0
    long_pairs: tuple          # mode "mix": (L1, L2) of the pairs with mates of 1 000 .. 1 030 bases
    crlf: tuple                # per mate file
    trail: tuple               # per mate file: the final newline is there
    adapters: tuple            # of bytes
    ad_min_overlap: int
    ad_max_error: tuple        # (num, den)
    min_q: int
    trim_q: int
    k: int                     # the window length of reads_quality
    max_ee: float
    trim: object               # "mott", "run" or None
    min_len: int
    phred_base: int
    q_cap: int
    ov_min_overlap: int
    ov_max_mism: int
    count_k: int
    sub_rate: float
    dirty_every: int
    layouts: tuple             # of Layout, bounds of mate 1; the first is the one the chain hands the parsed files over as
    layouts2: tuple            # the same layouts with the bounds of mate 2
    # ---- the calls on the second library
    dd_strand: bool
    dd_hash_bits: int
    dd_score: str              # "none", "strided" (the RQ_QSUM column as it stands) or "contiguous" (a copy of it)
    px_tail: int               # base masks
    px_head: int
    px_min_len: int
    px_max_error: tuple        # (num, den)
    px_penalty: int
    dust_max: int
    min_diff: tuple            # (num, den)
    fa_width: int
    name_skip: int

    @property
    def has_long(self):
        return bool(self.long_pairs)

    @property
    def longest(self):
        return (max([a for a, _ in self.long_pairs] + [self.mix_max, self.len1]), max([b for _, b in self.long_pairs] + [self.mix_max, self.len2]))

    def layout_names(self):
        return tuple(l.name for l in self.layouts)

    def qlead(self, l):
        """the lead of the quality bytes of a layout: another one mod 4 where the bases are misaligned"""
        return (l.lead + 1 + self.seed % 3) % 16 if l.name == "misaligned" else 0

    def first(self, l):
        """the first offset of a layout"""
        return 1 + (self.seed * 7) % 40 if l.name == "misaligned" and not l.uniform else 0

    @property
    def name_base(self):
        """the first generated name of fastx_format: the names wrap mod 2^64 after a few records"""
        return 2**64 - 5 - self.seed % 11

    @property
    def qual_fill(self):
        return 33 + self.seed % 90

    @property
    def px_args(self):
        return dict(tail=self.px_tail, head=self.px_head, min_len=self.px_min_len, max_error=self.px_max_error, penalty=self.px_penalty)


def _layouts(seed, mode, L, longest, lead):
    if mode == "one":
        out = [Layout("uniform", True, L), Layout("ragged0", False, 0), Layout("ragged_bound", False, longest),
               Layout("misaligned", seed % 4 >= 2, L if seed % 4 >= 2 else 0, lead)]
    else:
        out = [Layout("ragged0", False, 0), Layout("ragged_bound", False, longest), Layout("misaligned", False, 0 if seed % 4 >= 2 else longest, lead)]
    first = (seed // 3) % len(out)
    return tuple(out[first:] + out[:first])


def _adapter_set(seed, rng):
    n = 8 if seed % 6 == 1 else 1 if seed % 12 == 4 else int(rng.integers(2, 6))
    lens = [int(rng.integers(8, 31)) for _ in range(n)]
    if seed % 4 == 0:
        lens[-1] = 64
    if seed % 4 == 2 and n > 2:
        lens[-1] = 1 + (seed // 4) % 3            # 1 .. 3 bases: hits only where min_overlap lets them
    if seed % 8 == 5 and n == 1:
        lens[0] = 12
    ads = [rng.choice(_ACGT, L).astype(np.uint8) for L in lens]
    w = ads[0]                                     # the wildcards: in the first adapter, never among its first three bases
    if len(w) >= 8:
        w[rng.choice(np.arange(3, len(w)), max(1, len(w) // 8), replace=False)] = ord("N")
        if seed % 3 == 0:
            w[5] = ord("n")
    elif n > 1 and len(ads[1]) >= 8:
        ads[1][4] = ord("N")
    if seed % 5 == 1:
        ads[-1] |= 0x20                            # a lower-case adapter
    return tuple(a.tobytes() for a in ads)


def _scheduled(field, values, seed):
    """the value of one of the second library's plan fields: per block of N_DEFAULT seeds and per parity of the seed (the stream) every
    value comes equally often, in an order drawn per field, block and parity"""
    block, at = divmod(seed, N_DEFAULT)
    order = np.random.default_rng([70_000, field, block, seed % 2]).permutation(N_DEFAULT // 2)
    return values[int(order[at // 2]) % len(values)]


def plan(seed):
    """seed -> Plan.  Long mates come with seed % 8 in (3, 6) and force mode "mix"; of the others seed % 5 in (0, 3) are of mode "one";
    set sizes 8 and 1 with seed % 6 == 1 and seed % 12 == 4, an adapter of 64 bases with seed % 4 == 0; the rest is drawn from default_rng(seed)."""
    seed = int(seed)
    rng = np.random.default_rng(66_000 + seed)
    has_long = seed % 8 in (3, 6)
    mode = "one" if (not has_long and seed % 5 in (0, 3)) else "mix"
    if mode == "one":
        len1 = ONE_LENGTHS[(seed // 5 + seed) % 4]
        len2 = int(rng.choice({36: (250,), 100: (250,), 150: (150, 250), 250: (250, 100, 150)}[len1]))   # (merged reads reach 256 bases)
        mix_max, long_pairs, mean = 0, (), max(len1, len2)
    else:
        len1 = len2 = 0
        mix_max = int(rng.integers(180, 261))
        long_pairs = (LONG_AT[seed % 3], LONG_OVER[(seed // 2) % 4]) if has_long else ()
        mean = 0.62 * mix_max
    budget = MAX_BASES - sum(max(a, b) for a, b in long_pairs)
    n_pairs = int(max(40, min(300, budget // mean))) + len(long_pairs)
    adapters = _adapter_set(seed, rng)
    ad_min = int(rng.integers(1, 13))
    if ad_min < 3 and len(adapters) > 1:
        ad_min += 3                                # (several adapters at an overlap of one base hit every read: nothing left to miss)
    if min(len(a) for a in adapters) < 4:
        ad_min = max(ad_min, 4)                    # (an adapter of one to three bases is there to never reach min_overlap)
    ad_min = min(ad_min, max(len(a) for a in adapters))
    count_ks = [k for k in KS if k <= (34 if mode == "one" and min(len1, len2) == 36 else 64)]
    L1, L2 = max([a for a, _ in long_pairs] + [mix_max, len1]), max([b for _, b in long_pairs] + [mix_max, len2])
    lead = int(rng.integers(1, 16))
    return Plan(seed=seed, stream="side" if seed % 2 else "default", n_pairs=n_pairs, length_mode=mode, len1=len1, len2=len2, mix_max=mix_max,
                long_pairs=long_pairs, crlf=(bool(seed & 1), bool(seed & 4)), trail=(bool(seed & 2), not (seed & 2) or bool(seed & 8)),
                adapters=adapters, ad_min_overlap=ad_min, ad_max_error=MAX_ERRORS[int(rng.integers(0, len(MAX_ERRORS)))],
                min_q=(0, 3, 10)[seed % 3], trim_q=(10, 15, 20)[(seed // 3) % 3], k=(0, 5, 21, 31)[seed % 4], max_ee=(0.5, 1.0, 2.0, 5.0)[(seed // 2) % 4],
                trim=("mott", "run", None)[seed % 3], min_len=(0, 1, 20, 35)[(seed // 4) % 4], phred_base=64 if seed % 4 == 1 or seed % 8 == 6 else 33,
                q_cap=(41, 41, 93, 60)[seed % 4], ov_min_overlap=(8, 12) [(seed // 2) % 2] if mode == "one" and min(len1, len2) == 36 else (8, 12, 20, 30)[(seed // 2) % 4],
                ov_max_mism=(5, 2, 5, 1, 8)[seed % 5],
                count_k=count_ks[seed % len(count_ks)], sub_rate=float(rng.uniform(0.002, 0.008)), dirty_every=7,
                layouts=_layouts(seed, mode, len1, L1, lead), layouts2=_layouts(seed, mode, len2, L2, lead),
                dd_strand=_scheduled(1, (False, True), seed), dd_hash_bits=_scheduled(2, DD_HASH_BITS, seed), dd_score=_scheduled(3, DD_SCORES, seed),
                px_tail=_scheduled(4, PX_PAIRS, seed)[0], px_head=_scheduled(4, PX_PAIRS, seed)[1], px_min_len=_scheduled(5, PX_MIN_LENS, seed),
                px_max_error=_scheduled(6, PX_MAX_ERRORS, seed), px_penalty=_scheduled(7, PX_PENALTIES, seed), dust_max=_scheduled(8, DUST_MAXES, seed),
                min_diff=_scheduled(9, MIN_DIFFS, seed), fa_width=_scheduled(10, FA_WIDTHS, seed), name_skip=_scheduled(11, NAME_SKIPS, seed))


# ---------------------------------------------------------------- the pairs and the texts of a plan
@dataclasses.dataclass
class Case:
    texts: tuple               # the two FASTQ images (bytes)
    reads: tuple               # per mate file: list of uint8 arrays
    quals: tuple               # per mate file: list of uint8 arrays (the raw quality bytes)
    frags: list                # per pair: the fragment (uint8 array) or None for unrelated mates
    clean: np.ndarray          # per pair: both mates are error-free cuts of the fragment and overlap by 32 bases or more


def _quals(rng, p, L, errors, all_low, pristine=False):
    """the quality bytes of one mate: mostly high, a decaying 3' tail, low at most of the substituted positions"""
    if all_low or pristine:
        q = np.full(L, 2 if all_low else 37)
    else:
        q = rng.choice((30, 37, 37, 40), L)
        tail = int(rng.integers(0, L // 3 + 1)) if rng.random() < 0.7 else 0
        if tail:
            q[L - tail:] = np.maximum(2, 36 - (np.arange(tail) * 34) // tail - rng.integers(0, 5, tail))
        low = errors & (rng.random(L) < 0.7)
        q[low] = rng.choice((2, 8, 12), int(low.sum()))
    b = (q + p.phred_base).astype(np.uint8)
    if L and not all_low and not pristine:
        under = np.array([32, 32], np.uint8) if p.phred_base == 33 else np.array([c for c in QUAL_ALPHA if c < 64], np.uint8)
        hit = rng.random(L) < 0.002
        b[hit] = rng.choice(under, int(hit.sum()))           # bytes below phred_base
        hit = rng.random(L) < 0.003
        b[hit] = rng.choice(np.array(QUAL_ALPHA, np.uint8), int(hit.sum()))
        if rng.random() < 0.15:
            b[0] = rng.choice(np.frombuffer(b"@>+", np.uint8))   # a quality line that opens like a header
    return b


def _mate(rng, p, frag, L, adapter, errors_ok):
    """L bases: the fragment, then the read-through -- adapters of the plan's (their wildcards filled in) and junk; -> (mate, where
    it was substituted)"""
    ad = np.frombuffer(b"".join(adapter), np.uint8).copy()
    wild = (ad | 0x20) == ord("n")
    ad[wild] = rng.choice(_ACGT, int(wild.sum()))
    r = np.concatenate([frag, ad, rng.choice(_ACGT, max(L, 1))])[:L].astype(np.uint8)
    flip = (rng.random(L) < p.sub_rate) if errors_ok else np.zeros(L, bool)
    r[flip] = COMP[r[flip]]
    return r, flip


def _case_of(p):
    rng = np.random.default_rng(67_000 + p.seed)
    n = p.n_pairs
    lens = []
    for i in range(n):
        if p.length_mode == "one":
            lens.append((p.len1, p.len2))
        else:
            pick = lambda: 0 if (u := rng.random()) < 0.03 else int(rng.integers(1, 4)) if u < 0.07 else int(rng.integers(20, p.mix_max + 1))
            lens.append((pick(), pick()))
    long_at = {}
    if p.length_mode == "mix":
        lens[1] = (p.mix_max, p.mix_max)
        lens[n - 1] = (p.mix_max // 2, 25)        # (an image without its final newline ends in a quality line that has a byte)
        for j, LL in enumerate(p.long_pairs):
            long_at[(j * 17 + 5) % n] = LL
            lens[(j * 17 + 5) % n] = LL
    reads, quals, frags = ([], []), ([], []), []
    clean = np.zeros(n, bool)
    n_dirty = 0
    for i, (L1, L2) in enumerate(lens):
        lo, hi = min(L1, L2), max(L1, L2)
        u = rng.random()
        is_long = i in long_at
        low_complexity = not is_long and i % 16 == 9
        overhang = not is_long and i % 16 == 3 and L1 - p.ad_min_overlap - 2 >= 1
        if is_long:
            I = L1 + L2 - int(rng.integers(300, 600))
        elif overhang:
            I = L1 - p.ad_min_overlap - int(rng.integers(0, 3))                          # the adapter hangs over the read's end
        elif low_complexity or u < 0.36:
            I = int(rng.integers(min(20, max(lo // 4, 1)), max(lo, 2)))                  # shorter than both mates
        elif u < 0.50:
            I = int(rng.integers(lo, hi + 1))                                           # between the two
        elif u < 0.72:
            I = int(rng.integers(hi + 1, max(hi + 2, L1 + L2 - p.ov_min_overlap - 4)))  # longer than both, overlapping
        else:
            I = L1 + L2 + int(rng.integers(0, 60))                                      # no overlap at all
        unrelated = not is_long and not low_complexity and 0.90 <= u
        if low_complexity:
            I += int(rng.integers(0, hi + 1)) if i % 32 == 9 else 0
            unit = _ACGT[[int(rng.integers(0, 4))]] if i % 48 == 9 else _ACGT[rng.permutation(4)[:2]]
            frag = np.resize(unit, max(I, 1))
        else:
            frag = rng.choice(_ACGT, max(I, 1)).astype(np.uint8)
        if i % 9 == 4 and not is_long:
            frag[int(rng.integers(0, len(frag)))] = ord("N")                            # both mates see it: NONE where they overlap
        errors_ok = not is_long and i % 3 != 0
        usable = [a for a in p.adapters if len(a) >= p.ad_min_overlap] or list(p.adapters)
        j = int(rng.integers(0, len(usable)))
        a1 = (usable[j], usable[(j + 1 + int(rng.integers(0, max(len(usable) - 1, 1)))) % len(usable)])   # two adapters back to back
        a2 = (usable[int(rng.integers(0, len(usable)))],)
        if overhang:
            a1 = (max(p.adapters, key=len),)
        m1, f1 = _mate(rng, p, frag, L1, a1, errors_ok)
        m2, f2 = _mate(rng, p, rc_read(frag) if not unrelated else rng.choice(_ACGT, L2 + 1).astype(np.uint8), L2, a2, errors_ok)
        dirt = [False, False]
        for m, r in enumerate((m1, m2)):
            if (2 * i + m + p.seed) % p.dirty_every == 0 and len(r) and not is_long:
                _dirty(rng, r, n_dirty)
                n_dirty += 1
                dirt[m] = True
        all_low = i % 13 == 6
        q1, q2 = _quals(rng, p, L1, f1, all_low, is_long), _quals(rng, p, L2, f2, all_low and i % 2 == 0, is_long)
        over = min(L1, len(frag)) - max(len(frag) - L2, 0)
        clean[i] = (not (unrelated or low_complexity or dirt[0] or dirt[1] or f1.any() or f2.any()) and (frag != ord("N")).all()
                    and over >= 32 and max(L1, L2) <= A.RP_MAX_LEN and len(frag) == I)
        frags.append(None if unrelated else frag)
        for m, (r, q) in enumerate(((m1, q1), (m2, q2))):
            assert len(r) == len(q) == (L1, L2)[m]
            reads[m].append(np.ascontiguousarray(r))
            quals[m].append(np.ascontiguousarray(q))
    texts = []
    for m in range(2):
        nl = b"\r\n" if p.crlf[m] else b"\n"
        lines = []
        for i in range(n):
            head = b"@pair%d/%d" % (i, m + 1) + (b" >x@y+z", b"", b" +", b"@")[i % 4]
            lines += [head, reads[m][i].tobytes(), b"+" + (head[1:] if i % 5 == 0 else b""), quals[m][i].tobytes()]
        texts.append(nl.join(lines) + (nl if p.trail[m] else b""))
    return Case(tuple(texts), reads, quals, frags, clean)


@functools.lru_cache(maxsize=8)
def _case_cached(seed):
    return _case_of(plan(seed))


def case_of(p):
    return _case_cached(p.seed)


def handovers(p, case):
    """[{layout, layout2, bufs: (bases 1, quals 1, bases 2, quals 2), leads: likewise, nbytes: (mate 1, mate 2), first,
    offsets: (mate 1, mate 2) or (None, None)}]: every buffer holds GUARD_BYTES of '#', its lead more, the bytes, GUARD_BYTES again"""
    out = []
    for l, l2 in zip(p.layouts, p.layouts2):
        first = p.first(l)
        bufs, leads, nbytes, offs = [], [], [], []
        for m, lay in enumerate((l, l2)):
            b, off = ragged(case.reads[m])
            q, _ = ragged(case.quals[m])
            if lay.uniform:
                assert all(len(r) == lay.bound for r in case.reads[m])
            assert lay.uniform or lay.bound == 0 or lay.bound >= max(len(r) for r in case.reads[m])
            for data, lead in ((b, lay.lead), (q, p.qlead(lay))):
                bufs.append(np.concatenate([np.full(GUARD_BYTES + lead, ord("#"), np.uint8), data, np.full(GUARD_BYTES, ord("#"), np.uint8)]))
                leads.append(lead)
            nbytes.append(len(b))
            offs.append(None if lay.uniform else off + np.uint64(first))
        out.append(dict(layout=l, layout2=l2, bufs=tuple(bufs), leads=tuple(leads), nbytes=tuple(nbytes), first=first, offsets=tuple(offs)))
    return out


# ---------------------------------------------------------------- the reference chain
def gather_index(p, n_reads):
    """the index reads_gather is given: seeded, with repeats and a few indices outside the batch"""
    rng = np.random.default_rng(68_000 + p.seed)
    idx = rng.integers(0, n_reads, GATHER_N).astype(np.int64)
    idx[::7] = n_reads + rng.integers(0, 5, len(idx[::7]))
    idx[3] = -1
    return idx


def length_labels(merge_rows):
    """the label reads_partition is given: the length class of a merged read (< 64, < 256, longer), -1 for a pair that did not merge"""
    L = merge_rows[:, M.RM_LEN].astype(np.int64)
    return np.where(L == 0, -1, (L >= 64).astype(np.int64) + (L >= 256))


def quality_filter_np(p, bases, quals, n, offsets, max_ee, trim, min_len, weights):
    """reads_quality_filter out of its two references -> (bases, quals, offsets, index, masked, rows)"""
    masked, rows = Q.reads_quality_np(bases, quals, n, 0, offsets, p.phred_base, p.min_q, p.trim_q, p.k, weights)
    keep = None if max_ee is None else Q.expected_errors_np(rows) <= float(max_ee)
    span = None if trim is None else rows[:, Q.RQ_TRIM if trim == "mott" else Q.RQ_RUN]
    b, off, idx = reads_np.select_np(masked, n, 0, offsets, keep=keep, span=span, min_len=min_len)
    q, qoff, _ = reads_np.select_np(quals, n, 0, offsets, keep=keep, span=span, min_len=min_len)
    assert np.array_equal(off, qoff)
    return b, q, off, idx, masked, rows


def overlap_np(p, b1, o1, b2, o2, n):
    return A.reads_pair_overlap_np(b1, b2, n, 0, 0, o1, o2, p.ov_min_overlap, p.ov_max_mism, 1, 5)


def table_of_batch(orc, bases, offsets, k):
    n = len(offsets) - 1
    if n == 0 or int(offsets[-1]) == 0:
        return (np.zeros(0, np.uint64) if k <= 32 else np.zeros((0, 2), np.uint64)), np.zeros(0, np.uint64)
    return table_of(*orc_windows(orc, bases, n, 0, k, offsets=np.asarray(offsets, np.uint64)))


def host_pipeline(p, case=None):
    """the references end to end -> dict of arrays, keys as STAGES lists them"""
    from oracle import oracle as orc

    case = case_of(p) if case is None else case
    n = p.n_pairs
    H = {}
    # ---- 1. parse: by construction
    for m in (1, 2):
        H[f"p{m}_bases"], H[f"p{m}_offsets"] = ragged(case.reads[m - 1])
        H[f"p{m}_quals"], _ = ragged(case.quals[m - 1])
        lens = np.diff(H[f"p{m}_offsets"].astype(np.int64))
        H[f"p{m}_layout"] = np.array([n, int(lens.max(initial=0)), int(n > 0 and lens.min() == lens.max())], np.uint64)
    b1, q1, o1, b2, q2, o2 = H["p1_bases"], H["p1_quals"], H["p1_offsets"], H["p2_bases"], H["p2_quals"], H["p2_offsets"]
    # ---- 2. adapters off mate 1
    H["ad_rows"] = A.reads_adapter_np(b1, n, 0, p.adapters, p.ad_min_overlap, *p.ad_max_error, offsets=o1)
    span = H["ad_rows"][:, A.RA_KEEP]
    H["ta_bases"], H["ta_offsets"], H["ta_index"] = reads_np.select_np(b1, n, 0, o1, span=span, min_len=p.min_len)
    H["ta_quals"], qoff, _ = reads_np.select_np(q1, n, 0, o1, span=span, min_len=p.min_len)
    assert np.array_equal(qoff, H["ta_offsets"])
    # ---- 3. quality of what is left
    nt = len(H["ta_index"])
    H["qf_bases"], H["qf_quals"], H["qf_offsets"], H["qf_index"], H["q_masked"], H["q_rows"] = quality_filter_np(
        p, H["ta_bases"], H["ta_quals"], nt, H["ta_offsets"], p.max_ee, p.trim, p.min_len, Q.ee_weights(p.phred_base))
    # ---- 4. the count table of that
    H["table_k"], H["table_c"] = table_of_batch(orc, H["qf_bases"], H["qf_offsets"], p.count_k)
    # ---- 5. both mates trimmed by quality, in step
    for m, (b, q, o, trim) in enumerate(((b1, q1, o1, "mott"), (b2, q2, o2, "run")), 1):
        H[f"pq{m}_bases"], H[f"pq{m}_quals"], H[f"pq{m}_offsets"], H[f"pq{m}_index"], _, H[f"pq{m}_rows"] = quality_filter_np(
            p, b, q, n, o, None, trim, 0, None)
        assert np.array_equal(H[f"pq{m}_index"], np.arange(n, dtype=np.uint64))
    c1, cq1, co1, c2, cq2, co2 = H["pq1_bases"], H["pq1_quals"], H["pq1_offsets"], H["pq2_bases"], H["pq2_quals"], H["pq2_offsets"]
    # ---- 6. the overlap of the mates
    ov = H["ov_rows"] = overlap_np(p, c1, co1, c2, co2, n)
    keep = ((ov[:, A.RP_KEEP1] >> np.uint64(32)) >= p.min_len) & ((ov[:, A.RP_KEEP2] >> np.uint64(32)) >= p.min_len)
    H["tp1_bases"], H["tp1_offsets"], H["tp1_index"] = reads_np.select_np(c1, n, 0, co1, keep=keep, span=ov[:, A.RP_KEEP1])
    H["tp2_bases"], H["tp2_offsets"], H["tp2_index"] = reads_np.select_np(c2, n, 0, co2, keep=keep, span=ov[:, A.RP_KEEP2])
    # ---- 7. the merge
    ins = ov[:, A.RP_INSERT]
    H["mg_bases"], H["mg_quals"], H["mg_offsets"], H["mg_rows"] = M.reads_pair_merge_np(c1, c2, n, 0, 0, ins, cq1, cq2, co1, co2, p.phred_base, p.q_cap)
    H["mgn_bases"], _, H["mgn_offsets"], H["mgn_rows"] = M.reads_pair_merge_np(c1, c2, n, 0, 0, ins, None, None, co1, co2, p.phred_base, p.q_cap)
    # ---- 8. merged and unmerged apart
    mk = H["mg_rows"][:, M.RM_LEN] != 0
    H["mp_m_bases"], H["mp_m_offsets"], H["mp_m_index"] = reads_np.select_np(H["mg_bases"], n, 0, H["mg_offsets"], keep=mk)
    H["mp_mq_bases"] = reads_np.select_np(H["mg_quals"], n, 0, H["mg_offsets"], keep=mk)[0]
    H["mp_u1_bases"], H["mp_u1_offsets"], H["mp_u1_index"] = reads_np.select_np(c1, n, 0, co1, keep=~mk)
    H["mp_u2_bases"], H["mp_u2_offsets"], H["mp_u2_index"] = reads_np.select_np(c2, n, 0, co2, keep=~mk)
    H["mp_u1q_bases"] = reads_np.select_np(cq1, n, 0, co1, keep=~mk)[0]
    H["mp_u2q_bases"] = reads_np.select_np(cq2, n, 0, co2, keep=~mk)[0]
    H["mp_ov_rows"], H["mp_mg_rows"] = ov, H["mg_rows"]
    # ---- 9. the merged reads by length class
    H["pt_bases"], H["pt_offsets"], H["pt_index"], labels, groups = reads_np.partition_np(H["mg_bases"], n, 0, length_labels(H["mg_rows"]), H["mg_offsets"])
    H["pt_labels"], H["pt_groups"] = labels.astype(np.uint64), groups.astype(np.uint64)
    assert set(H) == {x for stage in FIRST_LIBRARY for x in STAGES[stage]}
    # ---- the route pass: the reads-form calls on the raw parsed mates
    H["rt_q_masked"], H["rt_q_rows"] = Q.reads_quality_np(b1, q1, n, 0, o1, p.phred_base, p.min_q, p.trim_q, p.k, Q.ee_weights(p.phred_base))
    rov = H["rt_ov_rows"] = overlap_np(p, b1, o1, b2, o2, n)
    H["rt_mg_bases"], H["rt_mg_quals"], H["rt_mg_offsets"], H["rt_mg_rows"] = M.reads_pair_merge_np(b1, b2, n, 0, 0, rov[:, A.RP_INSERT], q1, q2, o1, o2,
                                                                                                    p.phred_base, p.q_cap)
    H["rt_sel_bases"], H["rt_sel_offsets"], H["rt_sel_index"] = reads_np.select_np(b1, n, 0, o1, span=span, min_len=p.min_len)
    H["rt_gat_bases"], H["rt_gat_offsets"] = reads_np.gather_np(b1, n, 0, gather_index(p, n), o1, span=span)
    assert set(H) == {x for stage in FIRST_LIBRARY for x in STAGES[stage]} | set(ROUTES)
    H.update(library_pipeline(p, library_of(p, case), orc))
    assert set(H) == {x for names in STAGES.values() for x in names} | set(ROUTES) | set(ROUTES2)
    return H


def split(bases, offsets):
    o = np.asarray(offsets).astype(np.int64)
    return [bases[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def equal_n_tie(p, m1, m2):
    """adapter_np.pair_scan of one pair: two hits or more share the largest overlap"""
    if not len(m1) or not len(m2) or max(len(m1), len(m2)) > A.RP_MAX_LEN:
        return False
    n, m = A.pair_scan(m1, m2)
    hit = (n >= p.ov_min_overlap) & (m <= p.ov_max_mism) & (m * 5 <= n)
    return bool(hit.any()) and int((n[hit] == n[hit].max()).sum()) >= 2


def structure(p, H):
    """what the non-vacuity test asks of a seed, read off the reference's arrays alone -> dict of bools"""
    ad, qr, ov, mg = H["ad_rows"], H["q_rows"], H["ov_rows"], H["mg_rows"]
    u32 = np.uint64(0xFFFFFFFF)
    hit = ad[:, A.RA_HIT] != 0
    which = (ad[:, A.RA_HIT] & np.uint64(0xFFFF)).astype(np.int64) - 1
    hit_n = ((ad[:, A.RA_HIT] >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64)
    ad_len = np.array([len(a) for a in p.adapters])
    wild = [i for i, a in enumerate(p.adapters) if b"N" in a.upper()]
    wildcard_used = False
    for r in np.nonzero(hit & np.isin(which, wild))[0]:
        a = np.frombuffer(p.adapters[which[r]], np.uint8)[:hit_n[r]]
        wildcard_used = wildcard_used or bool(((a | 0x20) == ord("n")).any())
    ee = Q.expected_errors_np(qr)
    kept = ee <= p.max_ee
    trim_w = qr[:, Q.RQ_TRIM if p.trim != "run" else Q.RQ_RUN]
    hits = ov[:, A.RP_INSERT] != 0
    c1, c2 = split(H["pq1_bases"], H["pq1_offsets"]), split(H["pq2_bases"], H["pq2_offsets"])
    lens = mg[:, M.RM_LEN][mg[:, M.RM_LEN] != 0]
    lens12 = np.maximum(np.diff(H["p1_offsets"].astype(np.int64)), np.diff(H["p2_offsets"].astype(np.int64)))
    return {
        "adapter_hit_and_miss": bool(hit.any() and (~hit).any()),
        "adapter_overhang_hit": bool((hit & (hit_n < ad_len[np.maximum(which, 0)])).any()),
        "adapter_two_hit": bool(max((bin(int(x)).count("1") for x in ad[:, A.RA_HITS]), default=0) >= 2),
        "adapter_wildcard_used": wildcard_used,
        "trim_nonzero_start": bool(((trim_w & u32) != 0).any()),
        "all_low_read": bool(((qr[:, Q.RQ_BASES] > 0) & (qr[:, Q.RQ_LOW] == qr[:, Q.RQ_BASES])).any()) if p.min_q else
        bool(((qr[:, Q.RQ_BASES] > 0) & ((qr[:, Q.RQ_MINMAX] >> np.uint64(32)) <= 5)).any()),
        "ee_drops_some_keeps_some": bool(kept.any() and (~kept).any()),
        "empty_after_trim": bool((np.diff(H["pq1_offsets"].astype(np.int64)) == 0).any() or (np.diff(H["pq2_offsets"].astype(np.int64)) == 0).any()),
        "overlap_hit_and_miss": bool(hits.any() and (~hits).any()),
        "overlap_equal_n_tie": any(equal_n_tie(p, c1[r], c2[r]) for r in np.nonzero(hits)[0]),
        "merge_dis": bool(((mg[:, M.RM_OVERLAP] >> np.uint64(32)) != 0).any()),
        "merge_taken_from_2": bool(((mg[:, M.RM_TAKEN] & u32) != 0).any()),
        "merge_tie": bool(((mg[:, M.RM_TAKEN] >> np.uint64(32)) != 0).any()),
        "merge_one": bool(((mg[:, M.RM_INVALID] & u32) != 0).any()),
        "merge_none": bool(((H["rt_mg_rows"][:, M.RM_INVALID] >> np.uint64(32)) != 0).any()),
        "merged_and_unmerged": bool(len(lens) and len(lens) < len(mg)),
        "mate_over_1024": bool((lens12 > A.RP_MAX_LEN).any()),
        "lengths_cross_64_and_256": bool((lens < 64).any() and ((lens >= 64) & (lens < 256)).any() and (lens >= 256).any()),
        **library_structure(p, H, library_of(p)),
    }


# ---------------------------------------------------------------- the relations
def swapped_merge_expect(first, valid_pair):
    """what merging the swapped pairs must give, out of the first merge = (bases, quals, offsets, rows): per pair None (nothing is
    claimed: a tie, or a byte outside ACGTacgtN) or (bases & 0xDF, quals, row)"""
    bases, quals, offsets, rows = first
    out = []
    for r, (b, q) in enumerate(zip(split(bases, offsets), split(quals, offsets))):
        row = [int(x) for x in rows[r]]
        if row[M.RM_LEN] == 0:
            out.append((b, q, row))                        # not merged either way
        elif (row[M.RM_TAKEN] >> 32) or not valid_pair[r]:
            out.append(None)
        else:
            dis = row[M.RM_OVERLAP] >> 32
            out.append((M._COMP[b[::-1]] & 0xDF, q[::-1], [row[0], row[1], dis - (row[2] & 0xFFFFFFFF), row[3]]))
    return out


def pairs_over_acgtn(b1, o1, b2, o2):
    return np.array([bool(_VALID[x].all() and _VALID[y].all()) for x, y in zip(split(b1, o1), split(b2, o2))])


def check_swapped_merge(expect, got):
    """got = the merge of the swapped pairs (bases, quals, offsets, rows) -> the number of merged pairs the relation was checked on"""
    bases, quals, offsets, rows = got
    checked = 0
    for r, (b, q) in enumerate(zip(split(bases, offsets), split(quals, offsets))):
        if expect[r] is None:
            continue
        wb, wq, wrow = expect[r]
        assert [int(x) for x in rows[r]] == wrow, ("swapped merge: row", r, rows[r], wrow)
        assert np.array_equal(b & 0xDF, wb & 0xDF) and np.array_equal(q, wq), ("swapped merge: read", r)
        checked += wrow[0] != 0
    return checked


def swapped_overlap_expect(ov):
    return ov[:, [A.RP_INSERT, A.RP_OVERLAP, A.RP_KEEP2, A.RP_KEEP1]]


def permutation(p):
    return np.random.default_rng(69_000 + p.seed).permutation(p.n_pairs)


def permuted(H, perm):
    """the two quality-trimmed mate batches of the chain with their pairs in the order perm -> ((bases, quals, offsets), (...))"""
    out = []
    for m in (1, 2):
        b, o = ragged([split(H[f"pq{m}_bases"], H[f"pq{m}_offsets"])[r] for r in perm])
        q, _ = ragged([split(H[f"pq{m}_quals"], H[f"pq{m}_offsets"])[r] for r in perm])
        out.append((b, q, o))
    return out


def clean_pairs(case):
    """the raw mates of the error-free pairs, and their fragments -> ((bases 1, offsets 1), (bases 2, offsets 2), fragments)"""
    idx = np.nonzero(case.clean)[0]
    return ragged([case.reads[0][i] for i in idx]), ragged([case.reads[1][i] for i in idx]), [case.frags[i] for i in idx]


# ---------------------------------------------------------------- the second library: copies, poly-X ends, low complexity, names
@dataclasses.dataclass
class Library:
    texts: tuple               # the two FASTQ images (bytes)
    reads: tuple               # per mate file: list of uint8 arrays
    quals: tuple
    names: tuple               # per mate file: list of bytes, the header lines ('@' included)
    kind: list                 # per item: "orig", a copy's kind ("exact", "case", "other", "swapped", "rc"), one of NEAR_KINDS, or an extra's name
    src: np.ndarray            # per item: the item it was made from, -1 for none
    ends: dict                 # item -> (end, kind, run length) of the poly-X end planted on its mate 1

    @property
    def n(self):
        return len(self.kind)

    def where(self, *kinds):
        return [i for i, k in enumerate(self.kind) if k in kinds]


@dataclasses.dataclass(eq=False)
class _Item:
    r: list                    # [mate 1, mate 2]
    q: list
    kind: str = "orig"
    src: object = None
    end: object = None


def _letters(mask):
    return [b"ACGT"[x] for x in range(4) if (mask >> x) & 1]


def _fresh_quals(rng, p, L, pristine=False):
    return ((np.full(L, 37) if pristine else rng.choice((30, 37, 37, 40), L)) + p.phred_base).astype(np.uint8)


def _random_pair(rng, p, r1, L2=None):
    r1 = np.asarray(r1, np.uint8)
    r2 = rng.choice(_ACGT, len(r1) if L2 is None else L2).astype(np.uint8)
    return [r1, r2], [_fresh_quals(rng, p, len(r1)), _fresh_quals(rng, p, len(r2))]


def _plant_end(rng, p, r, end, kind):
    """overwrite one end of r in place with a poly-X end of `kind`, behind up to 2 min_len bases that alternate between two other
    letters (no suffix that starts further inside qualifies through them) -> (kind planted, run length), (None, 0) where r is too short"""
    ml, (num, den) = p.px_min_len, p.px_max_error
    letters = _letters(p.px_tail if end == "tail" else p.px_head)
    x = letters[int(rng.integers(0, len(letters)))]
    y, z = [c for c in rng.permutation(_ACGT).tolist() if c != x][:2]
    for kind in (kind, "exact", "minus"):
        if kind in ("minus", "exact", "plus"):
            R = ml + {"minus": -1, "exact": 0, "plus": 1}[kind]
            run = np.full(R, x, np.uint8)
        elif kind in ("lo", "hi"):                   # interruptions at about half / more than twice the rate max_error allows
            R = int(rng.integers(30, 51))
            run = np.full(R, x, np.uint8)
            n_int = (R * num) // (2 * den) if kind == "lo" else -(-2 * R * num // den) + 1
            run[rng.choice(np.arange(1, R - 1), min(n_int, R - 2), replace=False)] = y
        else:                                        # "pnx": the suffix that starts at the interruption has a base p that is not X
            R = ml + 6
            run = np.concatenate([np.full(3, x, np.uint8), [y], np.full(R, x, np.uint8)]).astype(np.uint8)
        g = min(2 * ml, len(r) - len(run) - 1)       # (a short read: a shorter guard, as long as it still stops every longer suffix)
        if g >= (len(run) * num) // den + 2:
            block = np.concatenate([np.resize(np.array([y, z], np.uint8), g), run])
            break
    else:
        return None, 0
    if rng.random() < 0.2:
        block = block | 0x20                         # (the case is ignored)
    if end == "tail":
        r[len(r) - len(block):] = block
    else:
        r[:len(block)] = block[::-1]
    return kind, R


_END_KINDS = ("exact", "minus", "plus", "lo", "hi", "pnx", "exact", "plus")


def _extras(rng, p):
    """the planted reads that are no copies -> [(kind, mate 1)]"""
    tail_l, head_l = _letters(p.px_tail or p.px_head), _letters(p.px_head or p.px_tail)
    pick = lambda letters: letters[int(rng.integers(0, len(letters)))]
    rand = lambda L: rng.choice(_ACGT, L).astype(np.uint8)
    out = [("homopolymer", np.full(80, pick(list(b"ACGT")), np.uint8))]
    for L in LC_LENGTHS:
        out.append((f"ac{L}", np.resize(rng.permutation(_ACGT)[:2], L)))
        out.append((f"acg{L}", np.resize(rng.permutation(_ACGT)[:3], L)))
    unit = rng.permutation(_ACGT)[:1 if p.dust_max >= 930 else 2]
    out.append(("dusty_mid", np.concatenate([rand(64), np.resize(unit, 64), rand(64)])))
    out.append(("all_x", np.full(50, pick(tail_l), np.uint8)))
    k = p.px_min_len + 2
    x1 = pick(head_l)
    x2 = ([c for c in tail_l if c != x1] or tail_l)[0]
    out.append(("overlap", np.concatenate([np.full(k, x1, np.uint8), np.full(k, x2, np.uint8)])))
    out.append(("cross", np.concatenate([rand(50), np.full(40, pick(tail_l), np.uint8)]) if p.px_tail else
                np.concatenate([np.full(70, pick(head_l), np.uint8), rand(30)])))
    out.append(("empty1", np.zeros(0, np.uint8)))
    out.append(("fa_line", rand(p.fa_width if p.fa_width >= 60 else 60)))
    return out


def _other_letter(rng, b):
    """a letter of ACGT with another code than the byte b"""
    return int(rng.choice([c for c in b"ACGT" if c != (b & 0xDF)]))


def _copy(rng, p, s, kind, qmode):
    """one planted item made from the item s; qmode 0: the source's quality bytes, 1: the best there are (a copy that outranks its
    source where the call has a score), 2: fresh ones"""
    r = [s.r[0].copy(), s.r[1].copy()]
    q = [s.q[0].copy(), s.q[1].copy()]
    if kind == "case":
        for m in range(2):
            letter = np.isin(r[m] & 0xDF, _ACGT)
            flip = (rng.random(len(r[m])) < 0.3) & letter
            if letter.any():
                flip[int(rng.choice(np.nonzero(letter)[0]))] = True
            r[m][flip] ^= 0x20
    elif kind == "other":                            # one byte that is no letter becomes another one that is none either
        m = 0 if (~np.isin(r[0] & 0xDF, _ACGT)).any() else 1
        at = np.nonzero(~np.isin(r[m] & 0xDF, _ACGT))[0]
        if len(at):
            a = int(at[int(rng.integers(0, len(at)))])
            r[m][a] = next(c for c in b"NnR.-*" if c != r[m][a])
    elif kind == "swapped":
        r, q = r[::-1], q[::-1]
    elif kind == "rc":                               # for the single-read stage: mate 1 on the other strand, an unrelated mate 2
        r = [rc_read(r[0]), rng.choice(_ACGT, len(r[1])).astype(np.uint8)]
        q = [q[0][::-1].copy(), q[1]]
    elif kind == "near_last":
        r[1][-1] = _other_letter(rng, int(r[1][-1]))
    elif kind == "near_first":
        r[0][0] = _other_letter(rng, int(r[0][0]))
    elif kind == "near_shorter":
        r[0], q[0] = r[0][:-1].copy(), q[0][:-1].copy()
    elif kind == "near_mate2":
        r[1] = rng.choice(_ACGT, len(r[1])).astype(np.uint8)
    else:
        assert kind == "exact", kind
    if qmode:
        q = [_fresh_quals(rng, p, len(x), pristine=qmode == 1) for x in r]
    return _Item(r, q, kind, s)


def _library_of(p, case):
    rng = np.random.default_rng(71_000 + p.seed)
    n = p.n_pairs
    items = [_Item([case.reads[0][i].copy(), case.reads[1][i].copy()], [case.quals[0][i].copy(), case.quals[1][i].copy()]) for i in range(n)]
    # ---- poly-X ends, overwritten onto mate 1 of a share of the pairs; only at the ends the plan looks at
    ends = [e for e, mask in (("tail", p.px_tail), ("head", p.px_head)) if mask]
    planted = 0
    for i, it in enumerate(items[:-1]):
        if len(it.r[0]) <= 260 and rng.random() < 0.45:
            end = ends[planted % len(ends)]
            kind, R = _plant_end(rng, p, it.r[0], end, _END_KINDS[(planted // len(ends)) % len(_END_KINDS)])
            if kind:
                it.end = (end, kind, R)
                planted += 1
    # ---- what is planted: the reads that are no copies ...
    new = []
    for kind, r1 in _extras(rng, p):
        r, q = _random_pair(rng, p, r1, 30 if kind == "empty1" else None)
        new.append(_Item(r, q, kind))
    # ... the copies that are duplicates, one class of five among them; enough of them that one item in ten is dropped ...
    pool = [it for it in items[:-1] if 20 <= len(it.r[0]) <= 260 and 20 <= len(it.r[1]) <= 260]
    pool = [pool[i] for i in rng.permutation(len(pool))]
    with_other = [it for it in pool if (~np.isin(np.concatenate(it.r) & 0xDF, _ACGT)).any()]
    five = pool.pop()
    new += [_copy(rng, p, five, kind, qmode) for kind, qmode in (("exact", 0), ("case", 1), ("exact", 2), ("case", 0))]
    n_dup = -(-(n - 13) // 9) + 1                    # (with the four above: one in ten of n + 17 + 4 + n_dup + 2 + 4 items)
    for j in range(n_dup):
        kind = ("exact", "case", "other")[j % 3]
        s = with_other[(j // 3) % len(with_other)] if kind == "other" and with_other else pool.pop()
        new.append(_copy(rng, p, s, kind if kind != "other" or with_other else "exact", j % 3 if kind != "other" else (j // 3) % 3))
    for kind in ("swapped", "rc"):
        new.append(_copy(rng, p, pool.pop(), kind, int(rng.integers(0, 3))))
    # ... the near-copies, which must stay ...
    for kind in NEAR_KINDS:
        new.append(_copy(rng, p, pool.pop(), kind, int(rng.integers(0, 3))))
    # ... and in a sixth of the seeds a class of 40: a short pair and 39 copies of it
    if p.seed % 6 == 2:
        r, q = _random_pair(rng, p, rng.choice(_ACGT, 30).astype(np.uint8))
        short = _Item(r, q, "short")
        new += [short] + [_copy(rng, p, short, ("exact", "case")[j % 2], j % 3) for j in range(39)]
    # ---- at drawn positions, the case's last pair staying last (an image without its final newline ends in a quality byte)
    order = items[:-1]
    for it in new:
        order.insert(int(rng.integers(1, len(order) + 1)), it)
    order.append(items[-1])
    at = {id(it): i for i, it in enumerate(order)}
    src = np.array([-1 if it.src is None else at[id(it.src)] for it in order], np.int64)
    plain = [i for i, it in enumerate(order) if i >= 16 and it.kind == "orig" and it.end is None and i not in set(src.tolist()) and
             20 <= len(it.r[0]) <= 260][:2]
    # ---- the names: the case's four header variants; one that is only '@', one of 300 bytes and more; the first sixteen records
    # padded so that |N| + 2 L + 6 takes every residue mod 16 (with N the name behind name_skip, L the record's own length)
    names, texts = ([], []), []
    for m in range(2):
        nl = b"\r\n" if p.crlf[m] else b"\n"
        lines = []
        for i, it in enumerate(order):
            head = b"@pair%d/%d" % (i, m + 1) + (b" >x@y+z", b"", b" +", b"@")[i % 4]
            if i < 16:
                head += b"_" * ((i - (len(head) - min(p.name_skip, len(head)) + 2 * len(it.r[m]) + 6)) % 16)
            elif i == plain[0]:
                head = b"@"
            elif i == plain[1]:
                head += b" " + b"long-name." * (30 + p.seed % 7)
            names[m].append(head)
            lines += [head, it.r[m].tobytes(), b"+" + (head[1:] if i % 5 == 0 else b""), it.q[m].tobytes()]
        texts.append(nl.join(lines) + (nl if p.trail[m] else b""))
    return Library(tuple(texts), tuple([np.ascontiguousarray(it.r[m]) for it in order] for m in range(2)),
                   tuple([np.ascontiguousarray(it.q[m]) for it in order] for m in range(2)), names, [it.kind for it in order], src,
                   {i: it.end for i, it in enumerate(order) if it.end})


@functools.lru_cache(maxsize=8)
def _library_cached(seed):
    p = plan(seed)
    return _library_of(p, case_of(p))


def library_of(p, case=None):
    """the library with copies of a plan (case: accepted for symmetry with host_pipeline; it is a function of the plan)"""
    return _library_cached(p.seed)


def lib_handovers(p, lib):
    """the second library's raw mates and the names of mate 1 as every ragged or misaligned layout of the plan hands them over:
    [{name, bounds: (mate 1, mate 2), bufs: (bases 1, quals 1, bases 2, quals 2, names 1), leads: likewise, nbytes: (mate 1, mate 2,
    names), first, nfirst, offsets: (mate 1, mate 2, names)}]; the names' lead differs mod 4 from the bases' and the quality bytes'"""
    out = []
    longest = [max(len(r) for r in lib.reads[m]) for m in range(2)]
    nm, noff = ragged([np.frombuffer(x, np.uint8) for x in lib.names[0]])
    for l in p.layouts:
        if l.name == "uniform":
            continue
        mis = l.name == "misaligned"
        bound = l.name == "ragged_bound" or (mis and p.seed % 4 < 2)
        first, nfirst = (1 + (p.seed * 7) % 40, 3 + p.seed % 5) if mis else (0, 0)
        qlead = (l.lead + 1 + p.seed % 3) % 16 if mis else 0
        nlead = next(v for v in range(1, 16) if (v - l.lead) % 4 and (v - qlead) % 4) if mis else 0
        bufs, leads, nbytes, offs = [], [], [], []
        for m in range(2):
            b, off = ragged(lib.reads[m])
            q, _ = ragged(lib.quals[m])
            for data, lead in ((b, l.lead), (q, qlead)):
                bufs.append(np.concatenate([np.full(GUARD_BYTES + lead, ord("#"), np.uint8), data, np.full(GUARD_BYTES, ord("#"), np.uint8)]))
                leads.append(lead)
            nbytes.append(len(b))
            offs.append(off + np.uint64(first))
        bufs.append(np.concatenate([np.full(GUARD_BYTES + nlead, ord("#"), np.uint8), nm, np.full(GUARD_BYTES, ord("#"), np.uint8)]))
        out.append(dict(name=l.name, bounds=tuple(longest[m] if bound else 0 for m in range(2)), bufs=tuple(bufs), leads=tuple(leads) + (nlead,),
                        nbytes=tuple(nbytes) + (len(nm),), first=first, nfirst=nfirst, offsets=tuple(offs) + (noff + np.uint64(nfirst),)))
    return out


def _layout_word(offsets):
    lens = np.diff(np.asarray(offsets).astype(np.int64))
    n = len(lens)
    return np.array([n, int(lens.max(initial=0)), int(n > 0 and lens.min() == lens.max())], np.uint64)


def dedup_np(reads, mates, p, score):
    """dedup_np.dedup with the plan's flags -> (rows, keep, summary)"""
    return D.dedup(reads, mates, strand=p.dd_strand, score=score, hash_bits=p.dd_hash_bits)


def complexity_np(p, bases, n, offsets, dust_max=None):
    return X.reads_complexity_np(bases, n, 0, p.px_tail, p.px_head, p.px_min_len, *p.px_max_error, p.px_penalty,
                                 p.dust_max if dust_max is None else dust_max, offsets=offsets)


def diff_keep(p, rows):
    """reads_complexity_filter's test: D * den >= num * P"""
    w = rows[:, X.RX_DIFF].astype(np.int64)
    return (w & 0xFFFFFFFF) * p.min_diff[1] >= (w >> 32) * p.min_diff[0]


def names_behind_skip(p, names, noffsets):
    """'@' and what name_skip leaves of every name: the names of the image fastx_format makes, parsed back"""
    return ragged([np.concatenate([[ord("@")], x[min(p.name_skip, len(x)):]]).astype(np.uint8) for x in split(names, noffsets)])


def library_pipeline(p, lib, orc):
    """the references of the second library's stages, each fed by the previous one's reference output -> dict of arrays"""
    H = {}
    n = lib.n
    # ---- records: by construction
    for m in (1, 2):
        H[f"r{m}_bases"], H[f"r{m}_offsets"] = ragged(lib.reads[m - 1])
        H[f"r{m}_quals"], _ = ragged(lib.quals[m - 1])
        H[f"r{m}_layout"] = _layout_word(H[f"r{m}_offsets"])
        H[f"r{m}_names"], H[f"r{m}_noffsets"] = ragged([np.frombuffer(x, np.uint8) for x in lib.names[m - 1]])
    b1, q1, o1, b2, q2, o2 = H["r1_bases"], H["r1_quals"], H["r1_offsets"], H["r2_bases"], H["r2_quals"], H["r2_offsets"]
    # ---- the pairs deduplicated, the score the quality sum of mate 1
    H["lq_rows"] = Q.reads_quality_np(b1, q1, n, 0, o1, p.phred_base, p.min_q, p.trim_q, p.k)[1]
    score = None if p.dd_score == "none" else H["lq_rows"][:, Q.RQ_QSUM]
    H["dd_rows"], H["dd_keep"], H["dd_summary"] = dedup_np(lib.reads[0], lib.reads[1], p, score)
    keep = H["dd_keep"]
    for m, (b, q, o) in enumerate(((b1, q1, o1), (b2, q2, o2)), 1):
        H[f"dp{m}_bases"], H[f"dp{m}_offsets"], H[f"dp{m}_index"] = reads_np.select_np(b, n, 0, o, keep=keep)
        H[f"dp{m}_quals"] = reads_np.select_np(q, n, 0, o, keep=keep)[0]
    H["dpn_bases"], H["dpn_offsets"] = reads_np.gather_np(H["r1_names"], n, 0, H["dp1_index"], H["r1_noffsets"])
    # ---- mate 1 of the survivors deduplicated alone
    b, q, o, idx = H["dp1_bases"], H["dp1_quals"], H["dp1_offsets"], H["dp1_index"].astype(np.int64)
    nd = len(idx)
    H["ds_rows"], H["ds_keep"], H["ds_summary"] = dedup_np(split(b, o), None, p, None if score is None else score[idx])
    H["ds_bases"], H["ds_offsets"], H["ds_index"] = reads_np.select_np(b, nd, 0, o, keep=H["ds_keep"])
    H["ds_quals"] = reads_np.select_np(q, nd, 0, o, keep=H["ds_keep"])[0]
    H["dsn_bases"], H["dsn_offsets"] = reads_np.gather_np(H["dpn_bases"], nd, 0, H["ds_index"], H["dpn_offsets"])
    # ---- poly-X ends and low complexity of that
    b, q, o = H["ds_bases"], H["ds_quals"], H["ds_offsets"]
    ns = len(H["ds_index"])
    H["cx_rows"], H["cx_masked"] = complexity_np(p, b, ns, o)
    H["xt_rows"], _ = complexity_np(p, b, ns, o, X.DUST_NEVER)
    H["xt_bases"], H["xt_offsets"], H["xt_index"] = reads_np.select_np(b, ns, 0, o, span=H["xt_rows"][:, X.RX_KEEP])
    H["xt_quals"] = reads_np.select_np(q, ns, 0, o, span=H["xt_rows"][:, X.RX_KEEP])[0]
    keep, span = diff_keep(p, H["cx_rows"]), H["cx_rows"][:, X.RX_KEEP]
    H["xf_bases"], H["xf_offsets"], H["xf_index"] = reads_np.select_np(b, ns, 0, o, keep=keep, span=span)
    H["xf_quals"] = reads_np.select_np(q, ns, 0, o, keep=keep, span=span)[0]
    H["xfn_bases"], H["xfn_offsets"] = reads_np.gather_np(H["dsn_bases"], ns, 0, H["xf_index"], H["dsn_offsets"])
    # ---- the table of the masked batch
    H["cm_k"], H["cm_c"] = table_of_batch(orc, H["cx_masked"], o, p.count_k)
    # ---- back to text, and the text parsed
    b, q, o, nf = H["xf_bases"], H["xf_quals"], H["xf_offsets"], len(H["xf_index"])
    named = dict(names=H["xfn_bases"], name_offsets=H["xfn_offsets"], name_skip=p.name_skip)
    H["fq_image"], H["fq_rec"] = FO.format_np(b, nf, 0, o, quals=q, fmt=FO.FASTQ, **named)
    H["fa_image"], H["fa_rec"] = FO.format_np(b, nf, 0, o, fmt=FO.FASTA, line_width=p.fa_width, **named)
    H["gq_image"], H["gq_rec"] = FO.format_np(b, nf, 0, o, name_base=p.name_base, fmt=FO.FASTQ, qual_fill=p.qual_fill)
    H["rp_bases"], H["rp_quals"], H["rp_offsets"], H["rp_layout"] = b, q, o, _layout_word(o)
    H["rp_names"], H["rp_noffsets"] = names_behind_skip(p, H["xfn_bases"], H["xfn_offsets"])
    # ---- the route pass: the raw mates
    H["rt2_dd_rows"], H["rt2_dd_keep"], H["rt2_dd_summary"] = (H["dd_rows"], H["dd_keep"], H["dd_summary"]) if score is None else \
        dedup_np(lib.reads[0], lib.reads[1], p, None)
    H["rt2_cx_rows"], H["rt2_cx_masked"] = complexity_np(p, b1, n, o1)
    H["rt2_fq_image"], H["rt2_fq_rec"] = FO.format_np(b1, n, 0, o1, quals=q1, names=H["r1_names"], name_offsets=H["r1_noffsets"], name_skip=p.name_skip)
    return H


# ---------------------------------------------------------------- what a seed of the second library has to be able to get wrong
# the flags that only some seeds can show: flag -> the plans that can
STRUCTURE_WHEN = {
    "dd_exact_dropped": lambda p: p.dd_hash_bits >= 8,
    "dd_case_dropped": lambda p: p.dd_hash_bits >= 8,
    "dd_other_byte_dropped": lambda p: p.dd_hash_bits >= 8,
    "dd_pair_flipped": lambda p: p.dd_strand and p.dd_hash_bits == 64,
    "ds_read_flipped": lambda p: p.dd_strand and p.dd_hash_bits == 64,
    "dd_collision": lambda p: p.dd_hash_bits <= 8,
    "dd_head_not_first": lambda p: p.dd_score != "none" and p.dd_hash_bits >= 8,
    "px_tail_found": lambda p: p.px_tail != 0,
    "px_head_found": lambda p: p.px_head != 0,
    "fmt_empty_name": lambda p: p.name_skip >= 1,
    "fa_one_full_line": lambda p: p.fa_width >= 60,
    "fa_partial_last_line": lambda p: p.fa_width >= 60,
}


def library_structure(p, H, lib):
    """the flags of the second library's stages, read off the reference's arrays and the library's record of what was planted"""
    u32 = np.uint64(0xFFFFFFFF)
    dd, keep = H["dd_rows"], H["dd_keep"]
    rep, flags = dd[:, D.REP].astype(np.int64), dd[:, D.FLAGS]
    root = lib.src.copy()
    for _ in range(3):
        root = np.where((root >= 0) & (lib.src[np.maximum(root, 0)] >= 0), lib.src[np.maximum(root, 0)], root)

    def dropped(kind):
        """a copy of this kind was dropped, or the item it was made from was dropped onto it"""
        return any(keep[i] == 0 or (keep[root[i]] == 0 and rep[root[i]] == i) for i in lib.where(kind))

    def near_kept(kind):
        return any(keep[i] == 1 and keep[lib.src[i]] == 1 for i in lib.where(kind))

    cx = H["cx_rows"]
    L = cx[:, X.RX_BASES].astype(np.int64)
    tail, head = (cx[:, X.RX_TAIL] & u32).astype(np.int64), (cx[:, X.RX_HEAD] & u32).astype(np.int64)
    item_of_row = H["dp1_index"].astype(np.int64)[H["ds_index"].astype(np.int64)]
    row_of_item = {int(i): r for r, i in enumerate(item_of_row)}
    end_len = lambda i, end: int((tail if end == "tail" else head)[row_of_item[i]])
    planted = [(i, end, kind, R) for i, (end, kind, R) in lib.ends.items() if i in row_of_item]
    n_dusty = (cx[:, X.RX_DUST] >> np.uint64(32)).astype(np.int64)
    n_win = np.array([X.n_windows(int(x)) for x in L])
    dk = diff_keep(p, cx)
    pairs = (cx[:, X.RX_DIFF] >> np.uint64(32)) > 0
    nlen = np.diff(H["xfn_offsets"].astype(np.int64))
    flen = np.diff(H["xf_offsets"].astype(np.int64))
    W = p.fa_width
    return {
        "dd_exact_dropped": dropped("exact"),
        "dd_case_dropped": dropped("case"),
        "dd_other_byte_dropped": dropped("other"),
        "dd_pair_flipped": bool((flags & np.uint64(D.F_FLIPPED)).any()),
        "ds_read_flipped": bool((H["ds_rows"][:, D.FLAGS] & np.uint64(D.F_FLIPPED)).any()),
        **{"dd_kept_" + kind: near_kept(kind) for kind in NEAR_KINDS},
        "dd_collision": bool((flags & np.uint64(D.F_COLLISION)).any()),
        "dd_head_not_first": bool(((keep == 0) & (rep > np.arange(len(rep)))).any()),
        "px_tail_found": bool((tail > 0).any()),
        "px_head_found": bool((head > 0).any()),
        "px_run_of_min_len": any(kind == "exact" and end_len(i, end) == p.px_min_len for i, end, kind, R in planted),
        "px_run_below_min_len": any(kind == "minus" and end_len(i, end) == 0 for i, end, kind, R in planted),
        "px_empty_keep": bool(((L > 0) & (cx[:, X.RX_KEEP] == 0)).any()),
        "dust_mixed_windows": bool(((n_dusty > 0) & (n_dusty < n_win)).any()),
        "diff_drops_and_keeps": bool((~dk & pairs).any() and (dk & pairs).any()),
        "fmt_empty_name": bool((nlen <= p.name_skip).any()),
        "fmt_long_name": bool((nlen - p.name_skip > 256).any()),
        "fmt_empty_read": bool((flen == 0).any()),
        "fa_one_full_line": bool(W and (flen == W).any()),
        "fa_partial_last_line": bool(W and ((flen > W) & (flen % max(W, 1) != 0)).any()),
    }


# ---------------------------------------------------------------- the relations of the second library
def dedup_permutation(n, seed):
    return np.random.default_rng(72_000 + seed).permutation(n)


def check_dedup_permuted(first, got, perm):
    """first = (rows, keep) of the items with score = the item's index, got = those of the items in the order perm (item j of got is
    item perm[j] of first) with score = perm: the kept set and every COUNT map through the permutation, every REP names the same item"""
    inv = np.argsort(perm)
    assert np.array_equal(got[1], first[1][perm]), "permuted dedup: the kept set"
    assert np.array_equal(got[0][:, D.COUNT], first[0][perm, D.COUNT]), "permuted dedup: COUNT"
    assert np.array_equal(got[0][:, D.REP].astype(np.int64), inv[first[0][perm, D.REP].astype(np.int64)]), "permuted dedup: REP"
    assert np.array_equal(got[0][:, D.HASH], first[0][perm, D.HASH]), "permuted dedup: HASH"


def check_dedup_exchanged(first, got, want_flags=None):
    """first = (rows, keep) of the pairs under the strand flag, got = those of the same pairs with every pair's mates exchanged: the
    same keep bytes, REP, COUNT and key; FLIPPED, KEPT and COLLISION as they were, OTHER as the reference of the exchanged pairs has it"""
    same = np.uint64(D.F_KEPT | D.F_FLIPPED | D.F_COLLISION)
    assert np.array_equal(got[1], first[1]), "exchanged mates: keep"
    for w in (D.REP, D.COUNT, D.HASH):
        assert np.array_equal(got[0][:, w], first[0][:, w]), ("exchanged mates: word", w)
    assert np.array_equal(got[0][:, D.FLAGS] & same, first[0][:, D.FLAGS] & same), "exchanged mates: FLIPPED / KEPT / COLLISION"
    if want_flags is not None:
        assert np.array_equal(got[0][:, D.FLAGS], want_flags), "exchanged mates: the flags of the reference"


def check_dedup_conserved(rows, keep, summary):
    n = len(keep)
    kept = int(keep.sum())
    assert int(rows[:, D.COUNT].sum()) == n and int(summary[D.S_KEPT]) == kept and int(summary[D.S_KEPT] + summary[D.S_DROPPED]) == n
    assert int(summary[D.S_COLLISIONS]) == int(((rows[:, D.FLAGS] & np.uint64(D.F_COLLISION)) != 0).sum())
    assert int(summary[D.S_LARGEST]) == int(rows[:, D.COUNT].max(initial=0))
    assert np.array_equal((rows[:, D.FLAGS] & np.uint64(D.F_KEPT)) != 0, keep != 0)


def comp_mask(mask):
    """the base mask of the complemented letters: A <-> T, C <-> G"""
    return sum(1 << (3 - x) for x in range(4) if (mask >> x) & 1)


def mirror_batch(bases, offsets):
    """every read reverse-complemented (the case kept, any byte that is no letter as it is) -> (bases, offsets)"""
    return ragged([rc_read(r) for r in split(bases, offsets)])


def mirror_args(p):
    """the poly-X arguments of the mirrored batch: head and tail masks exchanged and complemented"""
    return {**p.px_args, "tail": comp_mask(p.px_head), "head": comp_mask(p.px_tail)}


def check_complexity_mirror(rows, got):
    """rows: of a batch, got: of mirror_batch of it under mirror_args -> the number of reads whose DUST word was compared"""
    u32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    swap = lambda w: (w >> s32) | ((w & u32) << s32)
    other = lambda w: np.where(w == 0, w, (w & u32) | ((np.uint64(5) - (w >> s32)) << s32))
    t = rows[:, X.RX_TAIL] & u32
    keep = rows[:, X.RX_KEEP]
    assert np.array_equal(got[:, X.RX_BASES], rows[:, X.RX_BASES]) and np.array_equal(got[:, X.RX_DIFF], rows[:, X.RX_DIFF]), "mirror: BASES / DIFF"
    assert np.array_equal(got[:, X.RX_TAIL], other(rows[:, X.RX_HEAD])) and np.array_equal(got[:, X.RX_HEAD], other(rows[:, X.RX_TAIL])), "mirror: TAIL / HEAD"
    assert np.array_equal(got[:, X.RX_KEEP], np.where(keep == 0, keep, t | (keep & ~u32))), "mirror: KEEP"
    assert np.array_equal(got[:, X.RX_AC], swap(rows[:, X.RX_GT])) and np.array_equal(got[:, X.RX_GT], swap(rows[:, X.RX_AC])), "mirror: AC / GT"
    short = rows[:, X.RX_BASES] <= np.uint64(64)
    assert np.array_equal(got[short, X.RX_DUST], rows[short, X.RX_DUST]), "mirror: DUST of the reads of one window"
    return int(short.sum())


def fasta_of_fastq(image, rec):
    """the FASTQ image without its '+' and quality lines, '@' replaced by '>' -> uint8 array"""
    image = bytes(np.asarray(image, np.uint8).tobytes())
    out = []
    for a, e in zip(rec[:-1].tolist(), rec[1:].tolist()):
        r = image[int(a):int(e)]
        name, rest = r[1:].split(b"\n", 1)
        L = (len(r) - len(name) - 6) // 2
        assert r[:1] == b"@" and rest[L:L + 3] == b"\n+\n" and r[-1:] == b"\n" and len(rest) == 2 * L + 4
        out.append(b">" + name + b"\n" + rest[:L] + b"\n")
    return np.frombuffer(b"".join(out), np.uint8)


def record_offsets(p, H, fmt, width=0):
    """the cumulative sums of fastx_out_np.record_len over the formatted batch, for the named records of the format stage"""
    L = np.diff(H["xf_offsets"].astype(np.int64))
    N = np.diff(H["xfn_offsets"].astype(np.int64))
    N = N - np.minimum(N, p.name_skip)
    return np.concatenate([[0], np.cumsum([FO.record_len(int(l), int(k), fmt, width) for l, k in zip(L, N)])]).astype(np.uint64)
