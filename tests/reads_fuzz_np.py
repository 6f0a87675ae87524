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
* structure(plan, H): what a seed has to get wrong, read off the reference's arrays alone.

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

numpy only: the oracle is loaded inside host_pipeline, torch nowhere.
"""
import dataclasses
import functools

import numpy as np

from tests import adapter_np as A
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
}
# the references of the route pass, on the raw parsed mates: adapter rows are ad_rows; these are the rest
ROUTES = ("rt_q_masked", "rt_q_rows", "rt_ov_rows", "rt_mg_bases", "rt_mg_quals", "rt_mg_offsets", "rt_mg_rows", "rt_sel_bases", "rt_sel_offsets",
          "rt_sel_index", "rt_gat_bases", "rt_gat_offsets")


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
                layouts=_layouts(seed, mode, len1, L1, lead), layouts2=_layouts(seed, mode, len2, L2, lead))


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
    assert set(H) == {x for names in STAGES.values() for x in names}
    # ---- the route pass: the reads-form calls on the raw parsed mates
    H["rt_q_masked"], H["rt_q_rows"] = Q.reads_quality_np(b1, q1, n, 0, o1, p.phred_base, p.min_q, p.trim_q, p.k, Q.ee_weights(p.phred_base))
    rov = H["rt_ov_rows"] = overlap_np(p, b1, o1, b2, o2, n)
    H["rt_mg_bases"], H["rt_mg_quals"], H["rt_mg_offsets"], H["rt_mg_rows"] = M.reads_pair_merge_np(b1, b2, n, 0, 0, rov[:, A.RP_INSERT], q1, q2, o1, o2,
                                                                                                    p.phred_base, p.q_cap)
    H["rt_sel_bases"], H["rt_sel_offsets"], H["rt_sel_index"] = reads_np.select_np(b1, n, 0, o1, span=span, min_len=p.min_len)
    H["rt_gat_bases"], H["rt_gat_offsets"] = reads_np.gather_np(b1, n, 0, gather_index(p, n), o1, span=span)
    assert set(H) == {x for names in STAGES.values() for x in names} | set(ROUTES)
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
