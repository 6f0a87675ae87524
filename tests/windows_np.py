"""The window calls -- kmx_canonical_windows and kmx_canonical_windows2 -- on the host: the launchers' routing restated as a table of
kernel ARMS, the cases tests/test_gpu_windows_sweep.py runs, and what they must find in every slot.

* arm_of: which kernels a parameter set runs (kmx_api.hip; windows_uniform_passes, windows_ragged_passes, dispatch and scan_domain*
  in kmx_scan.hip / kmx_scan_kernel.h; launch_windows2_tiled* and the lane-per-read kernels in kmx_generic.hip; the segment plans of
  kmx_segments.hip; launch_sweep_windows in kmx_sweep.hip), the work UNIT of the launch and how many units one launch holds at once
  per compute unit.  ARMS names every arm; a case names the kernels of its passes ("ring<10,k>=18>+sinkflags<10,k>=18>"), the plan
  in front of them ("seg_uniform") and the ZERO sweep behind them ("zero<10,uniform,1w>").
* CASES: one parameter set or more per arm, each the smallest shape that reaches it.  EDGE: 1, 63, 64, 65 reads and exactly U units.
* build(case, n_cu): a batch of U + U // 3 + 6 units and a partial last tile.  U is the most units one launch can hold AT ONCE:
    - the ticket-queue scans (launch_one): n_cu x blocks_per_cu x 4 waves, a tile each -- at most 8 waves per SIMD, 32 n_cu tiles;
    - windows2_tiled_kernel: 16 n_cu waves by the launcher's cap, stride t += waves;
    - the lane-per-read kernels: grid_for caps at 8 n_cu blocks of 256 lanes, a read each;
    - segment arms: the same kernels over tiles of 64 SEGMENTS;
    - the ZERO sweep (cases with zero=True): the window sinks tell it "many", so all 8 n_cu waves of its 2 n_cu blocks sweep, a
      group of 64 mask words (tiles) each: 512 n_cu tiles.  (The 64-wave sweep of a batch with few marks cannot be reached from
      these calls: both window sinks store 1 << 40 for the marked count.)
  By pigeonhole at least U // 3 + 6 units are then some wave's (lane's) second or later unit, in whatever order tickets are drawn.
* The batch repeats a BLOCK of P random reads (ragged: and their lengths), P a prime above the batch's number of tiles: tile t
  starts at read 64 t mod P of the block, so no two tiles hold the same reads and a tile's words at another tile's slots cannot
  compare equal.  The expected arrays are the oracle's outputs for ONE block, repeated; test_windows_np.py shows that this equals
  the oracle on the whole batch.  windows_np restates the slot rule of include/kmx.h in numpy: slot(r, p) = win_off(r) + p, an
  invalid window's slot holds words 0 and flags 0.

What the launchers do where a first reading says otherwise:
* windows2: STAGE is every launch with a word array -- one launch per array, the flags riding with the first; the kernel without the
  staging block runs for the flags alone.  Fewer than 64 reads, or word arrays that are not 16-byte aligned, go to the lane-per-read kernel.
* the staged sink's non-temporal branch takes the blocks of 16 windows of a W % 8 == 0 read; at W % 16 == 8 the last block is plain.
* several word arrays WITHOUT flags are ring passes only; the flags alone (W % 16 != 0, W >= 32, aligned) are SinkFlags only.
* reads above 256 bases from a misaligned base are not planned as segments: the lane-per-read kernels.
* the ZERO sweep fields 64 waves for few marks and all 8 n_cu otherwise; the window sinks always say "many", so its waves take a
  second mask group only past 512 n_cu tiles.  The 16-word uniform frame needs reads of 161 bases for that: the two largest cases.

Not in the table: uniform reads with a caller's d_win_offsets (the lane-per-read kernels take them)."""
from __future__ import annotations

import dataclasses

import numpy as np

from tests import elem_np as E

OK = E.OK
POISON_U64, POISON_U8 = E.POISON_U64, E.POISON_U8
NAMES = ("fw", "rc", "canon", "flags")
ALL4 = NAMES
WIN_VALID, WIN_FW_CANONICAL = 1, 2
# device footprint of the largest case on 256 compute units (bases, offsets, poisoned outputs): every arm but two stays under 1.1 GiB;
# the ZERO sweep of the 16-word UNIFORM frame strides only past 512 n_cu tiles of reads of 161 bases -- 1.8 GB of bases and, flags
# alone, 1.1 to 1.5 GB of output
CAP_BYTES = 4 << 30
DIRTY_READS = 0.004                # share of a block's reads that get one invalid byte (besides the fixed ones)
_I = np.int64


# ------------------------------------------------------------------ the slot rule, in numpy

def _pack(codes: np.ndarray) -> np.ndarray:
    """(m, j <= 32) 2-bit codes -> m words, base 0 in the lowest bits"""
    return E._pack_words(codes) if codes.shape[1] else np.zeros(len(codes), np.uint64)


def windows_np(host, start, lens, win, k: int):
    """reads host[start[r] : start[r] + lens[r]] -> (fw, rc, canon, flags) with slot win[r] + p for window p of read r; k <= 31: u64
    arrays, k in 33..64: (slots, 2) arrays (low word, high word) of the 2k-bit little-endian integer"""
    start, lens, win = np.asarray(start).astype(_I), np.asarray(lens).astype(_I), np.asarray(win).astype(_I)
    two = k > 32
    nk = np.maximum(lens - k + 1, 0)
    total = int(win[-1]) if len(win) > len(lens) else int((win + nk).max(initial=0))
    shape = (total, 2) if two else (total,)
    fw, rc, canon, flags = np.zeros(shape, np.uint64), np.zeros(shape, np.uint64), np.zeros(shape, np.uint64), np.zeros(total, np.uint8)
    n_w = int(nk.sum())
    if n_w == 0:
        return fw, rc, canon, flags
    read = np.repeat(np.arange(len(lens)), nk)
    p = np.arange(n_w) - np.repeat(np.cumsum(nk) - nk, nk)
    at, slot = start[read] + p, win[read] + p
    codes, valid = E.base_codes(np.asarray(host, np.uint8))
    c = codes[at[:, None] + np.arange(k)]
    ok = valid[at[:, None] + np.arange(k)].all(axis=1)
    r = (3 - c)[:, ::-1]
    if two:
        f = np.stack([_pack(c[:, :32]), _pack(c[:, 32:])], axis=1)
        g = np.stack([_pack(r[:, :32]), _pack(r[:, 32:])], axis=1)
        lt = (f[:, 1] < g[:, 1]) | ((f[:, 1] == g[:, 1]) & (f[:, 0] < g[:, 0]))
        cn = np.where(lt[:, None], f, g)
        z = ok[:, None]
    else:
        f, g = _pack(c), _pack(r)
        lt = f < g
        cn = np.where(lt, f, g)
        z = ok
    fw[slot], rc[slot], canon[slot] = np.where(z, f, 0), np.where(z, g, 0), np.where(z, cn, 0)
    flags[slot] = np.where(ok, WIN_VALID | np.where(lt, WIN_FW_CANONICAL, 0), 0)
    return fw, rc, canon, flags


# ------------------------------------------------------------------ the arms

@dataclasses.dataclass(frozen=True)
class Arm:
    name: str            # the kernels of the passes, joined with "+"
    unit: str            # "tile" (64 reads), "segtile" (64 segments), "read"
    per_cu: int          # units one launch holds at once per compute unit
    plan: str = ""       # "seg_uniform", "seg_ragged", "seg2_uniform", "seg2_ragged": the segment plan in front of the passes
    zero: str = ""       # the ZERO sweep behind the passes

    @property
    def names(self):
        return tuple(self.name.split("+")) + tuple(x for x in (self.plan, self.zero) if x)


def word_arm(k: int) -> str:
    """dispatch: launch_one<NW, V, DW> = <1, 1>, <1, 2>, <2, 2>"""
    return "k<=16" if k <= 16 else "k=17" if k == 17 else "k>=18"


def segments_per_read(L: int, k: int) -> int:
    """uniform_segments_per_read: as few as the 16-word frame allows (at most 257 - k windows each)"""
    return -(-(L - k + 1) // (257 - k))


def seg_count(lens, k: int):
    """kmx_segments.hip: read r of W_r windows is cut into ceil(W_r / (257 - k)) segments"""
    return -(-np.maximum(np.asarray(lens).astype(_I) - k + 1, 0) // (257 - k))


def _ragged_sinks(n_arr: int, flags: bool, nw: int, wa: str) -> str:
    """windows_ragged_passes"""
    ring, staged = f"rring<{nw},{wa}>", f"rstaged<{nw},{wa}>"
    if n_arr == 1 and not flags:
        return ring
    if n_arr >= 2:
        return ring + ("+" + staged if flags else "")
    return staged


def arm_of(call: str, k: int, L: int, ragged: bool, lead: int, want, flags_shift: int = 0, words_shift: int = 0, n: int = 1 << 20,
           n_seg: int | None = None) -> Arm:
    """call: "windows" (k in 1..31) or "windows2" (k in 33..64); L: the one read length, or the bound handed in as read_len (0: none);
    lead: d_bases mod 16; want: the outputs that are not NULL; flags_shift: d_flags mod 16; words_shift: the word arrays mod 16;
    n: the number of reads (windows2 tiles from 64 on); n_seg: the segments ragged reads above 256 bases are cut into (default: one
    per read) -- windows2 decides by THEIR number, as windows2_segments hands them to launch_windows2_tiled_ragged as reads"""
    n_arr, flags = sum(x in want for x in NAMES[:3]), "flags" in want
    assert n_arr or flags
    if call == "windows2":
        assert 33 <= k <= 64 and (ragged or L >= k)
        g = lambda why: Arm(f"generic2[{why}]", "read", 8 * 256)
        kind = "STAGE" if n_arr else "FLAGS"        # one STAGE launch per word array (the flags ride with the first); FLAGS: the flags alone
        if L > 256:
            if lead:
                return g("L>256,misaligned")
            if (n_seg if n_seg is not None else n if ragged else n * segments_per_read(L, k)) < 64:
                return g("n<64")
            if n_arr and words_shift % 16:
                return g("words misaligned")
            return Arm("+".join([f"w2<16,{kind},segments>"] * max(n_arr, 1)), "segtile", 16, "seg2_ragged" if ragged else "seg2_uniform", "zero<16,ragged,2w>")
        if n < 64:
            return g("n<64")
        if n_arr and words_shift % 16:
            return g("words misaligned")
        if ragged:
            if lead:
                return g("ragged,misaligned")
            nw = 10 if max(L or 256, k + 15) <= 160 else 16
            return Arm("+".join([f"w2<{nw},{kind},ragged>"] * max(n_arr, 1)), "tile", 16, "", f"zero<{nw},ragged,2w>")
        if lead and L in (160, 256):
            return g(f"L={L},misaligned")
        nw = 10 if L <= 160 else 16
        return Arm("+".join([f"w2<{nw},{kind},uniform>"] * max(n_arr, 1)), "tile", 16, "", f"zero<{nw},uniform,2w>")
    assert call == "windows" and 1 <= k <= 31 and (ragged or L >= k), (call, k, L)
    g = lambda why: Arm(f"generic1[{why}]", "read", 8 * 256)
    wa = word_arm(k)
    if k == 1:
        return g("k=1")
    if L > 256:
        if lead:
            return g("L>256,misaligned")
        return Arm(_ragged_sinks(n_arr, flags, 16, wa), "segtile", 32, "seg_ragged" if ragged else "seg_uniform", "zero<16,ragged,1w>")
    if ragged:
        if lead:
            return g("ragged,misaligned")
        nw = 16 if L > 160 or L == 0 else 10
        return Arm(_ragged_sinks(n_arr, flags, nw, wa), "tile", 32, "", f"zero<{nw},ragged,1w>")
    if lead and L in (160, 256):
        return g(f"L={L},misaligned")
    nw, W = (16 if L > 160 else 10), L - k + 1
    zero = f"zero<{nw},uniform,1w>"
    ring, sflags = f"ring<{nw},{wa}>", f"sinkflags<{nw},{wa}>"
    if n_arr == 1 and not flags and W % 16:                              # SinkWindowsT<true>::wants_aligned
        return Arm(ring, "tile", 32, "", zero)
    if W % 16 and W >= 32 and (not flags or flags_shift % 16 == 0):      # one ring pass per array, the flags kernel
        return Arm("+".join([ring] * n_arr + [sflags] * flags), "tile", 32, "", zero)
    return Arm(f"staged<{nw},{wa},{'nt' if W % 8 == 0 else 'plain'}>", "tile", 32, "", zero)


_NWW = [(nw, wa) for nw in (10, 16) for wa in ("k<=16", "k=17", "k>=18")]
ARMS = (
    [f"{s}<{nw},{wa}>" for s in ("ring", "sinkflags", "rring", "rstaged") for nw, wa in _NWW]
    + [f"staged<{nw},{wa},{st}>" for nw, wa in _NWW for st in ("nt", "plain")]
    + ["seg_uniform", "seg_ragged", "seg2_uniform", "seg2_ragged"]
    + [f"w2<{nw},{kind},{lay}>" for nw in (10, 16) for kind in ("STAGE", "FLAGS") for lay in ("uniform", "ragged")]
    + ["w2<16,STAGE,segments>", "w2<16,FLAGS,segments>"]
    + [f"generic1[{why}]" for why in ("k=1", "ragged,misaligned", "L=160,misaligned", "L=256,misaligned", "L>256,misaligned")]
    + [f"generic2[{why}]" for why in ("ragged,misaligned", "L=160,misaligned", "L=256,misaligned", "L>256,misaligned", "words misaligned")]
    + [f"zero<{nw},{lay},{w}>" for nw in (10, 16) for lay in ("uniform", "ragged") for w in ("1w", "2w")]
)
# arms no batch past one sweep can reach: the size that selects them is below every sweep
EDGE_ONLY = {"generic2[n<64]": "kmx_canonical_windows2 of fewer than 64 reads: the edge sizes 1 and 63 run it"}


# ------------------------------------------------------------------ the cases

@dataclasses.dataclass(frozen=True)
class P:
    call: str
    k: int
    L: int                      # the one read length / the bound handed in as read_len (0: none)
    want: tuple = ("canon",)
    ragged: bool = False
    lead: int = 0               # d_bases mod 16
    flags_shift: int = 0        # d_flags mod 16
    words_shift: int = 0        # the word arrays mod 16 (0 or 8)
    lmax: int = 0               # ragged: the longest read (default: the bound)
    short: bool = False         # ragged: lengths k - 2 .. k + 2 (but the fixed reads)
    zero: bool = False          # sized for the ZERO sweep: U = 512 n_cu tiles

    @property
    def arm(self) -> Arm:
        return arm_of(self.call, self.k, self.L, self.ragged, self.lead, self.want, self.flags_shift, self.words_shift)

    @property
    def longest(self) -> int:
        return self.lmax or self.L if self.ragged else self.L

    @property
    def id(self) -> str:
        a = self.arm
        lay = f"ragged{self.L}" + (f"max{self.lmax}" if self.lmax else "") + ("short" if self.short else "") if self.ragged else f"L{self.L}"
        w = "all" if self.want == ALL4 else ",".join(self.want)
        return (f"{a.zero + '!' if self.zero else ''}{a.plan + ':' if a.plan else ''}{a.name}-k{self.k}-{lay}-{w}+{self.lead}"
                + (f"f{self.flags_shift}" if self.flags_shift else "") + (f"w{self.words_shift}" if self.words_shift else ""))


def _cases():
    W1, W2, F, C = "windows", "windows2", ("flags",), ("canon",)
    c = []
    # ---- one-word k, uniform reads, the 10-word frame: reads of 40..70 bases; k = 11, 17, 25 are the three word arms
    c += [P(W1, 11, 47, C), P(W1, 17, 61, ("fw",), lead=5), P(W1, 25, 70, ("rc",)),                        # the ring: W = 37, 45, 46 (it wraps)
          P(W1, 11, 43, C, lead=9),                                                                          # ... and W = 33 from a misaligned base
          P(W1, 11, 50, ALL4, lead=3), P(W1, 17, 53, ALL4), P(W1, 25, 67, ALL4, lead=15),                   # ring passes + SinkFlags: W = 40, 37, 43
          P(W1, 11, 58, ALL4), P(W1, 17, 48, ALL4, lead=1), P(W1, 25, 56, ALL4),                            # staged, W % 16 == 0: 48, 32, 32
          P(W1, 11, 50, ("canon", "flags"), flags_shift=4),                                                  # ... W = 40 behind a misaligned d_flags: two nt blocks, a plain one
          P(W1, 11, 40, ALL4, lead=7), P(W1, 17, 44, ALL4), P(W1, 25, 47, ALL4, lead=2),                    # staged, W < 32 with several outputs: 30, 28, 23
          P(W1, 25, 70, ("canon", "flags"), flags_shift=1)]                                                  # ... W = 46 behind a misaligned d_flags
    # ---- the 16-word frame: reads of 161..176 bases, one output
    c += [P(W1, 11, 161, C), P(W1, 17, 163, ("fw",), lead=4), P(W1, 25, 170, ("rc",)),                      # the ring: W = 151, 147, 146
          P(W1, 11, 165, F, lead=8), P(W1, 17, 161, F), P(W1, 25, 176, ("canon", "flags"), lead=6),          # SinkFlags (the last: a ring pass in front)
          P(W1, 6, 165, C), P(W1, 17, 176, F, lead=11), P(W1, 18, 161, F),                                  # staged, W = 160, 160, 144
          P(W1, 11, 161, F, flags_shift=3), P(W1, 17, 163, F, lead=13, flags_shift=8), P(W1, 25, 170, F, flags_shift=15)]   # staged, plain: misaligned d_flags
    # ---- one-word k, ragged reads: lengths 0 .. bound
    c += [P(W1, 11, 64, C, True), P(W1, 17, 60, ("fw",), True), P(W1, 25, 70, ("rc",), True),              # the ragged ring
          P(W1, 11, 64, ALL4, True), P(W1, 17, 64, ("fw", "rc"), True), P(W1, 25, 64, ALL4, True),           # ring passes (+ staged flags)
          P(W1, 11, 64, F, True), P(W1, 17, 64, ("canon", "flags"), True), P(W1, 25, 64, F, True),          # staged alone
          P(W1, 11, 170, C, True), P(W1, 17, 0, C, True, lmax=176), P(W1, 25, 165, ("fw",), True),           # the 16-word frame: a bound above 160, or none
          P(W1, 11, 161, ("fw", "canon", "flags"), True), P(W1, 17, 176, ("rc", "canon"), True), P(W1, 25, 0, ("canon", "rc", "flags"), True, lmax=170),
          P(W1, 11, 0, F, True, lmax=170), P(W1, 17, 170, F, True), P(W1, 25, 170, ("canon", "flags"), True)]
    # ---- reads above the frames, planned (uniform) or cut (ragged) into segments of at most 257 - k windows
    c += [P(W1, 31, 257, C), P(W1, 9, 300, F), P(W1, 31, 300, C, True), P(W1, 17, 290, F, True)]
    c += [P(W2, 33, 257, C), P(W2, 40, 300, F, True)]
    # ---- two-word k: windows2_tiled_kernel<NW, STAGE, RAGGED>
    c += [P(W2, 33, 47, ALL4), P(W2, 47, 70, C, lead=3), P(W2, 64, 161, C), P(W2, 40, 55, F, lead=12), P(W2, 33, 176, F, lead=7),
          P(W2, 33, 70, ALL4, True), P(W2, 33, 0, C, True, lmax=176), P(W2, 40, 64, F, True), P(W2, 64, 170, F, True)]
    # ---- the lane-per-read kernels
    c += [P(W1, 1, 12, ALL4), P(W1, 1, 24, ALL4, True, lead=5), P(W1, 11, 24, ALL4, True, lead=3),
          P(W1, 31, 160, C, lead=1), P(W1, 31, 256, F, lead=15), P(W1, 31, 257, F, lead=2),
          P(W2, 33, 44, ALL4, True, lead=9), P(W2, 64, 160, F, lead=4), P(W2, 64, 256, F, lead=8), P(W2, 64, 257, F, lead=6),
          P(W2, 33, 40, C, words_shift=8)]
    # ---- the ZERO sweep past its 8 n_cu waves: one window per read (uniform), reads around k bases (ragged: the bound picks the frame)
    c += [P(W1, 8, 8, C, zero=True), P(W1, 8, 12, C, True, short=True, zero=True), P(W1, 8, 170, C, True, short=True, zero=True),
          P(W2, 33, 33, F, zero=True), P(W2, 33, 40, F, True, short=True, zero=True), P(W2, 33, 170, F, True, short=True, zero=True)]
    # ... of the 16-word uniform frame: the shortest reads it takes, the largest k (the fewest windows), the flags alone
    c += [P(W1, 31, 161, F, zero=True), P(W2, 64, 161, F, zero=True)]
    return c


CASES = _cases()
SIZES = (1, 63, 64, 65, "U")
# the edge sets: each one-word and each two-word arm family
EDGE = [P("windows", 25, 70, ("canon",), lead=5), P("windows", 11, 50, ALL4), P("windows", 17, 48, ALL4, lead=1), P("windows", 11, 40, ALL4),
        P("windows", 25, 64, ("canon",), True), P("windows", 11, 64, ALL4, True), P("windows", 17, 64, ("flags",), True),
        P("windows", 31, 257, ("canon",)), P("windows", 1, 12, ALL4), P("windows", 11, 24, ALL4, True, lead=3),
        P("windows2", 33, 47, ALL4), P("windows2", 40, 55, ("flags",), lead=12), P("windows2", 33, 70, ALL4, True),
        P("windows2", 40, 64, ("flags",), True), P("windows2", 33, 257, ("canon",)), P("windows2", 33, 44, ALL4, True, lead=9),
        # the 16-word frame, and reads above it behind offsets (cut into segments), per call
        P("windows", 25, 170, ("rc",)), P("windows", 11, 170, ("canon",), True), P("windows", 31, 300, ("canon",), True),
        P("windows2", 64, 161, ("canon",)), P("windows2", 33, 0, ("canon",), True, lmax=176), P("windows2", 40, 300, ("flags",), True)]
# a dirty batch past one sweep, then a clean one of the same shape on the same context
DIRTY_THEN_CLEAN = [P("windows", 25, 70, ("rc",)), P("windows", 11, 50, ALL4, lead=3), P("windows", 11, 64, ALL4, True),
                    P("windows2", 33, 47, ALL4), P("windows2", 33, 70, ALL4, True), P("windows", 8, 8, ("canon",), zero=True)]
REPEAT = [P("windows", 11, 47, ("canon",)), P("windows2", 47, 70, ("canon",), lead=3)]


def past(U: int) -> int:
    return U + U // 3 + 6


def next_prime(x: int) -> int:
    x = max(int(x), 2)
    while any(x % d == 0 for d in range(2, int(x ** 0.5) + 1)):
        x += 1
    return x


def _case_seed(case: P) -> int:
    return CASES.index(case) if case in CASES else 900 + (EDGE.index(case) if case in EDGE else 77)


@dataclasses.dataclass
class Built:
    case: P
    arm: Arm
    U: int                       # units of one launch
    units: int                   # whole units of this batch
    n: int                       # reads
    J: int                       # segments per read (uniform segment arms; else 1)
    period: int                  # P: reads of the block
    bases: np.ndarray            # the block's bytes
    lens: np.ndarray             # (P) its reads' lengths
    off: np.ndarray              # (P + 1) i64 their offsets in the block
    win: np.ndarray              # (P + 1) i64 their first slots in the block
    seg: np.ndarray              # (P + 1) i64 their first segments in the block (segment arms of ragged reads; else None)
    exp: dict                    # name -> the block's expected array (u64; two-word: 2 per slot, flat; flags u8), wanted outputs only
    dirty: np.ndarray            # (P) bool: the read holds an invalid byte

    @property
    def two(self) -> bool:
        return self.case.call == "windows2"

    def _at(self, table, r):
        """the periodic continuation of a block table (off, win, seg) at read r"""
        r = np.asarray(r).astype(_I)
        return (r // self.period) * int(table[-1]) + table[r % self.period]

    @property
    def total_bytes(self) -> int:
        return int(self._at(self.off, self.n))

    @property
    def total(self) -> int:
        return int(self._at(self.win, self.n))

    def per_slot(self, name: str) -> int:
        return 2 if self.two and name != "flags" else 1

    def unit_of_read(self, r):
        r = np.asarray(r).astype(_I)
        if self.arm.unit == "read":
            return r
        if self.arm.unit == "tile" or self.case.zero:
            return r // 64
        return (r * self.J if self.seg is None else self._at(self.seg, r)) // 64

    def first_read_of_unit(self, t: int) -> int:
        if self.arm.unit == "read":
            return t
        if self.arm.unit == "tile" or self.case.zero:
            return 64 * t
        if self.seg is None:
            return -(-64 * t // self.J)
        q, rem = divmod(64 * t, int(self.seg[-1]))
        return q * self.period + int(np.searchsorted(self.seg[:-1], rem, side="left"))

    def read_of_slot(self, s: int) -> int:
        q, rem = divmod(int(s), int(self.win[-1]))
        return q * self.period + int(np.searchsorted(self.win, rem, side="right")) - 1

    def where(self, s: int):
        """(read, unit, past one launch?) of a slot: what a failure reports"""
        r = self.read_of_slot(s)
        t = int(self.unit_of_read(r))
        return r, t, t >= self.U

    def slots(self, name: str, s0: int, s1: int) -> np.ndarray:
        """the expected elements of slots [s0, s1)"""
        m = self.per_slot(name)
        return self.exp[name][np.arange(m * s0, m * s1) % len(self.exp[name])]

    # ---- the whole batch on the host (the CPU tests; the device builds the same from the block)
    def host_bases(self) -> np.ndarray:
        return np.tile(self.bases, self.total_bytes // len(self.bases) + 1)[: self.total_bytes]

    def host_offsets(self) -> np.ndarray:
        return self._at(self.off, np.arange(self.n + 1)).astype(np.uint64)

    def host_win_offsets(self) -> np.ndarray:
        return self._at(self.win, np.arange(self.n + 1)).astype(np.uint64)

    def expected(self, name: str) -> np.ndarray:
        return self.slots(name, 0, self.total)

    def dirty_reads(self) -> np.ndarray:
        return self.dirty[np.arange(self.n) % self.period]

    def tile_dirty(self) -> np.ndarray:
        """per tile of 64 reads (the last one partial): does it hold an invalid byte?"""
        d = self.dirty[np.arange(-(-self.n // 64) * 64) % self.period]
        d[self.n:] = False
        return d.reshape(-1, 64).any(axis=1)

    def footprint(self) -> int:
        """device bytes of the call: bases, offsets and window offsets, the poisoned outputs with their guards, the block"""
        out = sum(self.total * (1 if nm == "flags" else 8 * self.per_slot(nm)) + 512 for nm in self.case.want)
        return self.total_bytes + 16 + (16 * (self.n + 1) if self.case.ragged else 0) + out + len(self.bases) + sum(a.nbytes for a in self.exp.values())


def _lengths(case: P, rng, Pn: int) -> np.ndarray:
    if not case.ragged:
        return np.full(Pn, case.L, _I)
    k, top = case.k, case.longest
    lens = rng.integers(max(k - 2, 0), k + 3, Pn) if case.short else rng.integers(0, top + 1, Pn)
    lens = lens.astype(_I)
    lens[1:4] = max(top if not case.short else k + 2, 3)      # (the reads that get their N below)
    lens[4], lens[5], lens[6] = 0, k - 1, top                  # an empty read, one shorter than k, one at the bound
    return lens


def build(case: P, n_cu: int, size=None, clean: bool = False, seed: int = 1, oracle=None) -> Built:
    """size: None -- past one launch; "U" -- U units exactly; a number -- so many reads.  clean: no invalid byte."""
    if oracle is None:
        from oracle import oracle
    arm, k = case.arm, case.k
    if isinstance(size, int):
        arm = arm_of(case.call, k, case.L, case.ragged, case.lead, case.want, case.flags_shift, case.words_shift, n=size)
    U = (512 if case.zero else arm.per_cu) * n_cu
    rng = np.random.default_rng([seed, _case_seed(case), n_cu, 0 if size is None else 1 if size == "U" else 2 + int(size)])
    seg_ragged = case.ragged and case.L > 256 and not case.lead and k >= 2       # cut into segments on the device
    J = segments_per_read(case.L, k) if arm.unit == "segtile" and not case.ragged else 1
    assert 64 % J == 0
    per_unit = 1 if arm.unit == "read" else 64 // J           # reads per unit (ragged segments: worked out below)
    if isinstance(size, int):
        n = size
    else:
        units, partial = (past(U), 37) if size is None else (U, 0)
        if seg_ragged:
            mean = float(seg_count(_lengths(case, np.random.default_rng(5), 1 << 14), k).mean())
            n = int((64 * units + partial) / mean * 1.03) + 1      # ("U": what sizes the block; the reads are counted below)
        else:
            n = units * per_unit + partial // J
            n += 1 if partial and n % 64 == 0 else 0          # (lane-per-read arms: the last block of 64 stays partial too)
    Pn = next_prime(max(-(-n // 64), 1008) + 1)
    if (n - 1) % Pn < 8 and not isinstance(size, int):
        n += 8                                                # (the last read of the batch is none of the block's fixed reads)
    lens = _lengths(case, rng, Pn)
    last = (n - 1) % Pn
    if last >= 8:
        lens[last] = max(lens[last], min(k + 1, case.longest))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(_I)
    win = np.concatenate([[0], np.cumsum(np.maximum(lens - k + 1, 0))]).astype(_I)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(off[-1]))].copy()
    low = rng.random(Pn) < 0.05                               # some reads in lower case
    for r in np.flatnonzero(low & (lens > 0)):
        bases[off[r]: off[r + 1]] |= 0x20
    dirty = np.zeros(Pn, bool)
    if not clean:
        hit = rng.choice(np.arange(8, Pn), int(DIRTY_READS * Pn), replace=False)
        hit = hit[lens[hit] > 0]
        bases[off[hit] + rng.integers(0, lens[hit])] = np.frombuffer(b"NNNNnx\n-", np.uint8)[rng.integers(0, 8, len(hit))]
        bases[off[1]: off[2]] = ord("N")                      # a read that is all N
        bases[off[2]] = ord("N")                              # N as a read's first byte
        bases[off[4] - 1] = ord("N")                          # ... and as read 3's last
        dirty[hit] = True
        dirty[1:4] = True
        if last >= 8 and lens[last] > 0:
            bases[off[last] + lens[last] // 2] = ord("N")     # N in the last read of the batch
            dirty[last] = True
    fn = oracle.canonical_windows2 if case.call == "windows2" else oracle.canonical_windows
    outs = fn(bases, Pn, case.L, k, offsets=off.astype(np.uint64) if case.ragged else None)
    exp = {nm: np.ascontiguousarray(a).reshape(-1) for nm, a in zip(NAMES, outs) if nm in case.want}
    seg = np.concatenate([[0], np.cumsum(seg_count(lens, k))]).astype(_I) if seg_ragged else None
    if seg_ragged and isinstance(size, int):                  # (windows2 tiles from 64 SEGMENTS on)
        arm = arm_of(case.call, k, case.L, True, case.lead, case.want, case.flags_shift, case.words_shift, n=size, n_seg=int(seg[size]))
        U = arm.per_cu * n_cu
    b = Built(case, arm, U, 0, n, J, Pn, bases, lens, off, win, seg, exp, dirty)
    if seg_ragged and size == "U":
        b.n = b.first_read_of_unit(U)                         # the first read whose segments all lie past U tiles of them
        assert b.n <= n
    n = b.n
    b.units = int(b.unit_of_read(n - 1)) + 1 if arm.unit == "read" else int(b.unit_of_read(n)) if not seg_ragged else int(b._at(seg, n)) // 64
    return b


# ------------------------------------------------------------------ what a kernel that mishandles its later units would leave

def late_ranges(b: Built, first: int = 48, last: int = 16):
    """read ranges past the first launch to look at: the first `first` and the last `last` units past U (lane-per-read arms: runs of
    64 reads), the partial one included -> [(r0, r1)]"""
    R0 = b.first_read_of_unit(b.U)
    if b.arm.unit == "read":
        edges = list(range(R0, b.n, 64)) + [b.n]
    else:
        edges = [b.first_read_of_unit(t) for t in range(b.U, b.units + 1)]
        edges += [b.n] if edges[-1] < b.n else []
    pairs = list(zip(edges[:-1], edges[1:]))
    return pairs if len(pairs) <= first + last else pairs[:first] + pairs[-last:]


def faulty(b: Built, name: str, r0: int, r1: int):
    """the elements three broken kernels leave in the slots of reads [r0, r1), all past the first launch:
    stops     -- the launch ends after its first U units: poison;
    previous  -- a unit is written with the words of the unit U before it (a shorter source leaves poison behind it);
    elsewhere -- a unit is stored at the slots of the unit U before it: its own slots keep the poison (no unit lies U behind it:
                 the batch has fewer than 2 U units) -- on these slots the same as `stops`; what this fault adds is the earlier
                 unit's slots, which hold the wrong words: the pair returned last
    -> (expected, stops, previous, elsewhere, (expected, found) at the earlier unit's slots)"""
    R0 = b.first_read_of_unit(b.U)
    assert r0 >= R0 and b.units < 2 * b.U
    m = b.per_slot(name)
    s0, s1 = int(b._at(b.win, r0)), int(b._at(b.win, r1))
    e0, e1 = int(b._at(b.win, r0 - R0)), int(b._at(b.win, r1 - R0))
    want, src = b.slots(name, s0, s1), b.slots(name, e0, e1)
    poison = np.asarray(POISON_U8 if name == "flags" else POISON_U64, want.dtype)
    stops = np.full_like(want, poison)
    previous = stops.copy()
    previous[: min(len(src), len(want))] = src[: len(want)]
    moved = src.copy()
    moved[: min(len(src), len(want))] = want[: len(src)]
    return want, stops, previous, stops.copy(), (src, moved)


def table() -> str:
    """the arm table, as profiles/windows_sweep_tests.txt records it"""
    rows = ["arm | cases that name it"]
    for a in ARMS:
        ids = [c.id for c in CASES if a in c.arm.names and (not a.startswith("zero<") or c.zero)]
        rows.append(f"{a} | {len(ids)}: " + "; ".join(ids[:3]) + (" ..." if len(ids) > 3 else ""))
    rows += [f"{a} | edge sizes only: {why}" for a, why in EDGE_ONLY.items()]
    return "\n".join(rows)
