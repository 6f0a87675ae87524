"""The minimizer calls -- kmx_minimizers, kmx_seqvec_minimizers, kmx_minimizer_words and their _sip13 forms -- on the host: a numpy
reference, the launchers' routing restated as a table of kernel ARMS, and the cases tests/test_gpu_minimizers_sweep.py runs.

* reference / words_reference: the leftmost minimum-hash l-mer of every k-mer, hashes compared as full u64 (tests/sip13_np.py's
  lmers / sliding_minimizers / siphash13 and tests/elem_np.py's lex_hash).  tests/test_minimizers_np.py pins them against the oracle's
  monotone deque and the reference's own vectors.
* arm_of: which kernel a parameter set runs (launch_minimizers_reads, launch_seqvec_minimizers, kmx_sip13.hip), its work unit and the
  units one capped grid takes per compute unit.  ARMS names every arm; CASES holds one parameter set or more for each.
* build(case, n_cu): inputs and expected outputs of a case with U + U // 3 + 1 + 5 units (U = the arm's sweep on n_cu compute units):
  some blocks take two loop iterations, some one, the last block is partial.  EDGE: unit counts 1, 15, 16, 17 and U with L == k.
  BAD: batches whose invalid bytes all lie past the first sweep.

A UNIT is what a block (or wave, or lane) takes per loop iteration: a read, a piece of a uniform read above 256 bases, a k-mer of the
direct SeqVector kernel, a word.  Unit R is worked on in loop iteration R // U."""
from __future__ import annotations

import dataclasses

import numpy as np

from tests import elem_np as E
from tests import sip13_np as S

OK, E_INVALID_BASE = E.OK, E.E_INVALID_BASE
POISON_U64, POISON_U32 = E.POISON_U64, 0xA5A5A5A5
NO_BAD = E.M64                       # *h_first_bad of a clean batch
SIP_KEY = (0x0706050403020100, 0x0F0E0D0C0B0A0908)
_I = np.int64


# ------------------------------------------------------------------ hashers and the reference

@dataclasses.dataclass(frozen=True)
class Identity:
    pass


@dataclasses.dataclass(frozen=True)
class Lex:
    hk: int


@dataclasses.dataclass(frozen=True)
class Sip:
    k0: int = 0
    k1: int = 0


def hash_of(lm: np.ndarray, hasher) -> np.ndarray:
    if isinstance(hasher, Identity):
        return lm
    if isinstance(hasher, Lex):
        return E.lex_hash(lm, hasher.hk)
    flat = np.ascontiguousarray(lm).reshape(-1)       # (in blocks that stay in the cache: millions of l-mers)
    out = np.empty_like(flat)
    for lo in range(0, len(flat), 1 << 15):
        out[lo: lo + (1 << 15)] = S.siphash13(flat[lo: lo + (1 << 15)], hasher.k0, hasher.k1)
    return out.reshape(lm.shape)


def _windows(codes: np.ndarray, k: int, w: int, hasher):
    """(n, L) codes -> (words, pos) of shape (n, L - k + 1)"""
    lm = S.lmers(codes, w)
    return S.sliding_minimizers(lm, hash_of(lm, hasher), k, w)


def window_counts(offsets, k: int):
    """ragged reads -> (k-mers per read, win_offsets): a read shorter than k owns no slot"""
    nk = np.maximum(np.diff(np.asarray(offsets).astype(_I)) - k + 1, 0)
    return nk, np.concatenate([[0], np.cumsum(nk)]).astype(np.uint64)


def reference(host_bytes, offsets_or_L, k: int, w: int, hasher):
    """SeqVecMinimizerIter over every read -> (words u64, pos u32) in slot order; positions count from the read's first base.
    offsets_or_L: the n + 1 offsets of ragged reads, or the one length of uniform reads."""
    codes = S.codes_of(host_bytes)
    if np.ndim(offsets_or_L) == 0:
        L = int(offsets_or_L)
        n = len(codes) // L
        wd, pos = _windows(codes[: n * L].reshape(n, L), k, w, hasher)
        return np.ascontiguousarray(wd.reshape(-1)), np.ascontiguousarray(pos.reshape(-1)).astype(np.uint32)
    off = np.asarray(offsets_or_L).astype(_I)
    nk, win = window_counts(off, k)
    total = int(win[-1])
    if total == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    # the batch as ONE sequence: a window that lies inside a read sees that read's l-mers only
    wd, pos = _windows(codes[None, : int(off[-1])], k, w, hasher)
    read = np.repeat(np.arange(len(nk)), nk)
    at = off[:-1][read] + np.arange(total) - win[:-1].astype(_I)[read]
    return wd[0, at], (pos[0, at] - off[:-1][read]).astype(np.uint32)


def words_reference(words, k: int, w: int, hasher):
    """Kmer::minimizer_word of every k-mer word -> (l-mer u64, offset u32): the leftmost of equal hashes.  (w = 32 keeps the whole
    word, as the calls do -- tests/test_gpu_sip13.py -- where the reference's MASK_TABLE[32] == 0 yields 0; no case has w = 32 here.)"""
    words = E.u64(words)
    mm, off = np.zeros(len(words), np.uint64), np.zeros(len(words), np.uint32)
    sh = (2 * np.arange(k - w + 1)).astype(np.uint64)
    for lo in range(0, len(words), 1 << 18):
        sub = (words[lo: lo + (1 << 18), None] >> sh) & np.uint64(E.mask2k(w))
        arg = np.argmin(hash_of(sub, hasher), axis=1)
        mm[lo: lo + len(sub)] = np.take_along_axis(sub, arg[:, None], axis=1)[:, 0]
        off[lo: lo + len(sub)] = arg
    return mm, off


# ------------------------------------------------------------------ the arms

@dataclasses.dataclass(frozen=True)
class Arm:
    name: str
    unit: str        # "read", "piece", "k-mer", "word"
    per_cu: int      # units of one capped grid per compute unit

    def sweep(self, n_cu: int) -> int:
        return self.per_cu * n_cu


def pieces(L: int, k: int):
    """a uniform read of L > 256 bases -> (J pieces, T k-mers per piece)"""
    T = 257 - k
    return (L - k + 1 + T - 1) // T, T


def tiled_lds(Lmax: int, w: int) -> int:
    """bytes of dynamic LDS launch_minimizers_reads asks for (RB = 16); above 64 KiB it raises the kernel's limit first"""
    NLS, ND, RB = Lmax - w + 1, ((2 * Lmax + 31) >> 5) + 2, 16
    return 2 * RB * NLS * 8 + (2 * RB * ND + ((RB * ND) & 1)) * 4 + RB * 8 + (3 * RB + 1) * 4 + 16


def slide_lds(L: int, w: int) -> int:
    """the same for launch_seqvec_minimizers' slide kernel"""
    return 2 * 16 * (L - w + 1) * 8 + 2 * 16 * (((2 * L + 31) >> 5) + 2) * 4


def arm_of(call: str, k: int, w: int, hasher: str, hk: int, ragged: bool, L: int) -> Arm:
    """call: "minimizers", "seqvec_minimizers" or "minimizer_words"; hasher: "identity", "lex" or "sip" (the _sip13 form of the call);
    L: the one read length, or the longest read of a ragged batch"""
    if call == "minimizer_words":
        return Arm("minimizer_words_sip" if hasher == "sip" else f"minimizer_words<{hasher}>", "word", 4096)
    if hasher == "sip":
        form = "packed" if call == "seqvec_minimizers" else "ascii"
        if k > 256:
            return Arm(f"sip_generic<{form}>", "read", 64)
        return Arm(f"sip_piece<{form if form == 'packed' else form + (',ragged' if ragged else ',uniform')}>", "read", 64)
    bits = 2 * hk if hasher == "lex" else 2 * w
    keys_fit = bits <= 56 and w <= 28 and k > w
    mode = 0 if hasher == "identity" else 1 if hk == w else 2
    key = "k32" if bits + 8 <= 32 and 2 * w + 8 <= 32 else "k64"
    if call == "seqvec_minimizers":
        if keys_fit and L <= 256:
            return Arm(f"seqvec_slide<M{mode},{key}>", "read", 128)
        NL = L - w + 1
        if NL * 8 <= 48 * 1024:
            return Arm("seqvec_lds", "read", min(16, 48 * 1024 // (NL * 8)) * 8)
        return Arm("seqvec_direct", "k-mer", 4096)
    assert call == "minimizers", call
    if keys_fit and not ragged and L > 256 and k <= 256:
        return Arm(f"reads_tiled_cut<M{mode}>", "piece", 128)
    if keys_fit and k <= L <= 256:
        return Arm(f"reads_tiled<M{mode},{'ragged' if ragged else 'uniform'},{key}>", "piece", 128)
    why = "w>28" if w > 28 else "k==w" if k == w else "hash>56" if bits > 56 else "ragged>256" if ragged and L > 256 else "k>256"
    return Arm(f"reads_generic[{why}]", "read", 64)


ARMS = (
    [f"reads_tiled<M{m},{lay},{key}>" for m in range(3) for lay in ("uniform", "ragged") for key in ("k32", "k64")]
    + [f"reads_tiled_cut<M{m}>" for m in range(3)]
    + [f"reads_generic[{why}]" for why in ("w>28", "k==w", "hash>56", "ragged>256", "k>256")]
    + [f"seqvec_slide<M{m},{key}>" for m in range(3) for key in ("k32", "k64")]
    + ["seqvec_lds", "seqvec_direct", "minimizer_words<identity>", "minimizer_words<lex>", "minimizer_words_sip",
       "sip_piece<ascii,uniform>", "sip_piece<ascii,ragged>", "sip_piece<packed>", "sip_generic<ascii>", "sip_generic<packed>"]
)


# ------------------------------------------------------------------ the cases

@dataclasses.dataclass(frozen=True)
class P:
    call: str
    k: int
    w: int
    hasher: str = "identity"
    hk: int = 0
    ragged: bool = False
    L: int = 0              # the one read length / the longest read (minimizer_words: unused)
    shift: int = 0          # bytes of the input's first byte past a 16-byte boundary

    @property
    def arm(self) -> Arm:
        return arm_of(self.call, self.k, self.w, self.hasher, self.hk, self.ragged, self.L)

    @property
    def hasher_obj(self):
        return Identity() if self.hasher == "identity" else Lex(self.hk) if self.hasher == "lex" else Sip(*SIP_KEY)

    @property
    def id(self) -> str:
        h = {"identity": "id", "lex": f"lex{self.hk}", "sip": "sip"}[self.hasher]
        lay = "" if self.call == "minimizer_words" else f"-{'ragged' if self.ragged else 'L'}{self.L}"
        return f"{self.arm.name}-k{self.k}w{self.w}-{h}{lay}+{self.shift}"


def _cases():
    R, Sv, W = "minimizers", "seqvec_minimizers", "minimizer_words"
    c = []
    # the twelve instantiations of minimizers_reads_kernel: reads of 33..64 bases, k of 21 or 31
    for ragged in (False, True):
        Ls = iter((47, 61, 33, 64, 53, 39, 59)) if not ragged else iter((64,) * 7)
        c += [P(R, 21, 11, "identity", 0, ragged, next(Ls)), P(R, 31, 15, "identity", 0, ragged, next(Ls)),
              P(R, 21, 12, "lex", 12, ragged, next(Ls)), P(R, 31, 15, "lex", 15, ragged, next(Ls)),
              P(R, 21, 11, "lex", 6, ragged, next(Ls)), P(R, 31, 15, "lex", 6, ragged, next(Ls)),      # (hk = 6 fits a dword, w = 15 does not)
              P(R, 31, 15, "lex", 20, ragged, next(Ls))]
    # NLS at its largest (more than 64 KiB of LDS: the attribute path; tiled_lds, slide_lds) with few k-mers per read
    c += [P(R, 250, 11, "lex", 11, False, 256)]
    # uniform reads above 256 bases, cut into J = 8 pieces
    c += [P(R, 250, 15, "identity", 0, False, 300), P(R, 250, 12, "lex", 12, False, 300), P(R, 250, 15, "lex", 6, False, 300)]
    # the lane-per-k-mer kernel, every way into it
    c += [P(R, 31, 29, "identity", 0, False, 50), P(R, 21, 21, "lex", 21, True, 64), P(R, 31, 15, "lex", 29, False, 45),
          P(R, 31, 15, "lex", 15, True, 300), P(R, 257, 15, "lex", 15, False, 258)]
    # the six instantiations of seqvec_minimizers_slide_kernel, the LDS and the direct kernel
    c += [P(Sv, 21, 11, "identity", 0, False, 47), P(Sv, 31, 15, "identity", 0, False, 61), P(Sv, 21, 12, "lex", 12, False, 33),
          P(Sv, 31, 15, "lex", 15, False, 64), P(Sv, 21, 11, "lex", 6, False, 53), P(Sv, 31, 15, "lex", 20, False, 39),
          P(Sv, 248, 9, "identity", 0, False, 256), P(Sv, 21, 21, "lex", 21, False, 50), P(Sv, 16, 16, "identity", 0, False, 6160)]
    c += [P(W, 31, 15, "identity"), P(W, 32, 20, "lex", 20), P(W, 24, 17, "sip")]
    # SipHash: pieces of 256 bases (reads of 270: two pieces) and the kernel for k above a piece
    c += [P(R, 21, 15, "sip", 0, False, 270), P(R, 21, 11, "sip", 0, True, 64), P(R, 31, 15, "sip", 0, True, 300),
          P(Sv, 31, 20, "sip", 0, False, 61), P(R, 257, 31, "sip", 0, False, 258), P(Sv, 257, 32, "sip", 0, False, 258)]
    # the alignment, spread over the list: ASCII 0..3 bytes past a 16-byte boundary, u64 inputs 0 or 8
    return [dataclasses.replace(p, shift=(i % 4) if p.call == R else 8 * (i % 2)) for i, p in enumerate(c)]


CASES = _cases()
SIZES = (1, 15, 16, 17, "U")
# (parameter set, unit counts): L == k, one k-mer per read; and the single 12-base read that is the whole batch
EDGE = [(P("minimizers", 21, 11, "identity", 0, False, 21, 1), SIZES), (P("minimizers", 31, 15, "lex", 15, True, 31, 2), SIZES),
        (P("minimizers", 31, 15, "lex", 6, False, 31, 3), SIZES), (P("minimizers", 31, 29, "identity", 0, False, 31, 0), SIZES),
        (P("minimizers", 12, 5, "lex", 5, False, 12, 1), (1,)), (P("minimizers", 12, 5, "identity", 0, False, 12, 3), (1,)),
        (P("minimizers", 12, 5, "lex", 5, True, 12, 2), (1,)),
        (P("seqvec_minimizers", 21, 11, "identity", 0, False, 21, 0), SIZES), (P("seqvec_minimizers", 31, 15, "lex", 15, False, 31, 8), SIZES),
        (P("seqvec_minimizers", 21, 21, "lex", 21, False, 21, 0), SIZES),
        (P("minimizer_words", 31, 15, "identity", 0, False, 0, 8), SIZES), (P("minimizer_words", 31, 15, "lex", 15, False, 0, 0), SIZES),
        (P("minimizer_words", 24, 17, "sip", 0, False, 0, 8), SIZES),
        (P("minimizers", 31, 15, "sip", 0, False, 31, 1), SIZES), (P("minimizers", 31, 15, "sip", 0, True, 31, 3), SIZES),
        (P("minimizers", 12, 5, "sip", 0, False, 12, 1), (1,)), (P("seqvec_minimizers", 31, 15, "sip", 0, False, 31, 8), SIZES)]
# invalid bytes past the first sweep: uniform and ragged per reads call, and the cut of long uniform reads
BAD = [P("minimizers", 31, 15, "lex", 15, False, 61, 1), P("minimizers", 21, 11, "identity", 0, True, 64, 2),
       P("minimizers", 250, 15, "lex", 15, False, 300, 3), P("minimizers", 31, 15, "sip", 0, False, 61, 2),
       P("minimizers", 31, 15, "sip", 0, True, 64, 1)]


def past(U: int) -> int:
    return U + U // 3 + 1 + 5


@dataclasses.dataclass
class Built:
    case: P
    arm: Arm
    U: int                       # units of one sweep
    units: int                   # units of this batch (>= what was asked: whole reads)
    n: int                       # reads (words) the call receives
    J: int                       # units per read (pieces; the direct kernel: k-mers)
    first_past: int              # the first read whose units all lie past the first sweep
    inputs: dict                 # "bases" u8 / "words" u64, and "offsets", "win_offsets" u64 of ragged reads
    lens: np.ndarray | None      # ragged: the reads' lengths
    counts: np.ndarray           # slots per read (word)
    word: np.ndarray | None      # expected (None after an error: the outputs are unspecified)
    pos: np.ndarray | None
    status: int = OK
    first_bad: int = NO_BAD
    bad_at: tuple = ()           # (read, byte of the batch) of every invalid byte

    @property
    def total(self) -> int:
        return int(self.counts.sum())

    def slot_units(self) -> np.ndarray:
        """the unit that writes each slot"""
        if self.arm.unit == "k-mer":
            return np.arange(self.total)
        read = np.repeat(np.arange(self.n), self.counts)
        if self.J == 1:
            return read
        T = pieces(self.case.L, self.case.k)[1]
        return read * self.J + np.tile(np.arange(int(self.counts[0])) // T, self.n)

    def where(self, slot: int):
        """(read, unit, sweep) of a slot: what a failure reports"""
        read = int(np.searchsorted(np.cumsum(self.counts), slot, side="right"))
        unit = int(self.slot_units()[slot])
        return read, unit, unit // self.U


def _two_letters(rng, n: int, pair: bytes) -> np.ndarray:
    return np.frombuffer(pair, np.uint8)[rng.integers(0, 2, n)]


def build(case: P, n_cu: int, units=None, bad: bool = False, seed: int = 1) -> Built:
    """units: the unit count asked for (default: past one sweep; "U": one sweep exactly).  bad: plant three invalid bytes past the
    first sweep."""
    arm = case.arm
    U = arm.sweep(n_cu)
    asked = past(U) if units is None else U if units == "U" else int(units)
    k, w, L = case.k, case.w, case.L
    rng = np.random.default_rng([seed, CASES.index(case) if case in CASES else 977, n_cu, asked])
    if case.call == "minimizer_words":
        n = asked
        words = rng.integers(0, 2**64, n, dtype=np.uint64)
        for r0 in (0, U):       # two-letter words where a sweep begins: ties everywhere
            words[r0: r0 + 16] &= np.uint64(0x5555555555555555)
        words &= np.uint64(E.mask2k(k))
        mm, off = words_reference(words, k, w, case.hasher_obj)
        return Built(case, arm, U, n, n, 1, min(U, n), {"words": words}, None, np.ones(n, _I), mm, off)
    J = 1
    if arm.unit == "k-mer":
        J = L - k + 1
    elif arm.name.startswith("reads_tiled_cut"):
        J = pieces(L, k)[0]
    n = -(-asked // J)
    first_past = -(-U // J)
    marked = [r for r in (first_past + 3, first_past + 5, n - 1) if bad]
    assert not bad or first_past + 5 < n - 1
    lens = None
    if case.ragged:
        lens = rng.integers(0, L + 1, n).astype(_I)
        if units is None:
            # mirrored across the sweep: every LDS row meets a shorter successor and a longer one
            short = np.array([0, k - 1, k, w], _I)[np.arange(64) % 4]
            a, b = 20 + np.arange(64), 84 + np.arange(64)
            assert b[-1] + U < n
            lens[a], lens[a + U] = L, short
            lens[b], lens[b + U] = short, L
        else:
            lens[:] = L
        lens[marked] = L
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        counts, win = window_counts(off, k)
        start = off[:-1].astype(_I)
    else:
        counts = np.full(n, L - k + 1, _I)
        start = np.arange(n, dtype=_I) * L
    total_bytes = int(lens.sum()) if case.ragged else n * L
    host = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, total_bytes)].copy()
    length = lambda r: int(lens[r]) if case.ragged else L
    for r0, pair in ((0, b"AC"), (first_past, b"GT")):      # the first 16 reads of each sweep: two letters
        for r in range(r0, min(r0 + 16, n)):
            host[start[r]: start[r] + length(r)] = _two_letters(rng, length(r), pair)
        for r in range(r0 + 16, min(r0 + 20, n)):           # ... and four in lower case
            host[start[r]: start[r] + length(r)] |= 0x20
    bad_at = ()
    if bad:
        T = pieces(L, k)[1] if J > 1 else L // 2
        where = (L - 1, T + 3, 0)       # the read's last base; a base two pieces share (whole reads: any); its first
        bad_at = tuple((r, int(start[r]) + p) for r, p in zip(marked, where))
        for (_, at), byte in zip(bad_at, b"Nx\n"):
            host[at] = byte
    inputs = {"bases": host}
    if case.ragged:
        inputs.update(offsets=off, win_offsets=win)
    if case.call == "seqvec_minimizers":
        inputs = {"words": E.seqvec_pack(host)[0]}
    b = Built(case, arm, U, n * J, n, J, first_past, inputs, lens, counts, None, None, bad_at=bad_at)
    if bad:
        b.status, b.first_bad = E_INVALID_BASE, marked[0]
    else:
        b.word, b.pos = reference(host, off if case.ragged else L, k, w, case.hasher_obj)
        assert len(b.word) == b.total
    return b


# ------------------------------------------------------------------ what a kernel that mishandles its second iteration would write

def model_one_sweep(b: Built):
    """a kernel that stops after one sweep: the slots of the units >= U keep their poison"""
    late = b.slot_units() >= b.U
    return np.where(late, np.uint64(POISON_U64), b.word), np.where(late, np.uint32(POISON_U32), b.pos)


def model_previous_sweep(b: Built):
    """a kernel that works on the unit of the previous sweep again: unit R >= U writes, into its own slots, what unit R - U owns
    (and leaves the slots unit R - U has no answer for)"""
    unit = b.slot_units()
    n_units = int(unit[-1]) + 1
    count = np.bincount(unit, minlength=n_units)
    first = np.concatenate([[0], np.cumsum(count)])[:-1]
    i = np.arange(len(unit)) - first[unit]
    src = np.maximum(unit - b.U, 0)
    late, has = unit >= b.U, i < count[src]
    at = np.where(late & has, first[src] + i, 0)
    word = np.where(late, np.where(has, b.word[at], np.uint64(POISON_U64)), b.word)
    pos = np.where(late, np.where(has, b.pos[at], np.uint32(POISON_U32)), b.pos)
    return word, pos
