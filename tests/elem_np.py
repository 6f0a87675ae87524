"""Vectorised numpy references of the one-element-per-lane calls (kmx_elem.hip, the first half of kmx_seqvec.hip), and the input
builders of tests/test_gpu_elem_sweep.py.

Every reference works on whole arrays in u64 arithmetic and is pinned in tests/test_elem_np.py against what the suite already trusts:
the C oracle and the reference KATs.  SipHash-1-3 is tests/sip13_np.py's.

The builders are pure functions of (operation, parameters, size class, seed, S): S is the number of threads of one capped grid,
16 * n_cu * 256, which the GPU file reads from the device and the CPU file sets to a 256-CU device's.  A Case carries the inputs, the
expected outputs and, per output, `sweep2`: the index of the first element that a thread writes in its SECOND loop iteration.  The
CPU file checks on these very cases that a kernel which stopped after one sweep, or skipped the odd tail, could not pass."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from tests import sip13_np

M64 = (1 << 64) - 1
POISON_U64 = 0xA5A5A5A5A5A5A5A5      # the int64 -0x5A5A5A5A5A5A5A5B of test_gpu_count_fuzz.py
POISON_U8 = 0xA5
GUARD_WORDS, GUARD_BYTES = 16, 128
EDGE = (0, 1, 2, 3, 255, 256, 257)
S_256CU = 16 * 256 * 256             # one capped grid of a 256-CU device
OK, E_ARG, E_INVALID_BASE = 0, 1, 4
HASH_LEX, HASH_IDENTITY = 1, 2
ENCS = {"ACGT": 30, "ACTG": 27, "GTCA": 228}   # Naive discriminants (tests/golden/reference_kats.json): the default, Xor10's, one more

_U = np.uint64
_UNPACK4 = ((np.arange(256)[:, None] >> (2 * np.arange(4))) & 3).astype(np.uint8)      # byte -> its four 2-bit codes, lowest first
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_acgt = np.frombuffer(b"acgt", np.uint8)


def u64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64)


def same(got, want) -> bool:
    """the comparison of every test: same shape, same type, every element equal"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and bool((got == want).all())


# ------------------------------------------------------------------ word operations (naive_impl)

def _revgroups(w: np.ndarray) -> np.ndarray:
    """the 32 two-bit groups of each word in reverse order"""
    w = u64(w)
    w = ((w >> _U(2)) & _U(0x3333333333333333)) | ((w & _U(0x3333333333333333)) << _U(2))
    w = ((w >> _U(4)) & _U(0x0F0F0F0F0F0F0F0F)) | ((w & _U(0x0F0F0F0F0F0F0F0F)) << _U(4))
    return w.byteswap()


def mask2k(k: int) -> int:
    return M64 if k >= 32 else (1 << (2 * k)) - 1


def revcomp_word(w, k: int) -> np.ndarray:
    return _revgroups(~u64(w)) >> _U(2 * (32 - k))


def canonical(w, k: int):
    w = u64(w)
    rc = revcomp_word(w, k)
    return np.minimum(w, rc), (w <= rc).astype(np.uint8)


def lex_hash(w, hk: int) -> np.ndarray:
    return _revgroups(w) >> _U(2 * (32 - hk))


def match(fw, rc, other) -> np.ndarray:
    fw, rc, other = u64(fw), u64(rc), u64(other)
    return np.where(fw == other, 1, np.where(rc == other, 2, 0)).astype(np.uint8)


def ck_shift(fw, rc, bases, k: int, append: bool):
    """CanonicalKmer::append_base / prepend_base on (fw, rc) states; bases are 2-bit codes -> (fw, rc, dropped)"""
    fw, rc = u64(fw), u64(rc)
    b = (np.asarray(bases, np.uint8) & 3).astype(np.uint64)
    cb = _U(3) - b
    mask, top = _U(mask2k(k)), _U(2 * k - 2)
    if append:
        d = fw & _U(3)
        f = (fw >> _U(2)) | (b << top)
        r = mask & ((rc << _U(2)) | cb)
    else:
        d = (fw >> top) & _U(3)
        f = mask & ((fw << _U(2)) | b)
        r = (rc >> _U(2)) | (cb << top)
    return f, r, d.astype(np.uint8)


def sub_kmer(w, pos: int, width: int) -> np.ndarray:
    mask = 0 if width >= 32 else (1 << (2 * width)) - 1      # MASK_TABLE[32] == 0
    return (u64(w) >> _U(2 * pos)) & _U(mask)


def base_codes(ascii_bytes):
    """encode_binary_u8: -> (codes A0 C1 G2 T3 with 0 for an invalid byte, valid)"""
    c = np.asarray(ascii_bytes, np.uint8)
    i = (c >> 1) & 3
    expect = np.frombuffer(b"ACTG", np.uint8)[i]
    valid = (c & 0xDF) == expect
    return np.where(valid, i ^ (i >> 1), 0).astype(np.uint8), valid


def _first_bad(valid) -> int:
    bad = np.flatnonzero(~valid.ravel())
    return int(bad[0]) if len(bad) else M64


def _pack4(codes: np.ndarray) -> np.ndarray:
    """(..., 4m) 2-bit codes -> (..., m) bytes, code 0 lowest"""
    c = codes.reshape(codes.shape[:-1] + (codes.shape[-1] // 4, 4)).astype(np.uint8)
    return c[..., 0] | (c[..., 1] << 2) | (c[..., 2] << 4) | (c[..., 3] << 6)


def _pack_words(codes: np.ndarray) -> np.ndarray:
    """(n, m) codes, m <= 32 -> n u64 words, base 0 lowest"""
    n, m = codes.shape
    full = np.zeros((n, 32), np.uint8)
    full[:, :m] = codes
    return np.ascontiguousarray(_pack4(full)).view("<u8").reshape(n).astype(np.uint64)


def kmers_from_bytes(seqs, n: int, k: int):
    codes, valid = base_codes(np.asarray(seqs, np.uint8)[: n * k].reshape(n, k))
    return _pack_words(codes), _first_bad(valid)


def to_letters(words, k: int, upper: bool) -> np.ndarray:
    """String::from(Kmer) (lower case) / bitmer_to_bytes (upper case): n * k letters, base 0 first"""
    w = np.ascontiguousarray(u64(words)).astype("<u8")
    codes = _UNPACK4[w.view(np.uint8)].reshape(len(w), 32)[:, :k]
    return (_ACGT if upper else _acgt)[codes].reshape(-1)


# ------------------------------------------------------------------ encoding::Naive, any of the 24 discriminants

def nuc2bits(enc: int, nuc) -> np.ndarray:
    nuc = np.asarray(nuc, np.uint8).astype(np.uint32)
    return ((np.uint32(enc) >> (np.uint32(6) - np.uint32(2) * ((nuc >> 1) & 3))) & 3).astype(np.uint8)


def _tables(enc: int):
    """-> (letter of each code, code of the complement of each code)"""
    letters, comp = np.zeros(4, np.uint8), np.zeros(4, np.uint8)
    for x, y in zip(b"ACGT", b"TGCA"):
        c = int(nuc2bits(enc, x))
        letters[c] = x
        comp[c] = int(nuc2bits(enc, y))
    return letters, comp


def encode_bytes(seqs, n: int, seq_len: int, enc: int, nb: int) -> np.ndarray:
    """Encoding::encode on the byte image of [P; B]: -> (n, nb) bytes, unused high bits zero"""
    codes = np.zeros((n, 4 * nb), np.uint8)
    codes[:, :seq_len] = nuc2bits(enc, np.asarray(seqs, np.uint8)[: n * seq_len].reshape(n, seq_len))
    return _pack4(codes)


def rev_comp_bytes(arrays, K: int, enc: int) -> np.ndarray:
    """Encoding::rev_comp::<K>: base i = complement(base K-1-i) for i < K, bits >= 2K unchanged"""
    arrays = np.asarray(arrays, np.uint8)
    n, nb = arrays.shape
    codes = _UNPACK4[arrays].reshape(n, 4 * nb)
    out = codes.copy()
    out[:, :K] = _tables(enc)[1][codes[:, :K][:, ::-1]]
    return _pack4(out)


def decode_bytes(arrays, enc: int) -> np.ndarray:
    """Encoding::decode: ALL 4 * nb letters of each row"""
    arrays = np.asarray(arrays, np.uint8)
    return _tables(enc)[0][_UNPACK4[arrays]].reshape(arrays.shape[0], 4 * arrays.shape[1])


def _as_words(b: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(b).view("<u8").astype(np.uint64)


def _as_bytes(words, B: int) -> np.ndarray:
    return np.ascontiguousarray(u64(words).reshape(-1, B)).astype("<u8").view(np.uint8)


def encode(seqs, n: int, seq_len: int, enc: int, B: int) -> np.ndarray:
    """-> (n, B) u64 words"""
    return _as_words(encode_bytes(seqs, n, seq_len, enc, 8 * B))


def encode_windows(bases, n_reads: int, L: int, k: int, enc: int, B: int) -> np.ndarray:
    """every length-k window of every L-base read -> (n_reads * (L - k + 1), B) u64 words"""
    win = np.lib.stride_tricks.sliding_window_view(np.asarray(bases, np.uint8)[: n_reads * L].reshape(n_reads, L), k, axis=1)
    return encode(np.ascontiguousarray(win).reshape(-1), n_reads * (L - k + 1), k, enc, B)


def rev_comp(words, K: int, enc: int, B: int) -> np.ndarray:
    return _as_words(rev_comp_bytes(_as_bytes(words, B), K, enc))


def decode(words, enc: int, B: int) -> np.ndarray:
    """-> (n, 32 * B) letters"""
    return decode_bytes(_as_bytes(words, B), enc)


# ------------------------------------------------------------------ SeqVector

def _unpack_codes(words, n: int) -> np.ndarray:
    return _UNPACK4[np.ascontiguousarray(u64(words)).astype("<u8").view(np.uint8)].reshape(-1)[:n]


def _pack_vector(codes: np.ndarray) -> np.ndarray:
    full = np.zeros((len(codes) + 31) // 32 * 32, np.uint8)
    full[: len(codes)] = codes
    return np.ascontiguousarray(_pack4(full)).view("<u8").astype(np.uint64)


def seqvec_pack(ascii_bytes):
    """SeqVector::from(&[u8]) -> (ceil(n / 32) words, first_bad)"""
    codes, valid = base_codes(ascii_bytes)
    return _pack_vector(codes), _first_bad(valid)


def seqvec_push(words, n_before: int, ascii_bytes):
    """SeqVector::push_chars onto a vector of n_before bases held in `words` -> (the ceil((n_before + n) / 32) words, first_bad).
    What `words` holds past base n_before is dropped, as the call does."""
    codes, valid = base_codes(ascii_bytes)
    return _pack_vector(np.concatenate([_unpack_codes(words, n_before), codes])), _first_bad(valid)


def seqvec_unpack(words, n: int) -> np.ndarray:
    return _ACGT[_unpack_codes(words, n)]


def seqvec_field(words, n_bases: int, pos, k: int) -> np.ndarray:
    """SeqVector::get_kmer_u64(pos, k) for an array of positions inside the vector"""
    words, pos = u64(words), u64(pos)
    nw = (n_bases + 31) // 32
    wi = (pos >> _U(5)).astype(np.int64)
    sh = _U(2) * (pos & _U(31))
    lo = words[wi]
    hi = np.where((sh != 0) & (wi + 1 < nw), words[np.minimum(wi + 1, nw - 1)], _U(0))
    v = (lo >> sh) | np.where(sh != 0, hi << ((_U(64) - sh) & _U(63)), _U(0))
    return v & _U(mask2k(k))


# ------------------------------------------------------------------ generator, lengths

def splitmix64(x) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = u64(x) + _U(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U(27))) * _U(0x94D049BB133111EB)
        return x ^ (x >> _U(31))


def gen_reads(seed: int, first_byte: int, n: int) -> np.ndarray:
    """byte g of the stream = "ACGT"[(splitmix64(seed + g / 32) >> 2 * (g % 32)) & 3]"""
    if n == 0:
        return np.zeros(0, np.uint8)
    b0, b1 = first_byte >> 5, (first_byte + n - 1) >> 5
    with np.errstate(over="ignore"):
        z = splitmix64(_U(seed & M64) + np.arange(b0, b1 + 1, dtype=np.uint64))
    codes = _UNPACK4[z.astype("<u8").view(np.uint8)].reshape(-1)
    at = first_byte - 32 * b0
    return _ACGT[codes[at: at + n]]


def length_range(offsets):
    d = np.diff(np.asarray(offsets, np.uint64).astype(np.int64))
    return int(d.min()), int(d.max())


# ------------------------------------------------------------------ inputs

def past(S: int) -> int:
    """work items of the `past` size class: some threads take two iterations, some one, and the last block is partial"""
    return S + S // 3 + 1


@functools.lru_cache(maxsize=4)
def _rand_words(n: int, seed: int) -> np.ndarray:
    a = np.random.default_rng(seed).integers(0, 2**64, n, dtype=np.uint64)
    a.setflags(write=False)
    return a


def rand_words(n: int, seed: int, k: int = 32) -> np.ndarray:
    return _rand_words(n, seed) & _U(mask2k(k))


@functools.lru_cache(maxsize=4)
def rand_ascii(n: int, seed: int) -> np.ndarray:
    """random ACGTacgt letters"""
    a = np.frombuffer(b"ACGTacgt", np.uint8)[np.random.default_rng(seed).integers(0, 8, n)]
    a.setflags(write=False)
    return a


def palindrome(h, k: int) -> np.ndarray:
    """the even-k word whose low half is h and that equals its own reverse complement"""
    h = u64(h) & _U(mask2k(k // 2))
    return h | (revcomp_word(h, k // 2) << _U(k))


@dataclasses.dataclass
class Case:
    op: str
    params: dict
    n: int                                   # the n the call receives
    inputs: dict                             # name -> array (device inputs, never written)
    outputs: dict                            # name -> expected array
    sweep2: dict                             # name -> first index of `outputs[name]` written in a second loop iteration
    init: dict = dataclasses.field(default_factory=dict)     # name -> what an in-place output holds before the call
    status: int = OK
    first_bad: int | None = None             # what *h_first_bad receives (calls that have one)
    alias: tuple | None = None               # (input, output) the call may be given as ONE array
    vec: str | None = None                   # the input that map_words reads in 16-byte pairs
    items: int = 0                           # work items of the launch


def _n_of(S, size, per_item=1, odd=False):
    """(n, work items) of a size class: `past` counts work items of per_item elements each, an edge size is n itself"""
    if size != "past":
        return int(size), 0
    it = past(S)
    n = it * per_item
    return (n + 1 if odd and per_item == 2 else n), it


# op -> list of parameter sets: what tests/test_gpu_elem_sweep.py runs at `past` and at every edge size
OPS = {
    "kmers_from_bytes": [dict(k=k) for k in (1, 31, 32)],
    "revcomp_words": [dict(k=k) for k in (1, 16, 31, 32)],
    "canonical_words": [dict(k=k, form=f) for k in (16, 31) for f in ("both", "words", "flags")],
    "hash_words": [dict(hasher=HASH_LEX, hk=hk) for hk in (1, 20, 32)] + [dict(hasher=HASH_IDENTITY, hk=0)],
    "hash_words_sip13": [dict(k0=0, k1=0), dict(k0=0x0706050403020100, k1=0x0F0E0D0C0B0A0908)],
    "match_words": [dict()],
    "ck_shift": [dict(append=a, k=k, dropped=d) for a in (True, False) for k in (1, 31) for d in (True, False)],
    "sub_kmer_words": [dict(k=32, pos=5, width=20), dict(k=31, pos=3, width=28), dict(k=32, pos=0, width=32)],
    "kmers_to_strings": [dict(k=k) for k in (1, 2, 3, 4, 27, 32)],
    "bitmers_to_bytes": [dict(k=k) for k in (1, 2, 3, 4, 27, 32)],
    "encode_kmers": [dict(enc=e, seq_len=sl, B=B) for e in ENCS for sl, B in ((31, 1), (33, 2))],
    "encoding_rev_comp": [dict(enc=e, K=K, B=B) for e in ENCS for K, B in ((2, 1), (31, 1), (33, 2), (64, 2))],
    "encoding_decode": [dict(enc=e, B=B) for e in ENCS for B in (1, 2)],
    "encode_windows": [dict(enc=e, L=40, k=31, B=1) for e in ENCS],
    "encode_kmers_p": [dict(enc=e, bits=b, B=B) for e in ENCS for b, B in ((8, 3), (32, 1), (128, 1))],
    "encoding_rev_comp_p": [dict(enc=e, bits=b, B=B) for e in ENCS for b, B in ((8, 3), (32, 1), (128, 1))],
    "encoding_decode_p": [dict(enc=e, bits=b, B=B) for e in ENCS for b, B in ((8, 3), (32, 1), (128, 1))],
    "seqvec_push_chars": [dict(n_before=b) for b in (0, 5, 32, 37)],
    "seqvec_to_bytes": [dict()],
    "seqvec_get_kmers": [dict(k=k) for k in (1, 31, 32)],
    "seqvec_iter_kmers": [dict(k=k) for k in (1, 32)],
    "gen_reads": [dict(path="vec"), dict(path="bytes")],
}
MAP_WORDS = ("revcomp_words", "canonical_words", "hash_words", "hash_words_sip13")


def case_ids():
    return [(op, i) for op, ps in OPS.items() for i in range(len(ps))]


def case_name(op, i):
    return op + "".join(f"-{k}{v}" for k, v in OPS[op][i].items())


def _enc(p):
    return ENCS[p["enc"]]


def build(op: str, p: dict, S: int, size, seed: int = 1, even: bool = False, bad: tuple = ()) -> Case:
    """the case of `op` with parameters `p` at a size class ("past" or an edge n).  even: the map_words calls with an even n (no scalar
    tail).  bad: byte indices (kmers_from_bytes, seqvec_push_chars) or element indices (seqvec_get_kmers) made invalid."""
    mk = lambda **kw: Case(op=op, params=p, **kw)
    if op in MAP_WORDS and not (op == "canonical_words" and p["form"] != "words"):
        n, items = _n_of(S, size, 2, odd=not even)
        s2 = {"out": 2 * S}
    if op == "revcomp_words":
        w = rand_words(n, seed, p["k"])
        return mk(n=n, inputs={"in": w}, outputs={"out": revcomp_word(w, p["k"])}, sweep2=s2, alias=("in", "out"), vec="in", items=items)
    if op == "canonical_words":
        k = p["k"]
        if p["form"] != "words":
            n, items = _n_of(S, size)
            s2 = None
        w = rand_words(n, seed, k).copy()
        if k % 2 == 0 and n:                       # palindromes: fw == rc, the tie of `w <= rc`; one of them in the last element
            at = np.unique(np.concatenate([np.arange(0, n, 97), [n - 1]]))
            w[at] = palindrome(rand_words(n, seed + 1)[at], k)
        canon, flag = canonical(w, k)
        outs = {"both": {"out": canon, "flags": flag}, "words": {"out": canon}, "flags": {"flags": flag}}[p["form"]]
        first = 2 * S if p["form"] == "words" else S
        return mk(n=n, inputs={"in": w}, outputs=outs, sweep2={x: first for x in outs}, alias=None if p["form"] == "flags" else ("in", "out"),
                  vec="in" if p["form"] == "words" else None, items=items)
    if op == "hash_words":
        w = rand_words(n, seed)
        out = lex_hash(w, p["hk"]) if p["hasher"] == HASH_LEX else w.copy()
        return mk(n=n, inputs={"in": w}, outputs={"out": out}, sweep2=s2, alias=("in", "out"), vec="in", items=items)
    if op == "hash_words_sip13":
        w = rand_words(n, seed)
        return mk(n=n, inputs={"in": w}, outputs={"out": sip13_np.siphash13(w, p["k0"], p["k1"])}, sweep2=s2, alias=("in", "out"), vec="in", items=items)
    if op == "match_words":
        n, items = _n_of(S, size)
        fw = rand_words(n, seed, 31)
        rc = revcomp_word(fw, 31)
        sel = np.arange(n) % 3                     # other: the forward word, the twin, neither -- a third each
        other = np.where(sel == 0, fw, np.where(sel == 1, rc, rand_words(n, seed + 1, 31)))
        return mk(n=n, inputs={"fw": fw, "rc": rc, "other": other}, outputs={"out": match(fw, rc, other)}, sweep2={"out": S}, items=items)
    if op == "ck_shift":
        n, items = _n_of(S, size)
        k = p["k"]
        fw = rand_words(n, seed, k)
        rc = revcomp_word(fw, k)
        bases = (rand_words(n, seed + 1) >> _U(7)).astype(np.uint8)      # any byte: the call takes the low two bits
        f, r, d = ck_shift(fw, rc, bases, k, p["append"])
        outs = {"fw": f, "rc": r}
        if p["dropped"]:
            outs["dropped"] = d
        return mk(n=n, inputs={"bases": bases}, outputs=outs, sweep2={x: S for x in outs}, init={"fw": fw, "rc": rc}, items=items)
    if op == "sub_kmer_words":
        n, items = _n_of(S, size)
        w = rand_words(n, seed, p["k"])
        return mk(n=n, inputs={"in": w}, outputs={"out": sub_kmer(w, p["pos"], p["width"])}, sweep2={"out": S}, alias=("in", "out"), items=items)
    if op == "kmers_from_bytes":
        n, items = _n_of(S, size)
        k = p["k"]
        seqs = rand_ascii(n * k, seed).copy()
        seqs[list(bad)] = ord("N")
        words, fb = kmers_from_bytes(seqs, n, k)
        return mk(n=n, inputs={"seqs": seqs}, outputs={"out": words}, sweep2={"out": S}, status=E_INVALID_BASE if bad else OK, first_bad=fb, items=items)
    if op in ("kmers_to_strings", "bitmers_to_bytes"):
        k = p["k"]
        q = (k + 3) // 4                           # a thread writes 4 letters
        n, items = (-(-past(S) // q), past(S)) if size == "past" else (int(size), 0)
        items = n * q if items else 0
        w = rand_words(n, seed, k)
        return mk(n=n, inputs={"in": w}, outputs={"out": to_letters(w, k, op == "bitmers_to_bytes")}, sweep2={"out": (S // q) * k + 4 * (S % q)}, items=items)
    if op == "encode_kmers":
        n, items = _n_of(S, size)
        sl, B = p["seq_len"], p["B"]
        seqs = rand_ascii(n * sl, seed)
        return mk(n=n, inputs={"seqs": seqs}, outputs={"out": encode(seqs, n, sl, _enc(p), B).reshape(-1)}, sweep2={"out": S * B}, items=items)
    if op == "encoding_rev_comp":
        n, items = _n_of(S, size)
        K, B = p["K"], p["B"]
        w = rand_words(n * B, seed).copy()        # all 64 * B bits random: what lies at and above bit 2K has to come through
        if K < 32 * B:                             # ... and is never all zero (at K = 31 it is one base: a quarter of them would be)
            top = w.reshape(n, B)[:, K // 32]
            top[(top >> _U(2 * (K % 32))) == 0] |= _U(2 << (2 * (K % 32)))
        return mk(n=n, inputs={"in": w}, outputs={"out": rev_comp(w, K, _enc(p), B).reshape(-1)}, sweep2={"out": S * B}, alias=("in", "out"), items=items)
    if op == "encoding_decode":
        n, items = _n_of(S, size)
        B = p["B"]
        w = rand_words(n * B, seed)
        return mk(n=n, inputs={"in": w}, outputs={"out": decode(w, _enc(p), B).reshape(-1)}, sweep2={"out": S * B * 32}, items=items)
    if op == "encode_windows":
        L, k, B = p["L"], p["k"], p["B"]
        nwin = L - k + 1
        n, items = (-(-past(S) // nwin), past(S)) if size == "past" else (int(size), 0)
        items = n * nwin if items else 0
        bases = rand_ascii(n * L, seed)
        return mk(n=n, inputs={"bases": bases}, outputs={"out": encode_windows(bases, n, L, k, _enc(p), B).reshape(-1)}, sweep2={"out": S * B}, items=items)
    if op in ("encode_kmers_p", "encoding_rev_comp_p", "encoding_decode_p"):
        nb = p["bits"] // 8 * p["B"]               # a thread handles one byte of the image
        n, items = (-(-past(S) // nb), past(S)) if size == "past" else (int(size), 0)
        items = n * nb if items else 0
        if op == "encode_kmers_p":
            sl = 4 * nb - 1
            seqs = rand_ascii(n * sl, seed)
            return mk(n=n, inputs={"seqs": seqs}, outputs={"out": encode_bytes(seqs, n, sl, _enc(p), nb).reshape(-1)}, sweep2={"out": S}, items=items)
        img = np.ascontiguousarray(rand_words((n * nb + 7) // 8, seed)).view(np.uint8)[: n * nb].reshape(n, nb)
        if op == "encoding_rev_comp_p":
            return mk(n=n, inputs={"in": img.reshape(-1)}, outputs={"out": rev_comp_bytes(img, 4 * nb - 1, _enc(p)).reshape(-1)}, sweep2={"out": S}, items=items)
        return mk(n=n, inputs={"in": img.reshape(-1)}, outputs={"out": decode_bytes(img, _enc(p)).reshape(-1)}, sweep2={"out": 4 * S}, items=items)
    if op == "seqvec_push_chars":
        nbf = p["n_before"]
        w0 = nbf // 32
        # a thread writes one word; the last one is partial
        n, items = (32 * (past(S) - 1) + 7 - nbf % 32, past(S)) if size == "past" else (int(size), 0)
        data = rand_ascii(n, seed).copy()
        data[list(bad)] = ord("N")
        n_words = (nbf + n + 31) // 32
        before = np.full(max(n_words, w0 + 1), POISON_U64, np.uint64)      # every bit past base n_before is set to something the call must drop
        before[w0] = rand_words(1, seed + 2)[0]
        words, fb = seqvec_push(before, nbf, data)
        if n == 0:
            return mk(n=0, inputs={"bytes": data}, outputs={"words": before[w0:]}, sweep2={"words": S}, init={"words": before[w0:]}, first_bad=M64)
        return mk(n=n, inputs={"bytes": data}, outputs={"words": words[w0:]}, sweep2={"words": S}, init={"words": before[w0:n_words]},
                  status=E_INVALID_BASE if bad else OK, first_bad=fb, items=items)
    if op == "seqvec_to_bytes":
        n, items = _n_of(S, size)
        w = rand_words((n + 31) // 32, seed)
        return mk(n=n, inputs={"words": w}, outputs={"out": seqvec_unpack(w, n)}, sweep2={"out": S}, items=items)
    if op == "seqvec_get_kmers":
        n, items = _n_of(S, size)
        k = p["k"]
        n_bases = 100_003                          # not a multiple of 32: the last word is partial
        w = seqvec_pack(_ACGT[(rand_words(n_bases, seed) & _U(3)).astype(np.int64)])[0]
        pos = rand_words(n, seed + 1) % _U(n_bases - k + 1)
        fixed = np.array([0, n_bases - k, 31, 32, 33, 63, 64, 32 * ((n_bases - k) // 32)], np.uint64)   # ends and word boundaries
        pos[: min(n, len(fixed))] = fixed[:n]
        if n > len(fixed):
            pos[-len(fixed):] = fixed
        out = seqvec_field(w, n_bases, pos, k)
        for e in bad:
            pos[e] = n_bases - k + 1
            out[e] = 0
        return Case(op=op, params=dict(p, n_bases=n_bases), n=n, inputs={"words": w, "pos": pos}, outputs={"out": out}, sweep2={"out": S},
                    status=E_ARG if bad else OK, items=items)
    if op == "seqvec_iter_kmers":
        n, items = _n_of(S, size)                  # n = the k-mers of the slice
        k, start = p["k"], 37                      # the slice starts off a word boundary
        end = start + n + k - 1 if n else start
        n_bases = end + 45
        w = rand_words((n_bases + 31) // 32, seed)
        out = seqvec_field(w, n_bases, np.arange(start, start + n, dtype=np.uint64), k)
        return Case(op=op, params=dict(p, n_bases=n_bases, start=start, end=end), n=n, inputs={"words": w}, outputs={"out": out}, sweep2={"out": S}, items=items)
    if op == "gen_reads":
        seed64 = 0x6B6D6572735F7631 + seed
        if p["path"] == "vec":                     # a thread writes 16 bytes; a 1..15-byte tail follows
            n, items = (16 * past(S) + 11, past(S)) if size == "past" else (int(size), 0)
            first = 16 * 1_000_003
            s2 = 16 * S
        else:
            n, items = _n_of(S, size)
            first, s2 = 7, S
        return Case(op=op, params=dict(p, seed=seed64, first_byte=first), n=n, inputs={}, outputs={"out": gen_reads(seed64, first, n)}, sweep2={"out": s2}, items=items)
    raise KeyError(op)


# ------------------------------------------------------------------ offsets: length range and the uniform gate

def length_range_offsets(S8: int, where: str, seed: int = 1):
    """offsets of n_reads = S8 + S8 // 3 + 1 reads of 40 .. 200 bases with ONE shortest (7) and ONE longest (300) read, both in the
    second sweep of an 8 * n_cu grid ("second": the first indices past S8; "last": the last, partial block) -> (offsets, min, max)"""
    n_reads = S8 + S8 // 3 + 1
    lens = 40 + (rand_words(n_reads, seed) % _U(161)).astype(np.int64)
    lo, hi = (S8, S8 + 1) if where == "second" else (n_reads - 1, n_reads - 130)
    lens[lo], lens[hi] = 7, 300
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), 7, 300, (lo, hi)


GATE_K, GATE_L = 31, 33


def gate_reads(S8: int):
    """n_reads of the uniform-gate batch: n_reads + 1 offsets are an odd number, so the gate's scalar tail runs"""
    return 2 * S8 + S8 // 2 + 2


def gate_short_read(S8: int, where: str):
    """the read that is one base short, so that the FIRST offset off the uniform grid is: "second" -- the first offset pair of the
    gate's second sweep; "last" -- the last pair; "tail" -- the odd tail offset; None for "none" """
    n = gate_reads(S8)
    return {"second": 2 * S8 - 1, "last": n - 3, "tail": n - 1, "none": None}[where]


def gate_offsets(S8: int, where: str) -> np.ndarray:
    n = gate_reads(S8)
    lens = np.full(n, GATE_L, np.int64)
    r = gate_short_read(S8, where)
    if r is not None:
        lens[r] -= 1
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


# ------------------------------------------------------------------ models of the failures the sweep is there to catch

def truncated_at(case: Case, name: str) -> np.ndarray:
    """what a kernel that stopped after one grid sweep would leave in output `name` of a guarded, poisoned buffer"""
    exp = case.outputs[name]
    out = exp.copy()
    rest = case.init[name][case.sweep2[name]:] if name in case.init else (POISON_U64 if exp.dtype == np.uint64 else POISON_U8)
    out[case.sweep2[name]:] = rest
    return out


def without_odd_tail(case: Case, name: str = "out") -> np.ndarray:
    """what map_words would leave if it skipped the scalar tail behind the 16-byte pairs"""
    out = case.outputs[name].copy()
    if len(out) % 2:
        out[-1] = POISON_U64
    return out
