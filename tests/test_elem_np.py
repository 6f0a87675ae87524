"""CPU checks of tests/elem_np.py: every numpy reference against the C oracle and the reference KATs at small n, at every k / K the
GPU file (tests/test_gpu_elem_sweep.py) uses; then, on the GPU file's own `past` inputs built for the stride of a 256-CU device, the
conditions that keep that file honest -- the outputs of the second sweep differ from the poison (and, in place, from the input), every
class of an output is there, and the comparison rejects a model of a kernel that stops after one sweep or skips the odd tail."""
import ctypes as C

import numpy as np
import pytest

from tests import elem_np as E
from tests import sip13_np

N = 300
S = E.S_256CU


def _words(k, seed=5, n=N):
    w = E.rand_words(n, seed, k).copy()
    w[:3] = [0, E.mask2k(k), 1]
    return w


# ------------------------------------------------------------------ the references against the oracle

@pytest.mark.parametrize("k", [1, 2, 16, 31, 32])
def test_word_ops_equal_the_oracle(orc, k):
    L = orc.lib()
    w = _words(k)
    assert [int(x) for x in E.revcomp_word(w, k)] == [L.kmo_revcomp_word(int(x), k) for x in w]
    canon, flag = E.canonical(w, k)
    for x, c, f in zip(w, canon, flag):
        km = orc.Kmer(k, int(x))
        assert L.kmo_kmer_to_canonical(km).data == int(c) and bool(L.kmo_kmer_is_canonical(km)) == bool(f)
    full = E.rand_words(N, 6)
    for hk in (1, 20, 32):
        assert [int(x) for x in E.lex_hash(full, hk)] == [L.kmo_lex_hash_u64(int(x), hk) for x in full]
    if k % 2 == 0:
        p = E.palindrome(E.rand_words(N, 7), k)
        assert (E.revcomp_word(p, k) == p).all() and (p <= np.uint64(E.mask2k(k))).all()


@pytest.mark.parametrize("k", [1, 31])
@pytest.mark.parametrize("append", [True, False])
def test_ck_shift_and_match_equal_the_oracle(orc, k, append):
    L = orc.lib()
    fw = _words(k)
    rc = E.revcomp_word(fw, k)
    bases = (E.rand_words(N, 8) >> np.uint64(9)).astype(np.uint8)
    f, r, d = E.ck_shift(fw, rc, bases, k, append)
    step = L.kmo_ck_append_base if append else L.kmo_ck_prepend_base
    other = np.where(np.arange(N) % 3 == 0, fw, np.where(np.arange(N) % 3 == 1, rc, fw ^ np.uint64(1)))
    m = E.match(fw, rc, other)
    for i in range(N):
        ck = L.kmo_ck_from_u64(int(fw[i]), k)
        assert m[i] == L.kmo_ck_get_word_equivalency(C.byref(ck), int(other[i]))
        dropped = step(C.byref(ck), int(bases[i]) & 3)
        assert (ck.fw.data, ck.rc.data, dropped) == (int(f[i]), int(r[i]), int(d[i])), i


def test_sub_kmer_and_letters_equal_the_oracle(orc):
    for p in E.OPS["sub_kmer_words"]:
        w = _words(p["k"])
        assert [int(x) for x in E.sub_kmer(w, p["pos"], p["width"])] == [orc.sub_kmer_word(int(x), p["k"], p["pos"], p["width"]) for x in w]
    L = orc.lib()
    for k in (1, 2, 3, 4, 27, 32):
        w = _words(k)
        up = E.to_letters(w, k, True).reshape(N, k)
        lo = E.to_letters(w, k, False).reshape(N, k)
        for i in range(N):
            assert up[i].tobytes() == orc.bitmer_to_bytes(int(w[i]), k)
            assert lo[i].tobytes().decode() == orc.kmer_to_string(orc.Kmer(k, int(w[i])))


@pytest.mark.parametrize("k", [1, 31, 32])
def test_kmers_from_bytes_equals_the_oracle(orc, kats, k):
    seqs = E.rand_ascii(N * k, 9)
    words, bad = E.kmers_from_bytes(seqs, N, k)
    assert bad == E.M64
    assert [int(x) for x in words] == [orc.kmer_from_bytes(seqs[i * k:(i + 1) * k].tobytes()).data for i in range(N)]
    dirty = seqs.copy()
    dirty[[5 * k, 2 * k + k - 1]] = ord("N")
    assert E.kmers_from_bytes(dirty, N, k)[1] == 2 * k + k - 1
    for s, r in kats["reverse_complement"]["cases"]:
        w = E.kmers_from_bytes(np.frombuffer(s.encode(), np.uint8), 1, len(s))[0]
        assert int(E.revcomp_word(w, len(s))[0]) == orc.kmer_from_bytes(r.encode()).data


def test_encodings_equal_the_oracle(orc, kats):
    encs = kats["naive_encodings"]["enc_bytes"]
    assert all(encs[name] == v for name, v in E.ENCS.items())
    n = 40
    for name, enc in encs.items():                     # all 24, in the u64 form and in every byte-image form
        for seq_len, nb in ((31, 8), (33, 16), (64, 16), (2, 8), (11, 3), (15, 4), (63, 16), (7, 2)):
            seqs = E.rand_ascii(n * seq_len, 10)
            arr = E.encode_bytes(seqs, n, seq_len, enc, nb)
            hi = np.ascontiguousarray(E.rand_words(n * 2, 11)).view(np.uint8)[: n * nb].reshape(n, nb)      # all bits random: bits >= 2K must stay
            rc, rch, dec = E.rev_comp_bytes(arr, seq_len, enc), E.rev_comp_bytes(hi, seq_len, enc), E.decode_bytes(hi, enc)
            for i in range(n):
                want = orc.naive_encode(enc, seqs[i * seq_len:(i + 1) * seq_len].tobytes(), nb)
                assert (arr[i] == want).all(), (name, seq_len, nb)
                assert (rc[i] == orc.naive_rev_comp(enc, seq_len, want)).all(), (name, seq_len, nb)
                assert (rch[i] == orc.naive_rev_comp(enc, seq_len, hi[i])).all(), (name, seq_len, nb)
                assert dec[i].tobytes() == orc.naive_decode(enc, hi[i])
            if nb % 8 == 0:
                B = nb // 8
                w = E.encode(seqs, n, seq_len, enc, B)
                assert [int(x) for x in w.reshape(-1)] == orc.words(arr.reshape(-1), 64)
                assert [int(x) for x in E.rev_comp(w, seq_len, enc, B).reshape(-1)] == orc.words(rc.reshape(-1), 64)
                assert (E.decode(w, enc, B) == E.decode_bytes(arr, enc)).all()
    c = [x for x in kats["naive_encode_kats"]["cases"] if x["name"] == "k45pu64"][0]
    w = E.encode(np.frombuffer(c["seq"].encode(), np.uint8), 1, c["K"], encs["ACGT"], 2)
    assert E.decode(w, encs["ACGT"], 2).tobytes() == c["decode"].encode()
    assert E.decode(E.rev_comp(w, c["K"], encs["ACGT"], 2), encs["ACGT"], 2).tobytes() == c["decode_rev_comp"].encode()
    # windows: Naive::ACGT encode == naive_impl::Kmer::from on valid input, so the oracle's forward words serve
    L_, k = 40, 31
    bases = E.rand_ascii(7 * L_, 12)
    fw = orc.canonical_windows(bases, 7, L_, k)[0]
    assert (E.encode_windows(bases, 7, L_, k, encs["ACGT"], 1).reshape(-1) == fw).all()
    for enc in E.ENCS.values():
        win = E.encode_windows(bases, 7, L_, k, enc, 1)
        assert (win[13, 0] == E.encode(bases[L_ + 3: L_ + 3 + k], 1, k, enc, 1)[0, 0])


def test_seqvec_equals_the_oracle(orc):
    data = E.rand_ascii(1000 + 7, 13)
    sv = orc.SeqVector(data.tobytes())
    words, bad = E.seqvec_pack(data)
    nw = (len(data) + 31) // 32
    assert bad == E.M64 and (words == sv.words[:nw]).all()
    assert E.seqvec_unpack(words, len(data)).tobytes() == sv.to_bytes()
    for n_before in (0, 5, 32, 37):
        two = orc.SeqVector(data[:n_before].tobytes())
        two.push_chars(data[n_before:].tobytes())
        before = np.full(nw, E.POISON_U64, np.uint64)
        before[: (n_before + 31) // 32] = E.seqvec_pack(data[:n_before])[0]
        if n_before % 32:
            before[n_before // 32] |= np.uint64(E.POISON_U64 << (2 * (n_before % 32)) & E.M64)     # rubbish past base n_before: dropped
        got, bad = E.seqvec_push(before, n_before, data[n_before:])
        assert bad == E.M64 and (got == two.words[:nw]).all() and (got == words).all(), n_before
    dirty = data.copy()
    dirty[[700, 40]] = ord("n")
    assert E.seqvec_pack(dirty)[1] == 40 and E.seqvec_push(words[:1], 5, dirty[5:])[1] == 35
    for k in (1, 31, 32):
        pos = np.concatenate([[0, len(data) - k, 31, 32, 33, 63, 64], E.rand_words(200, 14) % np.uint64(len(data) - k + 1)]).astype(np.uint64)
        assert [int(x) for x in E.seqvec_field(words, len(data), pos, k)] == [sv.get_kmer_u64(int(p), k) for p in pos]
        it = sv.iter_kmers(k, 37, 900)
        assert (E.seqvec_field(words, len(data), np.arange(37, 37 + len(it), dtype=np.uint64), k) == it).all() and len(it) == 900 - 37 - k + 1


def test_gen_reads_and_length_range_equal_the_oracle(orc):
    for seed, first, n in ((0x6B6D6572735F7631, 0, 100), (5, 7, 1000), (2**64 - 3, 16 * 1_000_003, 16 * 40 + 11), (1, 31, 2), (1, 32, 0)):
        assert (E.gen_reads(seed, first, n) == orc.gen_reads(seed, first, n)).all(), (seed, first, n)
    assert int(E.splitmix64(np.array([12345], np.uint64))[0]) == orc.lib().kmo_splitmix64(12345)
    off = np.array([0, 10, 10, 300, 307], np.uint64)
    assert E.length_range(off) == (0, 290)
    assert sip13_np.siphash13(np.array([1], np.uint64), 2, 3)[0] == orc.lib().kmo_siphash13_u64(1, 2, 3)


# ------------------------------------------------------------------ the GPU file's inputs: non-vacuity

def _fresh(exp, poison):
    return float((exp != poison).mean())


@pytest.mark.parametrize("op,i", E.case_ids(), ids=[E.case_name(*c) for c in E.case_ids()])
def test_past_case_is_not_vacuous(op, i):
    p = E.OPS[op][i]
    c = E.build(op, p, S, "past")
    assert c.items >= E.past(S) > S
    if c.vec:
        assert c.n % 2 == 1 and c.n // 2 > S              # pairs past the stride AND the scalar tail
        assert not E.same(E.without_odd_tail(c), c.outputs["out"])
    total = sum(a.nbytes for a in list(c.inputs.values()) + list(c.outputs.values()) + list(c.init.values()))
    assert total + 2 * len(c.outputs) * E.GUARD_BYTES < 256 << 20
    for name, exp in c.outputs.items():
        s2 = c.sweep2[name]
        assert 0 < s2 < len(exp), name
        tail = exp[s2:]
        poison = E.POISON_U64 if exp.dtype == np.uint64 else E.POISON_U8
        assert _fresh(tail, poison) >= 0.99, name
        assert not E.same(E.truncated_at(c, name), exp), name                   # a kernel that stops after one sweep fails the comparison
    if c.alias:
        src, out = c.inputs[c.alias[0]], c.outputs[c.alias[1]]
        B = p.get("B", 1)                                  # (an element of encoding_rev_comp is B words)
        differ = float((out[c.sweep2[c.alias[1]]:] != src[c.sweep2[c.alias[1]]:]).reshape(-1, B).any(axis=1).mean())
        if op == "hash_words" and p["hasher"] == E.HASH_IDENTITY:
            assert differ == 0.0                           # exempt: the identity hasher's output IS its input
        elif op == "canonical_words":
            assert 0.25 <= differ <= 0.75                  # a canonical word is its own output: only the other strand changes
        elif op == "encoding_rev_comp" and p["K"] == 2:
            assert differ >= 0.70                          # 4 of the 16 two-base words are their own reverse complement
        else:
            assert differ >= 0.99
    tail = lambda name: c.outputs[name][c.sweep2[name]:]
    if op == "match_words":
        assert all(float((tail("out") == v).mean()) >= 0.10 for v in (0, 1, 2))
    if op == "canonical_words":
        flags = E.canonical(c.inputs["in"], p["k"])[1]
        first = c.sweep2[next(iter(c.outputs))]
        assert 0.25 <= float(flags[first:].mean()) <= 0.75
        if p["k"] % 2 == 0:
            w = c.inputs["in"][first:]
            assert int((E.revcomp_word(w, p["k"]) == w).sum()) >= 1 and E.revcomp_word(c.inputs["in"][-1:], p["k"])[0] == c.inputs["in"][-1]
    if op == "ck_shift" and p["dropped"]:
        assert set(np.unique(tail("dropped"))) == {0, 1, 2, 3}
    if op == "encoding_rev_comp" and p["K"] < 32 * p["B"]:
        w = c.inputs["in"].reshape(-1, p["B"])[S:]
        high = w[:, p["K"] // 32] >> np.uint64(2 * (p["K"] % 32))
        assert float((high != 0).mean()) >= 0.99          # "bits >= 2K unchanged" has bits to get wrong


@pytest.mark.parametrize("op", list(E.OPS))
def test_edge_cases_build(op):
    for p in E.OPS[op]:
        for n in E.EDGE:
            c = E.build(op, p, S, n)
            assert c.n == n and c.status == E.OK and c.items == 0
            assert all(a.dtype in (np.uint8, np.uint64) and a.ndim == 1 for a in list(c.inputs.values()) + list(c.outputs.values()) + list(c.init.values()))
            if n == 0:
                assert all(len(a) == 0 or name in c.init for name, a in c.outputs.items())


def test_planted_errors_lie_past_the_first_sweep():
    for op, p, per in (("kmers_from_bytes", dict(k=31), 31), ("seqvec_push_chars", dict(n_before=5), 32)):
        lo, hi = (S + 11) * per + 3, (S + S // 4) * per
        c = E.build(op, p, S, "past", bad=(hi, lo))
        assert c.status == E.E_INVALID_BASE and c.first_bad == lo and lo // per >= S
    c = E.build("seqvec_get_kmers", dict(k=31), S, "past", bad=(S + 5,))
    assert c.status == E.E_ARG and int(c.inputs["pos"][S + 5]) + 31 > c.params["n_bases"]


def test_offset_batches_put_the_deciding_element_where_they_say():
    S8 = S // 2
    for where in ("second", "last"):
        off, mn, mx, (lo, hi) = E.length_range_offsets(S8, where)
        n_reads = len(off) - 1
        assert n_reads == S8 + S8 // 3 + 1 and E.length_range(off) == (mn, mx)
        lens = np.diff(off.astype(np.int64))
        assert int((lens == mn).sum()) == 1 and int((lens == mx).sum()) == 1 and min(lo, hi) >= S8
        if where == "last":
            assert min(lo, hi) >= n_reads // 256 * 256 and n_reads % 256
    n = E.gate_reads(S8)
    assert (n + 1) % 2 == 1 and (n + 1) // 2 > S8            # an odd number of offsets, and pairs past one sweep of 8 * n_cu blocks
    grid = np.arange(n + 1, dtype=np.uint64) * np.uint64(E.GATE_L)
    for where, first_bad in (("second", 2 * S8), ("last", n - 2), ("tail", n), ("none", None)):
        wrong = np.flatnonzero(E.gate_offsets(S8, where) != grid)
        assert (first_bad is None and len(wrong) == 0) or int(wrong[0]) == first_bad, where
