"""tests/minimizers_np.py on the CPU: its references against the oracle's monotone deque and the reference's own vectors, its arm
table against the kernels that exist, and the proof that the cases of tests/test_gpu_minimizers_sweep.py could not pass with a
kernel that stops after one grid sweep or that works on the previous sweep's unit again."""
import time

import numpy as np
import pytest

from tests import elem_np as E
from tests import kernel_usage
from tests import minimizers_np as M
from tests import sip13_np as S

ALL = M.CASES + [p for p, _ in M.EDGE] + M.BAD


def _small_batch(rng, n, L):
    host = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n * L)].copy()
    host[:L] = np.frombuffer(b"AC", np.uint8)[rng.integers(0, 2, L)]          # two-letter reads: ties, the leftmost wins
    if n > 1:
        host[L: 2 * L] = np.frombuffer(b"gt", np.uint8)[rng.integers(0, 2, L)]
    return host


def test_reference_equals_the_oracles_deque(orc):
    """identity and Lex at every (k, w, hk) in use: uniform reads against kmo_seqvec_minimizers, ragged reads -- one of k - 1 bases,
    one of k, an empty one -- against the iterator read by read"""
    seen = sorted({(p.k, p.w, p.hk if p.hasher == "lex" else 0) for p in ALL if p.hasher != "sip" and p.call != "minimizer_words"})
    assert len(seen) >= 15
    rng = np.random.default_rng(3)
    for k, w, hk in seen:
        hasher = M.Lex(hk) if hk else M.Identity()
        n, L = 5, k + 9
        host = _small_batch(rng, n, L)
        ow, op = orc.seqvec_minimizers(orc.SeqVector(host.tobytes()), n, L, k, w, hk)
        gw, gp = M.reference(host, L, k, w, hasher)
        assert E.same(gw, ow) and E.same(gp, op), (k, w, hk)
        lens = np.array([L, k - 1, k, 0, L - 4, w, k + 1])
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        host = _small_batch(rng, -(-int(off[-1]) // L), L)[: int(off[-1])]
        words, pos = [], []
        for r in range(len(lens)):
            rd = host[int(off[r]): int(off[r + 1])]
            if len(rd) >= k:
                for a, b in orc.seqvec_iter_minimizers(orc.SeqVector(rd.tobytes()), k, w, hk):
                    words.append(a)
                    pos.append(b)
        gw, gp = M.reference(host, off, k, w, hasher)
        assert E.same(gw, np.array(words, np.uint64)) and E.same(gp, np.array(pos, np.uint32)), (k, w, hk, "ragged")
        assert len(gw) == int(M.window_counts(off, k)[1][-1])


def test_reference_equals_the_reference_vectors(kats):
    for t in kats["minimizers"]["iter"]:
        s = np.frombuffer(t["seq"].encode(), np.uint8)
        gw, gp = M.reference(s, len(s), t["k"], t["w"], M.Lex(t["hasher_k"]) if t["hasher_k"] else M.Identity())
        assert [[int(a), int(b)] for a, b in zip(gw, gp)] == t["expect"], t["name"]


def test_words_reference_equals_the_oracle(orc):
    seen = sorted({(p.k, p.w, p.hk if p.hasher == "lex" else 0) for p in ALL if p.hasher != "sip" and p.call == "minimizer_words"})
    assert seen
    words = np.random.default_rng(4).integers(0, 2**64, 96, dtype=np.uint64)
    words[:16] &= np.uint64(0x5555555555555555)
    # (width 32 is left out: the reference's MASK_TABLE[32] == 0 makes every sub-word 0 there, the calls keep the whole word --
    # tests/test_gpu_sip13.py pins that -- and no case uses it)
    for k, w, hk in seen + [(32, 31, 32), (32, 1, 0), (5, 5, 3)]:
        kw = words & np.uint64(E.mask2k(k))
        mm, off = M.words_reference(kw, k, w, M.Lex(hk) if hk else M.Identity())
        assert mm.dtype == np.uint64 and off.dtype == np.uint32
        for i, x in enumerate(kw):
            assert (int(mm[i]), int(off[i])) == orc.minimizer_word(int(x), k, w, hk), (k, w, hk, i)


def test_sip_form_equals_sip13_np():
    """the Sip hasher: SipHash-1-3 of every l-mer (tests/sip13_np.py, pinned in test_sip13_host.py), a strict `<` window by window"""
    rng = np.random.default_rng(5)
    k0, k1 = M.SIP_KEY
    for k, w in sorted({(p.k, p.w) for p in ALL if p.hasher == "sip" and p.call != "minimizer_words"}):
        L = k + 6
        host = _small_batch(rng, 3, L)
        gw, gp = M.reference(host, L, k, w, M.Sip(k0, k1))
        codes = S.codes_of(host).reshape(3, L)
        for r in range(3):
            lm = [sum(int(c) << (2 * b) for b, c in enumerate(codes[r, p: p + w])) for p in range(L - w + 1)]
            h = [int(x) for x in S.siphash13(np.array(lm, np.uint64), k0, k1)]
            for i in range(L - k + 1):
                best = min(range(i, i + k - w + 1), key=lambda p: (h[p], p))
                assert (int(gw[r * (L - k + 1) + i]), int(gp[r * (L - k + 1) + i])) == (lm[best], best), (k, w, r, i)
    words = rng.integers(0, 2**64, 40, dtype=np.uint64) & np.uint64(E.mask2k(24))
    mm, off = M.words_reference(words, 24, 17, M.Sip(k0, k1))
    for i, x in enumerate(words):
        sub = [(int(x) >> (2 * p)) & E.mask2k(17) for p in range(8)]
        h = [int(v) for v in S.siphash13(np.array(sub, np.uint64), k0, k1)]
        best = min(range(8), key=lambda p: (h[p], p))
        assert (int(mm[i]), int(off[i])) == (sub[best], best)


# ------------------------------------------------------------------ the arms

def test_every_arm_has_a_case():
    arms = {
        "reads_tiled<M0,uniform,k32>", "reads_tiled<M0,uniform,k64>", "reads_tiled<M0,ragged,k32>", "reads_tiled<M0,ragged,k64>",
        "reads_tiled<M1,uniform,k32>", "reads_tiled<M1,uniform,k64>", "reads_tiled<M1,ragged,k32>", "reads_tiled<M1,ragged,k64>",
        "reads_tiled<M2,uniform,k32>", "reads_tiled<M2,uniform,k64>", "reads_tiled<M2,ragged,k32>", "reads_tiled<M2,ragged,k64>",
        "reads_tiled_cut<M0>", "reads_tiled_cut<M1>", "reads_tiled_cut<M2>",
        "reads_generic[w>28]", "reads_generic[k==w]", "reads_generic[hash>56]", "reads_generic[ragged>256]", "reads_generic[k>256]",
        "seqvec_slide<M0,k32>", "seqvec_slide<M0,k64>", "seqvec_slide<M1,k32>", "seqvec_slide<M1,k64>", "seqvec_slide<M2,k32>",
        "seqvec_slide<M2,k64>", "seqvec_lds", "seqvec_direct",
        "minimizer_words<identity>", "minimizer_words<lex>", "minimizer_words_sip",
        "sip_piece<ascii,uniform>", "sip_piece<ascii,ragged>", "sip_piece<packed>", "sip_generic<ascii>", "sip_generic<packed>",
    }
    assert {c.arm.name for c in M.CASES} == arms == set(M.ARMS)
    assert len({c.id for c in M.CASES}) == len(M.CASES)
    # the sweep of every arm: blocks of the capped grid x units per block
    per_cu = {c.arm.name.split("<")[0].split("[")[0]: c.arm.per_cu for c in M.CASES}
    assert per_cu == {"reads_tiled": 8 * 16, "reads_tiled_cut": 8 * 16, "reads_generic": 16 * 4, "seqvec_slide": 8 * 16, "seqvec_lds": 8 * 16,
                      "seqvec_direct": 16 * 256, "minimizer_words": 16 * 256, "minimizer_words_sip": 16 * 256, "sip_piece": 16 * 4,
                      "sip_generic": 16 * 4}
    # the shapes the issue names
    # ... among them one tiled and one slide case whose launch needs more than 64 KiB of LDS (the launchers' formulas, restated)
    assert any(c.arm.name.startswith("reads_tiled<") and c.L == 256 and c.k >= 240 and M.tiled_lds(256, c.w) > 64 * 1024 for c in M.CASES)
    assert any(c.arm.name.startswith("seqvec_slide<") and c.L == 256 and c.k >= 240 and M.slide_lds(256, c.w) > 64 * 1024 for c in M.CASES)
    assert (M.tiled_lds(256, 11), M.slide_lds(256, 9), M.slide_lds(256, 15)) == (65620, 65792, 64256)
    assert M.tiled_lds(64, 15) < 64 * 1024 and M.slide_lds(64, 15) < 64 * 1024
    assert all(M.pieces(c.L, c.k)[0] == 8 for c in M.CASES if c.arm.name.startswith("reads_tiled_cut"))
    assert {c.shift for c in M.CASES if c.call == "minimizers"} == {0, 1, 2, 3}
    assert {c.shift for c in M.CASES if c.call != "minimizers"} == {0, 8}


def test_arm_routing_thresholds():
    a = lambda *x: M.arm_of(*x).name
    assert a("minimizers", 31, 28, "lex", 28, False, 256) == "reads_tiled<M1,uniform,k64>"
    assert a("minimizers", 31, 28, "lex", 29, False, 256) == "reads_generic[hash>56]"
    assert a("minimizers", 31, 29, "identity", 0, False, 150) == "reads_generic[w>28]"
    assert a("minimizers", 31, 15, "lex", 15, False, 257) == "reads_tiled_cut<M1>"
    assert a("minimizers", 31, 15, "lex", 15, True, 256) == "reads_tiled<M1,ragged,k64>"
    assert a("minimizers", 31, 15, "lex", 15, True, 257) == "reads_generic[ragged>256]"
    assert a("minimizers", 21, 12, "lex", 12, False, 100) == "reads_tiled<M1,uniform,k32>"
    assert a("minimizers", 21, 13, "lex", 12, False, 100) == "reads_tiled<M2,uniform,k64>"
    assert a("seqvec_minimizers", 31, 15, "identity", 0, False, 257) == "seqvec_lds"
    assert M.arm_of("seqvec_minimizers", 31, 15, "identity", 0, False, 700).per_cu == 8 * 8      # rb = 48 KiB / (686 * 8) = 8
    assert a("seqvec_minimizers", 16, 16, "identity", 0, False, 6159) == "seqvec_lds"
    assert a("seqvec_minimizers", 16, 16, "identity", 0, False, 6160) == "seqvec_direct"
    assert a("minimizers", 256, 15, "sip", 0, False, 300) == "sip_piece<ascii,uniform>"
    assert a("minimizers", 257, 15, "sip", 0, False, 300) == "sip_generic<ascii>"
    assert M.pieces(1000, 31) == (5, 226) and M.pieces(300, 250) == (8, 7)


def test_kernel_instances(tmp_path):
    """the arm table names twelve instantiations of the reads kernel and six of the slide kernel: so many exist"""
    reads = [ln for ln in kernel_usage.usage_lines("kmx_minimizers.hip", tmp_path) if "minimizers_reads_kernel" in ln]
    slide = [ln for ln in kernel_usage.usage_lines("kmx_seqvec.hip", tmp_path) if "seqvec_minimizers_slide_kernel" in ln]
    assert (len(reads), len(slide)) == (12, 6)
    assert len([n for n in M.ARMS if n.startswith("reads_tiled<")]) == 12 and len([n for n in M.ARMS if n.startswith("seqvec_slide<")]) == 6


# ------------------------------------------------------------------ the cases can fail

@pytest.mark.parametrize("n_cu", [8, 256])
def test_cases_could_not_pass_with_one_sweep(n_cu):
    cost = {}
    for c in M.CASES:
        t0 = time.perf_counter()
        b = M.build(c, n_cu)
        cost[c.id] = time.perf_counter() - t0
        U = c.arm.sweep(n_cu)
        assert b.U == U and b.units >= M.past(U) > U and b.units - M.past(U) < b.J, c.id
        assert b.status == M.OK and b.word.dtype == np.uint64 and b.pos.dtype == np.uint32 and len(b.word) == len(b.pos) == b.total
        unit = b.slot_units()
        assert len(unit) == b.total and (np.diff(unit) >= 0).all() and unit[-1] >= U, c.id
        for model in (M.model_one_sweep, M.model_previous_sweep):
            word, pos = model(b)
            early = unit < U
            assert E.same(word[early], b.word[early]) and E.same(pos[early], b.pos[early]), (c.id, model.__name__)
            assert (word[~early] != b.word[~early]).any(), (c.id, model.__name__)
            assert (word != b.word).sum() + (pos != b.pos).sum() > (~early).sum() // 4, (c.id, model.__name__)
        if c.ragged:
            lens, k = b.lens, c.k
            short = np.isin(lens, (0, k - 1, k, c.w))
            down = np.flatnonzero((lens[:b.n - U] == c.L) & short[U:])
            up = np.flatnonzero(short[:b.n - U] & (lens[U:] == c.L))
            assert len(down) >= 64 and len(up) >= 64, c.id
            assert set(down % 16) == set(up % 16) == set(range(16)), c.id          # every LDS row of a block
            for v in (0, k - 1, k, c.w):
                assert (lens[down + U] == v).any() and (lens[up] == v).any(), (c.id, v)
            assert int(lens.max()) == c.L
        if "bases" in b.inputs:
            host = b.inputs["bases"]
            assert E.base_codes(host)[1].all() and (host >= 0x61).any() and (host < 0x61).any(), c.id
    slowest = max(cost, key=cost.get)
    print(f"\nn_cu = {n_cu}: {sum(cost.values()):.1f} s for {len(cost)} builds, the slowest {slowest}: {cost[slowest]:.2f} s")


@pytest.mark.parametrize("n_cu", [8, 256])
def test_bad_byte_cases_lie_past_the_first_sweep(n_cu):
    assert {(c.hasher == "sip", c.ragged) for c in M.BAD} == {(False, False), (False, True), (True, False), (True, True)}
    assert any(c.arm.name.startswith("reads_tiled_cut") for c in M.BAD)
    for c in M.BAD:
        b = M.build(c, n_cu, bad=True)
        host = b.inputs["bases"]
        start = b.inputs["offsets"].astype(np.int64) if c.ragged else np.arange(b.n + 1) * c.L
        invalid = np.flatnonzero(~E.base_codes(host)[1])
        assert len(invalid) == 3 and sorted(at for _, at in b.bad_at) == list(invalid), c.id
        reads = np.searchsorted(start, invalid, side="right") - 1
        assert b.first_past * b.J >= b.U and (b.first_past - 1) * b.J < b.U
        assert (reads >= b.first_past).all() and invalid.min() >= start[b.first_past], c.id
        assert (b.status, b.first_bad) == (M.E_INVALID_BASE, int(reads.min())), c.id
        assert invalid[0] == start[reads[0] + 1] - 1, c.id                     # the lowest: its read's last base
        if b.J > 1:
            J, T = M.pieces(c.L, c.k)
            p = int(invalid[1] - start[reads[1]])
            assert T <= p < T + c.k - 1 and J == b.J, c.id                      # a base of piece 0 and of piece 1


def test_edge_cases():
    calls = {(p.call, p.hasher == "sip") for p, _ in M.EDGE}
    assert calls == {(call, sip) for call in ("minimizers", "seqvec_minimizers", "minimizer_words") for sip in (False, True)}
    for p, sizes in M.EDGE:
        for size in sizes:
            b = M.build(p, 8, size)
            assert b.units == (b.U if size == "U" else size) and b.total == b.n == b.units, (p.id, size)
            assert p.call == "minimizer_words" or p.L == p.k
    single = [M.build(p, 8, 1) for p, sizes in M.EDGE if sizes == (1,)]
    assert {(b.case.hasher, b.case.ragged) for b in single} >= {("lex", False), ("lex", True), ("identity", False), ("sip", False)}
    assert all(len(b.inputs["bases"]) == 12 for b in single)                   # fewer than 24 bytes: nothing to prefetch from
