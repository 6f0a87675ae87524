"""tests/adapter_np.py (the vectorised host reference of kmx_reads_adapter and kmx_reads_pair_overlap) against brute force: literal
per-position Python loops over the definitions of include/kmx.h, written without a look at the vectorised code.  Random reads over
ACGTacgtN of 0 to 200 bases, random adapters and thresholds, planted adapters and planted overlaps; the batches are checked to hold
hits and non-hits, a read on which two adapters hit at one position, and a pair whose best overlap length is reached by two
shifts -- so all three tie rules are exercised, not assumed.  No GPU."""
import numpy as np

from tests import adapter_np as A

ALPHA = np.frombuffer(b"ACGTACGTACGTACGTacgtN", np.uint8)
UP = {ord(c): ord(c.upper()) for c in "acgtACGT"}


def _is_base(b):
    return b in UP


def brute_adapter_row(read, adapters, min_overlap, err_num, err_den):
    """-> (row, the adapters that hit at the read's hit position)"""
    L = len(read)
    hits = 0
    first = {}   # adapter -> (p, n, m) of its leftmost hit
    for ai, ad in enumerate(adapters):
        for p in range(L):
            n = min(len(ad), L - p)
            m = 0
            for j in range(n):
                if ad[j] in b"Nn":
                    continue
                rb = read[p + j]
                if not (_is_base(rb) and UP[rb] == UP[ad[j]]):
                    m += 1
            if n >= min_overlap and m * err_den <= err_num * n:
                hits |= 1 << ai
                if ai not in first:
                    first[ai] = (p, n, m)
    if not first:
        return [L << 32, 0, L, 0], []
    p = min(v[0] for v in first.values())
    at_p = sorted(ai for ai, v in first.items() if v[0] == p)
    ai = at_p[0]
    _, n, m = first[ai]
    return [p << 32, (ai + 1) | (n << 16) | (m << 32), L, hits], at_p


def brute_pair_row(m1, m2, min_overlap, max_mism, err_num, err_den):
    """-> (row, the number of hits that share the largest n)"""
    comp = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}
    L1, L2 = len(m1), len(m2)
    none = [0, 0, L1 << 32, L2 << 32]
    if L1 > 1024 or L2 > 1024:
        return none, 0
    y = [comp[UP[b]] if _is_base(b) else None for b in reversed(m2)]
    hits = []   # (n, d, m)
    for d in range(-L2 + 1, L1):
        lo, hi = max(0, d), min(L1, d + L2)
        m = 0
        for i in range(lo, hi):
            xb = m1[i]
            if not (_is_base(xb) and y[i - d] is not None and UP[xb] == y[i - d]):
                m += 1
        n = hi - lo
        if n >= min_overlap and m <= max_mism and m * err_den <= err_num * n:
            hits.append((n, d, m))
    if not hits:
        return none, 0
    n = max(h[0] for h in hits)
    ties = [h for h in hits if h[0] == n]
    _, d, m = max(ties, key=lambda h: h[1])
    ins = d + L2
    return [ins, n | (m << 32), min(L1, ins) << 32, min(L2, ins) << 32], len(ties)


def _rand_seq(rng, n):
    return rng.choice(ALPHA, n).astype(np.uint8).tobytes()


def _mutate(rng, seq, k):
    s = bytearray(seq)
    for i in rng.choice(len(s), min(k, len(s)), replace=False) if len(s) else []:
        s[i] = ord("ACGT"[("ACGT".index(chr(UP.get(s[i], 65))) + 1) % 4])
    return bytes(s)


def test_adapter_reference_against_brute_force():
    rng = np.random.default_rng(2024)
    n_hit = n_miss = n_shared = n_overhang = 0
    for trial in range(6):
        n_ad = int(rng.integers(1, 9))
        adapters = []
        for _ in range(n_ad):
            ad = bytearray(rng.choice(np.frombuffer(b"ACGTACGTacgtNn", np.uint8), int(rng.integers(1, 65))).tobytes())
            adapters.append(bytes(ad))
        if n_ad >= 2:   # two adapters with a common start: they hit at one p wherever the first is planted
            adapters[1] = adapters[0][:max(1, len(adapters[0]) // 2)] + b"N"
            adapters[1] = adapters[1][:64]
        assert all(A.adapter_ok(ad) for ad in adapters)
        min_overlap = int(rng.integers(1, 9))
        err_den = int(rng.integers(1, 21))
        err_num = int(rng.integers(0, min(err_den, 4) + 1))
        reads = []
        for _ in range(28):
            L = int(rng.integers(0, 201))
            read = _rand_seq(rng, L)
            kind = int(rng.integers(0, 4))
            if kind and L:
                ad = adapters[int(rng.integers(0, n_ad))].replace(b"N", b"A").replace(b"n", b"c")
                p = int(rng.integers(0, L))
                planted = _mutate(rng, ad, int(rng.integers(0, 3)) if kind == 2 else 0)
                read = (read[:p] + planted + read[p:])[:L]   # the adapter may hang over the end
            reads.append(read)
        lens = [len(r) for r in reads]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64) + np.uint64(3)
        bases = np.frombuffer(b"..." + b"".join(reads), np.uint8)
        got = A.reads_adapter_np(bases, len(reads), 0, adapters, min_overlap, err_num, err_den, off)
        for r, read in enumerate(reads):
            want, at_p = brute_adapter_row(read, adapters, min_overlap, err_num, err_den)
            assert got[r].tolist() == want, (trial, r, got[r].tolist(), want)
            n_hit += bool(want[1])
            n_miss += not want[1]
            n_shared += len(at_p) >= 2
            if want[1]:
                n_overhang += ((want[1] >> 16) & 0xFFFF) < len(adapters[(want[1] & 0xFFFF) - 1])
    assert n_hit >= 20 and n_miss >= 20 and n_shared >= 1 and n_overhang >= 1, (n_hit, n_miss, n_shared, n_overhang)


def test_adapter_reference_uniform_layout_and_odd_reads():
    bases = np.frombuffer(b"ACGTAGATCGGAAGAGCTTTTTTTTAGATCGGAAG", np.uint8)
    got = A.reads_adapter_np(bases, 5, 7, [b"AGATCGGAAGAGC"], 3, 1, 10)
    for r in range(5):
        assert got[r].tolist() == brute_adapter_row(bytes(bases[7 * r:7 * r + 7]), [b"AGATCGGAAGAGC"], 3, 1, 10)[0]
    # a descending offsets pair counts as an empty read
    got = A.reads_adapter_np(bases, 2, 0, [b"AGAT"], 1, 0, 1, np.array([10, 4, 20], np.uint64))
    assert got[0].tolist() == [0, 0, 0, 0] and got[1, A.RA_BASES] == 16


def test_pair_reference_against_brute_force():
    rng = np.random.default_rng(2025)
    n_hit = n_miss = n_tie = n_neg = n_pos = 0
    for trial in range(5):
        min_overlap = int(rng.integers(1, 31))
        max_mism = int(rng.integers(0, 7))
        err_den = int(rng.integers(1, 21))
        err_num = int(rng.integers(0, min(err_den, 5) + 1))
        m1s, m2s = [], []
        for i in range(16):
            L1, L2 = int(rng.integers(0, 201)), int(rng.integers(0, 201))
            kind = i % 4
            if kind == 0:      # unrelated mates
                m1, m2 = _rand_seq(rng, L1), _rand_seq(rng, L2)
            elif kind == 1:    # a planted insert: both mates read one fragment, junk behind it
                ins = int(rng.integers(1, 260))
                frag = rng.choice(np.frombuffer(b"ACGT", np.uint8), ins).tobytes()
                m1 = (frag + _rand_seq(rng, 200))[:L1]
                m2 = (A.revcomp(frag) + _rand_seq(rng, 200))[:L2]
                m2 = _mutate(rng, m2, int(rng.integers(0, 4)))
            elif kind == 2:    # homopolymers: every shift hits
                m1, m2 = b"A" * L1, b"t" * L2
            else:              # a short period: many shifts hit, plateaus of n
                m1 = (b"ACG" * 70)[:L1]
                m2 = A.revcomp((b"ACG" * 70)[:L2])
            m1s.append(m1)
            m2s.append(m2)
        o1 = np.concatenate([[0], np.cumsum([len(m) for m in m1s])]).astype(np.uint64)
        o2 = np.concatenate([[0], np.cumsum([len(m) for m in m2s])]).astype(np.uint64) + np.uint64(5)
        b1 = np.frombuffer(b"".join(m1s), np.uint8)
        b2 = np.frombuffer(b"....." + b"".join(m2s), np.uint8)
        got = A.reads_pair_overlap_np(b1, b2, len(m1s), 0, 0, o1, o2, min_overlap, max_mism, err_num, err_den)
        for r in range(len(m1s)):
            want, ties = brute_pair_row(m1s[r], m2s[r], min_overlap, max_mism, err_num, err_den)
            assert got[r].tolist() == want, (trial, r, got[r].tolist(), want)
            n_hit += bool(want[0])
            n_miss += not want[0]
            n_tie += ties >= 2
            if want[0]:
                d = want[0] - len(m2s[r])
                n_neg += d < 0
                n_pos += d > 0
    assert n_hit >= 10 and n_miss >= 10 and n_tie >= 1 and n_neg >= 1 and n_pos >= 1, (n_hit, n_miss, n_tie, n_neg, n_pos)


def test_pair_reference_length_cap():
    m1 = b"ACGT" * 257   # 1028 bases
    m2 = A.revcomp(m1[:100])
    assert A.pair_row(np.frombuffer(m1, np.uint8), np.frombuffer(m2, np.uint8), 10, 0, 0, 1) == [0, 0, 1028 << 32, 100 << 32]
    assert A.pair_row(np.frombuffer(m1[:1024], np.uint8), np.frombuffer(m2, np.uint8), 10, 0, 0, 1)[0] > 0
