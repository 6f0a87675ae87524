"""tests/complexity_np.py (the host reference of kmx_reads_complexity) against brute force: literally the definitions of include/kmx.h,
loops over p, over letters, over windows and triplets, written without a look at the vectorised code.  Random reads over
ACGTacgtN with planted tails, heads and repeats, every L from 0 to 200, random thresholds; the batches are checked to hold tails
and heads, reads without either, both tie rules (an equal score at two lengths; two letters with an equal score), ends that meet,
an invalid byte inside a tail and inside a triplet of a repeat -- so the rules are exercised, not assumed.  The closed values of a
full window (1891, 930, 610) are asserted on both.  No GPU."""
import numpy as np

from tests import complexity_np as X

ALPHA = np.frombuffer(b"ACGTACGTACGTACGTacgtN", np.uint8)
UP = {ord(c): c.upper() for c in "acgtACGT"}


def brute_end(read, mask, min_len, num, den, penalty):
    """the tail of `read`: (t, bit + 1, the (score, length, bit) candidates that share the best score)"""
    L = len(read)
    best = None
    cands = []
    for x, X_ in enumerate("ACGT"):
        if not (mask >> x) & 1:
            continue
        best_x = None
        for p in range(L):
            if UP.get(read[p]) != X_:
                continue
            n = L - p
            m = sum(1 for i in range(p, L) if UP.get(read[i]) != X_)
            if n < min_len or m * den > num * n:
                continue
            s = n - (penalty + 1) * m
            cands.append((s, n, x))
            if best_x is None or s > best_x[0] or (s == best_x[0] and n > best_x[1]):
                best_x = (s, n, x)
        if best_x is not None and (best is None or best_x[0] > best[0] or (best_x[0] == best[0] and best_x[1] > best[1])):
            best = best_x
    if best is None:
        return 0, 0, []
    return best[1], best[2] + 1, [c for c in cands if c[0] == best[0]]


def brute_row(read, tail_bases, head_bases, min_len, num, den, penalty, dust_max):
    """-> (row, masked bytes, facts about the read for the coverage counters)"""
    L = len(read)
    t, tx, t_ties = brute_end(read, tail_bases, min_len, num, den, penalty)
    h, hx, h_ties = brute_end(read[::-1], head_bases, min_len, num, den, penalty)
    keep = 0 if h + t >= L else h | ((L - h - t) << 32)
    cnt = {c: 0 for c in "ACGT"}
    for b in read:
        if b in UP:
            cnt[UP[b]] += 1
    D = P = 0
    for i in range(L - 1):
        if read[i] in UP and read[i + 1] in UP:
            P += 1
            D += UP[read[i]] != UP[read[i + 1]]
    W = 0 if L == 0 else 1 if L <= 64 else (L - 64 + 31) // 32 + 1
    masked = bytearray(read)
    s_max = n_dusty = 0
    bad_triplet = False
    for j in range(W):
        lo, hi = 32 * j, min(32 * j + 64, L)
        c = {}
        for i in range(lo, hi - 2):
            tri = read[i:i + 3]
            if all(b in UP for b in tri):
                key = "".join(UP[b] for b in tri)
                c[key] = c.get(key, 0) + 1
            else:
                bad_triplet = True
        S = sum(v * (v - 1) // 2 for v in c.values())
        s_max = max(s_max, S)
        if S > dust_max:
            n_dusty += 1
            for i in range(lo, hi):
                masked[i] = ord("N")
    row = [keep, L, t | (tx << 32), h | (hx << 32), cnt["A"] | (cnt["C"] << 32), cnt["G"] | (cnt["T"] << 32), D | (P << 32),
           (s_max | (n_dusty << 32)) if L else 0]
    facts = dict(tail=t > 0, head=h > 0, meet=(h + t >= L and L > 0 and h > 0 and t > 0),
                 len_tie=any(len({c[1] for c in ties}) >= 2 for ties in (t_ties, h_ties)),
                 letter_tie=any(len({c[2] for c in ties}) >= 2 for ties in (t_ties, h_ties)),
                 tail_invalid=t > 0 and any(b not in UP for b in read[L - t:]), dusty=n_dusty, bad_triplet=bad_triplet and n_dusty > 0)
    return row, bytes(masked), facts


def _rand(rng, n):
    return rng.choice(ALPHA, n).astype(np.uint8).tobytes()


def _noisy(rng, seq, rate):
    s = bytearray(seq)
    for i in range(len(s)):
        if rng.random() < rate:
            s[i] = int(rng.choice(np.frombuffer(b"ACGTN", np.uint8)))
    return bytes(s)


def make_reads(rng, lens):
    """random reads; most get a planted tail, head or repeat (sometimes with errors or an invalid byte inside)"""
    reads = []
    for i, L in enumerate(lens):
        read = bytearray(_rand(rng, L))
        kind = i % 8
        x = "ACGTgt"[int(rng.integers(0, 6))].encode()
        if kind in (1, 2, 5) and L:     # a tail
            t = int(rng.integers(1, min(L, 70) + 1))
            read[L - t:] = _noisy(rng, x * t, 0.0 if kind == 1 else 0.08)
        if kind in (3, 5) and L:        # a head
            h = int(rng.integers(1, min(L, 70) + 1))
            read[:h] = _noisy(rng, x.swapcase() * h, 0.05)
        if kind == 4 and L:             # a whole read of one letter, or of two halves
            read[:] = x * L if rng.random() < 0.5 else (b"G" * (L // 2) + b"A" * (L - L // 2))
        if kind == 6 and L >= 10:       # a short tandem repeat somewhere, sometimes holding an invalid byte
            unit = [b"A", b"AC", b"ACG", b"ttg", b"ACGT"][int(rng.integers(0, 5))]
            n = int(rng.integers(10, L + 1))
            p = int(rng.integers(0, L - n + 1))
            rep = bytearray((unit * (n // len(unit) + 1))[:n])
            if rng.random() < 0.5:
                rep[int(rng.integers(0, n))] = ord("N")
            read[p:p + n] = rep
        if kind == 7 and L >= 20:       # two letters at the end: with penalty 0 their scores can tie
            read[L - 20:] = b"G" * 10 + b"A" * 10
        reads.append(bytes(read))
    return reads


def check(reads, params, counters, first=3):
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64) + np.uint64(first)
    bases = np.frombuffer(b"." * first + b"".join(reads), np.uint8)
    rows, masked = X.reads_complexity_np(bases, len(reads), 0, *params, offsets=off)
    assert masked[:first].tobytes() == b"." * first
    for r, read in enumerate(reads):
        want, want_m, facts = brute_row(read, *params)
        assert [int(w) for w in rows[r]] == want, (params, r, read, [int(w) for w in rows[r]], want)
        assert masked[int(off[r]):int(off[r + 1])].tobytes() == want_m, (params, r, read)
        for key, v in facts.items():
            counters[key] = counters.get(key, 0) + int(bool(v))
        counters["plain"] = counters.get("plain", 0) + (not facts["tail"] and not facts["head"])


def test_reference_against_brute_force():
    rng = np.random.default_rng(2026)
    counters = {}
    # every L from 0 to 200, at the defaults and at all letters on both ends
    lens = list(range(201))
    reads = make_reads(rng, lens)
    check(reads, (4, 0, 10, 1, 10, 2, 122), counters)
    check(reads, (15, 15, 10, 1, 10, 2, 122), counters)
    # random thresholds on random lengths; penalty 0 and a generous rate make the ties
    for trial in range(6):
        den = int(rng.integers(1, 13))
        num = int(rng.integers(0, min(den, 4) + 1))
        params = (int(rng.integers(0, 16)), int(rng.integers(0, 16)), int(rng.integers(1, 25)), num, den,
                  int(rng.choice([0, 0, 1, 2, 255])), int(rng.choice([0, 20, 60, 122, 929, 930, 1890, 1891])))
        check(make_reads(rng, rng.integers(0, 201, 48).tolist()), params, counters)
    check(make_reads(rng, rng.integers(0, 201, 64).tolist()), (15, 15, 5, 1, 2, 0, 122), counters)
    for key in ("tail", "head", "plain", "meet", "len_tie", "letter_tie", "tail_invalid", "dusty", "bad_triplet"):
        assert counters.get(key, 0) >= 1, (key, counters)
    assert counters["tail"] >= 40 and counters["head"] >= 20 and counters["plain"] >= 40, counters


def test_tie_rules_and_meeting_ends_by_hand():
    def row(read, *params):
        got = X.complexity_row(np.frombuffer(read, np.uint8), *params)[0]
        assert got == brute_row(read, *params)[0]
        return got

    # an equal score at two lengths: at penalty 1 the ten G score 10, and "GT" in front of them 12 - 2 * 1 = 10 as well: the longest
    r = row(b"TTTTGTGGGGGGGGGG", 4, 0, 5, 1, 2, 1, 1891)
    assert r[X.RX_TAIL] == 12 | (3 << 32) and r[X.RX_KEEP] == 0 | (4 << 32)
    # two letters with an equal score: G at n = 20, m = 10 (s = 10) and A at n = 10, m = 0 (s = 10): the longer, whatever the bit
    r = row(b"CCCCC" + b"G" * 10 + b"A" * 10, 15, 0, 5, 1, 1, 0, 1891)
    assert r[X.RX_TAIL] == 20 | (3 << 32)
    r = row(b"CCCCC" + b"A" * 10 + b"G" * 10, 15, 0, 5, 1, 1, 0, 1891)
    assert r[X.RX_TAIL] == 20 | (1 << 32)
    # ... and at penalty 2 the clean run wins
    r = row(b"CCCCC" + b"G" * 10 + b"A" * 10, 15, 0, 5, 1, 1, 2, 1891)
    assert r[X.RX_TAIL] == 10 | (1 << 32)
    # a head and a tail that meet, and that overlap: nothing is kept
    assert row(b"T" * 12 + b"G" * 12, 4, 8, 10, 0, 1, 2, 1891)[X.RX_KEEP] == 0
    assert row(b"A" * 30, 1, 1, 10, 0, 1, 2, 1891)[X.RX_KEEP:X.RX_HEAD + 1] == [0, 30, 30 | (1 << 32), 30 | (1 << 32)]
    assert row(b"T" * 12 + b"C" + b"G" * 12, 4, 8, 10, 0, 1, 2, 1891)[X.RX_KEEP] == 12 | (1 << 32)
    # both masks 0: the whole read; an empty read: a row of zeros
    assert row(b"G" * 30, 0, 0, 10, 1, 10, 2, 1891)[X.RX_KEEP] == 30 << 32
    assert row(b"", 15, 15, 1, 1, 1, 0, 0) == [0] * 8
    # an invalid byte inside a tail is a mismatch; lower case is a match
    assert row(b"ACAC" + b"GGGGGNgggggg", 4, 0, 10, 1, 10, 2, 1891)[X.RX_TAIL] == 12 | (3 << 32)
    assert row(b"ACAC" + b"GGGGGNNggggg", 4, 0, 10, 1, 10, 2, 1891)[X.RX_TAIL] == 0


def test_closed_window_values():
    for read, S in ((b"A" * 64, 1891), ((b"AC" * 32), 930), ((b"ACG" * 22)[:64], 610), (b"t" * 64, 1891)):
        for params in ((0, 0, 1, 0, 1, 0, S), (0, 0, 1, 0, 1, 0, S - 1)):
            row, masked = X.complexity_row(np.frombuffer(read, np.uint8), *params)
            want, want_m, _ = brute_row(read, *params)
            assert row == want and masked.tobytes() == want_m
            dusty = params[-1] < S
            assert row[X.RX_DUST] == S | (int(dusty) << 32) and masked.tobytes() == (b"N" * 64 if dusty else read)
    assert X.DUST_NEVER == 1891
    # the windows of a read: 65 bases are two, the second [32, 65); a triplet that holds an N is not counted
    assert [X.n_windows(L) for L in (0, 1, 64, 65, 96, 97, 128, 129, 150)] == [0, 1, 1, 2, 2, 3, 3, 4, 4]
    read = b"A" * 31 + b"N" + b"A" * 32
    row = X.complexity_row(np.frombuffer(read, np.uint8), 0, 0, 1, 0, 1, 0, 122)[0]
    assert row[X.RX_DUST] == (59 * 58 // 2) | (1 << 32) and row == brute_row(read, 0, 0, 1, 0, 1, 0, 122)[0]


def test_uniform_layout_and_odd_offsets():
    bases = np.frombuffer(b"ACGTGGGGGGGGGGGGTTTTTTTTTTTTACGTACGTGGGG", np.uint8)
    rows, masked = X.reads_complexity_np(bases, 5, 8, 4, 8, 4, 0, 1, 2, 3)
    for r in range(5):
        want, want_m, _ = brute_row(bytes(bases[8 * r:8 * r + 8]), 4, 8, 4, 0, 1, 2, 3)
        assert [int(w) for w in rows[r]] == want and masked[8 * r:8 * r + 8].tobytes() == want_m
    # a descending offsets pair counts as an empty read
    rows, _ = X.reads_complexity_np(bases, 2, 0, offsets=np.array([10, 4, 20], np.uint64))
    assert not rows[0].any() and rows[1, X.RX_BASES] == 16
