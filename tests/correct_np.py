"""Host reference of kmx_count_correct_reads(2): the rule of include/kmx.h as a plain loop over reads and positions.

* windows_of: the forward and reverse-complement words (Python integers, so one code serves one- and two-word keys) and the validity of
  every window of a read, spelled from its bytes.
* correct_reads: the corrected bytes and the (n_reads, 4) rows.  `count_of` answers a canonical word's count: dict_count(table) for a
  {word: count} dict (a count of 0 reads as absent), dict_count(table, membership=True) for d_counts == NULL.
* table_arrays / table_dict: a {word: count} dict as the sorted arrays the device takes ((n,) or (n, 2) uint64, rows (low, high)) and back.
* brute_correct: the same rule once more, every window spelled afresh from the substituted string: slow, an implementation of its own,
  what tests/test_correct_np.py pins correct_reads against.

numpy only; needs no GPU and nothing of the package.
"""
import numpy as np

_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i
LETTERS = b"ACGT"
M64 = (1 << 64) - 1


def windows_of(read, k):
    """(fw, rc, valid) per window of `read` (uint8 array): fw holds base w + i at bits [2i, 2i + 1], rc is its reverse complement
    (base w + i, complemented, at bits [2 (k - 1 - i), ...]); valid = no byte outside ACGTacgt in the window"""
    L = len(read)
    nw = max(L - k + 1, 0)
    fw, rc, valid = [0] * nw, [0] * nw, np.zeros(nw, bool)
    codes = _CODE[read]
    mask = (1 << (2 * k)) - 1
    f = r = 0
    last_bad = -1
    for i, c in enumerate(codes.tolist()):
        if c == 4:
            last_bad = i
            c = 0
        f = (f >> 2) | (c << (2 * k - 2))
        r = ((r << 2) | (3 - c)) & mask
        w = i - k + 1
        if w >= 0:
            fw[w], rc[w] = f, r
            valid[w] = i - last_bad >= k
    return fw, rc, valid


def dict_count(table, membership=False):
    if membership:
        return lambda key: 1 if key in table else 0
    return lambda key: table.get(key, 0)


def _correct_one(read, k, count_of, solid_min, min_cover, out):
    """one read: writes the corrected bytes into `out` (a copy of the read), returns its row"""
    L = len(read)
    nw = L - k + 1
    if nw <= 0:
        return (0, 0, 0, 0)
    fw, rc, valid = windows_of(read, k)
    solid = np.array([bool(valid[w]) and count_of(min(fw[w], rc[w])) >= solid_min for w in range(nw)], bool)
    weak = valid & ~solid
    codes = _CODE[read]
    n_cand = n_corr = n_amb = 0
    for p in range(L):
        if codes[p] == 4:
            continue
        lo, hi = max(0, p - k + 1), min(p, L - k)
        V = [w for w in range(lo, hi + 1) if valid[w]]
        if len(V) < min_cover or any(solid[w] for w in V):
            continue
        n_cand += 1
        fixing = []
        for a in range(4):
            if a == codes[p]:
                continue
            ok = True
            for w in V:
                i = p - w                                           # the base's place in window w
                f = (fw[w] & ~(3 << (2 * i))) | (a << (2 * i))
                j = k - 1 - i
                r = (rc[w] & ~(3 << (2 * j))) | ((3 - a) << (2 * j))
                if count_of(min(f, r)) < solid_min:
                    ok = False
                    break
            if ok:
                fixing.append(a)
        if len(fixing) == 1:
            n_corr += 1
            out[p] = LETTERS[fixing[0]] | (int(read[p]) & 0x20)
        elif len(fixing) >= 2:
            n_amb += 1
    return (int(weak.sum()), n_cand, n_corr, n_amb)


def correct_reads(host, n_reads, read_len, k, count_of, solid_min, min_cover, offsets=None):
    """-> (corrected copy of `host`, (n_reads, 4) uint64 rows).  offsets None: uniform reads of read_len; else read r is
    host[offsets[r]:offsets[r + 1]] and nothing outside [offsets[0], offsets[n_reads]) is touched"""
    out = host.copy()
    rows = np.zeros((n_reads, 4), np.uint64)
    for r in range(n_reads):
        a, b = (r * read_len, (r + 1) * read_len) if offsets is None else (int(offsets[r]), int(offsets[r + 1]))
        rows[r] = _correct_one(host[a:b], k, count_of, solid_min, min_cover, out[a:b])
    return out, rows


def word_of(s, k):
    """the forward word of the k bases s (bytes / str of ACGTacgt), spelled directly"""
    s = s.encode() if isinstance(s, str) else bytes(s)
    assert len(s) == k
    return sum(int(_CODE[c]) << (2 * i) for i, c in enumerate(s))


def canonical_of(s, k):
    s = s.encode() if isinstance(s, str) else bytes(s)
    comp = bytes(LETTERS[3 - int(_CODE[c])] for c in reversed(s))
    return min(word_of(s, k), word_of(comp, k))


def brute_correct(read, k, count_of, solid_min, min_cover):
    """the rule with every window spelled afresh from the substituted bytes -> (corrected bytes, row)"""
    read = bytes(read)
    L = len(read)
    out = bytearray(read)
    if L < k:
        return bytes(out), (0, 0, 0, 0)
    ok_byte = [c in b"ACGTacgt" for c in read]
    valid = [all(ok_byte[w:w + k]) for w in range(L - k + 1)]
    cnt = lambda s, w: count_of(canonical_of(s[w:w + k], k))
    solid = [valid[w] and cnt(read, w) >= solid_min for w in range(L - k + 1)]
    row = [sum(1 for w in range(L - k + 1) if valid[w] and not solid[w]), 0, 0, 0]
    for p in range(L):
        if not ok_byte[p]:
            continue
        V = [w for w in range(max(0, p - k + 1), min(p, L - k) + 1) if valid[w]]
        if len(V) < min_cover or any(solid[w] for w in V):
            continue
        row[1] += 1
        fixing = []
        for a in b"ACGT":
            if a == read[p] & 0xDF:
                continue
            s = read[:p] + bytes([a]) + read[p + 1:]
            if all(cnt(s, w) >= solid_min for w in V):
                fixing.append(a)
        if len(fixing) == 1:
            row[2] += 1
            out[p] = fixing[0] | (read[p] & 0x20)
        elif fixing:
            row[3] += 1
    return bytes(out), tuple(row)


def table_arrays(table, k):
    """{word: count} -> (keys, counts) as the device takes them: keys ascending as 2k-bit integers, (n,) uint64 for k <= 31,
    (n, 2) rows (low, high) above"""
    keys = sorted(table)
    tc = np.array([table[x] for x in keys], np.uint64)
    if k <= 31:
        return np.array(keys, np.uint64), tc
    tk = np.zeros((len(keys), 2), np.uint64)
    tk[:, 0] = [x & M64 for x in keys]
    tk[:, 1] = [x >> 64 for x in keys]
    return tk, tc


def count_kmers(host, n_reads, read_len, k, offsets=None, table=None):
    """{canonical word: occurrences} over the valid windows of a batch (added to `table` when given)"""
    table = {} if table is None else table
    for r in range(n_reads):
        a, b = (r * read_len, (r + 1) * read_len) if offsets is None else (int(offsets[r]), int(offsets[r + 1]))
        fw, rc, valid = windows_of(host[a:b], k)
        for w in np.nonzero(valid)[0].tolist():
            c = min(fw[w], rc[w])
            table[c] = table.get(c, 0) + 1
    return table


def revcomp_bytes(s):
    return np.frombuffer(bytes(LETTERS[3 - int(_CODE[c])] for c in reversed(bytes(s))), np.uint8)
