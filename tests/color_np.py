"""Host reference of the coloured-table calls (include/kmx.h): kmx_count_color_matrix and kmx_count_read_colors(2) as plain loops over
entries, reads and windows in Python integers, so one code serves one- and two-word keys.

* color_dict: the coloured table of a list of samples ({word: anything} dicts or sets, colour = list index) as a {word: mask} dict;
  table_arrays of tests/correct_np.py turns it into the arrays the device takes.
* color_matrix: (matrix (n_colors, n_colors), spectrum (n_colors + 1,)) of a sequence of masks.
* color_matrix_fast: the same through numpy bit unpacking and B.T @ B (float64, exact below 2^53), for the sizes the loop is too slow
  for; tests/test_color_np.py pins it against the loop.
* read_colors: the (n_reads, 8) rows and the (n_reads, n_colors) hit counts.  `mask_of` answers a canonical word's mask, unmasked:
  dict_count(color_dict(...)) of tests/correct_np.py does.
Only the low n_colors bits of a mask count, everywhere: the masked mask.

numpy only; needs no GPU and nothing of the package.
"""
import numpy as np

from tests.correct_np import windows_of

RC_N_VALID, RC_N_HIT, RC_N_UNIQUE, RC_ALL, RC_ANY, RC_THRESH, RC_BEST, RC_N_SWITCH = range(8)
RC_WORDS = 8


def color_dict(samples):
    """{word: mask}: bit i of a word's mask is set iff samples[i] holds the word"""
    out = {}
    for i, s in enumerate(samples):
        for key in s:
            out[key] = out.get(key, 0) | (1 << i)
    return out


def low_mask(n_colors):
    return (1 << n_colors) - 1


def color_matrix(masks, n_colors):
    cm = low_mask(n_colors)
    matrix = [[0] * n_colors for _ in range(n_colors)]
    spectrum = [0] * (n_colors + 1)
    for m in masks:
        m = int(m) & cm
        bits = [c for c in range(n_colors) if (m >> c) & 1]
        spectrum[len(bits)] += 1
        for i in bits:
            for j in bits:
                matrix[i][j] += 1
    return np.array(matrix, np.uint64).reshape(n_colors, n_colors), np.array(spectrum, np.uint64)


def color_matrix_fast(masks, n_colors):
    masks = np.ascontiguousarray(masks, np.uint64)
    B = np.unpackbits(masks.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")[:, :n_colors]
    Bf = B.astype(np.float64)
    matrix = (Bf.T @ Bf).astype(np.uint64).reshape(n_colors, n_colors)
    spectrum = np.bincount(B.sum(axis=1, dtype=np.int64), minlength=n_colors + 1).astype(np.uint64)
    return matrix, spectrum


def window_masks(read, k, mask_of, n_colors):
    """(valid, masked masks) per window of a read: the mask of an invalid window is 0"""
    fw, rc, valid = windows_of(read, k)
    cm = low_mask(n_colors)
    return valid, [mask_of(min(f, r)) & cm if v else 0 for f, r, v in zip(fw, rc, valid.tolist())]


def _colors_one(read, k, mask_of, n_colors, thr_num, thr_den):
    valid, masks = window_masks(read, k, mask_of, n_colors)
    hit = [m for m in masks if m != 0]
    n_valid = int(valid.sum())
    hits = [sum((m >> c) & 1 for m in hit) for c in range(n_colors)]
    all_, any_ = (low_mask(64) if hit else 0), 0
    for m in hit:
        all_ &= m
        any_ |= m
    thresh = sum(1 << c for c in range(n_colors) if hits[c] > 0 and hits[c] * thr_den >= thr_num * n_valid)
    best = 0
    if hit:
        top = max(hits)
        best = (top << 32) | hits.index(top)
    n_switch = sum(1 for p in range(len(masks) - 1) if masks[p] != 0 and masks[p + 1] != 0 and masks[p] != masks[p + 1])
    n_unique = sum(1 for m in hit if m & (m - 1) == 0)
    return (n_valid, len(hit), n_unique, all_, any_, thresh, best, n_switch), hits


def read_colors(host, n_reads, read_len, k, mask_of, n_colors, threshold=(1, 2), offsets=None):
    """-> ((n_reads, 8) uint64 rows, (n_reads, n_colors) uint32 hit counts).  offsets None: uniform reads of read_len; else read r is
    host[offsets[r]:offsets[r + 1]]"""
    rows = np.zeros((n_reads, RC_WORDS), np.uint64)
    hits = np.zeros((n_reads, n_colors), np.uint32)
    for r in range(n_reads):
        a, b = (r * read_len, (r + 1) * read_len) if offsets is None else (int(offsets[r]), int(offsets[r + 1]))
        row, h = _colors_one(host[a:b], k, mask_of, n_colors, int(threshold[0]), int(threshold[1]))
        rows[r] = np.array([int(x) for x in row], np.uint64)
        hits[r] = h
    return rows, hits


def interesting(rows):
    """what a table-driven test asserts of its own input: a read with ALL != ANY, one with N_SWITCH > 0, one with no hit, and one whose
    THRESH differs from both ALL and ANY -- a reference that produced only trivial rows could hide a failure"""
    rows = np.asarray(rows, np.uint64)
    return {"all_ne_any": bool((rows[:, RC_ALL] != rows[:, RC_ANY]).any()), "switch": bool((rows[:, RC_N_SWITCH] > 0).any()),
            "no_hit": bool((rows[:, RC_N_HIT] == 0).any()),
            "thresh_apart": bool(((rows[:, RC_THRESH] != rows[:, RC_ALL]) & (rows[:, RC_THRESH] != rows[:, RC_ANY])).any())}
