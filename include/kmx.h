/*
 * kmx.h -- C ABI of libkmx: the MI355X (gfx950) implementation of the streaming
 * 2-bit k-mer encode / canonicalise / hash hot path of COMBINE-lab/kmers.
 *
 * This header is the drop-in boundary.  The reference is a pure-Rust crate with
 * scalar per-k-mer calls; a GPU is a drop-in only at batch granularity, so every
 * entry point below is the batch restatement of one reference interface (cited
 * as file:line under /root/reference) with identical per-element results.
 * INTEGRATION.md shows the Rust `extern "C"` binding a maintainer would add.
 *
 * Conventions
 *   - plain C types only: pointers + sizes, no C++/torch types.
 *   - every `d_*` pointer is a DEVICE pointer valid on the ctx's GPU (from
 *     kmx_malloc, hipMalloc, or a torch CUDA tensor's data_ptr()).
 *   - all calls are asynchronous on the ctx's HIP stream unless stated; results
 *     are visible after kmx_ctx_synchronize() (or stream sync by the owner).
 *   - return value: KMX_OK or a KMX_E_* code; nothing ever unwinds across the ABI.
 *   - k-mer word layout (reference A.2): base i at bits [2i,2i+1], first base
 *     lowest; multi-word k-mers are little-endian by u64 word.
 */
#ifndef KMX_H
#define KMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMX_VERSION 2

/* ---- status codes (reference panics become codes; SURVEY 8b "Errors") ---- */
#define KMX_OK 0
#define KMX_E_ARG 1          /* null / inconsistent argument */
#define KMX_E_K_RANGE 2      /* k outside the supported domain of the call */
#define KMX_E_HIP 3          /* HIP runtime error; see kmx_last_error() */
#define KMX_E_INVALID_BASE 4 /* naive_impl::encode_binary panic (src/naive_impl/mod.rs:35) */
#define KMX_E_TOO_LONG 5     /* Kmer::from len>32 panic (src/naive_impl/kmer.rs:211-213,236-238); bit_field OOB in Encoding::encode */
#define KMX_E_NOMEM 6

/* ---- hashers (src/naive_impl/hash.rs) ---- */
#define KMX_HASH_NONE 0     /* no hash folded into the summary */
#define KMX_HASH_LEX 1      /* LexHasher{k}: hash.rs:22-72 */
#define KMX_HASH_IDENTITY 2 /* impl Hash for Kmer feeds write_u64(data) (hash.rs:4-8) into an identity hasher */

/* ---- MatchType (src/naive_impl/canonical_kmer.rs:7-12) ---- */
#define KMX_NO_MATCH 0
#define KMX_IDENTITY_MATCH 1
#define KMX_TWIN_MATCH 2

/* ---- per-window flags written by kmx_canonical_windows ---- */
#define KMX_WIN_VALID 1u        /* the iterator yields this position (no non-ACGTacgt byte in the window) */
#define KMX_WIN_FW_CANONICAL 2u /* CanonicalKmer::is_fw_canonical: fw < rc (canonical_kmer.rs:67-69) */

typedef struct kmx_ctx kmx_ctx;

/* A batch of reads resident in device memory.
 * offsets == NULL: uniform layout, read r = d_bases[r*read_len .. (r+1)*read_len).
 * offsets != NULL: ragged layout, read r = d_bases[offsets[r] .. offsets[r+1]) (n_reads+1 device u64); read_len may
 *   then carry an upper bound of the read lengths (0 = unknown): a bound <= 160 selects the smaller, faster frame of the
 *   tiled kernels, and the tighter it is the fewer windows a lane carries (150 bp reads: 7 % faster at k = 31 with 150
 *   than with 160 or 0).  Reads that are all of ONE length up to the bound (no bound: 160) -- untrimmed FASTQ -- are recognised on the
 *   device and take the uniform kernels whatever the bound says (round 5) in kmx_canonical_reduce (13 <= k <= 31, 16-byte aligned
 *   d_bases, a bound of at most 256, no KMX_REDUCE_SUM_FW) and in kmx_canonical_reduce2 (16-byte aligned d_bases, a bound of at most
 *   256); kmx_histogram, kmx_canonical_windows(2), kmx_minimizers and the Sum-fw reduce take such reads through their ragged kernels.
 *   It is only a hint -- tiles with a longer read take the exact per-read path, and the
 *   histogram's work buffer, sized from it, overflows into exact (slow) global atomics.  A bound ABOVE 256 says "long reads"
 *   (PacBio / ONT reads, contigs): kmx_canonical_reduce (13 <= k <= 31), kmx_canonical_reduce2, kmx_canonical_windows and
 *   kmx_canonical_windows2 (16-byte aligned d_bases) then cut every read into overlapping segments on the device and scan those (two
 *   host round trips: the batch's first and last offset, the number of segments; the segment arrays live in the context's work
 *   buffer); with 0 or a bound <= 256 a long read costs its tile the per-read path.  (kmx_canonical_reduce2 cuts ragged reads with
 *   any bound above 160 this way: the two-word ragged kernel holds 160 bases; with a bound of 161..256 it first reads the batch's
 *   first and last offset back -- one host round trip -- and skips the cut when they say "one length, k .. bound" -- untrimmed reads at
 *   the bound or below it; the device-side gate then confirms it, and the lane-per-read kernel counts if it does not.)
 *   EVERY call that takes one of these routes SYNCHRONISES the context's stream on the host (once or twice) and cannot be captured
 *   in a HIP graph; all other scan calls only enqueue work.
 * d_bases must be a device pointer whenever n_reads > 0, also when every read is empty (KMX_E_ARG otherwise). */
typedef struct {
    const uint8_t *d_bases;
    uint64_t n_reads;
    uint32_t read_len;
    const uint64_t *d_offsets;
} kmx_reads;
/* Limits: a single read is shorter than 2^31 bases (the iterator's positions are i32 in the reference as well,
 * canonical_kmer_iterator.rs:15); offsets and totals are 64-bit.  A ragged read of 2^31 bases or more -- e.g. a whole
 * chromosome out of kmx_fastx_parse's FASTA mode -- is DIAGNOSED, not scanned: the scan kernels skip it (it contributes no
 * window) and raise a sticky flag on the context, the next kmx_ctx_synchronize returns KMX_E_ARG with the text in
 * kmx_last_error and clears the flag; kmx_reads_length_range returns KMX_E_ARG for such a batch right away.  Cut such
 * records into overlapping pieces first (k - 1 bases of overlap, or hand the bytes over as uniform reads: reads longer
 * than 256 bases are scanned as overlapping segments by the tiled kernel, every k from 13 to 64).  Uniform reads may start at any byte address; ragged reads need a
 * 16-byte-aligned d_bases for the tiled kernels (any address is served, by the per-read kernel). */

/* Result of a streaming reduce pass (device-resident, 32 bytes).
 * == what a consumer loop over CanonicalKmerIterator accumulates
 * (src/naive_impl/canonical_kmer_iterator.rs:42-116; benches/simple_benchmark.rs:14-22 `.sum()` shape). */
typedef struct {
    uint64_t n_valid;   /* windows yielded */
    uint64_t sum_canon; /* wrapping sum of get_canonical_word() (canonical_kmer.rs:113-119) */
    uint64_t xor_hash;  /* xor of hash_one(hasher, canonical kmer) (hash.rs:10-20); 0 for KMX_HASH_NONE */
    uint64_t sum_fw;    /* wrapping sum of get_fw_word() == compute_naive on valid input; 0 unless KMX_REDUCE_SUM_FW */
} kmx_summary;

/* [u64;2] k-mers (k in 33..64), BUILD-DEFINED extension of the above */
typedef struct {
    uint64_t n_valid;
    uint64_t sum_lo, sum_hi;
    uint64_t xor_lo, xor_hi;
} kmx_summary2;

#define KMX_REDUCE_SUM_FW 1u /* also accumulate sum_fw */

/* ------------------------------------------------------------ context ---- */
int kmx_ctx_create(int device, kmx_ctx **out);                 /* owns a new non-blocking stream */
int kmx_ctx_create_on_stream(int device, void *hip_stream, kmx_ctx **out); /* borrows the caller's hipStream_t (NULL = default stream) */
void kmx_ctx_destroy(kmx_ctx *ctx);
int kmx_ctx_synchronize(kmx_ctx *ctx);                         /* also reports what the asynchronous scans could not: KMX_E_ARG after a read of >= 2^31 bases was skipped */
int kmx_ctx_device(const kmx_ctx *ctx);
/* The context owns ONE grow-only device work buffer (bucket-id streams of kmx_histogram above 2^14 buckets, chunk prefixes of
 * kmx_fastx_parse, the segment arrays of reads longer than 256 bases: 16-24 bytes per segment of <= 226 windows); the histogram
 * processes its reads in as many chunks as it takes, a batch of long reads whose segment arrays do not fit under a limit set
 * here takes the per-read kernels instead (same results, a tenth of the rate).  Its size is chosen per call -- an eighth of the device
 * memory, at most half of what is free -- unless a limit is set here (bytes; 0 = automatic again).  A server that shares the
 * device caps it; a small limit forces the chunked paths. */
int kmx_ctx_set_work_buffer_limit(kmx_ctx *ctx, size_t bytes);
/* what the context holds now, and how often the buffer has been (re)allocated since kmx_ctx_create (either pointer may be NULL) */
int kmx_ctx_work_buffer_info(const kmx_ctx *ctx, size_t *bytes_held, uint64_t *n_allocations);
const char *kmx_strerror(int status);
const char *kmx_last_error(const kmx_ctx *ctx); /* text of the last HIP failure on this ctx */
int kmx_version(void);

/* device memory helpers so a host language needs no HIP binding of its own */
int kmx_malloc(kmx_ctx *ctx, size_t nbytes, void **d_out);
int kmx_free(kmx_ctx *ctx, void *d_ptr);
int kmx_memcpy_h2d(kmx_ctx *ctx, void *d_dst, const void *h_src, size_t nbytes); /* synchronous */
int kmx_memcpy_d2h(kmx_ctx *ctx, void *h_dst, const void *d_src, size_t nbytes); /* synchronous */
int kmx_memset(kmx_ctx *ctx, void *d_dst, int value, size_t nbytes);

/* ------------------------------------------- the streaming hot path ---- */

/* Replaces: CanonicalKmerIterator::{from_u8_slice,find_next,inc,get} over every read
 * (src/naive_impl/canonical_kmer_iterator.rs:42-116) + CanonicalKmer::append_base /
 * get_canonical_word (canonical_kmer.rs:90-94,113-119) + Kmer::{append,prepend}_base
 * (kmer.rs:91-102) + encode_binary_u8 (mod.rs:40-50) + optional hash_one (hash.rs:10-20).
 * k in [1,31] (the reference's MASK_TABLE[32]==0, kmer.rs:617, breaks its own rolling at k=32).
 * hasher: KMX_HASH_*; hasher_k: LexHasher's k (usually == k), ignored otherwise.
 * d_out is OVERWRITTEN with this batch's summary. */
int kmx_canonical_reduce(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, uint32_t hasher, uint32_t hasher_k,
                         uint32_t flags, kmx_summary *d_out);
/* The same pass with xor_hash = the xor of SipHash-1-3(key0, key1; the 8 little-endian bytes of the canonical word) -- std's
 * DefaultHasher (key0 = key1 = 0) or a RandomState (its two keys) fed hash_one(state, kmer) (hash.rs:4-20): the hash of
 * kmx_hash_words_sip13.  n_valid, sum_canon and sum_fw are those of kmx_canonical_reduce on the same input; domain, layouts,
 * KMX_REDUCE_SUM_FW and codes as there.  Uniform and ragged reads of up to 256 bases (2 <= k <= 31, 16-byte aligned d_bases for
 * ragged reads) take the tiled word-domain scan; k = 1, longer reads and a misaligned ragged d_bases a lane per read -- correct,
 * but a batch of long reads then runs at the rate of its longest lanes (no segment cut here).  Bound by VALU work (five SipRounds,
 * ~110 instructions per window), not by HBM: 0.31e12 k-mers/s on 150 bp reads at k = 31, 2 % dirty 0.28e12 (Lex: ~5e12;
 * profiles/r07_sip13_bench.txt).  Asynchronous; d_out OVERWRITTEN. */
int kmx_canonical_reduce_sip13(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, uint64_t key0, uint64_t key1,
                               uint32_t flags, kmx_summary *d_out);

/* The same call with its answer in HOST memory when it returns (round 6): what a caller that reduces one small
 * batch at a time -- the reference's iterator over one read set, canonical_kmer_iterator.rs:42-116 -- pays is
 * the launch and the wait, not the bytes.  Uniform reads of up to 256 bases, k in [9,31], hasher NONE or
 * LEX(hasher_k == k): ONE kernel launch whose last block writes the summary to pinned host words this call
 * watches (1e5 reads of 150 bases: ~25 us against ~70 us for kmx_canonical_reduce + kmx_memcpy_d2h); a batch
 * with invalid bytes adds the sweep and a copy.  Every other input: kmx_canonical_reduce + the copy.
 * `reads` in device memory as always; *h_out is OVERWRITTEN.  Synchronous on the context's stream. */
int kmx_canonical_reduce_host(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, uint32_t hasher, uint32_t hasher_k,
                              uint32_t flags, kmx_summary *h_out);

/* Same pass, materialising per-window state: slot(read r, pos p) = win_off(r) + p with
 * win_off(r) = r*(read_len-k+1) (uniform) or d_win_offsets[r] (ragged; n_reads+1 device u64,
 * exclusive prefix sum of max(len-k+1,0)).  Any of the four outputs may be NULL.
 * d_fw/d_rc/d_canon: get_fw_word / get_rc_word / get_canonical_word of the iterator state at
 * that pos (canonical_kmer.rs:113-139); invalid slots are written as 0 with flags 0. */
int kmx_canonical_windows(kmx_ctx *ctx, const kmx_reads *reads, const uint64_t *d_win_offsets, uint32_t k,
                          uint64_t *d_fw, uint64_t *d_rc, uint64_t *d_canon, uint8_t *d_flags);

/* BUILD-DEFINED [u64;2] variants, k in [33,64] (word_for_k::<u64,K>() == 2, src/kmer.rs:67-69):
 * rolling = kmer.rs:91-102 carried across words, order = 2K-bit little-endian integer,
 * hash = 2-bit-group reversal of the 2K-bit value.  Outputs are 2 u64 per slot. */
int kmx_canonical_reduce2(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, uint32_t with_hash, kmx_summary2 *d_out);
int kmx_canonical_windows2(kmx_ctx *ctx, const kmx_reads *reads, const uint64_t *d_win_offsets, uint32_t k,
                           uint64_t *d_fw2, uint64_t *d_rc2, uint64_t *d_canon2, uint8_t *d_flags);

/* Per-bucket occupancy of hash(canonical k-mer): d_counts[bucket] += 1 for every yielded window;
 * bucket = (uint32_t)(lo32(hash) * 0x9E3779B1 + hi32(hash) * 0x85EBCA6B) >> (32 - log2_buckets)  (BUILD-DEFINED bucket
 * function: the top bits of a 32-bit multiplicative mix of the two halves; log2_buckets <= 30).
 * d_counts (2^log2_buckets device u64) is ACCUMULATED into; the caller zeroes it and, across
 * GPUs, all-reduces it (RCCL ncclSum/uint64).
 * With 2^15..2^22 buckets the reads (uniform or ragged) go through a grow-only work buffer owned by the context (sized to
 * the call: 3 bytes per window, at most an eighth of the device memory -- 8 GiB if that is more -- and at most half of
 * what is free; kmx_ctx_set_work_buffer_limit overrides): growing it synchronises the stream once. */
int kmx_histogram(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, uint32_t hasher, uint32_t hasher_k,
                  uint32_t log2_buckets, uint64_t *d_counts);
/* The same histogram of the SipHash-1-3(key0, key1) hash of the canonical word (as kmx_canonical_reduce_sip13), same bucket function,
 * ACCUMULATED into d_counts, through the routes of kmx_histogram: block-private LDS tables up to 2^14 buckets, the partitioned
 * passes through the context's work buffer for 2^15..2^28 (one level up to 2^22, two above), device atomics where there is no
 * scratch or above 2^28, a lane per read outside the scan's domain.  Bound by VALU work (the hash), not by HBM: 0.31e12 k-mers/s at
 * 2^10 buckets, 0.115e12 at 2^20 on 150 bp reads at k = 31 (profiles/r07_sip13_bench.txt). */
int kmx_histogram_sip13(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, uint64_t key0, uint64_t key1,
                        uint32_t log2_buckets, uint64_t *d_counts);

/* ---------------------------------------------------------------- exact k-mer counting ----
 * Exact count of the canonical k-mers of a batch (BUILD-DEFINED: the reference crate has no counter; the result is the multiset
 * CanonicalKmerIterator yields, canonical_kmer_iterator.rs:42-116, of get_canonical_word(), canonical_kmer.rs:113-119):
 * d_kmers[i] = the i-th distinct canonical word in ASCENDING order, d_counts[i] = how many windows yield it (u64, as kmx_histogram).
 * Windows holding a byte outside ACGTacgt are skipped as the iterator skips them (no error).  k in [1,31]; every input
 * kmx_canonical_windows accepts (uniform reads of any length, ragged reads with any bound, any d_bases alignment).  The table is
 * deterministic: the same input gives bit-identical output on every run.
 * *h_n_distinct (host) = the number of distinct k-mers.  If it exceeds max_distinct nothing is written, KMX_E_NOMEM is returned and
 * *h_n_distinct is set (the convention of kmx_fastx_parse's max_reads); with d_kmers == d_counts == NULL only the count is computed.
 * Working set: the call's arrays live in the context's work buffer (kmx_ctx_set_work_buffer_limit) -- at most 20 bytes per window
 * + 1 MiB (uniform reads: windows = n_reads * (read_len - k + 1); ragged reads: the batch's number of BASES stands for the windows,
 * plus 9 bytes per read), and reads longer than 256 bases add their segment plan (24 bytes per segment of at most 257 - k windows).
 * A batch above the cap (the automatic one: an eighth of the device memory, at least 8 GiB, at most half of what is free) returns
 * KMX_E_NOMEM BEFORE any kernel runs and writes nothing.  Split larger inputs into batches and combine their tables with
 * kmx_count_merge: at k = 31 a 150 bp read has 120 windows (2400 bytes), so 3.5e6 such reads fit the 8 GiB floor of the automatic
 * cap and 1.5e7 fit it on a device of 288 GB.  The call uses the work buffer: a following kmx_fastx_parse cannot reuse its chunk
 * prefixes (KMX_FASTX_SAME_TEXT is then ignored).
 * Synchronous (the count comes back to the host; one host round trip per 8 bits of key that a partition still needs, at most
 * ceil(2k / 8), plus two or three): not capturable in a HIP graph. */
int kmx_count_canonical(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, uint64_t *d_kmers, uint64_t *d_counts,
                        uint64_t max_distinct, uint64_t *h_n_distinct);
/* Union of two count tables as kmx_count_canonical writes them (ascending, distinct): equal k-mers are merged and their counts
 * added.  Same max_out / KMX_E_NOMEM / NULL-output convention; *h_n_out = the number of distinct k-mers of the union.  Outputs must
 * not alias inputs.  Working set in the work buffer: 16 bytes per input entry + 1 MiB.  Synchronous. */
int kmx_count_merge(kmx_ctx *ctx, const uint64_t *d_kmers_a, const uint64_t *d_counts_a, uint64_t n_a, const uint64_t *d_kmers_b,
                    const uint64_t *d_counts_b, uint64_t n_b, uint64_t *d_kmers_out, uint64_t *d_counts_out, uint64_t max_out,
                    uint64_t *h_n_out);

/* The same count for [u64;2] k-mers, k in [33,64] (k = 32 stays unsupported, as everywhere): the multiset kmx_canonical_windows2
 * yields.  d_kmers2[2i], d_kmers2[2i+1] = low and high word of the i-th distinct canonical k-mer (the slot layout of
 * kmx_canonical_windows2), ASCENDING as a 2k-bit unsigned integer -- high word first, then low, the order of [u64;2] above;
 * d_counts[i] = how many windows yield it (u64).  Windows without KMX_WIN_VALID are skipped.  Every input kmx_canonical_windows2
 * accepts is accepted (uniform reads of any length, ragged reads with any bound -- the window offsets are made on the device --, any
 * d_bases alignment, invalid bytes, lower case).  Deterministic: bit-identical tables on repeated calls.
 * d_kmers2 holds 2 * max_distinct u64 and must be 16-byte aligned (keys are moved as 16-byte elements; KMX_E_ARG otherwise).
 * *h_n_distinct, max_distinct / KMX_E_NOMEM with nothing written, both outputs NULL = count only, one NULL = KMX_E_ARG: as
 * kmx_count_canonical.
 * Working set in the context's work buffer: at most 36 bytes per window + 1 MiB (16 canonical words, 1 flags, 16 keys, 1 mark,
 * ~1.35 partition arrays; uniform reads: windows = n_reads * (read_len - k + 1); ragged reads: the batch's number of BASES stands
 * for the windows, plus 9 bytes per read), and reads longer than 256 bases add their segment plan (24 bytes per segment of at most
 * 257 - k windows).  A batch above the cap returns KMX_E_NOMEM BEFORE any kernel runs and writes nothing.  Split larger inputs and
 * combine their tables with kmx_count_merge2: at k = 47 a 150 bp read has 104 windows (3744 bytes), so 2.2e6 such reads fit the
 * 8 GiB floor of the automatic cap and 9.6e6 fit it on a device of 288 GB.  The call uses the work buffer (a following
 * kmx_fastx_parse cannot reuse its chunk prefixes).
 * Synchronous (one host round trip per 8 bits of key that a partition still needs, at most ceil(2k / 8) = 16, plus two or three;
 * random reads need as many as at k = 31: the number of levels follows the number of keys, not k): not capturable in a HIP graph. */
int kmx_count_canonical2(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, uint64_t *d_kmers2, uint64_t *d_counts,
                         uint64_t max_distinct, uint64_t *h_n_distinct);
/* Union of two tables as kmx_count_canonical2 writes them (2 u64 per key, ascending, distinct; 16-byte aligned key arrays): equal
 * k-mers are merged and their counts added.  Conventions of kmx_count_merge; outputs must not alias inputs.  Working set in the work
 * buffer: 24 bytes per input entry + 1 MiB.  Synchronous. */
int kmx_count_merge2(kmx_ctx *ctx, const uint64_t *d_kmers2_a, const uint64_t *d_counts_a, uint64_t n_a, const uint64_t *d_kmers2_b,
                     const uint64_t *d_counts_b, uint64_t n_b, uint64_t *d_kmers2_out, uint64_t *d_counts_out, uint64_t max_out,
                     uint64_t *h_n_out);

/* ---------------------------------------------------------------- the counting sketch ----
 * BUILD-DEFINED (the reference crate has no approximate structure).  A small approximate counter that every batch of a large input
 * is added to, so that the exact counter then only has to hold the k-mers that can be solid: kmx_count_canonical_min(2) counts the
 * windows whose estimate reaches a threshold, and over any number of batches
 *     merge of kmx_count_canonical_min(batch, min_est = m), filtered with kmx_count_filter(min_count = m)
 *  == kmx_count_filter(count of all batches together, min_count = m)        (1 <= m <= 255), key for key and count for count,
 * because an estimate is never below the true total (clipped to 255) -- the sketch only lets too MANY windows through, and the final
 * filter removes those.
 *
 * LAYOUT.  A blocked count-min sketch of saturating 8-bit cells in caller-owned device memory: d_sketch holds 64 << log2_blocks
 * bytes, 64-byte aligned, 0 <= log2_blocks <= 32 (KMX_E_ARG otherwise), zeroed by the caller and ACCUMULATED into, as kmx_histogram
 * accumulates into d_counts.  A block is 64 bytes -- 4 rows of 16 cells, one cache line.  A key touches exactly one block and exactly
 * one cell in each of its rows: the four cells of a key are always four distinct bytes.
 * KEY HASH.  One definition for both widths: a one-word key is (lo = the canonical word, hi = 0), a two-word key the (lo, hi) pair
 * of the slot layout of kmx_canonical_windows2.  Arithmetic mod 2^64, fmix64 = the murmur3 64-bit finaliser (x ^= x >> 33;
 * x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33):
 *     h     = fmix64(lo ^ fmix64(hi + seed + 0x9e3779b97f4a7c15))
 *     block = log2_blocks ? h >> (64 - log2_blocks) : 0
 *     the cell of row j (0..3) is byte  64 * block + 16 * j + ((h >> (4 * j)) & 15)  of d_sketch.
 * ADD.  Adding weight w to a key sets each of its four cells to min(255, cell + min(w, 255)).  Saturating adds commute: after any
 * set of adds in any order a cell holds min(255, the sum of the weights that hit it).  That is the whole determinism contract --
 * repeated calls, other streams and other launch shapes give identical bytes, and a host model reproduces the sketch exactly.
 * ESTIMATE.  The estimate of a key is the minimum of its four cells: >= min(255, the key's true total weight), never less.  Hence
 * every k-mer that occurs at least m <= 255 times in all that was added has an estimate >= m.
 * Argument checks, KMX_E_K_RANGE (k in [1,31]; the calls named ...2: k in [33,64], two-word keys 16-byte aligned) and the behaviour
 * on empty input (n == 0, n_reads == 0, no window: nothing is touched; d_sketch may then be NULL) follow the count family.  A NULL
 * d_sketch with work to do, one that is not 64-byte aligned, or log2_blocks > 32: KMX_E_ARG. */

/* Adds n keys as they are (a table's keys with its counts as weights, or the canon array of kmx_canonical_windows): key i with weight
 * d_weights[i] (u64; clipped to 255; 0 adds nothing), or 1 each with d_weights == NULL.  n up to 2^40.  No working set; asynchronous:
 * it only enqueues work on the context's stream. */
int kmx_sketch_add_words(kmx_ctx *ctx, const uint64_t *d_words, const uint64_t *d_weights, uint64_t n, uint8_t *d_sketch,
                         uint32_t log2_blocks, uint64_t seed);
int kmx_sketch_add_words2(kmx_ctx *ctx, const uint64_t *d_words2, const uint64_t *d_weights, uint64_t n, uint8_t *d_sketch,
                          uint32_t log2_blocks, uint64_t seed);
/* Adds weight 1 for every window of the batch that kmx_canonical_windows(2) marks KMX_WIN_VALID: kmx_sketch_add_words(2) over the
 * canon / flags of that call.  Every input those calls take is taken (uniform reads of any length, ragged reads with any bound --
 * the window offsets are made on the device --, any d_bases alignment, invalid bytes, lower case, reads above 256 bases).
 * Working set in the context's work buffer: 9 bytes per window (add2: 17; windows counted as for kmx_count_canonical: uniform reads
 * n_reads * (read_len - k + 1), ragged reads the batch's number of BASES plus 9 bytes per read), each array rounded up to 256, and
 * the segment plan of reads above 256 bases.  Above the cap: KMX_E_NOMEM BEFORE any kernel runs, the sketch untouched.  Ragged
 * reads bring two words back to the host (the span of the offsets, the number of windows); otherwise asynchronous. */
int kmx_sketch_add(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, uint8_t *d_sketch, uint32_t log2_blocks, uint64_t seed);
int kmx_sketch_add2(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, uint8_t *d_sketch, uint32_t log2_blocks, uint64_t seed);
/* d_est[i] (one byte) = the estimate of key i.  No working set; asynchronous. */
int kmx_sketch_lookup(kmx_ctx *ctx, const uint64_t *d_words, uint64_t n, const uint8_t *d_sketch, uint32_t log2_blocks, uint64_t seed,
                      uint8_t *d_est);
int kmx_sketch_lookup2(kmx_ctx *ctx, const uint64_t *d_words2, uint64_t n, const uint8_t *d_sketch, uint32_t log2_blocks, uint64_t seed,
                       uint8_t *d_est);
/* One byte per window slot, in the slot layout of kmx_canonical_windows(2) (r * (read_len - k + 1) + p, or d_win_offsets[r] + p;
 * ragged reads need their d_win_offsets): the estimate of the window's canonical k-mer, 0 for a window without KMX_WIN_VALID.  It IS
 * the windows call followed by the lookup, as kmx_count_lookup_reads(2) is, with that call's inputs, routes and synchronisation.
 * Working set: 9 (17) bytes per window, counted and refused as for kmx_sketch_add. */
int kmx_sketch_lookup_reads(kmx_ctx *ctx, const kmx_reads *reads, const uint64_t *d_win_offsets, uint32_t k, const uint8_t *d_sketch,
                            uint32_t log2_blocks, uint64_t seed, uint8_t *d_est);
int kmx_sketch_lookup_reads2(kmx_ctx *ctx, const kmx_reads *reads, const uint64_t *d_win_offsets, uint32_t k, const uint8_t *d_sketch,
                             uint32_t log2_blocks, uint64_t seed, uint8_t *d_est);
/* d_out = cellwise min(255, a + b) of two sketches of the same log2_blocks; d_out may be d_a or d_b.  Sketches of disjoint batches
 * built with the same seed and size merge into the sketch of their union, bit for bit -- the law that lets batches, streams and ranks
 * each fill a sketch of their own.  No working set; asynchronous. */
int kmx_sketch_merge(kmx_ctx *ctx, const uint8_t *d_a, const uint8_t *d_b, uint32_t log2_blocks, uint8_t *d_out);
/* d_hist[v] += the number of cells that hold v: 256 u64, ACCUMULATED into (the caller zeroes).  1 - d_hist[0] / cells, the share of
 * non-zero cells, is what a caller sizes the sketch by.  Integer atomics: deterministic.  No working set; asynchronous. */
int kmx_sketch_stats(kmx_ctx *ctx, const uint8_t *d_sketch, uint32_t log2_blocks, uint64_t *d_hist);
/* kmx_count_canonical(2) restricted to the windows whose estimate in the sketch is >= min_est: between the windows call and the sort
 * one kernel clears KMX_WIN_VALID of every other window.  Everything else is kmx_count_canonical(2)'s: order, max_distinct /
 * KMX_E_NOMEM with nothing written, both outputs NULL = count only, working set, synchrony.  min_est <= 1 on a sketch that has seen
 * the batch gives the unfiltered table (min_est == 0 does not read the sketch); min_est > 255 gives the empty table. */
int kmx_count_canonical_min(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, const uint8_t *d_sketch, uint32_t log2_blocks,
                            uint64_t seed, uint32_t min_est, uint64_t *d_kmers, uint64_t *d_counts, uint64_t max_distinct,
                            uint64_t *h_n_distinct);
int kmx_count_canonical_min2(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, const uint8_t *d_sketch, uint32_t log2_blocks,
                             uint64_t seed, uint32_t min_est, uint64_t *d_kmers2, uint64_t *d_counts, uint64_t max_distinct,
                             uint64_t *h_n_distinct);

/* ---------------------------------------------------------------- the distinct-key estimator ----
 * BUILD-DEFINED.  HOW MANY distinct canonical k-mers an input holds, from one streaming pass and before anything is counted: the
 * number a caller sizes a sketch (log2_blocks), a table (max_distinct) or a merge by, and -- from the registers of two samples -- a
 * first look at their Jaccard index and containment without either exact table.  A HyperLogLog: 2^p byte registers, each a maximum.
 *
 * REGISTERS.  Caller-owned device memory: d_regs holds 1 << log2_regs bytes, 16-byte aligned, 4 <= log2_regs <= 24 (KMX_E_ARG
 * otherwise), zeroed by the caller and ACCUMULATED into.
 * HASH.  The key hash of the counting sketch above, the same definition: h = fmix64(lo ^ fmix64(hi + seed + 0x9e3779b97f4a7c15)),
 * hi = 0 for a one-word key.
 * UPDATE.  With p = log2_regs, adding a key does
 *     idx  = h >> (64 - p)
 *     w    = h << p
 *     rank = min(clz64(w), 64 - p) + 1          (1 .. 65 - p; w == 0 gives 65 - p)
 *     regs[idx] = max(regs[idx], rank)
 * A maximum commutes and is idempotent.  That is the whole determinism contract -- repeated calls, other streams and other launch
 * shapes give identical bytes, adding the same keys again changes nothing, and a host model reproduces the registers exactly.  The
 * bytewise maximum of two register arrays of one size and seed IS the register array of the union of what they saw.
 * ESTIMATE.  A function of the 64 bins of kmx_hll_stats alone, computed on the host in double precision: the device never touches a
 * float.  Ertl's improved estimator (arXiv:1702.01284) -- no bias table, no empirical switch between ranges.  With m = 2^p,
 * q = 64 - p and bins C[0 .. q + 1] (C[v] = the number of registers that hold v):
 *     z = m * tau(1 - C[q + 1] / m)
 *     for j = q down to 1:  z = (z + C[j]) / 2
 *     z += m * sigma(C[0] / m)
 *     E = m * m / (2 ln 2) / z
 *     sigma(x): x == 1 -> infinity;  y = 1, z = x;  repeat { x *= x; z0 = z; z += x * y; y += y } until z == z0;  return z
 *     tau(x):   x == 0 or x == 1 -> 0;  y = 1, z = 1 - x;
 *               repeat { x = sqrt(x); z0 = z; y /= 2; z -= (1 - x)^2 * y } until z == z0;  return z / 3
 * All registers zero gives E = 0.  The relative standard error is about 1.04 / sqrt(m).  kmx::hll_estimate (kmx.hpp),
 * kmers_amd.api.hll_estimate and kmers_hip::hll_estimate implement exactly this.
 * Argument checks, KMX_E_K_RANGE (k in [1,31]; the calls named ...2: k in [33,64], two-word keys 16-byte aligned) and the behaviour
 * on empty input (n == 0, n_reads == 0, no window: nothing is touched; d_regs may then be NULL) follow kmx_sketch_*.  A NULL d_regs
 * with work to do, one that is not 16-byte aligned, or log2_regs outside [4, 24]: KMX_E_ARG. */

/* Adds n keys as they are (a table's keys, or the canon array of kmx_canonical_windows).  n up to 2^40.  No working set;
 * asynchronous: it only enqueues work on the context's stream. */
int kmx_hll_add_words(kmx_ctx *ctx, const uint64_t *d_words, uint64_t n, uint8_t *d_regs, uint32_t log2_regs, uint64_t seed);
int kmx_hll_add_words2(kmx_ctx *ctx, const uint64_t *d_words2, uint64_t n, uint8_t *d_regs, uint32_t log2_regs, uint64_t seed);
/* Adds every window of the batch that kmx_canonical_windows(2) marks KMX_WIN_VALID: kmx_hll_add_words(2) over the canon / flags of
 * that call.  Inputs, working set (9 bytes per window, add2: 17), KMX_E_NOMEM before any kernel runs with the registers untouched,
 * and synchrony are exactly those of kmx_sketch_add(2). */
int kmx_hll_add(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, uint8_t *d_regs, uint32_t log2_regs, uint64_t seed);
int kmx_hll_add2(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, uint8_t *d_regs, uint32_t log2_regs, uint64_t seed);
/* d_out = bytewise max(a, b) of two register arrays of the same log2_regs; d_out may be d_a or d_b.  Arrays built with the same
 * seed merge into the registers of the union of their inputs, bit for bit, whether or not the inputs overlap.  No working set;
 * asynchronous. */
int kmx_hll_merge(kmx_ctx *ctx, const uint8_t *d_a, const uint8_t *d_b, uint32_t log2_regs, uint8_t *d_out);
/* d_hist[v] += the number of registers of d_a that hold v: 64 u64, ACCUMULATED into (the caller zeroes); a byte above 63, which no
 * call writes, is counted in bin 63.  With d_b != NULL d_hist holds 192 words: the 64 bins of a, the 64 of b and the 64 of
 * max(a, b) -- the registers of the union -- so a comparison of two samples reads each array once and writes no third one.  Integer
 * atomics: deterministic.  No working set; asynchronous. */
int kmx_hll_stats(kmx_ctx *ctx, const uint8_t *d_a, const uint8_t *d_b, uint32_t log2_regs, uint64_t *d_hist);

/* ---------------------------------------------------------------- queries on a count table ----
 * BUILD-DEFINED, like the counters.  A TABLE is what kmx_count_canonical(2) / kmx_count_merge(2) / kmx_count_filter(2) write: n keys
 * ascending and distinct, one u64 count per key; two-word keys as (low, high) pairs, 16-byte aligned (KMX_E_ARG otherwise), ordered
 * as 2k-bit integers.  The calls assume that and do not check it: a table that is not sorted gives wrong answers, never an access
 * outside the arrays.  n and n_query up to 2^40 (KMX_E_ARG above). */

/* d_out[i] (u64) = the count of d_query[i] in the table, 0 if it is absent.  Queries are taken as they are (the caller
 * canonicalises: kmx_canonical_words, or the canon array of kmx_canonical_windows), in any order, with repeats; a query with a bit
 * set at or above bit 2k is absent.  d_query_flags may be NULL; where given, a query whose flag lacks KMX_WIN_VALID answers 0
 * whatever its word is, so the canon / flags pair of kmx_canonical_windows goes in unchanged.  d_counts == NULL = membership: 1 / 0.
 * n == 0 is a valid empty table (all answers 0), n_query == 0 a no-op.  k in [1,31], KMX_E_K_RANGE otherwise.  d_out must not
 * alias the table; it MAY be d_query itself (answers in place).
 * Working set: none, or a prefix directory over the keys' top bits in the context's work buffer -- 4 bytes per 8 table entries
 * (rounded up to a power of two, + 260 bytes; at most 1 GiB), built per call by one pass over the keys when n_query >= n / 64 (below
 * that the pass costs more bytes than it saves), n < 2^32 and it fits under the work buffer's cap; otherwise every query is a plain
 * binary search.  Same answers either way: the call never fails for lack of work buffer.
 * Asynchronous: it only enqueues work on the context's stream unless the work buffer has to grow. */
int kmx_count_lookup(kmx_ctx *ctx, const uint64_t *d_kmers, const uint64_t *d_counts, uint64_t n, uint32_t k, const uint64_t *d_query,
                     const uint8_t *d_query_flags, uint64_t n_query, uint64_t *d_out);
/* The same for two-word keys, k in [33,64]: d_kmers2 and d_query2 hold two u64 per key (low, high; both 16-byte aligned, KMX_E_ARG
 * otherwise), d_out one u64 per query (it may NOT alias d_query2).  Directory when n_query >= n / 32.  Working set and
 * synchronisation as kmx_count_lookup. */
int kmx_count_lookup2(kmx_ctx *ctx, const uint64_t *d_kmers2, const uint64_t *d_counts, uint64_t n, uint32_t k, const uint64_t *d_query2,
                      const uint8_t *d_query_flags, uint64_t n_query, uint64_t *d_out);
/* The same answer for every window of a batch of reads, in the dense slot layout of kmx_canonical_windows (r * (read_len - k + 1) + p,
 * or d_win_offsets[r] + p): d_out[slot] = the count of the window's canonical k-mer in the table, 0 for a window the iterator skips
 * (a byte outside ACGTacgt) and for one whose k-mer is absent.  It IS kmx_canonical_windows followed by the lookup: every input that
 * call accepts is accepted (uniform reads of any length, ragged reads with their d_win_offsets and any bound, any d_bases
 * alignment), with its routes and its synchronisation (ragged reads: two more words come back to the host first).  k in [1,31].
 * Working set in the context's work buffer: 1 byte per window (the flags; the canonical words are written into d_out and looked up
 * in place), rounded up to 256 -- uniform reads: windows = n_reads * (read_len - k + 1); ragged reads: the batch's number of BASES
 * stands for the windows -- and reads longer than 256 bases add their segment plan (24 bytes per segment of at most 257 - k
 * windows); the directory of kmx_count_lookup behind that when it pays and fits (it is left out, never refused).  Above the cap:
 * KMX_E_NOMEM BEFORE any kernel runs, nothing written.  The call uses the work buffer (a following kmx_fastx_parse cannot reuse its
 * chunk prefixes). */
int kmx_count_lookup_reads(kmx_ctx *ctx, const kmx_reads *reads, const uint64_t *d_win_offsets, uint32_t k, const uint64_t *d_kmers,
                           const uint64_t *d_counts, uint64_t n, uint64_t *d_out);
/* The same for two-word keys, k in [33,64]: kmx_canonical_windows2 followed by the lookup; d_out one u64 per window.  Working set:
 * 17 bytes per window (16 canonical words, 1 flags; each array rounded up to 256), windows counted as above, + the segment plan of
 * long reads, + the directory when it pays and fits. */
int kmx_count_lookup_reads2(kmx_ctx *ctx, const kmx_reads *reads, const uint64_t *d_win_offsets, uint32_t k, const uint64_t *d_kmers2,
                            const uint64_t *d_counts, uint64_t n, uint64_t *d_out);
/* The abundance spectrum of a table: d_spectrum[min(d_counts[i], n_bins - 1)] += 1 for every entry -- bin c = how many distinct
 * k-mers occur c times, the last bin collects everything at or above it.  n_bins u64 bins, ACCUMULATED into as kmx_histogram
 * accumulates into its buckets (the caller zeroes).  It reads counts only: one call for both key widths.  n_bins >= 2, KMX_E_ARG
 * otherwise.  Working set: none (16 KiB of LDS per block).  Asynchronous: it only enqueues work on the context's stream. */
int kmx_count_spectrum(kmx_ctx *ctx, const uint64_t *d_counts, uint64_t n, uint64_t n_bins, uint64_t *d_spectrum);
/* The entries of a table with min_count <= count <= max_count, order kept: a table again (it feeds merge, lookup, spectrum and
 * filter).  *h_n_out (host) = how many there are; max_out / KMX_E_NOMEM with nothing written and *h_n_out set, both outputs NULL =
 * count only, one NULL = KMX_E_ARG: the conventions of kmx_count_merge.  Outputs must not alias inputs.  Working set in the work
 * buffer: 1 byte per entry (rounded up to 16384) + 8 bytes per 16384 entries + 528 bytes; above the cap KMX_E_NOMEM before any
 * kernel runs.  n up to 2^38 (KMX_E_ARG above).  Synchronous (the count comes back to the host: one round trip). */
int kmx_count_filter(kmx_ctx *ctx, const uint64_t *d_kmers, const uint64_t *d_counts, uint64_t n, uint64_t min_count, uint64_t max_count,
                     uint64_t *d_kmers_out, uint64_t *d_counts_out, uint64_t max_out, uint64_t *h_n_out);
/* The same for two-word keys (16-byte aligned key arrays, KMX_E_ARG otherwise).  Working set and synchronisation as kmx_count_filter. */
int kmx_count_filter2(kmx_ctx *ctx, const uint64_t *d_kmers2, const uint64_t *d_counts, uint64_t n, uint64_t min_count, uint64_t max_count,
                      uint64_t *d_kmers2_out, uint64_t *d_counts_out, uint64_t max_out, uint64_t *h_n_out);

/* ---- per-read abundance statistics against a table ----
 * One row of KMX_RS_WORDS u64 per read, row r at d_stats + KMX_RS_WORDS * r; the words of a row: */
#define KMX_RS_WORDS 8u
#define KMX_RS_N_VALID 0u   /* windows of the read the iterator yields (no byte outside ACGTacgt in the window) */
#define KMX_RS_N_PRESENT 1u /* valid windows whose canonical k-mer is in the table (its count is not 0) */
#define KMX_RS_N_SOLID 2u   /* valid windows with count >= solid_min */
#define KMX_RS_MIN 3u       /* smallest count over the valid windows (an absent k-mer counts 0); 0 when there is no valid window */
#define KMX_RS_MAX 4u       /* largest count over the valid windows; 0 when there is none */
#define KMX_RS_SUM 5u       /* sum of the counts over the valid windows, wrapping mod 2^64 */
#define KMX_RS_MEDIAN 6u    /* c[n_valid / 2] of the valid windows' counts sorted ascending as u64 (the upper median); 0 when n_valid == 0 */
#define KMX_RS_SPAN 7u      /* the longest run of consecutive window positions that are all valid with count >= solid_min: low 32 bits =
                             * the position of its first window in the read, high 32 bits = its length in windows; the earliest such run
                             * on ties; 0 when there is none.  The bases to keep are [start, start + length + k - 1). */
/* The count of a window is what kmx_count_lookup_reads answers for it: d_counts == NULL = membership (1 / 0); n == 0 = a valid empty
 * table (N_VALID is counted, everything else is 0 -- except with solid_min == 0, where every valid window is solid, so N_SOLID and
 * SPAN describe the valid windows: the longest stretch free of invalid bytes).  A table entry whose count is 0 reads as absent.  An
 * invalid window breaks a run of SPAN and contributes to nothing else.  Compares are unsigned; exact for any count up to 2^64 - 1.
 * Every input kmx_canonical_windows accepts is accepted, through its routes and with its synchronisation: uniform reads of any
 * length and d_bases alignment; ragged reads with any bound -- NO window offsets are asked of the caller: they are made on the
 * device, which costs one host round trip.  Uniform reads of at most 256 bases only enqueue work unless the work buffer grows.
 * EVERY row is written: a read without a window (shorter than k, empty, uniform read_len < k, a ragged read of 2^31 bases or more,
 * which the scans skip) gets eight zeros; only n_reads == 0 is a no-op.  Deterministic: repeated calls give identical bytes.
 * k in [1,31], KMX_E_K_RANGE otherwise; NULL ctx / reads, n > 2^40, d_stats == NULL with n_reads > 0: KMX_E_ARG.
 * Working set in the context's work buffer, each array rounded up to 256 bytes (a256), laid out before any kernel runs.  With
 * windows = n_reads * (read_len - k + 1) for uniform reads and the batch's number of BASES for ragged ones:
 *     a256(8 * windows) + a256(windows)                                                  the counts and the flags
 *   + ragged reads:  a256(8 * (n_reads + 1)) + a256(8 * (ceil(n_reads / 4096) + 2))      the window offsets
 *   + reads longer than 256 bases: the segment plan (24 bytes per segment of at most 257 - k windows; 16-byte aligned d_bases)
 * and, behind that, the directory of kmx_count_lookup when it pays and fits (left out, never refused).  The canonical words are
 * written into the counts array and looked up in place.  150 bp reads at k = 31: 1080 bytes per read here, 64 bytes per read out.
 * Above the cap (kmx_ctx_set_work_buffer_limit): KMX_E_NOMEM BEFORE any kernel runs, nothing written.  The call uses the work
 * buffer (a following kmx_fastx_parse cannot reuse its chunk prefixes). */
int kmx_count_read_stats(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, const uint64_t *d_kmers, const uint64_t *d_counts, uint64_t n,
                         uint64_t solid_min, uint64_t *d_stats);
/* The same for two-word keys, k in [33,64] (d_kmers2 16-byte aligned, KMX_E_ARG otherwise): kmx_canonical_windows2 and its routes.
 * Working set: as above + a256(16 * windows) for the canonical words. */
int kmx_count_read_stats2(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, const uint64_t *d_kmers2, const uint64_t *d_counts, uint64_t n,
                          uint64_t solid_min, uint64_t *d_stats);

/* ---- substitution errors corrected against a table ----
 * BUILD-DEFINED (the crate corrects nothing).  Conservative two-sided spectral correction: a base is replaced only where every
 * window that covers it says so.  The rule is defined on the arrays alone, so any bytes give one answer.
 * For one read of L bytes b[0..L), k, a table and solid_min, with windows w = 0 .. L - k:
 *     valid(w)  what the iterator says (no byte outside ACGTacgt in the window);
 *     count(w)  what kmx_count_lookup_reads answers for it: an absent key counts 0, an entry whose count is 0 reads as absent,
 *               d_counts == NULL gives membership 1 / 0;
 *     solid(w)  valid(w) and count(w) >= solid_min;     weak(w)  valid(w) and not solid(w);
 *     C(p)      the windows max(0, p - k + 1) .. min(p, L - k) that cover base p;     V(p)  the valid windows of C(p).
 * Position p is a CANDIDATE iff b[p] is one of ACGTacgt, |V(p)| >= min_cover, and every window of V(p) is weak (no solid window
 * covers p).  A base a of {A, C, G, T}, other than b[p] read case-insensitively, FIXES p iff every window of V(p), spelled with a at
 * p and the read's ORIGINAL bytes everywhere else, has a canonical k-mer whose count is >= solid_min (validity of a window cannot
 * change through such a substitution).  A candidate is CORRECTED iff exactly one base fixes it -- the output byte is that base in
 * the case of the byte it replaces (lowercase stays lowercase) --, AMBIGUOUS if two or three bases fix it (the byte is left as it
 * is), and left unchanged otherwise.
 * Every decision is taken against the original read: decisions do not see each other, and all corrected positions are written.
 * Two errors less than k apart therefore leave each other's windows weak and stay uncorrected (k or more apart: both are
 * restored); run the call again on its output to reach them.  Out of scope: bytes outside ACGTacgt (an N is never replaced, and
 * the windows around it are not in V(p)), insertions and deletions, and any cap on the corrections per read.
 * What follows from the rule:
 *   - solid_min == 0: every valid window is solid, so there is no candidate and the output equals the input;
 *   - n == 0 (an empty table) with solid_min >= 1: every valid window is weak, nothing fixes, the output equals the input; the
 *     candidates are still counted;
 *   - a read with no window (shorter than k, empty, uniform read_len < k, a ragged read of 2^31 bases or more, which the scans skip)
 *     is copied through and its row is four zeros;
 *   - deterministic: repeated calls give identical bytes.
 * One row of KMX_CR_WORDS u64 per read, row r at d_fixes + KMX_CR_WORDS * r: */
#define KMX_CR_WORDS 4u
#define KMX_CR_N_WEAK 0u       /* weak windows of the read: KMX_RS_N_VALID - KMX_RS_N_SOLID of kmx_count_read_stats for the same arguments */
#define KMX_CR_N_CANDIDATES 1u /* candidate positions */
#define KMX_CR_N_CORRECTED 2u  /* candidates with exactly one fixing base: the bytes that differ from the input */
#define KMX_CR_N_AMBIGUOUS 3u  /* candidates with two or three fixing bases */
/* d_out_bases is addressed exactly as reads->d_bases: byte i of the one corresponds to byte i of the other.  Uniform reads:
 * n_reads * read_len bytes are written; ragged reads: the bytes [offsets[0], offsets[n_reads]) and nothing outside them.  Every byte
 * of that range is written on every successful call that has reads (a device-to-device copy, then the corrected bytes).  It must
 * not overlap d_bases over that range (KMX_E_ARG): decisions are against the original bytes, so there is no in-place form.  Every
 * row of d_fixes is written; d_fixes == NULL skips the rows.  Only n_reads == 0 is a no-op.
 * min_cover in 1 .. k (KMX_E_ARG otherwise): 1 lets the bases at a read's two ends, which a single window covers, be corrected;
 * k restricts the call to bases that all k windows cover and that are all valid.  k in [1,31], KMX_E_K_RANGE otherwise (checked
 * first); NULL ctx / reads / d_out_bases with n_reads > 0, n > 2^40: KMX_E_ARG.
 * Every input kmx_count_read_stats accepts is accepted, through its routes and with its synchronisation (ragged reads: window
 * offsets are made on the device, and the first and last read offset come back to the host).
 * Working set in the context's work buffer: that of kmx_count_read_stats for the same reads -- a256(8 * windows) + a256(windows),
 * ragged reads the window offsets, long reads the segment plan -- laid out before any kernel runs, and, behind it, the directory of
 * kmx_count_lookup when it pays for one query per window and fits (left out, never refused); the decision's own searches use that
 * directory when it is there and need nothing else.  150 bp reads at k = 31: 1080 bytes per read here, 150 + 32 bytes per read out.
 * Above the cap (kmx_ctx_set_work_buffer_limit): KMX_E_NOMEM BEFORE any kernel runs or any byte is written.  The call uses the work
 * buffer (a following kmx_fastx_parse cannot reuse its chunk prefixes). */
int kmx_count_correct_reads(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, const uint64_t *d_kmers, const uint64_t *d_counts, uint64_t n,
                            uint64_t solid_min, uint32_t min_cover, uint8_t *d_out_bases, uint64_t *d_fixes);
/* The same for two-word keys, k in [33,64] (d_kmers2 16-byte aligned, KMX_E_ARG otherwise): the routes and the working set of
 * kmx_count_read_stats2 (+ a256(16 * windows) for the canonical words). */
int kmx_count_correct_reads2(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, const uint64_t *d_kmers2, const uint64_t *d_counts, uint64_t n,
                             uint64_t solid_min, uint32_t min_cover, uint8_t *d_out_bases, uint64_t *d_fixes);

/* ---------------------------------------------------------------- coloured tables: more than two samples at once ----
 * BUILD-DEFINED (the crate has no colours).  A COLOURED TABLE is a TABLE as above whose u64 per key is not a count but a bit mask of
 * the samples -- COLOURS, at most 64, colour c = bit c -- that hold the key: d_colors in the place of d_counts.  It is built from
 * what exists: kmx_count_setop(2) with KMX_SETOP_UNION and KMX_RULE_SUM of the coloured table and a sample's keys carrying
 * 1 << c, which is OR as long as bit c is clear in the table.  EVERY call that takes a table takes a coloured one unchanged, because
 * none of them reads the u64 beyond "0 = absent": kmx_count_lookup(2) and kmx_count_lookup_reads(2) answer the mask of a key,
 * kmx_count_filter(2) selects by the mask read as a number, the graph calls with d_counts == NULL see every key.  The two calls below
 * are the reductions that make the masks useful.
 * n_colors in 1 .. 64 (KMX_E_ARG otherwise) says how many colours are in use.  Only the low n_colors bits of a mask count, everywhere
 * in these calls: the MASKED mask.  Bits at or above n_colors are ignored, also where that leaves a mask empty.
 *
 * The pairwise matrix and the spectrum of a coloured table, from the masks alone (no keys: one call for both key widths):
 *     d_matrix[i * n_colors + j]   entries whose masked mask has bits i and j set: n_colors * n_colors u64, row-major, symmetric; the
 *                                  diagonal is the size of each sample, and Jaccard / containment of every pair follow from it;
 *     d_spectrum[j]                entries whose masked mask has exactly j bits set: n_colors + 1 u64, bin 0 = entries with none;
 *                                  may be NULL (core = bin n_colors, private = bin 1, accessory = what lies between).
 * Both outputs are OVERWRITTEN, not accumulated into (unlike kmx_count_spectrum); n == 0 gives all zeros.  Exact, and bit-identical
 * between calls.  NULL ctx / d_matrix, d_colors == NULL with n > 0, n > 2^40: KMX_E_ARG.
 * Working set in the context's work buffer: one partial result per block of the grid, (B * B + 65) * 8 bytes each with B = n_colors
 * rounded up to 8 / 16 / 32 / 64, for min(ceil(n / 256), max(4 * CUs, 512)) blocks -- 32.5 MiB at most on 256 compute units; above the
 * cap KMX_E_NOMEM before any kernel runs.  Asynchronous: it only enqueues work on the context's stream. */
int kmx_count_color_matrix(kmx_ctx *ctx, const uint64_t *d_colors, uint64_t n, uint32_t n_colors, uint64_t *d_matrix, uint64_t *d_spectrum);

/* Which samples a read is compatible with (pseudoalignment against a coloured table): one row of KMX_RC_WORDS u64 per read, row r at
 * d_rows + KMX_RC_WORDS * r, from the masked masks of its windows.  The mask of a window is what kmx_count_lookup_reads answers for
 * it with d_colors as the counts: 0 for an absent key and for an invalid window.  A HIT window is a valid window whose masked mask is
 * not 0; hits_c is the number of hit windows of the read whose masked mask has bit c. */
#define KMX_RC_WORDS 8u
#define KMX_RC_N_VALID 0u  /* as KMX_RS_N_VALID */
#define KMX_RC_N_HIT 1u    /* valid windows whose masked mask is not 0 */
#define KMX_RC_N_UNIQUE 2u /* hit windows whose masked mask has exactly one bit */
#define KMX_RC_ALL 3u      /* AND of the masked masks of the hit windows; 0 when there is none */
#define KMX_RC_ANY 4u      /* OR of them */
#define KMX_RC_THRESH 5u   /* colours c with hits_c > 0 and hits_c * thr_den >= thr_num * n_valid */
#define KMX_RC_BEST 6u     /* (largest hits_c << 32) | c, the smallest such c; 0 when n_hit == 0 */
#define KMX_RC_N_SWITCH 7u /* window positions p such that p and p + 1 are both hit windows of the read and their masked masks differ */
/* d_hits may be NULL; otherwise n_reads * n_colors u32, row r at d_hits + n_colors * r, element c = hits_c: every element is written.
 * thr_den >= 1 and thr_num <= thr_den, KMX_E_ARG otherwise; thr_num == 0 makes THRESH equal ANY, thr_num == thr_den asks for every
 * valid window.  The products are taken in 64 bits: exact.  d_colors == NULL with n > 0 is KMX_E_ARG (membership has no colours);
 * n == 0 is a valid empty table (N_VALID is counted, everything else is 0).  A pair of N_SWITCH never spans two reads, and an invalid
 * or absent window between two hit windows separates them: they are no pair.
 * Inputs, routes, synchronisation, alignment rules and the working set are exactly those of kmx_count_read_stats: uniform and ragged
 * reads of any length, ragged ones without window offsets from the caller; a256(8 * windows) + a256(windows), ragged reads the window
 * offsets, long reads the segment plan, the lookup's directory behind that when it pays and fits; above the cap KMX_E_NOMEM BEFORE
 * any kernel runs, nothing written.  150 bp reads at k = 31: 1080 bytes per read here, 64 (+ 4 * n_colors) bytes per read out --
 * against 8 bytes per window and sample through kmx_count_lookup_reads.
 * EVERY row (and every element of d_hits) is written: a read without a window gets zeros, as does a batch without any; only
 * n_reads == 0 is a no-op.  Every row has one writer: repeated calls give identical bytes.
 * k in [1,31], KMX_E_K_RANGE otherwise; NULL ctx / reads, n > 2^40, n_colors outside 1 .. 64, d_rows == NULL with n_reads > 0:
 * KMX_E_ARG. */
int kmx_count_read_colors(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, const uint64_t *d_kmers, const uint64_t *d_colors, uint64_t n,
                          uint32_t n_colors, uint32_t thr_num, uint32_t thr_den, uint64_t *d_rows, uint32_t *d_hits);
/* The same for two-word keys, k in [33,64] (d_kmers2 16-byte aligned, KMX_E_ARG otherwise): the routes and the working set of
 * kmx_count_read_stats2 (+ a256(16 * windows) for the canonical words). */
int kmx_count_read_colors2(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, const uint64_t *d_kmers2, const uint64_t *d_colors, uint64_t n,
                           uint32_t n_colors, uint32_t thr_num, uint32_t thr_den, uint64_t *d_rows, uint32_t *d_hits);

/* ---------------------------------------------------------------- a count table as the node set of a de Bruijn graph ----
 * BUILD-DEFINED (the crate has no graph).  A TABLE as above.  With x the key of entry i read as the forward strand and
 * mask = 2^(2k) - 1, its eight possible neighbours are, for a base c in 0..3,
 *     edge slot c:      the successor   S_c(x) = (x >> 2) | (c << (2k - 2))     (Kmer::append_base)
 *     edge slot 4 + c:  the predecessor P_c(x) = ((x << 2) | c) & mask          (Kmer::prepend_base)
 * and the NODE of a neighbouring word w is canon(w) = min(w, rc(w)) as 2k-bit integers: the word the counters store.  An entry is
 * PRESENT if d_counts == NULL or d_counts[i] >= min_count; an entry that is not present has no edges and is nobody's neighbour. */
#define KMX_NO_ENTRY 0xFFFFFFFFFFFFFFFFu /* d_nbr: no such edge (a u64, ~0) */

/* d_edges[i] (one byte per entry): bit e is set iff entry i is present, canon(w_e) is a key of the table and that entry is present.
 * A self-loop is an edge like any other (the all-A k-mer: S_0(x) = P_0(x) = x).
 * d_flips[i] (may be NULL): bit e is set iff edge e exists and rc(w_e) < w_e -- the neighbour's stored key is the reverse complement
 * of the word as spelled on x's strand.  A palindromic neighbour (even k, w == rc(w)) is not flipped; bits of absent edges are 0.
 * d_nbr[8 * i + e] (may be NULL): the table index of that neighbour, KMX_NO_ENTRY where the edge is absent.
 * Every byte and word of every output asked for is written.  k in [2,31], KMX_E_K_RANGE otherwise (k = 1 included).  n up to 2^40;
 * n == 0 is a no-op.  d_edges == NULL with n > 0: KMX_E_ARG.  Outputs must not alias the table.  A table that is not sorted gives
 * wrong answers, never an access outside the arrays.
 * Per side four of the eight spellings are four consecutive integers: one search and the keys behind it answer them, and a further
 * search is made only for a spelling that is the smaller of its pair -- about five searches per entry, not eight.
 * Working set: the prefix directory of kmx_count_lookup (4 bytes per 8 entries rounded up to a power of two, + 260 bytes), built by
 * one pass over the keys when n > 8, n < 2^32 and it fits under the work buffer's cap; otherwise it is left out and every search is
 * a plain binary search.  Same answers either way: the call never fails for lack of work buffer.  With the directory the call uses
 * the work buffer (a following kmx_fastx_parse cannot reuse its chunk prefixes).
 * Asynchronous: it only enqueues work on the context's stream unless the work buffer has to grow. */
int kmx_count_adjacency(kmx_ctx *ctx, const uint64_t *d_kmers, const uint64_t *d_counts, uint64_t n, uint32_t k, uint64_t min_count,
                        uint8_t *d_edges, uint8_t *d_flips, uint64_t *d_nbr);
/* The same for two-word keys, k in [33,64] (k = 32 is KMX_E_K_RANGE for both calls); d_kmers2 16-byte aligned, KMX_E_ARG otherwise. */
int kmx_count_adjacency2(kmx_ctx *ctx, const uint64_t *d_kmers2, const uint64_t *d_counts, uint64_t n, uint32_t k, uint64_t min_count,
                         uint8_t *d_edges, uint8_t *d_flips, uint64_t *d_nbr);
/* d_hist[b] += the number of entries whose edge byte is b: 256 u64 bins, ACCUMULATED into as kmx_count_spectrum accumulates (the
 * caller zeroes).  Every degree statistic follows on the host: the low nibble of b holds the successor edges, the high nibble the
 * predecessor edges -- directed edge slots, isolated entries (b == 0), tips, branching entries, (in = 1, out = 1) interiors.  It
 * reads edge bytes only: one call for both key widths.  Working set: none (4 KiB of LDS per block).  Asynchronous. */
int kmx_count_edge_histogram(kmx_ctx *ctx, const uint8_t *d_edges, uint64_t n, uint64_t *d_hist);
/* Where the non-branching paths (unitigs) end, from the three outputs of kmx_count_adjacency(2) -- it reads indices, not keys: one
 * call for both key widths.  Bit 0 of d_ends[i] = the successor side of entry i (edge slots 0..3, the low nibble of its edge byte)
 * is an END, bit 1 = its predecessor side (slots 4..7, the high nibble) is.  A side is an END iff its nibble does not have exactly
 * one bit set, or its one neighbour j is i itself, or the nibble of j at the side the edge ENTERS does not have exactly one bit set.
 * A successor edge enters j at its predecessor side, a predecessor edge at its successor side; a flipped edge (its bit in
 * d_flips[i]) at the other one.  A d_nbr value >= n under a set edge bit (inconsistent inputs) makes that side an END; nothing is
 * read there.  Entries with edge byte 0 -- isolated, or not present: the counts tell -- have both bits set.  The set bits are twice
 * the number of unitigs that have an end (a cycle without a branch has none).  All four arrays are required for n > 0 (KMX_E_ARG).
 * Working set: none.  Asynchronous. */
int kmx_count_unitig_ends(kmx_ctx *ctx, const uint8_t *d_edges, const uint8_t *d_flips, const uint64_t *d_nbr, uint64_t n,
                          uint8_t *d_ends);

/* ---------------------------------------------------------------- the unitigs of that graph ----
 * BUILD-DEFINED.  From a table and the three outputs of kmx_count_adjacency(2) (same d_counts / min_count: PRESENT as above) to the
 * maximal non-branching paths, as lists of oriented nodes, and to their bases.
 * The ORIENTED NODE v = 2 i + o is entry i read forward (o = 0: its word is the key x, it is left through the successor side) or
 * reverse (o = 1: its word is rc(x), it is left through the predecessor side); mirror(v) = v ^ 1.
 * next(v) = 2 j + (o ^ f) exists iff entry i is present; side o of i is not an END by the rule of kmx_count_unitig_ends; the one
 * set edge slot e of that side has d_nbr[8 i + e] = j < n, with flip bit f; neither i nor j is a palindrome (x == rc(x), even k
 * only: without this rule a path y -> palindrome z -> rc(y) makes next non-injective); and the link is mutual,
 * next(mirror(next(v))) == mirror(v).  For inputs that are the adjacency of the table mutuality follows from the rest; it is there
 * so that ANY bytes in d_edges / d_flips / d_nbr give disjoint simple paths and cycles: the call ends, succeeds and reads nothing
 * outside its arrays.  prev(v) = mirror(next(mirror(v))).  A palindromic entry is a unitig of its own.
 * A chain runs from a head (no prev) along next to a tail; its mirror chain has head mirror(tail) and tail mirror(head).  Of the
 * two the CANONICAL one has the smaller head entry index, at equal indices (one node) the one with o = 0.  Oriented nodes on no
 * chain lie on cycles, which come in mirror pairs too: the canonical one contains 2 i*, i* the cycle's smallest entry index, and
 * is written starting there.  Unitigs are ordered by ascending head entry index (an entry heads at most one); every present entry
 * lies in exactly one, entries that are not present in none.
 * d_nodes (room for n u64): the oriented nodes of the canonical unitigs, one unitig after another.  d_offsets (room for n + 1):
 * U + 1 offsets into d_nodes.  d_circular (may be NULL; room for n bytes): 1 for a cycle.  d_count_sums (may be NULL; room for n
 * u64): the wrapping sum of the counts of the unitig's entries; with d_counts == NULL every entry counts 1.  Only the first
 * *h_n_nodes, U + 1, U and U elements are written, U = *h_n_unitigs.  Exact and deterministic.
 * d_kmers is read at even k only (it may be NULL at odd k).  k in [2,31] (KMX_E_K_RANGE); n up to 2^40; n == 0 is a no-op with both
 * host counts 0.  A required array missing with n > 0: KMX_E_ARG.  Outputs must not alias inputs.
 * Working set: 64 bytes per entry + n / 16 + 2 KiB in the work buffer -- two 16-byte rank records per oriented node (pointer
 * jumping reads one set and writes the other) -- KMX_E_NOMEM above the cap (kmx_ctx_set_work_buffer_limit), nothing written then.
 * ceil(log2(longest unitig)) + 2 rounds at most, each a pass over the records with one 16-byte gather per unfinished node and one
 * host read-back.  Synchronous, as kmx_count_canonical is. */
int kmx_count_unitigs(kmx_ctx *ctx, const uint64_t *d_kmers, const uint64_t *d_counts, uint64_t n, uint32_t k, uint64_t min_count,
                      const uint8_t *d_edges, const uint8_t *d_flips, const uint64_t *d_nbr, uint64_t *d_nodes, uint64_t *d_offsets,
                      uint8_t *d_circular, uint64_t *d_count_sums, uint64_t *h_n_unitigs, uint64_t *h_n_nodes);
/* The same for two-word keys, k in [33,64]; d_kmers2 16-byte aligned, KMX_E_ARG otherwise. */
int kmx_count_unitigs2(kmx_ctx *ctx, const uint64_t *d_kmers2, const uint64_t *d_counts, uint64_t n, uint32_t k, uint64_t min_count,
                       const uint8_t *d_edges, const uint8_t *d_flips, const uint64_t *d_nbr, uint64_t *d_nodes, uint64_t *d_offsets,
                       uint8_t *d_circular, uint64_t *d_count_sums, uint64_t *h_n_unitigs, uint64_t *h_n_nodes);
/* The bases of the unitigs, ASCII ACGT.  A unitig of m nodes spells m + k - 1 bases: the k bases of its first oriented node's word
 * (base 0 = the lowest two bits), then the top base of each following oriented word (o = 1: the complement of the key's lowest
 * base).  A circular unitig is spelled the same way from its start; the wrap-around is not repeated.  Unitig u starts at byte
 * d_offsets[u] + u (k - 1) of d_seq -- a closed form, there is no second offsets array -- and d_seq holds
 * d_offsets[n_unitigs] + n_unitigs (k - 1) bytes.  n is the table's entry count (nodes naming an entry >= n are skipped).
 * n_unitigs == 0 is a no-op; n_unitigs > n or a missing array: KMX_E_ARG.  Working set: none.  Asynchronous. */
int kmx_count_unitig_sequences(kmx_ctx *ctx, const uint64_t *d_kmers, uint64_t n, uint32_t k, const uint64_t *d_nodes, const uint64_t *d_offsets,
                               uint64_t n_unitigs, uint8_t *d_seq);
int kmx_count_unitig_sequences2(kmx_ctx *ctx, const uint64_t *d_kmers2, uint64_t n, uint32_t k, const uint64_t *d_nodes, const uint64_t *d_offsets,
                                uint64_t n_unitigs, uint8_t *d_seq);

/* ---------------------------------------------------------------- reads threaded through the unitigs ----
 * BUILD-DEFINED.  The way back from the unitigs to the reads: where every window of a read lies on them. */
#define KMX_PLACE_NONE 0u /* d_place: the entry lies in no unitig */
/* d_place[i] (one u64 per table entry, n of them) = KMX_PLACE_NONE for an entry no node of d_nodes names (an entry that was not
 * present when the unitigs were made), otherwise
 *     ((p + 1) << 3) | (last << 2) | (first << 1) | o
 * with p the index into d_nodes with d_nodes[p] >> 1 == i, o = d_nodes[p] & 1, and first / last set when p is the first / last node
 * of its unitig AS WRITTEN (both for a one-node unitig; for a circular unitig they mark the written start and end).  A place is
 * never 0 for a placed entry, so d_place can be handed to kmx_count_lookup(2) / kmx_count_lookup_reads(2) as the counts array:
 * "count 0 reads as absent" then means "in no unitig".
 * d_nodes / d_offsets / n_unitigs as kmx_count_unitigs(2) wrote them (d_nodes holds d_offsets[n_unitigs] nodes); n = the table's
 * entry count.  Every word of d_place[0 .. n) is written.  Nodes naming an entry >= n are skipped, as
 * kmx_count_unitig_sequences skips them.  It reads indices only: one call for both key widths.  n_unitigs == 0 writes n zeros;
 * n == 0 is a no-op; a missing array with n > 0 (d_place; d_nodes / d_offsets with n_unitigs > 0), n or n_unitigs above 2^40:
 * KMX_E_ARG.  Working set: none.  Asynchronous. */
int kmx_count_unitig_index(kmx_ctx *ctx, const uint64_t *d_nodes, const uint64_t *d_offsets, uint64_t n_unitigs, uint64_t n,
                           uint64_t *d_place);

/* The segments of every read over the unitigs: KMX_PATH_WORDS u64 per segment, segment s at d_segments + KMX_PATH_WORDS * s. */
#define KMX_PATH_WORDS 4u
#define KMX_PATH_READ 0u   /* the read index */
#define KMX_PATH_SPAN 1u   /* low 32 bits = the position of the segment's first window in the read, high 32 bits = its length in windows
                            * (the packing of KMX_RS_SPAN); its bases are [start, start + length + k - 1) */
#define KMX_PATH_UNITIG 2u /* u, the unitig */
#define KMX_PATH_POS 3u    /* (q << 1) | d, q = p - d_offsets[u] of the FIRST window: window start + t of the read sits at node q + t of
                            * the unitig for d = 0 and at node q - t for d = 1 */
/* Window j of a read is MAPPED if it is valid (KMX_WIN_VALID), its canonical word is entry i of the table (d_kmers, n) and
 * d_place[i] != 0.  It then has p, o, first, last from the place, the read's strand s (0 if KMX_WIN_FW_CANONICAL is set, else 1) and
 * the direction d = s ^ o: d = 0, the read walks the unitig as written; d = 1, it walks the mirror.  (A palindromic window has
 * fw == rc, so s = 1; it is a one-node unitig with o = 0, so it reads d = 1 -- and is a segment of its own either way.)
 * Window j + 1 CONTINUES window j (consecutive positions of ONE read) iff both are mapped, their d is equal, and
 *     d = 0:  p' == p + 1 and first' is clear        d = 1:  p' + 1 == p and last' is clear.
 * A SEGMENT is a maximal run of such windows.  So a run never crosses a unitig boundary, never crosses an unmapped or invalid
 * window, never crosses from one read into the next, and never crosses the written start of a cycle: a read going round a circular
 * unitig starts a new segment at each passage.
 * Segments are ordered by read, then by start.  d_path_offsets (n_reads + 1 u64): read r owns the segments
 * [d_path_offsets[r], d_path_offsets[r + 1]); every read gets its offset, one without a window too.  *h_n_segments (host) is always
 * set.  Both output arrays NULL = count only; one NULL = KMX_E_ARG.  More segments than max_segments: KMX_E_NOMEM with d_segments
 * untouched and d_path_offsets STILL WRITTEN in full -- its size does not depend on the count, and it says how to batch.
 * Deterministic: repeated calls give identical bytes.
 * d_place as kmx_count_unitig_index writes it for the unitigs d_offsets / n_unitigs describe (the node list itself is not read).
 * Places that are inconsistent with d_offsets give meaningless records, never an access outside the arrays; a p at or beyond
 * d_offsets[n_unitigs] reads as unmapped.
 * Every input kmx_count_read_stats accepts is accepted, through the same routes and with the same synchronisation: uniform reads of
 * any length and d_bases alignment, ragged reads with any bound (the window offsets are made on the device), reads longer than 256
 * bases through the segment plan.  k in [2,31], the unitig calls' domain: KMX_E_K_RANGE otherwise (k = 1 included).  n == 0 or
 * n_unitigs == 0 is valid and gives zero segments (every offset 0); n_reads == 0 is a no-op with *h_n_segments = 0.  NULL ctx /
 * reads / h_n_segments, n or n_unitigs above 2^40, d_kmers or d_place NULL with n > 0, d_offsets NULL with n_unitigs > 0: KMX_E_ARG.
 * Working set in the context's work buffer, each array rounded up to 256 bytes (a256), laid out before any kernel runs.  With
 * windows = n_reads * (read_len - k + 1) for uniform reads and the batch's number of BASES for ragged ones, g = ceil(windows / 64):
 *     a256(8 * windows) + a256(windows)                                                  the places and the flags
 *   + 2 * a256(8 * g) + a256(4 * g) + a256(8 * (ceil(windows / 4096) + 2))               head / tail ballots, counts, scan partials
 *   + ragged reads:  a256(8 * (n_reads + 1)) + a256(8 * (ceil(n_reads / 4096) + 2))      the window offsets
 *   + reads longer than 256 bases: the segment plan (24 bytes per segment of at most 257 - k windows; 16-byte aligned d_bases)
 * and, behind that, the directory of kmx_count_lookup when it pays and fits (left out, never refused).  The canonical words are
 * written into the places array and looked up in place.  150 bp reads at k = 31: 1118 bytes per read here; out, 8 bytes per read
 * and 32 per segment.  Above the cap (kmx_ctx_set_work_buffer_limit): KMX_E_NOMEM BEFORE any kernel runs, nothing written.  The call
 * uses the work buffer (a following kmx_fastx_parse cannot reuse its chunk prefixes).
 * Synchronous (the count comes back to the host: one round trip, after those of the windows route). */
int kmx_count_read_paths(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, const uint64_t *d_kmers, uint64_t n, const uint64_t *d_place,
                         const uint64_t *d_offsets, uint64_t n_unitigs, uint64_t *d_path_offsets, uint64_t *d_segments,
                         uint64_t max_segments, uint64_t *h_n_segments);
/* The same for two-word keys, k in [33,64] (d_kmers2 16-byte aligned, KMX_E_ARG otherwise; k = 32 is KMX_E_K_RANGE for both calls):
 * kmx_canonical_windows2 and its routes.  Working set: as above + a256(16 * windows) for the canonical words. */
int kmx_count_read_paths2(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, const uint64_t *d_kmers2, uint64_t n, const uint64_t *d_place,
                          const uint64_t *d_offsets, uint64_t n_unitigs, uint64_t *d_path_offsets, uint64_t *d_segments,
                          uint64_t max_segments, uint64_t *h_n_segments);

/* ---------------------------------------------------------------- the unitigs as a graph ----
 * BUILD-DEFINED.  Which unitig follows which, and in which orientation: the compacted de Bruijn graph.
 * The ORIENTED UNITIG t = 2 u + s is unitig u as written (s = 0: its ENTRY node is d_nodes[d_offsets[u]], its EXIT node is
 * d_nodes[d_offsets[u + 1] - 1]) or its mirror (s = 1: ENTRY = mirror(last node), EXIT = mirror(first node)); mirror(t) = t ^ 1.
 * The LINKS of t.  Let v = 2 i + o be the EXIT node of t.  For c = 0 .. 3 in ascending order let e = 4 o + c (an oriented node with
 * o = 1 is left through the predecessor side, edge slots 4 .. 7).  If bit e of d_edges[i] is set: j = d_nbr[8 i + e], f = bit e of
 * d_flips[i], w = 2 j + (o ^ f).  j >= n or d_place[j] == 0 gives no link.  Otherwise p, first, last and o_j come from d_place[j],
 * and u' is the unitig that holds position p -- the largest u' with d_offsets[u'] <= p, one upper-bound search of d_offsets; a p at
 * or beyond d_offsets[n_unitigs] gives no link.  Then
 *     t -> 2 u' + 0   if (w & 1) == o_j and first is set        (w is the entry node of u' as written)
 *     t -> 2 u' + 1   if (w & 1) != o_j and last is set         (w is the entry node of the mirror of u')
 * and anything else gives no link (this cannot happen for the adjacency of the table: an edge that leaves a unitig's exit enters
 * another's entry).  EVERY set edge bit on the exit side counts, whether or not that side is an END by the rule of
 * kmx_count_unitig_ends: a circular unitig links to itself across its written start (2 u -> 2 u, and 2 u + 1 -> 2 u + 1), a chain
 * cut by the palindrome rule links to the palindromic one-node unitig, and a hairpin links t -> mirror(t).  Consecutive nodes
 * overlap by k - 1 bases, so every link is an overlap of k - 1 bases between the sequences of t and t' (the sequence of 2 u + 1 is
 * the reverse complement of that of u).
 * MIRROR SYMMETRY.  For inputs that are the adjacency, unitigs and index of one table, and unitigs none of which is a palindromic
 * k-mer (every table at odd k): t -> t' is a link iff mirror(t') -> mirror(t) is, and no link occurs twice.  A palindromic entry
 * (even k) is a one-node unitig P whose two orientations spell the same bases, and the rule does not pretend otherwise: 2 P and
 * 2 P + 1 have the same neighbours (in opposite order of c), while a link INTO P names one orientation only -- 2 P + o, o the
 * orientation of the exit node it comes from (a palindromic neighbour is never flipped).  What holds instead: with the orientation
 * bit of every palindromic unitig cleared on both ends, the set of links is closed under (t, t') -> (mirror(t'), mirror(t)).
 * d_link_offsets (2 U + 1 u64, U = n_unitigs): t owns d_links[d_link_offsets[t] .. d_link_offsets[t + 1]), at most four, in
 * ascending c; d_links[x] = the target t'.  *h_n_links (host) is always set.  Both output arrays NULL = count only; one NULL =
 * KMX_E_ARG.  More links than max_links: KMX_E_NOMEM with d_links untouched and d_link_offsets STILL WRITTEN in full -- the
 * conventions of kmx_count_read_paths.  Exact and deterministic: repeated calls give identical bytes.
 * d_edges / d_flips / d_nbr as kmx_count_adjacency(2) wrote them for the table's n entries, d_nodes / d_offsets / n_unitigs as
 * kmx_count_unitigs(2) wrote them, d_place as kmx_count_unitig_index wrote it.  It reads indices only: one call for both key
 * widths.  ANY bytes in the inputs give a result and never an access outside the arrays: an exit node naming an entry >= n, a
 * unitig with d_offsets[u] >= d_offsets[u + 1] or d_offsets[u + 1] > d_offsets[n_unitigs] has no links; offsets that do not ascend
 * give meaningless targets; every target is < 2 U.
 * n_unitigs == 0 writes the single offset 0 (*h_n_links = 0); n == 0 with n_unitigs == 0 is a no-op with *h_n_links = 0.  NULL ctx /
 * h_n_links, n or n_unitigs above 2^40, an input array missing with n_unitigs > 0 (d_nodes, d_offsets; with n > 0 also d_edges,
 * d_flips, d_nbr, d_place): KMX_E_ARG.
 * Working set in the context's work buffer, laid out before any kernel runs, with r = ceil((2 U + 1) / 4096) and each array rounded
 * up to 256 bytes (a256):
 *     a256(4096 * r) + a256(8 * (r + 1))                    a degree byte per oriented unitig, a scan partial per 4096 of them
 * Above the cap (kmx_ctx_set_work_buffer_limit): KMX_E_NOMEM BEFORE any kernel runs, nothing written.  The call uses the work buffer
 * (a following kmx_fastx_parse cannot reuse its chunk prefixes).  Synchronous (the count comes back to the host: one round trip). */
int kmx_count_unitig_links(kmx_ctx *ctx, const uint8_t *d_edges, const uint8_t *d_flips, const uint64_t *d_nbr, uint64_t n,
                           const uint64_t *d_nodes, const uint64_t *d_offsets, uint64_t n_unitigs, const uint64_t *d_place,
                           uint64_t *d_link_offsets, uint64_t *d_links, uint64_t max_links, uint64_t *h_n_links);

/* The entries of a table that lie in kept unitigs, order kept: a table again (it feeds every other table call, the adjacency
 * included: cut, then compact again).  Entry i is kept iff d_place[i] != 0, its position p (d_place as kmx_count_unitig_index wrote
 * it) lies below d_offsets[n_unitigs], and d_keep[u] != 0 for the unitig u that holds p (the search of kmx_count_unitig_links);
 * d_keep holds one byte per unitig.  An entry in no unitig -- one that was not present when the unitigs were made -- is dropped; a p
 * outside the offsets reads as not kept.
 * *h_n_out (host) = how many entries are kept; max_out / KMX_E_NOMEM with nothing written and *h_n_out set, both outputs NULL =
 * count only, one NULL = KMX_E_ARG, outputs must not alias inputs: the conventions of kmx_count_filter.  n == 0 or n_unitigs == 0
 * keeps nothing (*h_n_out = 0, nothing read).  NULL ctx / h_n_out, n above 2^38, n_unitigs above 2^40, d_kmers / d_counts / d_place
 * NULL with n > 0, d_offsets / d_keep NULL with n_unitigs > 0: KMX_E_ARG.
 * Working set in the work buffer, kmx_count_filter's: a256(16384 * ceil(n / 16384)) + a256(8 * (ceil(n / 16384) + 2)) -- a mark byte
 * per entry and a partial per 16384 entries; above the cap KMX_E_NOMEM before any kernel runs.  Synchronous (one round trip). */
int kmx_count_unitig_select(kmx_ctx *ctx, const uint64_t *d_kmers, const uint64_t *d_counts, uint64_t n, const uint64_t *d_place,
                            const uint64_t *d_offsets, uint64_t n_unitigs, const uint8_t *d_keep, uint64_t *d_kmers_out,
                            uint64_t *d_counts_out, uint64_t max_out, uint64_t *h_n_out);
/* The same for two-word keys (16-byte aligned key arrays, KMX_E_ARG otherwise). */
int kmx_count_unitig_select2(kmx_ctx *ctx, const uint64_t *d_kmers2, const uint64_t *d_counts, uint64_t n, const uint64_t *d_place,
                             const uint64_t *d_offsets, uint64_t n_unitigs, const uint8_t *d_keep, uint64_t *d_kmers2_out,
                             uint64_t *d_counts_out, uint64_t max_out, uint64_t *h_n_out);

/* Which unitigs to drop to clean the compacted graph: one keep byte per unitig, exactly what kmx_count_unitig_select(2) takes, and
 * optionally the reason.  Three rules, exclusive by degree: a short DEAD END (tip) that loses to a sibling by mean count, the weaker
 * branch of a SIMPLE BUBBLE, a short ISLAND with no link at all.  The rule is defined on the arrays alone: any bytes give the answer
 * stated here and never an access outside the arrays.
 * NOTATION.  U = n_unitigs.  m(u) = d_offsets[u + 1] - d_offsets[u], read as 0 if d_offsets[u + 1] < d_offsets[u].  S(u) =
 * d_count_sums[u] as a u64 (d_count_sums == NULL: S(u) = m(u), a mean of 1).  t = 2 u + s is an oriented unitig, mirror(t) = t ^ 1.
 * L(t) is the list d_links[lo .. hi) with lo = d_link_offsets[t], hi = d_link_offsets[t + 1] -- but only if lo <= hi <= n_links,
 * hi - lo <= 4 and every listed target is < 2 U; otherwise L(t) is empty.  deg(t) = |L(t)|.
 * THE ORDER.  u LOSES to y at (a, b) iff S(u) m(y) b < S(y) m(u) a, or the two sides are equal and u > y: the mean count per node
 * of u is below a / b of y's, ties going to the smaller index.  The comparison is exact, in integers (the products are formed in
 * full, for any S and m; no floating point).  With a = b it is a strict total order on distinct unitigs; with 1 <= a <= b no two
 * unitigs lose to each other.
 * PARAMETERS.  tip_max_nodes (0 turns the tip rule off), tip_num / tip_den (the ratio a / b of the tip rule; tip_num == 0: the tip
 * rule is topological), bubble_max_nodes (0 turns the bubble rule off), bubble_max_diff, island_max_nodes (0 turns the island rule
 * off).  tip_num > tip_den, tip_den == 0 with tip_max_nodes > 0, tip_num or tip_den above 65535: KMX_E_ARG.
 * THE REASON of unitig u.  A circular unitig (d_circular[u] != 0; d_circular == NULL: none is) has reason KMX_CLEAN_KEEP.  For
 * the rest let d0 = deg(2 u), d1 = deg(2 u + 1):
 *   KMX_CLEAN_ISLAND  d0 = d1 = 0, island_max_nodes > 0 and m(u) <= island_max_nodes.
 *   KMX_CLEAN_TIP     exactly one of d0, d1 is 0, tip_max_nodes > 0 and m(u) <= tip_max_nodes; let t be the side that has links.
 *                     tip_num == 0: dropped (all of this is then "not circular, short, one side open").  Otherwise dropped iff some
 *                     x in L(t) and some z in L(x ^ 1) with z >> 1 != u have u LOSES to z >> 1 at (tip_num, tip_den): z ^ 1 is a
 *                     SIBLING of t at x, another oriented unitig that enters x.  A tip without a sibling stays.
 *   KMX_CLEAN_BUBBLE  d0 = d1 = 1, bubble_max_nodes > 0 and m(u) <= bubble_max_nodes; let x = L(2 u)[0], s = L(2 u + 1)[0] ^ 1.
 *                     All of: L(s) has exactly two elements, distinct, one of them 2 u -- the other is y, yu = y >> 1; L(x ^ 1) has
 *                     exactly two elements and they are 2 u + 1 and y ^ 1 in either order; L(y) = [x] and L(y ^ 1) = [s ^ 1];
 *                     u != yu, and neither u nor yu equals s >> 1 or x >> 1; yu is not circular; m(yu) <= bubble_max_nodes;
 *                     |m(u) - m(yu)| <= bubble_max_diff; u LOSES to yu at (1, 1).
 *   KMX_CLEAN_KEEP    everything else.
 * The bubble condition is symmetric under u <-> yu and under mirroring, and (1, 1) is a total order: for any input exactly one
 * branch of each simple bubble is dropped.  d_keep[u] = 1 iff the reason is KMX_CLEAN_KEEP, else 0; d_reason[u] = the reason.
 * PALINDROMIC UNITIGS (even k).  Where a palindromic one-node unitig sits at a junction the links lack mirror symmetry (above), so
 * L(x ^ 1) can miss an oriented unitig that enters x.  The rule is not bent for it: such a tip finds no sibling, such a bubble does
 * not close, and the unitig stays.
 * One round drops tips, branches and islands that the SAME graph shows; dropping them makes new unitigs (the two stems around a
 * popped bubble join), so cleaning is run in rounds: clean, select, adjacency, unitigs, index, links, clean.
 * d_offsets / d_circular / d_count_sums / n_unitigs as kmx_count_unitigs(2) wrote them, d_link_offsets (2 U + 1 u64) / d_links /
 * n_links as kmx_count_unitig_links wrote them.  Indices only: one call for both key widths.  d_keep and d_reason hold U bytes each
 * and nothing beyond them is written; d_reason may be NULL.  Outputs must not alias inputs.  Deterministic: repeated calls give
 * identical bytes.  n_unitigs == 0 is a no-op (nothing read, nothing written).  NULL ctx, n_unitigs above 2^40, n_links above 2^43
 * (four links per oriented unitig), the parameter errors above; with n_unitigs > 0 also d_keep, d_offsets or d_link_offsets NULL, or
 * d_links NULL with n_links > 0: KMX_E_ARG.  Working set: none.  Asynchronous. */
#define KMX_CLEAN_KEEP 0
#define KMX_CLEAN_TIP 1
#define KMX_CLEAN_BUBBLE 2
#define KMX_CLEAN_ISLAND 3
int kmx_count_unitig_clean(kmx_ctx *ctx, const uint64_t *d_offsets, const uint8_t *d_circular, const uint64_t *d_count_sums,
                           uint64_t n_unitigs, const uint64_t *d_link_offsets, const uint64_t *d_links, uint64_t n_links,
                           uint64_t tip_max_nodes, uint32_t tip_num, uint32_t tip_den, uint64_t bubble_max_nodes,
                           uint64_t bubble_max_diff, uint64_t island_max_nodes, uint8_t *d_keep, uint8_t *d_reason);

/* Which unitigs hang together: the connected components of the compacted graph -- a label and an id per unitig, a record per
 * component.  The cleaning rules above look at one unitig and its neighbours; this is the global question: how many pieces, how big
 * is each, and which piece is a unitig (and, through kmx_count_read_paths, a read) in.  The rule is defined on the arrays alone: any
 * bytes give the answer stated here and never an access outside the arrays.
 * NOTATION.  U, m(u), S(u), t = 2 u + s and L(t) exactly as for kmx_count_unitig_clean: L(t) is empty unless lo <= hi <= n_links,
 * hi - lo <= 4 and every listed target is < 2 U; m(u) reads as 0 where the offsets descend; d_count_sums == NULL: S(u) = m(u).
 * In addition d_offsets == NULL: m(u) = 1.
 * ALIVE.  u is alive iff d_mask == NULL or d_mask[u] != 0 (d_mask: U bytes, for instance the keep bytes of kmx_count_unitig_clean).
 * A unitig that is not alive takes no part: its links, and links into it, do not exist.
 * ADJACENCY.  Alive unitigs u and v are adjacent iff some target t' in L(2 u) or L(2 u + 1) has t' >> 1 == v, or the same with u and
 * v swapped.  A link listed in one direction only still joins the two (palindromic junctions make such links at even k, see
 * kmx_count_unitig_links); self-links and hairpins join nothing new.  Orientation plays no part.
 * COMPONENTS are the classes of the reflexive-transitive closure of adjacency over the alive unitigs; C is their number.
 * OUTPUTS.  d_labels[u] (U u64, required) = the smallest unitig index in u's component, KMX_COMPONENT_NONE for a unitig that is not
 * alive.  d_ids[u] (U u64, may be NULL) = the rank of u's label among all distinct labels in ascending order, 0 .. C - 1, and
 * KMX_COMPONENT_NONE where the label is.  d_components (max_components records of 4 u64, may be NULL): for component c its root
 * (the label), its number of unitigs, the sum of m(u) and the wrapping u64 sum of S(u) over its unitigs.  *h_n_components (host) = C,
 * always set.  *h_rounds (host, may be NULL) = the hook / jump rounds the call ran (at least 1 for U > 0: the round that finds
 * nothing left to do).
 * C > max_components with d_components != NULL: KMX_E_NOMEM with d_components untouched and d_labels and d_ids STILL WRITTEN in
 * full -- the convention of kmx_count_unitig_links.
 * Exact and deterministic: only integer minima and wrapping integer sums, so repeated calls give identical bytes.  Nothing beyond
 * U, U and 4 * min(C, max_components) words is written.  Outputs must not alias inputs.  d_offsets (U + 1 u64) / d_count_sums as
 * kmx_count_unitigs(2) wrote them, d_link_offsets (2 U + 1 u64) / d_links / n_links as kmx_count_unitig_links wrote them.  Indices
 * only: one call for both key widths.  n_unitigs == 0 is a no-op with *h_n_components = 0 and *h_rounds = 0.  NULL ctx /
 * h_n_components, n_unitigs above 2^40, n_links above 2^43, d_labels or d_link_offsets NULL with n_unitigs > 0, d_links NULL with
 * n_links > 0: KMX_E_ARG.
 * Working set in the context's work buffer, laid out before any kernel runs, each array rounded up to 256 bytes (a256):
 *     a256(8 * (ceil(U / 4096) + 1)) + 256                   a scan partial per 4096 unitigs (+ the total), the change counter
 *   + d_components != NULL and d_ids == NULL:  a256(8 * U)   the roots' ids, which d_ids holds otherwise
 * The labels are their own parent array: no second array of U words.  Above the cap (kmx_ctx_set_work_buffer_limit): KMX_E_NOMEM
 * BEFORE any kernel runs, nothing written.  The call uses the work buffer (a following kmx_fastx_parse cannot reuse its chunk
 * prefixes).  Synchronous: one small read-back per round, one for C. */
#define KMX_COMPONENT_NONE 0xFFFFFFFFFFFFFFFFu /* a label or id of a unitig that is not alive (a u64, ~0) */
int kmx_count_unitig_components(kmx_ctx *ctx, const uint64_t *d_offsets, const uint64_t *d_count_sums, uint64_t n_unitigs,
                                const uint64_t *d_link_offsets, const uint64_t *d_links, uint64_t n_links, const uint8_t *d_mask,
                                uint64_t *d_labels, uint64_t *d_ids, uint64_t *d_components, uint64_t max_components,
                                uint64_t *h_n_components, uint32_t *h_rounds);

/* How many reads walk each link: the evidence that an edge of the graph is real.  A link exists because two present k-mers overlap by
 * k - 1 bases, whether or not any read ever passed from one to the other; the segments of kmx_count_read_paths(2) say where reads
 * did.  The rule is defined on the arrays alone: any bytes give the answer stated here and never an access outside the arrays.
 * NOTATION.  U = n_unitigs; m(u) = d_offsets[u + 1] - d_offsets[u], read as 0 where the offsets descend; segment s is the record
 * d_segments + KMX_PATH_WORDS * s with read(s), start(s) and length(s) (the low and high 32 bits of KMX_PATH_SPAN), u(s), and q(s), d(s)
 * (KMX_PATH_POS = (q << 1) | d); t(s) = 2 u(s) + d(s), the oriented unitig the segment walks.  L(t), for t < 2 U, is the list
 * d_links[lo .. hi), lo = d_link_offsets[t], hi = d_link_offsets[t + 1]; it is empty unless lo <= hi <= n_links and hi - lo <= 4.
 * JUNCTION.  Segments s and s + 1 (s + 1 < n_segments) form a junction iff read(s + 1) == read(s) and start(s + 1) == start(s) +
 * length(s): the next run of windows begins one base after the last window of this one.  A gap -- an N, a window that is not
 * mapped -- is no junction, nor is the step from one read to the next.
 * CROSSING.  A junction crosses link slot l iff u(s) < U, u(s + 1) < U, and with t = t(s), t' = t(s + 1), as integers without wrap:
 *     s ends on the exit node of t:            d(s) = 0:  q(s) + length(s) == m(u(s))      d(s) = 1:  q(s) + 1 == length(s)
 *     s + 1 starts on the entry node of t':    d(s + 1) = 0:  q(s + 1) == 0                d(s + 1) = 1:  q(s + 1) + 1 == m(u(s + 1))
 *     l is the first slot of L(t) with d_links[l] == t'.
 * Then d_support[l] += 1, and if the MIRROR link mirror(t') -> mirror(t) has a slot m -- the first slot of L(t' ^ 1) whose target is
 * t ^ 1 -- and m != l, also d_support[m] += 1.  A hairpin t -> t ^ 1 is its own mirror and counts once.  Every other junction is
 * UNLINKED: a unitig index at or above U, an end condition that fails, or no slot l.
 * d_support (n_links u64) and d_summary (KMX_LS_WORDS u64: junctions, crossed, unlinked; junctions == crossed + unlinked) are
 * ACCUMULATED into, as kmx_count_spectrum accumulates (the caller zeroes): batches of reads stream against one graph.
 * WHAT IT COUNTS.  For segments made over the unitigs the links were made of (same table, adjacency, unitigs, index), at odd k:
 * d_support[l] = the number of occurrences in the reads, on either strand, of the (k + 1)-mer link l spells -- the last k bases of t
 * followed by base k - 1 of t' -- a (k + 1)-mer that is its own reverse complement counted once; a link and its mirror carry the same
 * number; and unlinked is 0: two consecutive mapped windows of a read are an edge of the adjacency, and where they lie in different
 * runs that edge is a link.  unlinked != 0 says the paths and the links belong to different graphs.  The support is a property of
 * the pair of NODES the link joins, not of the compaction.
 * EVEN k.  A link into a palindromic one-node unitig names one orientation only and may have no mirror slot (see
 * kmx_count_unitig_links): the rule above then adds to one slot, and the two directions of such an edge need not carry the same
 * number.  And a palindromic window always reads d = 1 (kmx_count_read_paths) while a link into the palindrome names the orientation
 * of the node it comes from: where the two differ the junction finds no slot and is UNLINKED.  At even k unlinked counts such
 * junctions, and only such, for paths and links of one graph.
 * d_segments / n_segments as kmx_count_read_paths(2) wrote them, d_offsets (U + 1 u64) as kmx_count_unitigs(2), d_link_offsets
 * (2 U + 1 u64) / d_links / n_links as kmx_count_unitig_links.  Indices only: one call for both key widths.  Exact and
 * deterministic: integer sums only, so repeated calls give identical bytes.  n_segments < 2 is a no-op.  NULL ctx / d_summary,
 * n_segments or n_unitigs above 2^40, n_links above 2^43, d_segments NULL with n_segments > 0, d_offsets or d_link_offsets NULL with
 * n_unitigs > 0, d_links or d_support NULL with n_links > 0: KMX_E_ARG.  Working set: none.  Asynchronous. */
#define KMX_LS_WORDS 3u
#define KMX_LS_JUNCTIONS 0u /* pairs of consecutive segments of one read without a gap between them */
#define KMX_LS_CROSSED 1u   /* ... that cross a link slot */
#define KMX_LS_UNLINKED 2u  /* ... that do not: 0 for paths over the graph the links were made of */
int kmx_count_link_support(kmx_ctx *ctx, const uint64_t *d_segments, uint64_t n_segments, const uint64_t *d_offsets, uint64_t n_unitigs,
                           const uint64_t *d_link_offsets, const uint64_t *d_links, uint64_t n_links, uint64_t *d_support,
                           uint64_t *d_summary);

/* The adjacency without chosen links: d_edges_out (n bytes) = d_edges with one bit cleared per cut link slot.  Slot
 * l = d_link_offsets[t] + d is the d-th link of oriented unitig t as kmx_count_unitig_links derives it from these same arrays: it
 * comes from bit 4 o + c of d_edges[i], v = 2 i + o the exit node of t and c the d-th base, in ascending order, that gives a link.
 * If l < n_links and d_cut[l] != 0 (d_cut: one byte per link slot), that bit is 0 in d_edges_out[i]; every other bit is copied.  The
 * call re-derives the links, it does not read them: d_link_offsets must be the offsets kmx_count_unitig_links wrote for these
 * arrays, or the slots mean something else (any bytes still give a result and no access outside the arrays).
 * d_flips and d_nbr go on unchanged with d_edges_out: a neighbour word behind a cleared bit is stale and harmless --
 * kmx_count_unitig_ends, kmx_count_unitigs(2) and kmx_count_unitig_links read d_nbr only under a set edge bit.  The result feeds
 * kmx_count_unitigs(2) and kmx_count_unitig_links: cut, then compact again.
 * ONE-SIDED CUTS are legal: a bit cleared at one end of an edge only leaves the other end pointing at a node that no longer points
 * back, which the unitigs' mutual-link rule and the END rule already handle.  To remove an edge in both directions pass a mask that
 * is closed under the mirror, (t -> t') with (t' ^ 1 -> t ^ 1); d_support[l] < min_support is one wherever mirrors exist.
 * What a cut does not see: a false join INSIDE a unitig is not a link.
 * d_edges_out must not overlap d_edges (the bits are re-derived from the input while the output is cut): KMX_E_ARG.  The bits are
 * cleared by atomic ANDs on the aligned 32-bit word that holds the byte -- neighbouring entries share it -- so up to three bytes
 * before and after an output array that is not 4-byte aligned are ANDed with ones: rewritten with the value they hold.
 * n == 0 is a no-op; n_unitigs == 0 or n_links == 0 copies the edges.  NULL ctx, n or n_unitigs above 2^40, n_links above 2^43,
 * d_edges or d_edges_out NULL with n > 0, any other array NULL with n, n_unitigs and n_links > 0: KMX_E_ARG.  One call for both key
 * widths.  Deterministic.  Working set: none.  Asynchronous. */
int kmx_count_adjacency_cut(kmx_ctx *ctx, const uint8_t *d_edges, const uint8_t *d_flips, const uint64_t *d_nbr, uint64_t n,
                            const uint64_t *d_nodes, const uint64_t *d_offsets, uint64_t n_unitigs, const uint64_t *d_place,
                            const uint64_t *d_link_offsets, uint64_t n_links, const uint8_t *d_cut, uint8_t *d_edges_out);

/* ---------------------------------------------------------------- set algebra and comparison of two count tables ----
 * BUILD-DEFINED.  Two TABLES (as above: keys ascending and distinct, one u64 count per key; two-word keys as (low, high) pairs in
 * 16-byte aligned arrays, KMX_E_ARG otherwise) go in, a table comes out -- it feeds every other table call -- or a record of sums.
 * The calls assume sorted tables and do not check: tables that are not sorted give wrong answers (a result that is not a table,
 * even one longer than n_a + n_b, which max_out then refuses like any other), never an access outside the arrays.  n_a, n_b up to 2^40 (KMX_E_ARG above); an empty table on either side is valid and its pointers may be NULL. */
#define KMX_SETOP_INTERSECT 0
#define KMX_SETOP_UNION 1
#define KMX_SETOP_SUBTRACT 2
#define KMX_SETOP_SYMDIFF 3
#define KMX_SETOP_COUNTER_SUBTRACT 4
#define KMX_RULE_SUM 0
#define KMX_RULE_MIN 1
#define KMX_RULE_MAX 2
#define KMX_RULE_LEFT 3
#define KMX_RULE_RIGHT 4
/* op:   KMX_SETOP_INTERSECT         the keys both tables hold
 *       KMX_SETOP_UNION             the keys either table holds
 *       KMX_SETOP_SUBTRACT          the keys of a that b does not hold, with a's counts
 *       KMX_SETOP_SYMDIFF           the keys exactly one table holds, with that table's count
 *       KMX_SETOP_COUNTER_SUBTRACT  the keys of a; count_a - count_b where b holds the key, the key dropped where count_a <= count_b
 * rule: the count of a key BOTH tables hold, for INTERSECT and UNION -- KMX_RULE_SUM (count_a + count_b, wrapping mod 2^64 exactly
 *       as kmx_count_merge adds), KMX_RULE_MIN, KMX_RULE_MAX, KMX_RULE_LEFT (count_a), KMX_RULE_RIGHT (count_b).  A key of UNION that
 *       one table holds keeps that table's count whatever the rule.  The other three operations take no rule: it must be 0.
 * An op or rule outside these lists, or a rule on an operation that takes none: KMX_E_ARG.  UNION with KMX_RULE_SUM is
 * bit-identical to kmx_count_merge on the same inputs.
 * A count array the operation never reads may be NULL: d_counts_b for SUBTRACT and for INTERSECT with KMX_RULE_LEFT ("the entries
 * of a whose key is / is not in the key SET b"), d_counts_a for INTERSECT with KMX_RULE_RIGHT.  NULL anywhere else with n > 0:
 * KMX_E_ARG.
 * Outputs: the conventions of kmx_count_merge -- *h_n_out (host) is always set; both outputs NULL = count only; one NULL =
 * KMX_E_ARG; n_out > max_out = KMX_E_NOMEM with nothing written; outputs must not alias inputs.  Deterministic: repeated calls
 * are bit-identical.
 * Working set in the context's work buffer, per TILE of 2048 merged entries, not per entry: with tiles = ceil((n_a + n_b) / 2048),
 * 16 * (tiles + 1) bytes rounded up to 256 plus 8 * (tiles + 2) bytes rounded up to 256 (24 bytes per 2048 entries; 512 bytes for
 * one tile).  Above the cap (kmx_ctx_set_work_buffer_limit): KMX_E_NOMEM before any kernel runs.  The call uses the work buffer (a
 * following kmx_fastx_parse cannot reuse its chunk prefixes).
 * Synchronous (the size comes back to the host: one round trip): not capturable in a HIP graph. */
int kmx_count_setop(kmx_ctx *ctx, uint32_t op, uint32_t rule, const uint64_t *d_kmers_a, const uint64_t *d_counts_a, uint64_t n_a,
                    const uint64_t *d_kmers_b, const uint64_t *d_counts_b, uint64_t n_b, uint64_t *d_kmers_out, uint64_t *d_counts_out,
                    uint64_t max_out, uint64_t *h_n_out);
/* The same for two-word keys (k = 33..64): d_kmers2_a, d_kmers2_b and d_kmers2_out hold two u64 per key and must be 16-byte
 * aligned (KMX_E_ARG otherwise).  Working set and synchronisation as kmx_count_setop. */
int kmx_count_setop2(kmx_ctx *ctx, uint32_t op, uint32_t rule, const uint64_t *d_kmers2_a, const uint64_t *d_counts_a, uint64_t n_a,
                     const uint64_t *d_kmers2_b, const uint64_t *d_counts_b, uint64_t n_b, uint64_t *d_kmers2_out, uint64_t *d_counts_out,
                     uint64_t max_out, uint64_t *h_n_out);

/* What kmx_count_compare(2) fills: all u64, sums wrap mod 2^64. */
typedef struct kmx_table_compare {
    uint64_t n_both, n_only_a, n_only_b; /* keys in both tables, in a only, in b only */
    uint64_t sum_a, sum_b;               /* all counts of a / of b */
    uint64_t sum_a_both, sum_b_both;     /* the counts of a / of b over the shared keys */
    uint64_t sum_min, sum_max;           /* over the union: a key one table holds contributes min 0, max its count */
} kmx_table_compare;
/* How two tables relate, without writing a table: Jaccard = n_both / (n_both + n_only_a + n_only_b), containment of a in b =
 * n_both / (n_both + n_only_a), weighted Jaccard = sum_min / sum_max.  h_out (host) points at a kmx_table_compare (declared
 * void * so that bindings generated from the prototypes pass the record's address without a type of their own); NULL: KMX_E_ARG.
 * With BOTH count arrays NULL the three n_* fields are filled and the sums are 0; one of them NULL with n > 0: KMX_E_ARG.
 * Working set as kmx_count_setop.  Synchronous (the record comes back to the host: one round trip).  Deterministic. */
int kmx_count_compare(kmx_ctx *ctx, const uint64_t *d_kmers_a, const uint64_t *d_counts_a, uint64_t n_a, const uint64_t *d_kmers_b,
                      const uint64_t *d_counts_b, uint64_t n_b, void *h_out);
/* The same for two-word keys (16-byte aligned key arrays, KMX_E_ARG otherwise). */
int kmx_count_compare2(kmx_ctx *ctx, const uint64_t *d_kmers2_a, const uint64_t *d_counts_a, uint64_t n_a, const uint64_t *d_kmers2_b,
                       const uint64_t *d_counts_b, uint64_t n_b, void *h_out);

/* Deterministic synthetic reads (BUILD-DEFINED; the reference bench input is unseeded,
 * benches/simple_benchmark.rs:59-65): byte g of the stream = "ACGT"[(splitmix64(seed + g/32) >> 2*(g%32)) & 3].
 * Writes nbytes bytes for stream positions [first_byte, first_byte+nbytes). */
int kmx_gen_reads(kmx_ctx *ctx, uint64_t seed, uint64_t first_byte, uint8_t *d_out, uint64_t nbytes);

/* -------------------------------------- element-wise batch operations ---- */

/* naive_impl::Kmer::from(&[u8]) for n sequences of k bytes each, contiguous (kmer.rs:234-251).
 * Strict semantics: returns KMX_E_INVALID_BASE if any byte is not ACGTacgt (the reference panics,
 * mod.rs:35); *h_first_bad (host, may be NULL) receives the lowest offending byte index.
 * k in [1,32].  SYNCHRONOUS (it has to report the status). */
int kmx_kmers_from_bytes(kmx_ctx *ctx, const uint8_t *d_seqs, uint64_t n, uint32_t k, uint64_t *d_words,
                         uint64_t *h_first_bad);

/* Kmer::to_reverse_complement / get_reverse_complement_word (kmer.rs:124-147), k in [1,32].  d_out may equal d_in (in place). */
int kmx_revcomp_words(kmx_ctx *ctx, const uint64_t *d_in, uint64_t n, uint32_t k, uint64_t *d_out);

/* Kmer::to_canonical + is_canonical (kmer.rs:55-74): d_canon[i] = min(w, rc(w)); d_is_canonical[i] = (w <= rc(w)).
 * Either output may be NULL.  d_canon may equal d_in (in place). */
int kmx_canonical_words(kmx_ctx *ctx, const uint64_t *d_in, uint64_t n, uint32_t k, uint64_t *d_canon,
                        uint8_t *d_is_canonical);

/* hash_one(&state, Kmer) with state = LexHasherState::new(hasher_k) (hash.rs:10-20,60-71) or identity.  d_out may equal d_in
 * (in place). */
int kmx_hash_words(kmx_ctx *ctx, const uint64_t *d_in, uint64_t n, uint32_t hasher, uint32_t hasher_k, uint64_t *d_out);

/* hash_one(&state, Kmer) with one of std's BuildHashers (hash.rs:10-20; the reference uses DefaultHasher at kmer.rs:546-557 and
 * RandomState at :564-575): std's DefaultHasher is SipHash-1-3 (one compression round, three finalisation rounds), `Hash for Kmer`
 * feeds it ONE write_u64(data) (hash.rs:4-8) -- so d_out[i] = SipHash-1-3(key0, key1; the 8 little-endian bytes of d_in[i]).
 * DefaultHasher::new() / BuildHasherDefault: key0 = key1 = 0; RandomState: its pair of random keys, which the caller holds.
 * The algorithm lives in Rust's standard library, not in the crate: restated from the SipHash paper (Aumasson, Bernstein 2012);
 * the restatement reproduces the paper's SipHash-2-4 test vectors through the same round function (tests/test_oracle_golden.py),
 * its 1-3 instance the first row of Rust's own SipHasher13 test table (library/core/tests/hash/sip.rs); no reference value for
 * 1-3 exists in the crate itself (its two tests check properties): parity is pinned to that extent.  d_out may equal d_in (in place). */
int kmx_hash_words_sip13(kmx_ctx *ctx, const uint64_t *d_in, uint64_t n, uint64_t key0, uint64_t key1, uint64_t *d_out);

/* CanonicalKmer::get_word_equivalency (canonical_kmer.rs:152-161): out[i] in KMX_{NO,IDENTITY,TWIN}_MATCH */
int kmx_match_words(kmx_ctx *ctx, const uint64_t *d_fw, const uint64_t *d_rc, const uint64_t *d_other, uint64_t n,
                    uint8_t *d_out);

/* CanonicalKmer::append_base / prepend_base on n independent (fw, rc) states, in place
 * (canonical_kmer.rs:90-101; Kmer::append_base/prepend_base kmer.rs:91-102).  d_bases are 2-bit
 * codes (A0 C1 G2 T3); d_dropped (may be NULL) receives the shifted-off base.  k in [1,31]. */
int kmx_ck_append_bases(kmx_ctx *ctx, uint64_t *d_fw, uint64_t *d_rc, const uint8_t *d_bases, uint64_t n, uint32_t k,
                        uint8_t *d_dropped);
int kmx_ck_prepend_bases(kmx_ctx *ctx, uint64_t *d_fw, uint64_t *d_rc, const uint8_t *d_bases, uint64_t n, uint32_t k,
                         uint8_t *d_dropped);

/* Encoding::encode for encoding::Naive (src/encoding/naive.rs:116-124) / Xor10 (xor10.rs:52-60):
 * n sequences of seq_len bytes each (contiguous) -> words_per_kmer u64 each, i.e.
 * Kmer::<u64,K,B>::new(seq, &enc).  enc_byte is the Naive discriminant (naive.rs:48-74);
 * Xor10 == 0x1B (Naive::ACTG).  No validity check (naive.rs:14-16 maps every byte).
 * KMX_E_TOO_LONG if seq_len > 32*words_per_kmer (bit_field would panic). */
int kmx_encode_kmers(kmx_ctx *ctx, const uint8_t *d_seqs, uint64_t n, uint32_t seq_len, uint8_t enc_byte,
                     uint32_t words_per_kmer, uint64_t *d_words);
/* Same for every length-k window of every read: the benches' `b.windows(K).map(Kmer::new)` shape
 * (benches/simple_benchmark.rs:24-34); slot layout as kmx_canonical_windows (uniform reads only). */
int kmx_encode_windows(kmx_ctx *ctx, const kmx_reads *reads, uint32_t k, uint8_t enc_byte, uint32_t words_per_kmer,
                       uint64_t *d_words);
/* Encoding::rev_comp::<K> (naive.rs:138-154; xor10.rs:86-103 B>1 loop): result base i =
 * complement(base K-1-i) for i<K, bits >= 2K unchanged.  K in [2, 32*words_per_kmer].  d_out may equal d_in (in place: a lane
 * holds all the words of its k-mer before it writes any). */
int kmx_encoding_rev_comp(kmx_ctx *ctx, const uint64_t *d_in, uint64_t n, uint32_t K, uint8_t enc_byte,
                          uint32_t words_per_kmer, uint64_t *d_out);
/* Encoding::decode (naive.rs:126-136): emits ALL 32*words_per_kmer letters per k-mer */
int kmx_encoding_decode(kmx_ctx *ctx, const uint64_t *d_in, uint64_t n, uint8_t enc_byte, uint32_t words_per_kmer,
                        uint8_t *d_seqs);

/* ---------------------------------------------------------------- decode / display direction ---- */
/* Kmer::sub_kmer_word(word, k, pos, width) (src/naive_impl/kmer.rs:156-162) for n words: (word >> 2*pos) & MASK_TABLE[width].
 * The reference asserts pos < k and pos + width <= k: KMX_E_ARG otherwise.  1 <= k <= 32 (width 32 would meet
 * MASK_TABLE[32] == 0, kmer.rs:617, and give 0 like the reference).  d_out may equal d_words (in place). */
int kmx_sub_kmer_words(kmx_ctx *ctx, const uint64_t *d_words, uint64_t n, uint32_t k, uint32_t pos, uint32_t width,
                       uint64_t *d_out);
/* String::from(Kmer) (src/naive_impl/kmer.rs:196-207, BASE_TABLE :24): n words -> n*k LOWER-case letters, base 0 first. */
int kmx_kmers_to_strings(kmx_ctx *ctx, const uint64_t *d_words, uint64_t n, uint32_t k, uint8_t *d_out);
/* kmer::bitmer_to_bytes(mer, len) (src/kmer.rs:71-91): n words -> n*len UPPER-case letters, base 0 first.  len <= 32. */
int kmx_bitmers_to_bytes(kmx_ctx *ctx, const uint64_t *d_mers, uint64_t n, uint32_t len, uint8_t *d_out);

/* ---------------------------------------------------------------- Encoding<P, B> for every utils::Data word type ----
 * src/utils.rs:4-24 implements Data for u8, u16, u32, u64 and u128; encoding::Naive is generic over it
 * (src/encoding/naive.rs:112-154; Xor10 == Naive::ACTG for u64 / u128, xor10.rs:50).  bit_field's BitArray puts flat bit i
 * into word i / BITS, bit i % BITS, so the little-endian byte image of a [P; B] is the same flat bit string for every P:
 * the arrays are passed as bytes, word_bits * words_per_kmer / 8 per k-mer, and P only decides the capacity
 * (KMX_E_TOO_LONG where bit_field would panic) and the number of letters decode() emits (word_bits * words_per_kmer / 2).
 * word_bits in {8, 16, 32, 64, 128}; at most 64 bytes per k-mer.  kmx_encoding_rev_comp_p works a byte per lane, so unlike
 * kmx_encoding_rev_comp it cannot run in place: d_out == d_in is KMX_E_ARG. */
int kmx_encode_kmers_p(kmx_ctx *ctx, const uint8_t *d_seqs, uint64_t n, uint32_t seq_len, uint8_t enc_byte,
                       uint32_t word_bits, uint32_t words_per_kmer, void *d_arrays);
int kmx_encoding_rev_comp_p(kmx_ctx *ctx, const void *d_in, uint64_t n, uint32_t K, uint8_t enc_byte, uint32_t word_bits,
                            uint32_t words_per_kmer, void *d_out);
int kmx_encoding_decode_p(kmx_ctx *ctx, const void *d_in, uint64_t n, uint8_t enc_byte, uint32_t word_bits,
                          uint32_t words_per_kmer, uint8_t *d_seqs);

/* ----------------------------------------------------------------------------------------------------------------
 * SeqVector -- the reference's 2-bit packed sequence container (src/naive_impl/seq_vector.rs).
 * Layout: base i at flat bits [2i, 2i+1] of a little-endian u64 word array, codes A0 C1 G2 T3 (it is built from
 * Kmer::from of 32-base chunks, seq_vector.rs:230-242); a vector of n bases owns ceil(n/32) words, bits past 2n are 0.
 * The caller owns `d_words`; reads stored back to back are slices [r*L, (r+1)*L) of one vector (SeqVector::slice).
 * -------------------------------------------------------------------------------------------------------------- */
/* SeqVector::push_chars (seq_vector.rs:141-161) / From<&[u8]> (:230-242, n_bases_before = 0): append `n` ASCII bases
 * to a vector that holds `n_bases_before`.  Strict like Kmer::from (kmer.rs:234-251 panics on a bad base):
 * KMX_E_INVALID_BASE with *h_first_bad = index into d_bytes of the first offending byte (the words are then
 * unspecified).  d_words must have room for ceil((n_bases_before + n)/32) words. */
int kmx_seqvec_push_chars(kmx_ctx *ctx, uint64_t *d_words, uint64_t n_bases_before, const uint8_t *d_bytes, uint64_t n,
                          uint64_t *h_first_bad);
/* String::from(&SeqVector) (seq_vector.rs:171-182): n upper-case letters */
int kmx_seqvec_to_bytes(kmx_ctx *ctx, const uint64_t *d_words, uint64_t n_bases, uint8_t *d_bytes);
/* SeqVector::get_kmer_u64(pos, k) (seq_vector.rs:96-99; get_base = k 1) for n positions; k in [1,32].
 * A position whose k-mer does not lie inside the vector (the reference asserts pos < len) gives KMX_E_ARG. */
int kmx_seqvec_get_kmers(kmx_ctx *ctx, const uint64_t *d_words, uint64_t n_bases, const uint64_t *d_pos, uint64_t n,
                         uint32_t k, uint64_t *d_out);
/* SeqVectorSlice::iter_kmers(k) (seq_vector.rs:64-71, 117-124) over the slice [start, end): end-start-k+1 forward
 * words (not canonicalised), in order. */
int kmx_seqvec_iter_kmers(kmx_ctx *ctx, const uint64_t *d_words, uint64_t n_bases, uint64_t start, uint64_t end,
                          uint32_t k, uint64_t *d_out);
/* kmx_canonical_reduce over reads held in a SeqVector: read r = slice [r*read_len, (r+1)*read_len).  Every 2-bit code
 * is a base, so every window counts.  0.25 B per base read from HBM instead of 1.  d_words 16-byte aligned for the
 * fast kernel (k in [13,31]); any k in [1,31] is served. */
int kmx_seqvec_canonical_reduce(kmx_ctx *ctx, const uint64_t *d_words, uint64_t n_reads, uint32_t read_len, uint32_t k,
                                uint32_t hasher, uint32_t hasher_k, uint32_t flags, kmx_summary *d_out);

/* ---------------------------------------------------------------- minimizers ----
 * hasher: KMX_HASH_LEX with hasher_k (LexHasherState::new(hasher_k): the k of the hasher is independent of the l-mer
 * length, minimizers.rs:240 uses 6 for 3-mers) or KMX_HASH_IDENTITY.  std's DefaultHasher / RandomState: the *_sip13 calls
 * below each counterpart. */
/* Kmer::minimizer_word(word, k, width, state) (kmer.rs:170-192) for n k-mer words: the leftmost minimum-hash
 * sub-word of `width` bases and its offset.  1 <= width <= k <= 32. */
int kmx_minimizer_words(kmx_ctx *ctx, const uint64_t *d_words, uint64_t n, uint32_t k, uint32_t width, uint32_t hasher,
                        uint32_t hasher_k, uint64_t *d_mmer, uint32_t *d_offset);
/* The same with hash_one(SipHash-1-3 state (key0, key1), l-mer) (kmer.rs:182): a lane per word, a strict `<` against a running
 * minimum that starts at u64::MAX (kmer.rs:176-189).  VALU-bound: k - width + 1 hashes per word. */
int kmx_minimizer_words_sip13(kmx_ctx *ctx, const uint64_t *d_words, uint64_t n, uint32_t k, uint32_t width,
                              uint64_t key0, uint64_t key1, uint64_t *d_mmer, uint32_t *d_offset);
/* SeqVectorSlice::iter_minimizers(k, w, hasher) (seq_vector.rs:73-80; SeqVecMinimizerIter, minimizers.rs:39-141) for
 * every read slice [r*read_len, (r+1)*read_len) of a SeqVector: MappedMinimizer{word, pos} per k-mer, slot
 * r*(read_len-k+1) + i, pos relative to the slice.  read_len >= k (the iterator asserts it), 1 <= w <= k, w <= 32. */
int kmx_seqvec_minimizers(kmx_ctx *ctx, const uint64_t *d_words, uint64_t n_reads, uint32_t read_len, uint32_t k,
                          uint32_t w, uint32_t hasher, uint32_t hasher_k, uint64_t *d_word, uint32_t *d_pos);
/* The same iterator with SipHash-1-3(key0, key1) of each l-mer (minimizers.rs:88,113): std's DefaultHasher / RandomState.  The
 * 64-bit hash does not fit the (hash << 8) | position key of the Lex kernel: a wave per slice and per piece of 256 bases, every
 * l-mer hashed once into LDS, each k-mer the leftmost minimum of its k - w + 1 hashes (the deque's tie rule, minimizers.rs:71).
 * k above 256: a lane per k-mer (each l-mer hashed once per window that holds it).  Slots, positions and codes as
 * kmx_seqvec_minimizers.  VALU-bound: 0.12e12 k-mers/s at k = 31 / w = 15 on 150-base slices (profiles/r07_sip13_bench.txt). */
int kmx_seqvec_minimizers_sip13(kmx_ctx *ctx, const uint64_t *d_words, uint64_t n_reads, uint32_t read_len, uint32_t k,
                                uint32_t w, uint64_t key0, uint64_t key1, uint64_t *d_word, uint32_t *d_pos);

/* The same iterator over READS (round 6): what SeqVector::from(read).slice(..).iter_minimizers(k, w, hasher) yields
 * (seq_vector.rs:73-80, 230-242; minimizers.rs:39-141) for every read of a batch -- ASCII, one length or behind offsets, as
 * kmx_fastx_parse hands them over -- without building the SeqVector.  MappedMinimizer{word, pos} of k-mer i of read r at slot
 * r*(read_len-k+1) + i (uniform; read_len >= k) or d_win_offsets[r] + i (ragged: n_reads + 1 entries as for kmx_canonical_windows;
 * a read shorter than k owns no slot), pos relative to the read.  1 <= w <= k, w <= 32.
 * A byte outside ACGTacgt: the reference panics (Kmer::from, kmer.rs:45-60).  With h_first_bad != NULL the call synchronises, stores
 * the index of the first read that holds one (else ~0) and returns KMX_E_INVALID_BASE; that read's slots then hold what the codes
 * (byte >> 1) & 3 spell.  With NULL nothing is checked on the host and the call stays asynchronous for uniform reads (reads behind
 * offsets cost one host round trip: their longest length selects the kernel).
 * Reads of up to 256 bases, and uniform reads of any length (cut into pieces of 256 bases), take the sliding-minimum kernel when the
 * hash fits 56 bits (w <= 28; LexHasher: hasher_k <= 28); anything else a lane-per-k-mer kernel. */
int kmx_minimizers(kmx_ctx *ctx, const kmx_reads *reads, const uint64_t *d_win_offsets, uint32_t k, uint32_t w, uint32_t hasher,
                   uint32_t hasher_k, uint64_t *d_word, uint32_t *d_pos, uint64_t *h_first_bad);
/* The same over reads with SipHash-1-3(key0, key1) of each l-mer, through the kernel of kmx_seqvec_minimizers_sip13 (a wave per read,
 * read by read in pieces of 256 bases: reads of any length, uniform or ragged).  Slots, positions, h_first_bad, KMX_E_INVALID_BASE
 * and synchronisation as kmx_minimizers (ragged reads: one host round trip for the longest read; a batch with no read of k bases
 * returns KMX_OK before any kernel runs).  k above 256: a lane per k-mer.  VALU-bound: 0.11e12 k-mers/s at k = 31 / w = 15 on
 * 150 bp reads (profiles/r07_sip13_bench.txt). */
int kmx_minimizers_sip13(kmx_ctx *ctx, const kmx_reads *reads, const uint64_t *d_win_offsets, uint32_t k, uint32_t w,
                         uint64_t key0, uint64_t key1, uint64_t *d_word, uint32_t *d_pos, uint64_t *h_first_bad);

/* ---------------------------------------------------------------- FASTA / FASTQ ingestion ----
 * BUILD-DEFINED: the reference has no parser (its iterators take `&[u8]` reads, canonical_kmer_iterator.rs:72-83);
 * this call produces, from a file image in device memory, the ragged-reads input of the calls above:
 * d_bases = the reads back to back, d_offsets[r] = first base of read r, d_offsets[n_reads] = n_bases.
 *   KMX_FASTX_FASTQ: strict 4-line records, line i is a read iff i % 4 == 1.
 *   KMX_FASTX_FASTA: a line starting with '>' opens a record; every other line up to the next '>' line is its sequence.
 *   KMX_FASTX_AUTO:  by the first byte ('@' / '>').
 * Lines end at '\n'; every '\r' on a sequence line is dropped; the last line may lack its '\n'.  Bases are copied as
 * they are (lower case, N, ...: the k-mer calls treat them as the reference's iterator does).  A text that does not
 * start with '@' / '>' gives KMX_E_ARG.
 * d_text 16-byte aligned.  d_bases: room for n_bases bytes (n_bytes always suffices); d_offsets: max_reads+1 words.
 * With d_bases == d_offsets == NULL only the counts are computed; if n_reads > max_reads nothing is written, the counts
 * are returned and the status is KMX_E_NOMEM.  Synchronises the context's stream (the counts come back to the host). */
#define KMX_FASTX_AUTO 0
#define KMX_FASTX_FASTQ 1
#define KMX_FASTX_FASTA 2
/* OR-ed into `format` on the second call of the usual pair (counts first, then the emit into buffers of exactly that
 * size): "d_text / n_bytes are the image the previous kmx_fastx_parse call on this context counted, unchanged, and no
 * kmx_histogram call came in between" -- the emit then reuses the chunk summaries of the counting call instead of
 * reading the text a third time (the pair: 1.06 -> 1.4 TB/s of text).  Ignored when the context has nothing to reuse. */
#define KMX_FASTX_SAME_TEXT 0x100u
int kmx_fastx_parse(kmx_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint32_t format, uint8_t *d_bases,
                    uint64_t *d_offsets, uint64_t max_reads, uint64_t *h_n_reads, uint64_t *h_n_bases);
/* The longest and the shortest read of a ragged batch (d_offsets: n_reads+1 device u64, as kmx_fastx_parse writes them):
 * what kmx_reads.read_len wants as its bound for ragged input (the tiled kernels size their frame and the windows per
 * lane from it; a tight bound is up to 7 % faster than none), and whether the batch is uniform after all (min == max:
 * hand it over with d_offsets = NULL, or pack it with kmx_seqvec_push_chars).  Lengths of 2^32 or more come back as
 * UINT32_MAX.  BUILD-DEFINED helper; synchronises the context's stream (the two values come back to the host). */
int kmx_reads_length_range(kmx_ctx *ctx, const uint64_t *d_offsets, uint64_t n_reads, uint32_t *h_min_len, uint32_t *h_max_len);

/* ---------------------------------------------------------------- a new batch of reads from an old one: select, trim, gather ----
 * BUILD-DEFINED.  The per-read answers of the count family -- a median, a longest solid run, a colour, a component -- acted on: reads
 * are kept or dropped, clipped to a span, reordered or repeated, and the result is a ragged batch again (bytes back to back, n + 1
 * offsets starting at 0) that every call taking kmx_reads accepts.  Both calls take every layout of kmx_reads: uniform reads
 * (d_offsets == NULL), ragged reads with d_offsets[0] > 0, any d_bases alignment, empty reads.
 * THE SPAN OF A READ.  d_span == NULL: the whole read.  Otherwise the span word of SOURCE read r is w = d_span[r * span_stride]
 * (span_stride: the u64 words between the span words of consecutive reads, >= 1; 0 with a non-NULL d_span is KMX_E_ARG), with
 * start = w & 0xFFFFFFFF, len = w >> 32, and L the read's length:
 *     span_k == 0:  len counts bases:                 keep [start, start + len) within [0, L)
 *     span_k  > 0:  len counts windows of span_k bases, the packing of KMX_RS_SPAN and KMX_PATH_SPAN: len == 0 keeps nothing,
 *                   otherwise keep [start, start + len + span_k - 1) within [0, L)
 * All arithmetic is in 64 bits; start >= L keeps nothing: any bytes give one defined answer.  A source read of 2^31 bases or more
 * counts as empty (L = 0), in line with the scans, which skip it; an offsets pair that descends likewise.
 * With d_stats the rows of kmx_count_read_stats(2) for the same reads, (d_stats + KMX_RS_SPAN, KMX_RS_WORDS, k) trims every read to
 * its longest run of solid windows without an array in between.
 *
 * kmx_reads_select.  Source read r is KEPT iff (d_keep == NULL or d_keep[r] != 0) and its clipped length is >= min_len; with
 * min_len == 0 a kept read whose clip is empty stays in the batch as an empty read.  The clips of the kept reads are written back to
 * back in source order to d_out_bases; d_out_offsets gets n_out + 1 words, the first 0, the last n_bases; d_out_index (optional) gets
 * n_out words, the source index of every output read.  *h_n_reads / *h_n_bases (host) = n_out / n_bases, always.  Both of d_out_bases
 * and d_out_offsets NULL = count only; exactly one of them NULL = KMX_E_ARG.  n_out > max_reads or n_bases > max_bases:
 * KMX_E_NOMEM with nothing written and the counts set (d_out_offsets holds max_reads + 1 words, d_out_bases max_bases bytes,
 * d_out_index max_reads words).  Not one byte of d_out_bases at or past n_bases is written, nor a word of the other two past
 * what is stated here.  d_out_bases must not overlap the source reads: KMX_E_ARG where the host can tell (the bytes the batch spans
 * against the n_bases bytes written).  n_reads == 0 is a no-op with both counts 0 (nothing is written).  n_reads up to 2^40.
 *
 * kmx_reads_gather.  Output read j, j < n_index, is the clip of source read d_index[j]; the span is looked up by the SOURCE index.
 * Repeats are allowed; an index >= n_reads gives an empty read.  Exactly n_index output reads and n_index + 1 offsets are written,
 * n_bases bytes of d_out_bases, *h_n_bases = n_bases; count only and KMX_E_NOMEM (n_bases > max_bases) as above.  n_index == 0 is a
 * no-op with a count of 0.  n_index up to 2^32 (the sum of 2^32 clips of less than 2^31 bases fits 64 bits).  The primitive for
 * reordering and partitioning: a stable sort of labels gives the index.
 *
 * Working set in the work buffer, laid out before any kernel runs, with m = n_reads (select) or n_index (gather):
 * a256(8 * m) + a256(8 * (2 * ceil(m / 2048) + 4)) -- the source start of every output read (its length is the difference of its
 * output offsets), and two partial sums per 2048 reads with the four words that come back to the host.  Above the cap
 * (kmx_ctx_set_work_buffer_limit): KMX_E_NOMEM before any kernel runs, nothing written.  Deterministic: repeated calls give
 * identical bytes.  NULL ctx / reads / host pointers, d_index NULL with n_index > 0: KMX_E_ARG.  Both calls are synchronous (the
 * counts come back to the host; they return after the copy has finished). */
int kmx_reads_select(kmx_ctx *ctx, const kmx_reads *reads, const uint8_t *d_keep, const uint64_t *d_span, uint64_t span_stride,
                     uint32_t span_k, uint64_t min_len, uint8_t *d_out_bases, uint64_t *d_out_offsets, uint64_t *d_out_index,
                     uint64_t max_reads, uint64_t max_bases, uint64_t *h_n_reads, uint64_t *h_n_bases);
int kmx_reads_gather(kmx_ctx *ctx, const kmx_reads *reads, const uint64_t *d_index, uint64_t n_index, const uint64_t *d_span,
                     uint64_t span_stride, uint32_t span_k, uint8_t *d_out_bases, uint64_t *d_out_offsets, uint64_t max_bases,
                     uint64_t *h_n_bases);

/* ---------------------------------------------------------------- FASTQ qualities: parse, mask, trim, per-read rows ----
 * BUILD-DEFINED.  kmx_fastx_parse keeps line 1 of every FASTQ record; the two calls here bring line 3 to the device and act on it.
 *
 * kmx_fastx_parse_quals.  The contract of kmx_fastx_parse(KMX_FASTX_FASTQ) with line i % 4 == 3 in place of line i % 4 == 1:
 * d_quals = the quality lines back to back, d_qoffsets[r] = first byte of quality line r, d_qoffsets[n_reads] = n_bytes out.  Lines
 * end at '\n'; every '\r' is dropped; the last line may lack its '\n'; a quality line may hold any other byte ('@' and '>' included:
 * the records are four lines, whatever the lines hold).  A quality line exists as soon as it has a byte or its '\n': a text cut off
 * before its last quality line has one quality line fewer than reads.  format: KMX_FASTX_AUTO or KMX_FASTX_FASTQ; KMX_FASTX_FASTA, or a
 * text that does not begin with '@', gives KMX_E_ARG.  d_text 16-byte aligned; d_quals: room for the bytes (n_bytes always suffices);
 * d_qoffsets: max_reads + 1 words.  d_quals == d_qoffsets == NULL: only the counts; n_reads > max_reads: KMX_E_NOMEM with nothing
 * written and the counts set.  *h_n_reads / *h_n_bytes (host, optional) = quality lines / bytes kept.
 * With d_read_offsets (what kmx_fastx_parse wrote for the same image: at least n_reads + 1 words) and h_first_mismatch both given, the
 * lengths of the two offsets arrays are compared on the device: *h_first_mismatch = the smallest r whose quality line and sequence
 * line differ in length, ~0 if there is none.  The status stays KMX_OK: what a mismatch means is the caller's business.
 * KMX_FASTX_SAME_TEXT may be OR-ed into `format` under the contract stated at kmx_fastx_parse, where "the previous call" is any of
 * the parse calls (kmx_fastx_parse_names below included): the chunk summaries of pass 1 serve them all, so reads and qualities of one image cost one summarising pass less,
 * and a count-then-emit pair of this call reuses the count whole.  Synchronous. */
int kmx_fastx_parse_quals(kmx_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint32_t format, uint8_t *d_quals,
                          uint64_t *d_qoffsets, uint64_t max_reads, const uint64_t *d_read_offsets, uint64_t *h_n_reads,
                          uint64_t *h_n_bytes, uint64_t *h_first_mismatch);

/* kmx_reads_quality.  One pass over the bases and the quality bytes of a batch.  d_quals is laid out as the reads are: the quality
 * byte of base i of read r is d_quals[d_offsets[r] + i] (uniform reads: d_quals[r * read_len + i]).  Every layout kmx_reads_select
 * takes is taken: uniform and ragged reads, d_offsets[0] > 0, empty reads, any alignment of d_bases, and any alignment of d_quals
 * independently.  A read of 2^31 bases or more, or an offsets pair that descends, counts as empty.
 *     q = byte >= phred_base ? byte - phred_base : 0          a base is GOOD iff it is one of ACGTacgt and q >= min_q
 * d_masked (optional): same layout, same offsets; a base with q < min_q becomes 'N', every other byte is copied as it is -- so every
 * k-mer call skips the windows over a low base.  d_masked == d_bases (in place) is allowed; any other overlap of d_masked with the
 * bases, and any with the quality bytes, is KMX_E_ARG where the host can tell (the bytes the batch spans; ragged reads: one round
 * trip for its first and last offset).  Not one byte outside the bytes of the reads is written, and no load touches an aligned dword
 * that holds no byte of the batch.
 * d_rows (optional): KMX_RQ_WORDS u64 per read, the words below.  At least one of d_masked and d_rows must be given.
 * THE TRIM SPAN (Mott / BWA).  s_i = q_i - trim_q (signed), P_0 = 0, P_{i+1} = P_i + s_i, V = max over 0 <= a <= b <= L of P_b - P_a.
 * V == 0: the word is 0.  Otherwise b* = the smallest b with max_{a <= b}(P_b - P_a) = V, a* = the largest a < b* with
 * P_b* - P_a = V, and the word is a* | (b* - a*) << 32: the first and the last base of the span both have q > trim_q.  All sums are
 * 64-bit.  KMX_RQ_TRIM and KMX_RQ_RUN are span words in bases: kmx_reads_select takes (d_rows + KMX_RQ_TRIM, KMX_RQ_WORDS, 0).
 * d_weights (optional): 256 device words, indexed by the RAW quality byte; with a table of round(2^32 * 10^(-q / 10)) KMX_RQ_WEIGHT is
 * the read's expected errors in exact integer arithmetic.
 * phred_base, min_q or trim_q above 255, d_quals NULL with bases present, both outputs NULL, NULL ctx / reads: KMX_E_ARG.  n_reads
 * up to 2^40; n_reads == 0 is a no-op.  Deterministic (no atomics: a row is written by the one wave that owns its read).
 * Asynchronous on the context's stream (ragged reads with d_masked: after the one round trip above). */
#define KMX_RQ_WORDS 8u
#define KMX_RQ_BASES 0u   /* L */
#define KMX_RQ_LOW 1u     /* bases with q < min_q */
#define KMX_RQ_QSUM 2u    /* sum of q */
#define KMX_RQ_WEIGHT 3u  /* sum of d_weights[byte] over the raw quality bytes, wrapping mod 2^64; 0 when d_weights == NULL */
#define KMX_RQ_MINMAX 4u  /* min q | max q << 32; 0 for an empty read */
#define KMX_RQ_TRIM 5u    /* the trim span: start | len << 32, in bases; 0 when V == 0 */
#define KMX_RQ_RUN 6u     /* the longest run of GOOD bases: start | len << 32, of equal runs the leftmost; 0 when there is none */
#define KMX_RQ_WINDOWS 7u /* windows of k bases that are all GOOD (what a k-mer call yields on the masked read); 0 for k == 0 */
int kmx_reads_quality(kmx_ctx *ctx, const kmx_reads *reads, const uint8_t *d_quals, uint32_t phred_base, uint32_t min_q,
                      uint32_t trim_q, uint32_t k, const uint64_t *d_weights, uint8_t *d_masked, uint64_t *d_rows);

/* ---------------------------------------------------------------- adapter read-through: 3' adapters, the overlap of two mates ----
 * BUILD-DEFINED (the reference has nothing like it): what cutadapt, fastp and Trimmomatic do between the parse and the count.  Both
 * calls produce rows only; kmx_reads_select clips the reads by a word of a row.  Both take every layout kmx_reads_select takes:
 * uniform and ragged reads, d_offsets[0] > 0, empty reads, any alignment of d_bases; a read of 2^31 bases or more, or an offsets pair
 * that descends, counts as empty (L = 0).  No load touches an aligned dword that holds no byte of the batch.  Both are asynchronous
 * on the context's stream, use no work buffer and no atomics (a row is written by the one wave that owns its read: repeated calls
 * give identical bytes), and n_reads == 0 is a no-op (its arguments are still checked).  n_reads up to 2^40.
 *
 * kmx_reads_adapter.  The leftmost 3' adapter hit of every read.  h_adapters (HOST): the adapters back to back, h_adapter_lens[a]
 * (HOST) bytes each; 1 <= n_adapters <= KMX_RA_MAX_ADAPTERS, 1 <= length <= KMX_RA_MAX_ADAPTER_LEN.  An adapter byte is one of
 * ACGTacgt, or N / n: a wildcard.  They travel as bit planes in the kernel arguments: no upload, no host round trip.
 * With L the read's length and A the length of adapter a, for a position p in [0, L):
 *     n(p) = min(A, L - p)                                        the overlap
 *     read base p + j MATCHES adapter base j  iff  the adapter base is a wildcard, or both are one of ACGTacgt and the same letter
 *                                                  whatever the case (a read byte that is not ACGTacgt matches only a wildcard)
 *     m(p) = the number of j < n(p) that do not match
 *     p is a HIT of a  iff  n(p) >= min_overlap  and  m(p) * err_den <= err_num * n(p)                       (64-bit arithmetic)
 * The read's hit is the smallest p that is a hit of any adapter; of the adapters that hit there, the smallest index.
 * (d_rows + KMX_RA_KEEP, KMX_RA_WORDS, 0) is what kmx_reads_select takes; a hit at p = 0 keeps nothing (an adapter dimer).
 * NULL ctx / reads / d_rows / h_adapters / h_adapter_lens, n_adapters or a length out of range, any other adapter byte,
 * min_overlap == 0, err_den == 0, err_num > err_den: KMX_E_ARG. */
#define KMX_RA_MAX_ADAPTERS 8u
#define KMX_RA_MAX_ADAPTER_LEN 64u
#define KMX_RA_WORDS 4u
#define KMX_RA_KEEP 0u  /* span word in bases, 0 | len << 32: len = p on a hit, otherwise L */
#define KMX_RA_HIT 1u   /* 0 without a hit, otherwise (a + 1) | n(p) << 16 | m(p) << 32 */
#define KMX_RA_BASES 2u /* L */
#define KMX_RA_HITS 3u  /* bit a set iff adapter a hits anywhere in the read */
int kmx_reads_adapter(kmx_ctx *ctx, const kmx_reads *reads, const uint8_t *h_adapters, const uint32_t *h_adapter_lens,
                      uint32_t n_adapters, uint32_t min_overlap, uint32_t err_num, uint32_t err_den, uint64_t *d_rows);

/* kmx_reads_pair_overlap.  The insert size of every mate pair from the overlap of the mates: read-through found without knowing
 * the adapter.  Pair r is read r of reads1 and read r of reads2 (reads1->n_reads != reads2->n_reads: KMX_E_ARG); the two batches
 * have layouts, offsets and alignments of their own.  X = mate 1 (L1 bases), Y = the reverse complement of mate 2 (L2 bases); a
 * byte that is not ACGTacgt matches nothing, and there are no wildcards.  For an integer d with -L2 < d < L1:
 *     X[i] is compared with Y[i - d] for i in [max(0, d), min(L1, d + L2));  n(d) = the length of that range, m(d) = the mismatches
 *     d is a HIT  iff  n(d) >= min_overlap  and  m(d) <= max_mism  and  m(d) * err_den <= err_num * n(d)     (64-bit arithmetic)
 * Of all hits the one with the largest n is taken, of equal n the largest d (the longer insert: less is trimmed).  The insert size
 * is I = d + L2.  A pair of which either mate is longer than KMX_RP_MAX_LEN bases has no hit, by definition (paired reads do not
 * get there, and it bounds the plane words a wave keeps).  The argument errors of kmx_reads_adapter. */
#define KMX_RP_MAX_LEN 1024u
#define KMX_RP_WORDS 4u
#define KMX_RP_INSERT 0u  /* I on a hit, 0 without */
#define KMX_RP_OVERLAP 1u /* n | m << 32, 0 without a hit */
#define KMX_RP_KEEP1 2u   /* span word in bases for mate 1: 0 | min(L1, I) << 32; without a hit 0 | L1 << 32 */
#define KMX_RP_KEEP2 3u   /* the same for mate 2 in its own orientation: 0 | min(L2, I) << 32; without a hit 0 | L2 << 32 */
int kmx_reads_pair_overlap(kmx_ctx *ctx, const kmx_reads *reads1, const kmx_reads *reads2, uint32_t min_overlap, uint32_t max_mism,
                           uint32_t err_num, uint32_t err_den, uint64_t *d_rows);

/* ---------------------------------------------------------------- overlapping mate pairs merged into consensus reads ----
 * BUILD-DEFINED (the reference has nothing like it): what fastp --merge, PEAR, FLASH and vsearch --fastq_mergepairs do with the
 * insert size kmx_reads_pair_overlap finds.  kmx_reads_pair_merge writes a new ragged batch -- bases, quality bytes, offsets -- out
 * of two: output read r is the merged read of pair r, or EMPTY where the pair does not merge, so the output has exactly n_reads
 * reads and stays in step with the pairs (a kmx_reads_select with min_len = 1 compacts it).
 *
 * Pair r is read r of reads1 and read r of reads2 (reads1->n_reads != reads2->n_reads: KMX_E_ARG).  Every layout
 * kmx_reads_pair_overlap takes is taken: uniform or ragged, d_offsets[0] > 0, empty mates, alignments of their own; a mate of 2^31
 * bases or more, or an offsets pair that descends, has length 0.  d_quals1 / d_quals2 are laid out as their bases are (the rule of
 * kmx_reads_quality), each at any alignment of its own.  d_insert[r * insert_stride] is the insert size of pair r:
 * (d_rows of kmx_reads_pair_overlap + KMX_RP_INSERT, KMX_RP_WORDS) is handed over with no array in between.
 *
 * WHICH PAIRS MERGE.  L1, L2 = the mates' lengths, I = the insert word, d = I - L2 (signed).  The pair merges iff
 *     1 <= L1, L2 <= KMX_RP_MAX_LEN   and   0 < I < L1 + L2            (that is -L2 < d < L1: at least one position overlaps)
 * Any other word (0 = no hit, garbage, too large) means not merged: any bytes give one defined answer.  The insert is trusted: no
 * mismatch threshold is tested again, what is found goes into the row.
 *
 * THE MERGED READ M has I bases.  X[i] = byte i of mate 1; Y[j] = the complement of byte L2 - 1 - j of mate 2 (A<->T, C<->G,
 * a<->t, c<->g: the case is kept; any other byte becomes 'N').  Position i of M, in [0, I), is covered by X iff i < L1 and by Y iff
 * i >= max(d, 0), as Y[i - d]; X at or past I and Y before 0 are read-through and dropped.  q of a quality byte is
 * byte >= phred_base ? byte - phred_base : 0.
 *     X alone: the base and the quality byte of mate 1, raw.     Y alone: Y[i - d] and the raw quality byte L2 - 1 - (i - d) of mate 2.
 *     both ("valid" = one of ACGTacgt); the quality byte written is phred_base + q:
 *       AGREE  both valid, the same letter whatever the case    X's byte                                       q = min(qx + qy, q_cap)
 *       DIS    both valid, the letters differ                   Y's byte iff qy > qx, else X's (a tie: mate 1)  q = min(|qx - qy|, q_cap)
 *       ONE    exactly one valid                                that one's byte                                q = min(its q, q_cap)
 *       NONE   neither valid                                    'N'                                            q = 0
 * d_quals1 == d_quals2 == NULL: every q is 0 (mate 1 wins every DIS) and d_out_quals must be NULL; exactly one of the two NULL, or
 * d_out_quals without them: KMX_E_ARG.  With them d_out_quals is optional.
 *
 * OUTPUTS.  d_out_offsets: n_reads + 1 words, the first 0, the last n_bases; d_out_bases and d_out_quals: the reads back to back by
 * those offsets, each at any alignment.  d_rows (optional): KMX_RM_WORDS u64 per pair.  *h_n_merged, *h_n_bases: always set.
 * d_out_bases == d_out_offsets == NULL (d_out_quals NULL as well): only the counts, and the rows where d_rows is given; exactly one
 * of the two NULL: KMX_E_ARG.  n_bases > max_bases: KMX_E_NOMEM with the counts set and no byte of the three batch outputs written.
 * No byte at or past n_bases is written, no word past n_reads + 1 offsets or KMX_RM_WORDS * n_reads row words; no load touches an
 * aligned dword that holds no byte of its batch.  An output that overlaps an input (bases, quality bytes, offsets, insert words),
 * where the host can tell: KMX_E_ARG.  phred_base + q_cap > 255, insert_stride == 0 or d_insert NULL with pairs present, NULL ctx /
 * reads / h_n_merged / h_n_bases: KMX_E_ARG.  n_reads == 0 is a no-op with both counts 0, its arguments still checked; n_reads up
 * to 2^40.  Working set: the partial sums of the plan, 16 bytes per 2048 pairs and six words, laid out in the work buffer before any
 * kernel runs; above the work buffer's cap KMX_E_NOMEM with nothing written.  Synchronous (the counts come back to the host); no
 * atomics: repeated calls give identical bytes. */
#define KMX_RM_WORDS 4u
#define KMX_RM_LEN 0u     /* I if merged, otherwise 0 (and the other words 0) */
#define KMX_RM_OVERLAP 1u /* n | DIS << 32: n = min(L1, I) - max(d, 0) overlapping positions, DIS of them disagree */
#define KMX_RM_TAKEN 2u   /* DIS positions taken from mate 2 | DIS positions with qx == qy << 32 */
#define KMX_RM_INVALID 3u /* ONE | NONE << 32 */
int kmx_reads_pair_merge(kmx_ctx *ctx, const kmx_reads *reads1, const kmx_reads *reads2, const uint8_t *d_quals1,
                         const uint8_t *d_quals2, const uint64_t *d_insert, uint64_t insert_stride, uint32_t phred_base,
                         uint32_t q_cap, uint8_t *d_out_bases, uint8_t *d_out_quals, uint64_t *d_out_offsets, uint64_t *d_rows,
                         uint64_t max_bases, uint64_t *h_n_merged, uint64_t *h_n_bases);

/* ---------------------------------------------------------------- poly-X ends, base composition, low complexity ----
 * BUILD-DEFINED (the reference has nothing like it): what fastp --trim_poly_g / --trim_poly_x / --low_complexity_filter, cutadapt
 * --poly-a and the DUST score of prinseq / sdust do between the parse and the count.  kmx_reads_complexity is one pass over the
 * bases of a batch, without quality bytes and without a table.  Every layout kmx_reads_quality takes is taken: uniform and ragged
 * reads, d_offsets[0] > 0, empty reads, any alignment of d_bases and of d_masked independently.  A read of 2^31 bases or more, or an
 * offsets pair that descends, counts as empty (L = 0).  Letters are compared with the case ignored; a byte that is not one of
 * ACGTacgt is INVALID: it matches no letter.
 *
 * THE POLY-X RULE.  The bits of tail_bases and head_bases select letters: bit 0 A, bit 1 C, bit 2 G, bit 3 T (tail_bases = 4 is
 * fastp's --trim_poly_g, 15 its --trim_poly_x).  For a letter X and the suffix of the read that starts at p:
 *     n = L - p        m = the number of its bases that are not X        s = n - (penalty + 1) * m            (signed, 64-bit)
 *     the suffix QUALIFIES  iff  base p is X  and  n >= min_len  and  m * err_den <= err_num * n        (64-bit arithmetic)
 * With penalty = 2 a match is worth +1 and a mismatch -2: cutadapt's poly-A scoring.  The tail for X is the qualifying suffix with
 * the largest s, of equal s the longest; the read's tail is the best over the selected letters by the same order, then the lowest
 * bit.  The head is the mirror image on the prefixes that END at p, base p being X, with head_bases.  With t and h the two lengths
 * (0 where there is none) the KEEP span is empty (the word 0) if h + t >= L, otherwise start h, length L - h - t; with both masks 0
 * it is the whole read.  (d_rows + KMX_RX_KEEP, KMX_RX_WORDS, 0) is what kmx_reads_select takes.
 *
 * COMPOSITION AND NEIGHBOURS.  The counts of A, C, G and T; P = the positions i with bases i and i + 1 both valid, D = those of
 * them whose two letters differ.  D / P is fastp's complexity with invalid bytes left out (its filter drops reads below 0.30).
 *
 * THE DUST NUMERATORS.  Window j covers the bases [32 j, min(32 j + 64, L)); there are W = 0 windows for L = 0, 1 for L <= 64,
 * ceil((L - 64) / 32) + 1 otherwise.  A triplet of a window COUNTS when it lies wholly inside the window and its three bases are
 * valid; c_t = the counted triplets that spell t; S_j = the sum over t of c_t * (c_t - 1) / 2.  A full window of one letter has
 * S = 1891, (AC)n 930, (ACG)n 610, random bases about 30; S / 61 is the sdust / prinseq score of a full window (sdust's threshold of
 * 2 is a dust_max of about 122).  Window j is DUSTY iff S_j > dust_max; dust_max >= 1891 means never.  The windows are taken over
 * the WHOLE read, not over the keep span: a caller who wants the trimmed read scored selects first and calls again.
 * d_masked (optional): same layout, same offsets; a base becomes 'N' iff it lies in at least one DUSTY window, every other byte of
 * every read is copied as it is -- so every k-mer call skips the windows over a masked base.  d_masked == d_bases (in place) is
 * allowed; any other overlap with the bases is KMX_E_ARG where the host can tell, exactly as kmx_reads_quality decides it.  Not one
 * byte outside the bytes of the reads is written, and no load touches an aligned dword that holds no byte of the batch.
 * d_rows (optional): KMX_RX_WORDS u64 per read, the words below.  At least one of d_masked and d_rows must be given; without d_rows
 * the poly-X arguments are checked and not used.
 * Not done here: entropy over k-mers (BBDuk), soft (lower-case) masking, the merging of DUST intervals as sdust does it.
 * A base mask above 15, err_den == 0, err_num > err_den, min_len == 0 with a nonzero base mask, penalty > 255, both outputs NULL,
 * NULL ctx / reads: KMX_E_ARG.  n_reads up to 2^40; n_reads == 0 is a no-op whose arguments are still checked.  No work buffer, no
 * atomics: a row and the bytes of a read are written by the one wave that owns the read, so repeated calls give identical bytes.
 * Asynchronous on the context's stream (ragged reads with d_masked: after the one round trip for the batch's first and last
 * offset). */
#define KMX_RX_WORDS 8u
#define KMX_RX_KEEP 0u  /* span word in bases: start | len << 32 (what kmx_reads_select takes with span_k = 0) */
#define KMX_RX_BASES 1u /* L */
#define KMX_RX_TAIL 2u  /* 0 without a tail, otherwise t | (bit index of X + 1) << 32 */
#define KMX_RX_HEAD 3u  /* the same for the head */
#define KMX_RX_AC 4u    /* count of A | count of C << 32 */
#define KMX_RX_GT 5u    /* count of G | count of T << 32 */
#define KMX_RX_DIFF 6u  /* D | P << 32 */
#define KMX_RX_DUST 7u  /* max over j of S_j | (number of DUSTY windows) << 32; 0 for an empty read */
int kmx_reads_complexity(kmx_ctx *ctx, const kmx_reads *reads, uint32_t tail_bases, uint32_t head_bases, uint32_t min_len,
                         uint32_t err_num, uint32_t err_den, uint32_t penalty, uint32_t dust_max, uint8_t *d_masked,
                         uint64_t *d_rows);

/* ---------------------------------------------------------------- duplicate reads and read pairs ----
 * BUILD-DEFINED (the reference has nothing like it): what fastp --dedup, clumpify dedupe and samtools markdup do -- reads, or mate
 * pairs, whose whole content was sequenced before are found and all but one of each class dropped.  EXACT: items are grouped by a
 * 64-bit fingerprint and every candidate is then compared with the one it would be dropped for, letter by letter.  An ITEM is read
 * r of `reads` (mates == NULL) or the pair of read r of `reads` and read r of `mates` (mates->n_reads != reads->n_reads:
 * KMX_E_ARG).  Every layout kmx_reads_pair_overlap takes is taken: uniform or ragged, d_offsets[0] > 0, empty reads, any alignment
 * of d_bases, the two batches with layouts of their own; a read of 2^31 bases or more, or an offsets pair that descends, has
 * length 0 (so has, in this call, a read of 2^31 - 4 bases or more: its last dword position does not fit the fetch's 32 bits).
 *
 * CODES.  c(b) = 0, 1, 2, 3 for A/a, C/c, G/g, T/t and 4 for any other byte; comp(c) = 3 - c for c < 4, comp(4) = 4.  A read IS its
 * code sequence S (case is ignored, all other bytes are one letter), L codes long; rc(S)[i] = comp(S[L - 1 - i]).
 *
 * FINGERPRINT.  Arithmetic mod 2^64, G = 0x9E3779B97F4A7C15, fmix = the murmur3 64-bit finaliser (x ^= x >> 33;
 * x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33):
 *     v_p  = sum_{j < 4} code(4 p + j) << 4 j        for p < ceil(L / 4), with code = 0xF at positions >= L
 *     H(S) = fmix( (sum_p fmix(((p << 16) | v_p) + G))  ^  (L * G) )                         (H of the empty read is 0)
 *     P(x, y) = fmix(fmix(x + G) + y)                                                        (a pair)
 * THE KEY of item r, with t(x) = x >> (64 - hash_bits), 1 <= hash_bits <= 64 (normally 64; fewer bits only make more items share a
 * key, which costs compares and can only keep more):
 *     singles:  F_a = t(H(S)),                 F_b = t(H(rc S))
 *     pairs:    F_a = t(P(H(m1), H(m2))),      F_b = t(P(H(m2), H(m1)))     (the other strand of a fragment is its mates exchanged)
 * Without KMX_DD_STRAND: Hc = F_a, OTHER = 0.  With it: Hc = min(F_a, F_b), OTHER = (F_b < F_a).
 *
 * RANK within a key: s = min(d_score[r * score_stride], 2^32 - 1), 0 for every item where d_score == NULL; higher s first, then the
 * smaller index.  The HEAD of a key is its first item in that order: (d_rows of kmx_reads_quality + KMX_RQ_QSUM, KMX_RQ_WORDS) as
 * the score keeps the best copy, no score keeps the first.
 *
 * DECISION.  Item r is DROPPED iff it is not the head of its key and EQUALS the head: singles -- the same length and the same code at
 * every position, or, under KMX_DD_STRAND, rc of it is; pairs -- both mates equal the head's mates, or, under the flag, the head's
 * mates exchanged.  Both orientations count wherever both can hold ("either").  A non-head that does not equal its head is KEPT
 * and flagged COLLISION: an item that has no equal is never dropped, and a duplicate is missed only where its key collides with a
 * different, better ranked item -- which the summary counts.
 *
 * OUTPUTS.  d_rows: KMX_DD_WORDS u64 per item in source order (required).  d_keep (optional): one byte per item, 1 iff kept -- what
 * kmx_reads_select takes, for both mates.  h_summary (host, required): KMX_DD_SUMMARY_WORDS u64.  Nothing else is written; no
 * load touches an aligned dword that holds no byte of its batch.
 * mates->n_reads != reads->n_reads, hash_bits out of range, unknown flag bits, score_stride == 0 with d_score, NULL ctx / reads /
 * d_rows / h_summary, n_reads >= 2^32 (the index shares a word with the score): KMX_E_ARG.  n_reads == 0 checks its arguments,
 * zeroes the summary and launches nothing.
 * Working set, laid out in the work buffer before any kernel runs: 42 bytes per item (the sort's records and flags 17, the sorted
 * records 16, the group of every sorted position and the head of every group 4 + 4 -- they lie where the sort left its counts --
 * and a byte for OTHER), the two-word counter's area, 18.4 bytes per item, and 32 bytes per wave of the verify kernel's grid (at
 * most 4 KiB per compute unit): 42 n + count area(n) + 32 waves <= 61 n + 64 KiB + 4 KiB per compute unit bytes.  Above
 * the cap (kmx_ctx_set_work_buffer_limit): KMX_E_NOMEM with nothing written.  Synchronous (the sort reads a record back per digit
 * it descends: a class of many equal items goes through all 16).  COUNT is summed with integer atomics: repeated calls give
 * identical bytes. */
#define KMX_DD_STRAND 1u /* flags: the other strand is the same item */
#define KMX_DD_WORDS 4u
#define KMX_DD_REP 0u   /* the head's index for a dropped item, the item's own index otherwise */
#define KMX_DD_COUNT 1u /* a head: 1 + the items dropped onto it; any other kept item: 1; a dropped item: 0 */
#define KMX_DD_FLAGS 2u /* KMX_DD_F_* */
#define KMX_DD_HASH 3u  /* Hc */
#define KMX_DD_F_KEPT 1u
#define KMX_DD_F_FLIPPED 2u   /* dropped, and equal to the head only in the other orientation / exchanged */
#define KMX_DD_F_COLLISION 4u /* kept although not the head of its key: it differs from the head */
#define KMX_DD_F_OTHER 8u     /* F_b < F_a */
#define KMX_DD_SUMMARY_WORDS 4u
#define KMX_DD_S_KEPT 0u
#define KMX_DD_S_DROPPED 1u
#define KMX_DD_S_LARGEST 2u /* the largest COUNT */
#define KMX_DD_S_COLLISIONS 3u
int kmx_reads_dedup(kmx_ctx *ctx, const kmx_reads *reads, const kmx_reads *mates /* NULL: single reads */, uint32_t flags,
                    uint32_t hash_bits, const uint64_t *d_score, uint64_t score_stride, uint64_t *d_rows, uint8_t *d_keep,
                    uint64_t *h_summary /* KMX_DD_SUMMARY_WORDS, host */);

/* ---------------------------------------------------------------- back to a file: record names, and a batch as FASTQ / FASTA text ----
 * BUILD-DEFINED.  Every read-preparation call ends in a batch -- bytes and offsets in device memory.  The two calls here close the
 * loop: the names of a FASTQ image are kept, and names, bases and quality bytes are laid out as a FASTQ or FASTA image on the
 * device, so that one device-to-host copy is the output file.
 *
 * kmx_fastx_parse_names.  The contract of kmx_fastx_parse_quals with line i % 4 == 0 in place of line i % 4 == 3.  On the text alone:
 * split it at '\n'; a final empty piece (the text is empty or ends in '\n') is not a line; name r is line 4r with every '\r'
 * removed, for every 4r below the number of lines.  The name is the header line as it stands, its first byte ('@') included: no
 * byte is interpreted (kmx_fastx_format has name_skip for the marker).  A text that ends inside a record has one name more than
 * quality lines.  d_names = the names back to back, d_noffsets[r] = first byte of name r, d_noffsets[n_names] = the byte total:
 * a ragged kmx_reads batch, so kmx_reads_gather reorders names by the d_out_index of kmx_reads_select.  format: KMX_FASTX_AUTO or
 * KMX_FASTX_FASTQ; KMX_FASTX_FASTA, or a text that does not begin with '@', gives KMX_E_ARG (the names of FASTA records are not
 * parsed by this library).  d_text 16-byte aligned; d_names: room for the bytes (n_bytes always suffices); d_noffsets: max_reads + 1
 * words.  d_names == d_noffsets == NULL: only the counts; n_names > max_reads: KMX_E_NOMEM with nothing written and the counts
 * set.  *h_n_names / *h_n_bytes (host, optional) = names / bytes kept.  KMX_FASTX_SAME_TEXT as at kmx_fastx_parse_quals, where "the
 * previous call" is any of the three parse calls.  Synchronous.
 *
 * kmx_fastx_format.  Record r of the image, r < reads->n_reads, is defined on the arrays alone, in 64-bit arithmetic; any bytes
 * give one answer.
 *     L, B   the length and the bases of read r under THE SPAN OF A READ above (an offsets pair that descends: 0; 2^31 bases or
 *            more: 0); the bases are copied verbatim.  Every layout kmx_reads_select takes is taken.
 *     N      names != NULL (names->n_reads must equal reads->n_reads: KMX_E_ARG otherwise): with len the length of name r under
 *            the same two rules, the bytes of name r from byte min(name_skip, len) on.  names == NULL: name_base + r (wrapping
 *            mod 2^64) in decimal without leading zeros.
 *     KMX_FASTX_FASTQ   '@' N '\n' B '\n' '+' '\n' Q '\n': |N| + 2 L + 6 bytes.  Q = the L bytes of d_quals, laid out as the bases
 *            are and at any alignment of its own (kmx_reads_quality); d_quals == NULL: L copies of the byte qual_fill
 *            (qual_fill > 255: KMX_E_ARG).  line_width must be 0: KMX_E_ARG otherwise.
 *     KMX_FASTX_FASTA   '>' N '\n', then B in lines of line_width bases, each line ended by '\n'; line_width == 0: one line.  Every
 *            record has at least one sequence line (an empty read: one empty line).  With lines = line_width ? max(1, ceil(L /
 *            line_width)) : 1 the record is |N| + 2 + L + lines bytes.  d_quals and qual_fill are ignored.
 *     any other `format` (KMX_FASTX_AUTO included): KMX_E_ARG.
 * The records lie back to back in d_text; *h_n_bytes (host) = their total, always.  d_rec_offsets (optional): n_reads + 1 words,
 * where each record starts, the total last.  d_text == NULL = count only (d_rec_offsets is still written if given).  n_bytes >
 * max_bytes: KMX_E_NOMEM with not one byte of d_text and not one word of d_rec_offsets written, and the count set.  n_reads == 0
 * is a no-op with a count of 0 (nothing is written).  n_reads up to 2^40, an image below 2^44 bytes.
 * Memory, as at kmx_reads_select: d_text may have any alignment; not one byte outside [0, n_bytes) is written; no aligned dword
 * that holds no byte of its batch is loaded from the bases, the quality bytes or the names; d_text overlapping one of the three
 * sources or d_rec_offsets is KMX_E_ARG where the host can tell.  Deterministic, no atomics.  Synchronous (the count comes back to
 * the host).  Working set in the work buffer: a256(8 * (n_reads + 1)) for the record offsets when the caller gives none, plus
 * a256(8 * (2 * ceil(n_reads / 2048) + 6)); above the cap KMX_E_NOMEM before any kernel runs.  NULL ctx / reads / h_n_bytes:
 * KMX_E_ARG.
 * Not done: the names of FASTA records, two mates interleaved in one image, multi-line FASTQ, plain gzip (BGZF: the two sections
 * below), writing to disk from the device. */
int kmx_fastx_parse_names(kmx_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint32_t format, uint8_t *d_names,
                          uint64_t *d_noffsets, uint64_t max_reads, uint64_t *h_n_names, uint64_t *h_n_bytes);
int kmx_fastx_format(kmx_ctx *ctx, const kmx_reads *reads, const uint8_t *d_quals, const kmx_reads *names, uint32_t name_skip,
                     uint64_t name_base, uint32_t format, uint32_t line_width, uint32_t qual_fill, uint8_t *d_text,
                     uint64_t *d_rec_offsets, uint64_t max_bytes, uint64_t *h_n_bytes);

/* ---------------------------------------------------------------- BGZF-compressed images (kmx_bgzf.hip) ----
 * BUILD-DEFINED.  A .fastq.gz written by bgzip / htslib / samtools is BGZF: a chain of independent gzip members ("blocks") of at most
 * 64 KiB, each one DEFLATE stream with its own CRC-32 and length.  The two calls here turn such an image in device memory into the
 * text kmx_fastx_parse takes.  A block header is the 18 bytes htslib writes: 1f 8b 08 04, six ignored bytes, XLEN = 6, 'B' 'C' 02 00,
 * BSIZE; the block's size is BSIZE + 1, at least 28, inside the file; its last eight bytes are CRC-32 and ISIZE.  Plain single-member
 * gzip, and headers with further extra subfields, are NOT taken: there is nothing to split them at.
 *
 * kmx_bgzf_index.  d_file: the image, any alignment.  The chain of blocks is followed exactly from byte 0 (a header pattern inside
 * compressed or stored data is not a block): d_block_offsets[b] = first byte of block b, d_block_offsets[n_blocks] = the end of the
 * last complete block; d_text_offsets = the exclusive prefix sum of the blocks' ISIZE words (n_blocks + 1 words); both arrays hold
 * max_blocks + 1 words.  h_info (host, four words): n_blocks, n_text_bytes, the bytes behind the last complete block (0 for a sound
 * file), 1 if the last block is the 28-byte EOF marker.  Empty blocks (ISIZE 0) are blocks wherever they stand.  A chain that comes
 * to a byte which is no header, or to a block that would pass the end of the file, ends there.  With both arrays NULL only h_info is
 * written; with n_blocks > max_blocks: KMX_E_NOMEM, nothing written to the device, h_info set (the convention of kmx_fastx_parse).  A
 * file that does not begin with the 18-byte header pattern (plain gzip, plain text, fewer than 18 bytes): KMX_E_ARG; n_bytes == 0: no
 * blocks.  Working set in the work buffer: 4 bytes per KiB of file and 24 bytes per header pattern found; above the cap KMX_E_NOMEM.
 * Synchronous.
 *
 * kmx_bgzf_inflate.  Block b of d_block_offsets / d_text_offsets (n_blocks + 1 device words each, as the index wrote them, or
 * both advanced by i to inflate blocks i.. alone) is written at d_text + (d_text_offsets[b] - d_text_offsets[0]).  d_text: 16-byte
 * aligned, text_capacity bytes; the span d_text_offsets[n_blocks] - d_text_offsets[0] is read back first and a larger one is
 * KMX_E_NOMEM with nothing written.  d_status (device, n_blocks u32, optional): 0 or the KMX_BGZF_ST_* reason of block b;
 * *h_first_bad (host, optional) = the lowest block with a non-zero status, or ~0; a bad block makes the call return KMX_E_ARG, with
 * the sound blocks written in full and nothing written outside a bad block's own output range.  A block is sound iff its header
 * is the one above with BSIZE + 1 == d_block_offsets[b+1] - d_block_offsets[b]; its DEFLATE stream decodes under zlib's rules and
 * reaches the end-of-block of a final block inside the payload (whole unused bytes behind it are tolerated, as zlib tolerates them);
 * it produced exactly ISIZE == d_text_offsets[b+1] - d_text_offsets[b] bytes; and -- unless flags holds KMX_BGZF_NO_CRC -- their
 * CRC-32 is the footer's.  No byte outside [d_block_offsets[b], d_block_offsets[b+1]) and [0, n_bytes) is read for block b.
 * Deterministic.  Synchronous.  Uses the work buffer when d_status is NULL. */
#define KMX_BGZF_NO_CRC 1
#define KMX_BGZF_ST_HEADER 1   /* not the 18-byte header, or BSIZE + 1 is not the distance to the next offset, or the offsets are unsound */
#define KMX_BGZF_ST_BTYPE 2    /* block type 3 */
#define KMX_BGZF_ST_STORED 3   /* stored block: LEN != ~NLEN, or longer than the input or the room */
#define KMX_BGZF_ST_COUNTS 4   /* HLIT above 286 or HDIST above 30 */
#define KMX_BGZF_ST_REPEAT 5   /* repeat code with no previous length, or running past HLIT + HDIST */
#define KMX_BGZF_ST_NO_EOB 6   /* no code for symbol 256 */
#define KMX_BGZF_ST_CODESET 7  /* a code-length set over-subscribed or incomplete (zlib's inflate_table rule) */
#define KMX_BGZF_ST_BADCODE 8  /* a bit pattern that is no code */
#define KMX_BGZF_ST_SYMBOL 9   /* length symbol 286 / 287 or distance symbol 30 / 31 */
#define KMX_BGZF_ST_DISTANCE 10 /* a distance larger than the bytes the block has produced */
#define KMX_BGZF_ST_OUTPUT 11  /* output passing ISIZE */
#define KMX_BGZF_ST_INPUT 12   /* input running out */
#define KMX_BGZF_ST_LENGTH 13  /* produced bytes != ISIZE, or ISIZE != d_text_offsets[b+1] - d_text_offsets[b] */
#define KMX_BGZF_ST_CRC 14     /* CRC-32 differs from the footer's */
int kmx_bgzf_index(kmx_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, uint64_t *d_block_offsets, uint64_t *d_text_offsets,
                   uint64_t max_blocks, uint64_t *h_info);
int kmx_bgzf_inflate(kmx_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const uint64_t *d_block_offsets,
                     const uint64_t *d_text_offsets, uint64_t n_blocks, uint32_t flags, uint8_t *d_text, uint64_t text_capacity,
                     uint32_t *d_status, uint64_t *h_first_bad);

/* ---------------------------------------------------------------- text compressed to BGZF (kmx_bgzf.hip) ----
 * BUILD-DEFINED.  The way back: a text in device memory (the image kmx_fastx_format wrote, or any bytes) becomes a BGZF image there,
 * so that one device-to-host copy is the .gz file.  The text is cut into ceil(n_bytes / block_bytes) pieces; block_bytes in
 * [1, 65280], 0 = 65280 (what htslib takes), anything else KMX_E_ARG.  Each piece becomes one block: the 18-byte header above with
 * the six ignored bytes 00 00 00 00 00 ff, one raw DEFLATE stream whose last block is final, CRC-32 and ISIZE.  The 28-byte EOF
 * marker follows the last block; n_bytes == 0 gives the marker alone.
 * The DEFLATE stream of a piece of n bytes is either dynamic blocks (greedy LZ77 over a one-entry hash table of 4-byte strings and
 * the distance-1 candidate, one block per 4096 tokens, code lengths limited to 15 / 7 bits) or the stored form, which is zlib's at
 * level 0 byte for byte (one final stored block of n + 5 bytes below 32768 bytes of text; from there on a stored block and an empty
 * final one, n + 10): the dynamic form is taken iff it is shorter in whole bytes.  flags = KMX_BGZF_DEFLATE_STORED stores every
 * piece (zlib's level 0).
 * The bytes are a function of the text, block_bytes and flags alone: the same across calls, streams, contexts and devices, and the
 * ones tests/cpp/bgzf_encode_check.cpp writes on the host.
 * d_text, d_file: any alignment.  d_block_offsets (optional): n_blocks + 1 device words as kmx_bgzf_index would write them for the
 * image (the EOF marker is a block: n_blocks = pieces + 1).  h_info (host, four words, always set on KMX_OK / KMX_E_NOMEM):
 * n_blocks (the marker counted, as kmx_bgzf_index counts it), the bytes of the image (the marker included), the stored blocks, the
 * bytes of text.  d_file == NULL: compresses and reports only (d_block_offsets is still written if given).  An image larger than
 * file_capacity: KMX_E_NOMEM with not one byte of d_file and not one word of d_block_offsets written and h_info set.  No byte at or
 * behind the image's end is written.  kmx_bgzf_deflate_bound(n_bytes, block_bytes): the capacity that always suffices (every piece
 * stored: 31 bytes around a piece below 32768 bytes, 36 from there on, and the marker); 0 for a block_bytes out of range.
 * Working set in the work buffer: 16 bytes per block and one slot of a256(block_bytes + 16) bytes per piece coded at a time; when the
 * cap does not hold a slot for every piece the pieces are coded in chunks, and -- as the size must be known before the first byte
 * is written -- coded twice; not even one slot: KMX_E_NOMEM before any kernel runs.  Synchronous.  NULL ctx / h_info, flags other
 * than the one below, n_bytes != 0 with d_text NULL, n_bytes of 2^44 or more: KMX_E_ARG.
 * Not done: lazy matching, hash chains, compression levels, plain single-member gzip. */
#define KMX_BGZF_DEFLATE_STORED 1
uint64_t kmx_bgzf_deflate_bound(uint64_t n_bytes, uint32_t block_bytes);
int kmx_bgzf_deflate(kmx_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint32_t block_bytes, uint32_t flags,
                     uint8_t *d_file, uint64_t file_capacity, uint64_t *d_block_offsets, uint64_t *h_info);

/* ---------------------------------------------------------------- multi-GPU exchange ----
 * The reference has no distributed code; reads shard embarrassingly (k-mers never span reads,
 * canonical_kmer_iterator.rs:72-83), so the scans need no collective.  What is exchanged is the optional bucket
 * histogram -- ncclAllReduce(ncclUint64, ncclSum) over RCCL/xGMI -- and the 32-byte summaries.  One kmx_comm per
 * kmx_ctx (one process or thread per GPU); the collectives run on the context's stream.
 * Bootstrap: rank 0 calls kmx_comm_get_unique_id and hands the KMX_COMM_ID_BYTES bytes to the other ranks by any
 * means (file, environment, socket, MPI, a torch.distributed broadcast); then every rank calls kmx_comm_create. */
#define KMX_COMM_ID_BYTES 128
typedef struct kmx_comm kmx_comm;
int kmx_comm_get_unique_id(uint8_t *h_id /* KMX_COMM_ID_BYTES, host */);
int kmx_comm_create(kmx_ctx *ctx, const uint8_t *h_id, int n_ranks, int rank, kmx_comm **out); /* collective over the ranks */
void kmx_comm_destroy(kmx_comm *comm);
int kmx_comm_size(const kmx_comm *comm);
int kmx_comm_rank(const kmx_comm *comm);
/* d_counts[i] = sum over ranks of d_counts[i], in place, n_counts u64 (2^log2_buckets of kmx_histogram) */
int kmx_histogram_allreduce(kmx_comm *comm, uint64_t *d_counts, uint64_t n_counts);
/* the per-shard kmx_summary of every rank combined in place: wrapping sums of n_valid / sum_canon / sum_fw, xor of xor_hash */
int kmx_summary_allreduce(kmx_comm *comm, kmx_summary *d_summary);

/* ---------------------------------------------------------------- measurement helper ----
 * Read-only pass over [d_buf, d_buf + nbytes) with the load shape of the scan kernels (16 bytes per lane, non-temporal,
 * one 9600-byte tile = 64 reads x 150 bytes per wave and step, the next tile requested before the current one is
 * consumed), xor-folded into *d_out (8 bytes, overwritten): the same-run ceiling of the HBM read stream next to which
 * bench.py reports kmx_canonical_reduce, and the known-byte-count kernel the FETCH_SIZE counter is calibrated on.
 * d_buf 16-byte aligned. */
int kmx_calib_stream_read(kmx_ctx *ctx, const uint8_t *d_buf, uint64_t nbytes, uint64_t *d_out);

#ifdef __cplusplus
}
#endif
#endif /* KMX_H */
