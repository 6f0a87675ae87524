// kmx_launch.h -- the one declaration of the host-side launchers kmx_api.hip calls, included by kmx_api.hip and by every
// translation unit that defines one of them (so each definition is compiled against its declaration).  Default arguments are
// written here only.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/kmx.h"

namespace kmx {
typedef uint32_t u32;
typedef uint64_t u64;
// every array of a work-buffer layout starts on a 256-byte boundary (the working-set formulas of kmx.h round with it)
inline size_t align256(size_t b) { return (b + 255u) & ~(size_t)255u; }
// kmx_scan.hip
hipError_t launch_scan_uniform(const uint8_t* bases, u64 n_reads, u32 L, u32 k, bool want_hash, bool want_sumfw,
                               kmx_summary* out, unsigned long long* queue, int n_cu, hipStream_t stream, bool* handled, const u64* offsets);
hipError_t launch_windows_uniform(const uint8_t* bases, u64 n_reads, u32 L, u32 k, u64* fw, u64* rc, u64* canon,
                                  uint8_t* flags, unsigned long long* queue, int n_cu, hipStream_t stream, bool* handled);
hipError_t launch_windows_ragged(const uint8_t* bases, const u64* offsets, const u64* win_offsets, u64 n_reads, u32 L, u32 k,
                                 u64* fw, u64* rc, u64* canon, uint8_t* flags, unsigned long long* queue, int n_cu,
                                 hipStream_t stream, bool* handled, const u64* ends = nullptr /* the reads' ends: nullptr = offsets + 1 */);
// kmx_hist.hip
hipError_t launch_hist_uniform(const uint8_t* bases, u64 n_reads, u32 L, u32 k, u32 hasher, u32 hk, u32 log2_buckets,
                               u64* counts, unsigned long long* queue, int n_cu, hipStream_t stream, bool* handled,
                               void* (*get_scratch)(void*, size_t), void* user, size_t scratch_budget, const u64* offsets, u64 k0 = 0, u64 k1 = 0);
// kmx_bitslice.hip
hipError_t launch_scan_bitsliced(const uint8_t* bases, u64 n_reads, u32 L, u32 k, bool want_hash, u32 mode /* KMX_BS_* (kmx_device.h): bit 0 = sum_fw */,
                                 kmx_summary* out, unsigned long long* queue, int n_cu, hipStream_t stream, bool* handled);
hipError_t launch_scan_bitsliced2(const uint8_t* bases, u64 n_reads, u32 L, u32 k, bool want_hash, kmx_summary2* out,
                                  unsigned long long* queue, int n_cu, hipStream_t stream, bool* handled);
u64 bitsliced_segments_per_read(u32 L, u32 k);
hipError_t launch_scan_bitsliced2_ragged(const uint8_t* bases, const u64* offsets, u64 n_reads, u32 L_hint, u32 k, bool want_hash,
                                         kmx_summary2* out, unsigned long long* queue, int n_cu, hipStream_t stream, bool* handled,
                                         const u64* ends = nullptr);
hipError_t launch_scan_bitsliced_ragged(const uint8_t* bases, const u64* offsets, u64 n_reads, u32 L_hint, u32 k, bool want_hash,
                                        kmx_summary* out, unsigned long long* queue, int n_cu, hipStream_t stream, bool* handled,
                                        bool want_sumfw = false, const u64* ends = nullptr /* the reads' ends: nullptr = offsets + 1 */);
hipError_t launch_scan_bitsliced_packed(const uint64_t* words, u64 n_reads, u32 L, u32 k, bool want_hash, bool want_sumfw,
                                        kmx_summary* out, unsigned long long* queue, int n_cu, hipStream_t stream, bool* handled);
// kmx_sweep.hip
hipError_t launch_sweep_uniform(const uint8_t* bases, u64 n_reads, u32 L, u32 k, bool want_hash, bool want_sumfw, kmx_summary* out,
                                unsigned long long* queue, int n_cu, hipStream_t stream);
hipError_t launch_sweep_windows(const uint8_t* bases, u64 n_reads, u32 L, u32 k, u64* fw, u64* rc, u64* canon, uint8_t* flags,
                                const u64* win_offsets, unsigned long long* queue, int n_cu, hipStream_t stream, const u64* offsets,
                                const u64* ends, bool two_words);
hipError_t launch_sweep_hist(const uint8_t* bases, u64 n_reads, u32 L, u32 k, u32 hasher, u32 hk, u32 log2_buckets, u64* counts,
                             unsigned long long* queue, int n_cu, hipStream_t stream, const u64* offsets);
// kmx_segments.hip
size_t uniform_segments_scratch_bytes(u64 n_seg);
hipError_t launch_uniform_segments_plan(u64 n_reads, u32 L, u32 k, u32 T, void* scratch, const u64** starts, const u64** ends, const u64** wins, u64* n_seg_out,
                                        hipStream_t stream);
size_t segments_scratch_bytes(u64 n_reads, u64 seg_capacity, bool with_wins = false);
u64 segments_capacity(u64 n_reads, u64 total_bases, u32 t_max);
hipError_t launch_segments_build(const u64* offsets, u64 n_reads, u32 k, u32 t_max, u64 seg_capacity, void* scratch,
                                 const u64** starts_out, const u64** ends_out, const u64** total_out, unsigned long long* too_long,
                                 hipStream_t stream, const u64* win_offsets = nullptr, const u64** wins_out = nullptr);
// kmx_fastx.hip
size_t fastx_scratch_bytes(u64 n_bytes);
hipError_t launch_fastx_count(const uint8_t* text, u64 n, bool fasta, void* scratch, unsigned long long* totals, hipStream_t st, u32 entry = 0u,
                              bool summarise = true);
hipError_t launch_fastx_length_mismatch(const u64* a, const u64* b, u64 n_reads, unsigned long long* first_bad, int n_cu, hipStream_t st);
hipError_t launch_fastx_emit(const uint8_t* text, u64 n, bool fasta, const void* scratch, const unsigned long long* totals,
                             uint8_t* bases, u64* offsets, hipStream_t st, u32 entry = 0u);
// kmx_seqvec.hip
hipError_t launch_seqvec_push(u64* words, u64 first, const uint8_t* bytes, u64 n, unsigned long long* first_bad, int n_cu, hipStream_t st);
hipError_t launch_seqvec_to_bytes(const u64* words, u64 n, uint8_t* out, int n_cu, hipStream_t st);
hipError_t launch_seqvec_get_kmers(const u64* words, u64 n_bases, const u64* pos, u64 n, u32 k, u64* out,
                                   unsigned long long* first_bad, int n_cu, hipStream_t st);
hipError_t launch_seqvec_iter_kmers(const u64* words, u64 n_bases, u64 start, u64 count, u32 k, u64* out, int n_cu, hipStream_t st);
hipError_t launch_minimizer_words(const u64* in, u64 n, u32 k, u32 w, u32 hasher, u32 hk, u64* out_mm, u32* out_off, int n_cu, hipStream_t st);
hipError_t launch_seqvec_minimizers(const u64* words, u64 n_reads, u32 L, u32 k, u32 w, u32 hasher, u32 hk, u64* out_word,
                                    u32* out_pos, int n_cu, hipStream_t st);
hipError_t launch_reduce_packed_generic(const u64* words, u64 n_reads, u32 L, u32 k, bool want_hash, bool want_sumfw,
                                        kmx_summary* out, int n_cu, hipStream_t st);
// kmx_generic.hip
hipError_t launch_reduce_generic(const kmx_reads* r, u32 k, u32 hasher, u32 hk, u32 want_sumfw, kmx_summary* out,
                                 int n_cu, hipStream_t st, unsigned long long* too_long);
hipError_t launch_windows_generic(const kmx_reads* r, const u64* win_off, u32 k, u64* fw, u64* rc, u64* canon,
                                  uint8_t* flags, int n_cu, hipStream_t st, unsigned long long* too_long);
hipError_t launch_histogram_generic(const kmx_reads* r, u32 k, u32 hasher, u32 hk, u32 log2_buckets, u64* counts,
                                    int n_cu, hipStream_t st, unsigned long long* too_long);
hipError_t launch_reduce2_generic(const kmx_reads* r, u32 k, u32 with_hash, kmx_summary2* out, int n_cu, hipStream_t st, unsigned long long* too_long,
                                  const u32* gate);
hipError_t launch_windows2_tiled(const kmx_reads* r, u32 k, u64* fw, u64* rc, u64* canon, uint8_t* flags, int n_cu, hipStream_t st,
                                 bool* handled, unsigned long long* queue);
hipError_t launch_windows2_tiled_ragged(const kmx_reads* r, const u64* win_offsets, u32 k, u64* fw, u64* rc, u64* canon, uint8_t* flags, int n_cu,
                                        hipStream_t st, bool* handled, unsigned long long* too_long, const u64* ends, unsigned long long* queue);
hipError_t launch_windows2_generic(const kmx_reads* r, const u64* win_off, u32 k, u64* fw, u64* rc, u64* canon,
                                   uint8_t* flags, int n_cu, hipStream_t st, unsigned long long* too_long);
// kmx_elem.hip
hipError_t launch_gen_reads(u64 seed, u64 first_byte, uint8_t* out, u64 nbytes, int n_cu, hipStream_t st);
hipError_t launch_kmers_from_bytes(const uint8_t* seqs, u64 n, u32 k, u64* words, unsigned long long* first_bad, int n_cu, hipStream_t st);
hipError_t launch_revcomp_words(const u64* in, u64 n, u32 k, u64* out, int n_cu, hipStream_t st);
hipError_t launch_canonical_words(const u64* in, u64 n, u32 k, u64* canon, uint8_t* is_canon, int n_cu, hipStream_t st);
hipError_t launch_hash_words(const u64* in, u64 n, u32 hasher, u32 hk, u64* out, int n_cu, hipStream_t st);
hipError_t launch_hash_words_sip13(const u64* in, u64 n, u64 k0, u64 k1, u64* out, int n_cu, hipStream_t st);
hipError_t launch_match_words(const u64* fw, const u64* rc, const u64* other, u64 n, uint8_t* out, int n_cu, hipStream_t st);
hipError_t launch_ck_shift(bool append, u64* fw, u64* rc, const uint8_t* bases, u64 n, u32 k, uint8_t* dropped, int n_cu, hipStream_t st);
hipError_t launch_encode_kmers(const uint8_t* seqs, u64 n, u32 seq_len, u32 enc, u32 B, u64* words, int n_cu, hipStream_t st);
hipError_t launch_encode_windows(const uint8_t* bases, u64 n_reads, u32 L, u32 k, u32 enc, u32 B, u64* words, int n_cu, hipStream_t st);
hipError_t launch_encoding_rev_comp(const u64* in, u64 n, u32 K, u32 comp_lut, u32 B, u64* out, int n_cu, hipStream_t st);
hipError_t launch_encoding_decode(const u64* in, u64 n, u32 nuc_lut, u32 B, uint8_t* seqs, int n_cu, hipStream_t st);
hipError_t launch_sub_kmer_words(const u64* in, u64 n, u32 pos, u32 width, u64* out, int n_cu, hipStream_t st);
hipError_t launch_kmers_to_bytes(const u64* in, u64 n, u32 k, bool upper, uint8_t* out, int n_cu, hipStream_t st);
hipError_t launch_encode_kmers_bytes(const uint8_t* seqs, u64 n, u32 seq_len, u32 enc, u32 nb, uint8_t* arrays, int n_cu, hipStream_t st);
hipError_t launch_encoding_rev_comp_bytes(const uint8_t* in, u64 n, u32 K, u32 comp_lut, u32 nb, uint8_t* out, int n_cu, hipStream_t st);
hipError_t launch_encoding_decode_bytes(const uint8_t* in, u64 total_bytes, u32 nuc_lut, uint8_t* seqs, int n_cu, hipStream_t st);
hipError_t launch_calib_stream_read(const uint8_t* buf, u64 nbytes, unsigned long long* out, int n_cu, hipStream_t st);
hipError_t launch_length_range(const u64* offsets, u64 n_reads, u32* out, int n_cu, hipStream_t st);
hipError_t launch_offsets_uniform_gate(const u64* offsets, u64 n_reads, u32 bound, u32 k, u32* gate, int n_cu, hipStream_t st);
hipError_t launch_fix_hash_fold(kmx_summary* out, u32 k, u32 hasher, u32 hk, hipStream_t st);
// kmx_minimizers.hip (first_bad: the context's scratch word -- the 24 bytes from it are readable: the tiled kernel's idle prefetch)
hipError_t launch_minimizers_reads(const uint8_t* bases, u64 total_bytes, const u64* offsets, const u64* win_offsets, u64 n_reads, u32 L,
                                   u32 bound, u32 k, u32 w, u32 hasher, u32 hk, u64* out_word, u32* out_pos,
                                   unsigned long long* first_bad, int n_cu, hipStream_t st, bool* tiled);
// the *_sip13 calls (SipHash-1-3 under std's DefaultHasher / RandomState): kmx_scan.hip, kmx_hist.hip, kmx_generic.hip, kmx_sip13.hip
constexpr u32 KMX_HASH_SIP13_INTERNAL = 0x5313u;   // the hasher id launch_hist_uniform takes for them (not an ABI value: kmx.h's hashers stop at KMX_HASH_IDENTITY)
hipError_t launch_scan_reduce_sip(const uint8_t* bases, u64 n_reads, u32 L, u32 k, u64 k0, u64 k1, bool want_sumfw, kmx_summary* out,
                                  unsigned long long* queue, int n_cu, hipStream_t stream, bool* handled, const u64* offsets);
hipError_t launch_reduce_generic_sip(const kmx_reads* r, u32 k, u64 k0, u64 k1, u32 want_sumfw, kmx_summary* out, int n_cu, hipStream_t st,
                                     unsigned long long* too_long);
hipError_t launch_histogram_generic_sip(const kmx_reads* r, u32 k, u64 k0, u64 k1, u32 log2_buckets, u64* counts, int n_cu, hipStream_t st,
                                        unsigned long long* too_long);
hipError_t launch_minimizer_words_sip(const u64* in, u64 n, u32 k, u32 w, u64 k0, u64 k1, u64* out_mm, u32* out_off, int n_cu, hipStream_t st);
hipError_t launch_minimizers_reads_sip(const uint8_t* bases, const u64* offsets, const u64* win_offsets, u64 n_reads, u32 L, u32 k, u32 w,
                                       u64 k0, u64 k1, u64* out_word, u32* out_pos, unsigned long long* first_bad, int n_cu, hipStream_t st);
hipError_t launch_seqvec_minimizers_sip(const u64* words, u64 n_reads, u32 L, u32 k, u32 w, u64 k0, u64 k1, u64* out_word, u32* out_pos,
                                        int n_cu, hipStream_t st);
// kmx_count.hip: the counter and the merge (`words` u64 per key: 1 or 2; two-word keys low word first, their arrays 16-byte aligned)
size_t count_area_bytes(u32 words, u64 n_win);
size_t win_offsets_bytes(u64 n_reads);
hipError_t launch_count_win_offsets(const u64* offsets, u64 n_reads, u32 k, void* area, u64** wo_out, unsigned long long* h_pinned,
                                    u64* h_total, hipStream_t st);
hipError_t launch_count_sort(u32 words, u64* canon, const uint8_t* flags, u64 n_win, u32 k, void* area, unsigned long long* h_pinned, u64* h_valid,
                             u64* h_distinct, bool* bad, hipStream_t st);
hipError_t launch_count_emit(u32 words, const u64* canon, u64 n_win, u64 n_valid, void* area, u64* out_k, u64* out_c, hipStream_t st);
size_t count_merge_bytes(u32 words, u64 n);
hipError_t launch_count_merge(u32 words, const u64* ka, const u64* ca, u64 na, const u64* kb, const u64* cb, u64 nb, void* area,
                              unsigned long long* h_pinned, u64* h_out, hipStream_t st);
hipError_t launch_count_merge_emit(u32 words, u64 n, const void* area, u64* out_k, u64* out_c, hipStream_t st);
// kmx_count_query.hip: lookup, spectrum and filter of a count table (`words` u64 per key: 1 or 2)
size_t count_lookup_dir_bytes(u64 n, u32 k, u32* p_out);
bool count_lookup_wants_dir(u64 n, u64 n_query, u32 words);
hipError_t launch_count_lookup(u32 words, const u64* keys, const u64* counts, u64 n, u32 k, const u64* query, const uint8_t* qflags, u64 n_query,
                               u64* out, void* dir_area, u32 p, hipStream_t st);
hipError_t launch_count_spectrum(const u64* counts, u64 n, u64 n_bins, u64* spectrum, int n_cu, hipStream_t st);
size_t count_filter_bytes(u64 n);
hipError_t launch_count_filter_mark(const u64* counts, u64 n, u64 mn, u64 mx, void* area, unsigned long long* h_pinned, u64* h_out, hipStream_t st);
hipError_t launch_count_filter_emit(u32 words, const u64* keys, const u64* counts, u64 n, const void* area, u64* out_k, u64* out_c, hipStream_t st);
// kmx_count_read_stats.hip: KMX_RS_WORDS u64 per read out of the counts / flags of its windows (win_offsets == nullptr: uniform reads of
// W windows; ragged reads: W = the most windows a read is expected to have, 0 = unknown)
hipError_t launch_count_read_stats(const u64* counts, const uint8_t* flags, const u64* win_offsets, u64 n_reads, u32 W, u64 solid_min, u64* stats,
                                   int n_cu, hipStream_t st);
// kmx_count_correct.hip: the corrected bytes of the reads into `out` (a copy of the reads already) and KMX_CR_WORDS u64 per read (fixes may
// be nullptr) out of the counts / flags of its windows and searches of the table (offsets == nullptr: uniform reads of L >= k bases;
// dir_area: the directory launch_count_lookup built for the table, prefix bits p, or nullptr = the plain search)
hipError_t launch_count_correct(u32 words, const uint8_t* bases, uint8_t* out, const u64* offsets, const u64* win_offsets, u64 n_reads, u32 L,
                                const u64* wcounts, const uint8_t* wflags, const u64* keys, const u64* tcounts, u64 n, u32 k, const void* dir_area,
                                u32 p, u64 solid_min, u32 min_cover, u64* fixes, int n_cu, hipStream_t st);
// kmx_count_color.hip: a coloured table's pairwise matrix and spectrum (area: count_color_matrix_bytes(n, n_colors, n_cu) bytes of
// per-block partials, none for n == 0; spectrum may be nullptr; both outputs are overwritten), and KMX_RC_WORDS u64 per read plus,
// unless hits == nullptr, n_colors u32 per read out of the masks / flags of its windows (win_offsets == nullptr: uniform reads of W
// windows)
size_t count_color_matrix_bytes(u64 n, u32 n_colors, int n_cu);
hipError_t launch_count_color_matrix(const u64* colors, u64 n, u32 n_colors, void* area, u64* matrix, u64* spectrum, int n_cu, hipStream_t st);
hipError_t launch_count_read_colors(const u64* answers, const uint8_t* flags, const u64* win_offsets, u64 n_reads, u32 W, u32 n_colors, u32 thr_num,
                                    u32 thr_den, u64* rows, u32* hits, int n_cu, hipStream_t st);
// kmx_count_graph.hip: a count table as the node set of a de Bruijn graph (dir_area: room for count_lookup_dir_bytes(n, k, &p), or
// nullptr = the plain search; flips and nbr may be nullptr)
hipError_t launch_count_adjacency(u32 words, const u64* keys, const u64* counts, u64 n, u32 k, u64 min_count, uint8_t* edges, uint8_t* flips,
                                  u64* nbr, void* dir_area, u32 p, hipStream_t st);
hipError_t launch_count_edge_histogram(const uint8_t* edges, u64 n, u64* hist, int n_cu, hipStream_t st);
hipError_t launch_count_unitig_ends(const uint8_t* edges, const uint8_t* flips, const u64* nbr, u64 n, uint8_t* ends, hipStream_t st);
// kmx_count_unitigs.hip: the unitigs of that graph (keys is read at even k only; circular and sums may be nullptr; *bad: the rounds
// ran out) and their bases
size_t count_unitigs_bytes(u64 n);
hipError_t launch_count_unitigs(u32 words, const u64* keys, const u64* counts, u64 n, u32 k, u64 min_count, const uint8_t* edges, const uint8_t* flips,
                                const u64* nbr, u64* nodes, u64* offsets, uint8_t* circular, u64* sums, void* area, unsigned long long* h_pinned,
                                u64* n_unitigs, u64* n_nodes, u32* rounds, bool* bad, hipStream_t st);
hipError_t launch_count_unitig_sequences(u32 words, const u64* keys, u64 n, u32 k, const u64* nodes, const u64* offsets, u64 n_unitigs, uint8_t* seq,
                                         hipStream_t st);
// kmx_count_paths.hip: where each entry sits in the unitigs (place), and the segments of reads over them -- mark counts them (one host
// round trip), emit writes the reads' offsets and, unless segments == nullptr, the records (win_offsets == nullptr: uniform reads of
// W windows)
hipError_t launch_count_unitig_index(const u64* nodes, const u64* offsets, u64 n_unitigs, u64 n, u64* place, hipStream_t st);
size_t count_paths_bytes(u64 n_win);
hipError_t launch_count_paths_mark(const u64* places, uint8_t* flags, const u64* win_offsets, u64 n_reads, u32 W, u64 n_win, const u64* unitig_offsets,
                                   u64 n_unitigs, void* area, unsigned long long* h_pinned, u64* h_segments, hipStream_t st);
hipError_t launch_count_paths_emit(const u64* places, const uint8_t* flags, const u64* win_offsets, u64 n_reads, u32 W, u64 n_win,
                                   const u64* unitig_offsets, u64 n_unitigs, const void* area, u64* path_offsets, u64* segments, hipStream_t st);
// kmx_count_links.hip: the links between the unitigs -- count counts them (one host round trip), emit writes the 2 U + 1 offsets and,
// unless links == nullptr, the targets (n_unitigs >= 1) -- and the mark of the entries of kept unitigs, in the filter's area
// (count_filter_bytes(n)) and for the filter's emit
size_t count_links_bytes(u64 n_unitigs);
hipError_t launch_count_links_count(const uint8_t* edges, const uint8_t* flips, const u64* nbr, u64 n, const u64* nodes, const u64* offsets, u64 n_unitigs,
                                    const u64* place, void* area, unsigned long long* h_pinned, u64* h_links, hipStream_t st);
hipError_t launch_count_links_emit(const uint8_t* edges, const uint8_t* flips, const u64* nbr, u64 n, const u64* nodes, const u64* offsets, u64 n_unitigs,
                                   const u64* place, const void* area, u64 n_links, u64* link_offsets, u64* links, hipStream_t st);
hipError_t launch_count_select_mark(const u64* place, u64 n, const u64* offsets, u64 n_unitigs, const uint8_t* keep_u, void* area,
                                    unsigned long long* h_pinned, u64* h_out, hipStream_t st);
// kmx_count_clean.hip: which unitigs to drop -- a keep byte and, unless reason == nullptr, a reason byte per unitig (n_unitigs >= 1;
// circular and sums may be nullptr); no working set, asynchronous
hipError_t launch_count_unitig_clean(const u64* offsets, const uint8_t* circular, const u64* sums, u64 n_unitigs, const u64* link_offsets,
                                     const u64* links, u64 n_links, u64 tip_max, u32 tip_num, u32 tip_den, u64 bubble_max, u64 bubble_diff,
                                     u64 island_max, uint8_t* keep, uint8_t* reason, hipStream_t st);
// kmx_count_components.hip: the connected components of the unitig graph -- label writes the labels and counts the components (one
// host round trip per round and one for the count; mask may be nullptr; *bad: the rounds ran out), emit writes, unless nullptr, the
// ids and the records (offsets and sums may be nullptr).  own_rank: the area holds a word per unitig for the roots' ids (records
// without ids)
size_t count_components_bytes(u64 n_unitigs, bool own_rank);
hipError_t launch_count_components_label(const u64* link_offsets, const u64* links, u64 n_links, const uint8_t* mask, u64 n_unitigs, u64* labels,
                                         void* area, bool own_rank, unsigned long long* h_pinned, u64* h_components, u32* h_rounds, bool* bad,
                                         hipStream_t st);
hipError_t launch_count_components_emit(const u64* labels, u64 n_unitigs, const u64* offsets, const u64* sums, const void* area, bool own_rank, u64* ids,
                                        u64* records, u64 n_components, hipStream_t st);
// kmx_count_link_support.hip: support[l] += the junctions of the segments that cross link slot l or its mirror, summary[0 .. 3) +=
// junctions, crossed, unlinked (n_segments >= 2; n_unitigs == 0 reads no offsets: every junction is unlinked); and the edges with
// the bit of every cut link slot cleared (n >= 1; the slots are those of launch_count_links_emit over the same arrays).  Both
// asynchronous, no work buffer
hipError_t launch_count_link_support(const u64* segments, u64 n_segments, const u64* offsets, u64 n_unitigs, const u64* link_offsets, const u64* links,
                                     u64 n_links, u64* support, u64* summary, hipStream_t st);
hipError_t launch_count_adjacency_cut(const uint8_t* edges, const uint8_t* flips, const u64* nbr, u64 n, const u64* nodes, const u64* offsets,
                                      u64 n_unitigs, const u64* place, const u64* link_offsets, u64 n_links, const uint8_t* cut, uint8_t* edges_out,
                                      hipStream_t st);
// The four kmx_reads_*.hip units share kmx_reads_common.h (the span of a read, "is one of ACGTacgt", the wave-per-read launch shape);
// the two that produce a batch, edit and merge, and kmx_fastx_format.hip share kmx_reads_plan.h on top of it (the plan's place in the
// work area, the body of its count kernel, the scans and the read-back; the block search and dword assembly of the two copies).
// kmx_reads_edit.hip: a new ragged batch from an old one (kmx_reads_select / kmx_reads_gather).  A ROW is a source read (select:
// index == nullptr, n_rows == n_reads) or an entry of the index (gather).  The count plans every row in an area of
// reads_edit_bytes(n_rows) and brings back h_out[0 .. 4) = output reads, output bases, the batch's first and last offset (0, 0 for
// uniform reads): synchronous, one round trip.  The emit writes offsets, index (optional) and bytes from the same area (n_out,
// n_bases: what the count returned); asynchronous.
struct ReadsEdit {
    const uint8_t* bases;
    const u64* offsets;   // nullptr: uniform reads of read_len bases
    u64 n_reads;
    u32 read_len;
    const uint8_t* keep;  // nullptr: every read
    const u64* span;      // nullptr: the whole read
    u64 span_stride;
    u32 span_k;
    u64 min_len;
    const u64* index;     // gather: the source read of every row
    u64 n_rows;
};
size_t reads_edit_bytes(u64 n_rows);
hipError_t launch_reads_edit_count(const ReadsEdit& e, void* area, unsigned long long* h_pinned, u64* h_out, hipStream_t st);
hipError_t launch_reads_edit_emit(const ReadsEdit& e, void* area, u64 n_out, u64 n_bases, uint8_t* out_bases, u64* out_offsets, u64* out_index,
                                  hipStream_t st);
// kmx_fastx_format.hip: the batch as a FASTQ / FASTA image (kmx_fastx_format).  The count plans every record in an area of
// fastx_format_bytes(n_reads, own_offsets) and brings back h_out[0 .. 6) = records, bytes of the image, the first and last offset of
// the reads and of the names (0, 0 for a uniform batch): synchronous, one round trip.  The emit writes the record offsets (into the
// area with own_offsets, else into rec_offsets) and, with text != nullptr, the image; asynchronous.
struct FastxFormat {
    const uint8_t* bases;
    const u64* offsets;        // nullptr: uniform reads of read_len bases
    u64 n_reads;
    u32 read_len;
    const uint8_t* quals;      // laid out as the bases are; nullptr: `fill`
    const uint8_t* names;      // has_names: a batch of n_reads names
    const u64* name_offsets;   // nullptr: uniform names of name_len bytes
    u32 name_len;
    u32 name_skip;
    u64 name_base;             // !has_names: record r is named name_base + r in decimal
    u32 width;                 // FASTA: bases per line, 0 = one line
    u32 fill;
    bool has_names, fastq;
};
size_t fastx_format_bytes(u64 n_reads, bool own_offsets);
hipError_t launch_fastx_format_count(const FastxFormat& f, void* area, bool own_offsets, unsigned long long* h_pinned, u64* h_out, hipStream_t st);
hipError_t launch_fastx_format_emit(const FastxFormat& f, void* area, bool own_offsets, u64* rec_offsets, u64 n_bytes, uint8_t* text, hipStream_t st);
// kmx_reads_quality.hip: the masked copy and / or KMX_RQ_WORDS u64 per read out of the bases and the quality bytes (kmx_reads_quality;
// a wave per read, asynchronous)
struct ReadsQuality {
    const uint8_t* bases;
    const u64* offsets;   // nullptr: uniform reads of read_len bases
    u64 n_reads;
    u32 read_len;
    const uint8_t* quals;
    u32 phred, min_q, trim_q, k;
    const u64* weights;   // 256 words or nullptr
    uint8_t* masked;      // or nullptr
    u64* rows;            // KMX_RQ_WORDS per read, or nullptr
};
hipError_t launch_reads_quality(const ReadsQuality& a, int n_cu, hipStream_t st);
// kmx_reads_adapter.hip: KMX_RA_WORDS u64 per read (kmx_reads_adapter) and KMX_RP_WORDS u64 per mate pair (kmx_reads_pair_overlap); a
// wave per read or pair, asynchronous, no work buffer.  The adapters travel in the kernel arguments as bit planes: bit j of lo / hi =
// the low / high bit of the code (byte >> 1) & 3 of adapter base j, bit j of care = base j exists and is no wildcard.
struct ReadsAdapter {
    const uint8_t* bases;
    const u64* offsets;   // nullptr: uniform reads of read_len bases
    u64 n_reads;
    u32 read_len;
    u32 n_adapters;       // 1 .. KMX_RA_MAX_ADAPTERS
    u64 lo[KMX_RA_MAX_ADAPTERS], hi[KMX_RA_MAX_ADAPTERS], care[KMX_RA_MAX_ADAPTERS];
    u32 len[KMX_RA_MAX_ADAPTERS];
    u32 min_overlap, err_num, err_den;
    u64* rows;
};
struct ReadsPairOverlap {
    const uint8_t *bases1, *bases2;
    const u64 *offsets1, *offsets2;   // nullptr: uniform reads of read_len1 / read_len2 bases
    u64 n_reads;
    u32 read_len1, read_len2;
    u32 min_overlap, max_mism, err_num, err_den;
    u64* rows;
};
hipError_t launch_reads_adapter(const ReadsAdapter& a, int n_cu, hipStream_t st);
hipError_t launch_reads_pair_overlap(const ReadsPairOverlap& a, int n_cu, hipStream_t st);
// kmx_reads_complexity.hip: the masked copy and / or KMX_RX_WORDS u64 per read out of the bases alone (kmx_reads_complexity; a wave
// per read, asynchronous, no work buffer)
struct ReadsComplexity {
    const uint8_t* bases;
    const u64* offsets;   // nullptr: uniform reads of read_len bases
    u64 n_reads;
    u32 read_len;
    u32 tail_bases, head_bases;   // letters looked for at either end: bit 0 A, 1 C, 2 G, 3 T
    u32 min_len, err_num, err_den, penalty;
    u32 dust_max;
    uint8_t* masked;      // or nullptr
    u64* rows;            // KMX_RX_WORDS per read, or nullptr
};
hipError_t launch_reads_complexity(const ReadsComplexity& a, int n_cu, hipStream_t st);
// kmx_reads_merge.hip: the consensus read of every mate pair (kmx_reads_pair_merge).  The count lays the plan's partial sums (merged
// pairs, merged bases, per block of pairs) into `area` of reads_merge_bytes(n_reads) and brings back h_out[0 .. 6) = merged pairs,
// merged bases, then the first and last offset of batch 1 and of batch 2 (0, 0 for uniform reads): synchronous, one round trip.
// The emit writes the offsets from the same area (where out_offsets is given), then bases, quality bytes and rows, a wave per pair;
// asynchronous.  out_bases == nullptr with rows: the rows alone.
struct ReadsPairMerge {
    const uint8_t *bases1, *bases2;
    const u64 *offsets1, *offsets2;   // nullptr: uniform reads of read_len1 / read_len2 bases
    const uint8_t *quals1, *quals2;   // both or neither
    const u64* insert;                // insert[r * insert_stride]: the insert size of pair r
    u64 insert_stride;
    u64 n_reads;
    u32 read_len1, read_len2;
    u32 phred_base, q_cap;
    uint8_t *out_bases, *out_quals;
    u64 *out_offsets, *rows;
};
size_t reads_merge_bytes(u64 n_reads);
hipError_t launch_reads_merge_count(const ReadsPairMerge& a, void* area, unsigned long long* h_pinned, u64* h_out, hipStream_t st);
hipError_t launch_reads_merge_emit(const ReadsPairMerge& a, void* area, int n_cu, hipStream_t st);
// kmx_reads_dedup.hip: duplicate reads and pairs (kmx_reads_dedup).  Keys, the two-word counter's sort (launch_count_sort /
// launch_count_emit), groups and the verification, all in `area` of reads_dedup_bytes(n_reads, n_cu); h_summary[0 .. KMX_DD_SUMMARY_WORDS)
// comes back.  Synchronous: the sort's round trips and one for the summary.  *bad: the sort did not give n_reads distinct records
// or overflowed its level arrays (a bug, never expected); nothing of the rows is to be trusted then.
struct ReadsDedup {
    const uint8_t *bases1, *bases2;
    const u64 *offsets1, *offsets2;   // nullptr: uniform reads of read_len1 / read_len2 bases
    u64 n_reads;
    u32 read_len1, read_len2;
    u32 pairs;                        // an item is a pair (0: a read of batch 1; batch 2 is not looked at)
    u32 strand;                       // KMX_DD_STRAND
    u32 hash_bits;                    // 1 .. 64
    const u64* score;                 // score[r * score_stride], or nullptr
    u64 score_stride;
    u64* rows;
    uint8_t* keep;                    // or nullptr
};
size_t reads_dedup_bytes(u64 n_reads, int n_cu);
hipError_t launch_reads_dedup(const ReadsDedup& a, void* area, unsigned long long* h_pinned, u64* h_summary, bool* bad, int n_cu, hipStream_t st);
// kmx_count_setop.hip: set algebra and comparison of two count tables (`words` u64 per key: 1 or 2; n = n_a + n_b)
size_t count_setop_bytes(u64 n);
hipError_t launch_count_setop(u32 words, u32 op, const u64* ka, const u64* ca, u64 na, const u64* kb, const u64* cb, u64 nb, void* area,
                              unsigned long long* h_pinned, u64* h_out, hipStream_t st);
hipError_t launch_count_setop_emit(u32 words, u32 op, u32 rule, const u64* ka, const u64* ca, u64 na, const u64* kb, const u64* cb, u64 nb,
                                   const void* area, u64* out_k, u64* out_c, hipStream_t st);
hipError_t launch_count_compare(u32 words, const u64* ka, const u64* ca, u64 na, const u64* kb, const u64* cb, u64 nb, void* area,
                                unsigned long long* h_pinned, u64* h_rec, hipStream_t st);
// kmx_sketch.hip: the counting sketch (`words` u64 per key: 1 or 2; sketch: 64 << log2_blocks bytes, 64-byte aligned).  add: weights
// may be nullptr (1 each); flags may be nullptr, otherwise a key counts where its flag has KMX_WIN_VALID.  lookup: est[i] = 0 where the
// flag lacks it.  filter: clears KMX_WIN_VALID where the estimate is below min_est (1..255).  All asynchronous, no working set.
hipError_t launch_sketch_add(u32 words, const u64* keys, const u64* weights, const uint8_t* flags, u64 n, uint8_t* sketch, u32 log2_blocks, u64 seed,
                             int n_cu, hipStream_t st);
hipError_t launch_sketch_lookup(u32 words, const u64* keys, const uint8_t* flags, u64 n, const uint8_t* sketch, u32 log2_blocks, u64 seed,
                                uint8_t* est, int n_cu, hipStream_t st);
hipError_t launch_sketch_filter(u32 words, const u64* keys, uint8_t* flags, u64 n, const uint8_t* sketch, u32 log2_blocks, u64 seed, u32 min_est,
                                int n_cu, hipStream_t st);
hipError_t launch_sketch_merge(const uint8_t* a, const uint8_t* b, u32 log2_blocks, uint8_t* out, int n_cu, hipStream_t st);
hipError_t launch_sketch_stats(const uint8_t* sketch, u32 log2_blocks, u64* hist, int n_cu, hipStream_t st);
// kmx_hll.hip: the distinct-key estimator (`words` u64 per key: 1 or 2; regs: 1 << log2_regs bytes, 16-byte aligned, 4 <= log2_regs
// <= 24).  add: flags may be nullptr, otherwise a key counts where its flag has KMX_WIN_VALID.  stats: b may be nullptr (64
// bins), otherwise 192: a, b, max(a, b).  All asynchronous, no working set.
hipError_t launch_hll_add(u32 words, const u64* keys, const uint8_t* flags, u64 n, uint8_t* regs, u32 log2_regs, u64 seed, int n_cu, hipStream_t st);
hipError_t launch_hll_merge(const uint8_t* a, const uint8_t* b, u32 log2_regs, uint8_t* out, int n_cu, hipStream_t st);
hipError_t launch_hll_stats(const uint8_t* a, const uint8_t* b, u32 log2_regs, u64* hist, int n_cu, hipStream_t st);
// kmx_bgzf.hip: the block index of a BGZF image and its inflation.  The index's working set: `units` bytes for the counting pass, the
// whole once the number of candidates (header patterns) is known.  Its first words (`stats`) after count_candidates: [2] = candidates;
// after chain: [0] = text bytes, [1] = end of the last block, [3] = blocks, [5] = start of the last block.  All asynchronous.
size_t bgzf_index_units_bytes(u64 n_bytes);
size_t bgzf_index_scratch_bytes(u64 n_bytes, u64 n_candidates);
hipError_t launch_bgzf_count_candidates(const uint8_t* file, u64 n_bytes, void* scratch, int n_cu, hipStream_t st);
hipError_t launch_bgzf_chain(const uint8_t* file, u64 n_bytes, void* scratch, u32 n_candidates, int n_cu, hipStream_t st);
hipError_t launch_bgzf_write_index(const uint8_t* file, u64 n_bytes, void* scratch, u32 n_candidates, u64 n_blocks, u64 end, u64* block_offsets,
                                   u64* text_offsets, int n_cu, hipStream_t st);
hipError_t launch_bgzf_inflate(const uint8_t* file, u64 n_bytes, const u64* block_offsets, const u64* text_offsets, u64 n_blocks, u64 span, uint8_t* text,
                               u32* status, unsigned long long* first_bad, bool check_crc, hipStream_t st);
// kmx_bgzf.hip: a text compressed to BGZF.  The working set: bgzf_deflate_meta_bytes for the per-piece words, and behind them one
// slot of bgzf_deflate_slot_bytes per piece coded at a time (slot_bytes 0: every piece stored, no slots).  Its first words (`stats`,
// cleared by the caller) after deflate_offsets: [0] = bytes of the image, [1] = stored blocks; bgzf_deflate_offsets: the n_pieces + 2
// offsets (the marker's, the image's end).  blocks(sizing) over all pieces, offsets, then copy -- or, where the slots do not hold all
// pieces, per chunk blocks(!sizing) and copy.  All asynchronous.
size_t bgzf_deflate_meta_bytes(u64 n_pieces);
u32 bgzf_deflate_slot_bytes(u32 block_bytes);
const void* bgzf_deflate_offsets(void* scratch);
hipError_t launch_bgzf_deflate_blocks(const uint8_t* text, u64 n_bytes, u32 block_bytes, u64 n_pieces, u64 b0, u64 b1, u32 slot_bytes, bool sizing,
                                      void* scratch, int n_cu, hipStream_t st);
hipError_t launch_bgzf_deflate_offsets(u64 n_pieces, void* scratch, hipStream_t st);
hipError_t launch_bgzf_deflate_copy(const uint8_t* text, u64 n_bytes, u32 block_bytes, u64 n_pieces, u64 slot_b0, u64 b0, u64 b1, u32 slot_bytes,
                                    void* scratch, u64 bytes_about, uint8_t* file, int n_cu, hipStream_t st);
}  // namespace kmx
