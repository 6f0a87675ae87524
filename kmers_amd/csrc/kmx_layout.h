// kmx_layout.h -- the one definition of the context's scratch block (kmx_ctx::d_scratch, u64 words), of the queue block inside it and
// of the pinned host words kmx_api.hip uses (kmx_ctx::h_pinned).  Host and device code address them through these names only.
#pragma once

#include <cstddef>
#include <cstdint>

namespace kmx {

// ---- d_scratch, zeroed at kmx_ctx_create:
//   [KMX_S_FIRST_BAD]     the first invalid / out-of-range element an element-wise call found (~0: none)
//   [KMX_S_FASTX_TOTALS]  two words: reads and bases of kmx_fastx_parse's last counting pass
//   [KMX_S_LEN_RANGE]     kmx_reads_length_range's {min, max}, two u32
//   [KMX_S_TOO_LONG]      the sticky flag: a read of 2^31 bases or more was skipped (kmx_ctx_synchronize); kernels reach it as
//                         queue + KMX_TOOLONG_FROM_QUEUE
//   [KMX_S_QUEUE]         the queue block: `queue` = d_scratch + KMX_S_QUEUE
constexpr size_t KMX_SCRATCH_BYTES = 8192;
constexpr uint32_t KMX_S_FIRST_BAD = 0, KMX_S_FASTX_TOTALS = 2, KMX_S_LEN_RANGE = 4, KMX_S_TOO_LONG = 8, KMX_S_QUEUE = 16;
constexpr int KMX_TOOLONG_FROM_QUEUE = (int)KMX_S_TOO_LONG - (int)KMX_S_QUEUE;

// ---- the queue block (u64 words from `queue`), as the tiled scans use it:
//   [q * KMX_Q_HEAD_STRIDE], q < KMX_Q_HEADS   ticket heads, 128 bytes apart
//   [KMX_Q_MARKED]      reads marked so far (running count of the launch)
//   [KMX_Q_GATE]        the uniform / ragged gate, two u32: {verdict (1 = armed), the length the gate found}
//   [KMX_Q_MASKS]       address of the context's mask array (one 64-bit read mask per tile; 0 = no array)
//   [KMX_Q_MARKED_OUT]  the marked reads of the LAST bit-sliced launch, for its sweep (overwritten, never cleared)
//   [KMX_Q_HOST]        the context's pinned host words as the device sees them (written once, kmx_ctx_create)
//   [KMX_Q_RESULT]      kmx_canonical_reduce_host's summary (four words)
//   [KMX_Q_QUIET]       a quiet line of KMX_Q_QUIET_WORDS (stand-in source of loads that must not fault)
//   [KMX_Q_DONE]        blocks of the launch that have handed in their sums
//   [KMX_Q_SLOTS + KMX_Q_SLOT_STRIDE * s + i]   partial summary s < KMX_Q_N_SLOTS (block b adds into s = b & 15), word i < 6
// The bit-sliced scan CLOSES its own launch: the last block to hand in adds the partial summaries up, writes the result, and puts
// the heads, [KMX_Q_MARKED], [KMX_Q_DONE] and the partials back to zero -- so a caller that knows only such launches ran since its
// last clear need not clear again (two fill kernels and their gaps: 11 us of a small batch's 70, profiles/r06_small_batches.txt).
constexpr uint32_t KMX_Q_HEADS = 32, KMX_Q_HEAD_STRIDE = 16, KMX_Q_MARKED = 512, KMX_Q_GATE = 513, KMX_Q_MASKS = 515, KMX_Q_MARKED_OUT = 516,
                   KMX_Q_HOST = 517, KMX_Q_RESULT = 528, KMX_Q_QUIET = 544, KMX_Q_QUIET_WORDS = 16, KMX_Q_DONE = 560, KMX_Q_SLOTS = 576,
                   KMX_Q_SLOT_STRIDE = 16, KMX_Q_N_SLOTS = 16;
// What a clear ahead of a launch zeroes, in bytes from `queue`: the heads; the heads and [KMX_Q_MARKED]; those and the gate.
constexpr size_t KMX_Q_CLEAR_HEADS = 8u * KMX_Q_HEADS * KMX_Q_HEAD_STRIDE, KMX_Q_CLEAR_THROUGH_MARKED = 8u * (KMX_Q_MARKED + 1u),
                 KMX_Q_CLEAR_THROUGH_GATE = 8u * (KMX_Q_GATE + 1u);

// ---- h_pinned: [KMX_PIN_READ] two words of read-backs (the sticky flag, a first-bad word, a batch's first and last offset; the
// launchers of kmx_count.hip read up to seven words from here); [KMX_PIN_SUMMARY] four words, a kmx_summary
// (kmx_canonical_reduce_host); [KMX_PIN_HOST_VIEW] where KMX_Q_HOST is staged at kmx_ctx_create
constexpr size_t KMX_PIN_BYTES = 64;
constexpr uint32_t KMX_PIN_READ = 0, KMX_PIN_SUMMARY = 2, KMX_PIN_HOST_VIEW = 7;

// (minimizers_reads_kernel's idle threads load the 20 bytes from [KMX_S_FIRST_BAD] as a stand-in and ignore them: kmx_minimizers.hip)
static_assert(8u * (KMX_S_FIRST_BAD + 3u) <= KMX_SCRATCH_BYTES, "three readable words from KMX_S_FIRST_BAD");
static_assert(KMX_S_FASTX_TOTALS > KMX_S_FIRST_BAD && KMX_S_LEN_RANGE >= KMX_S_FASTX_TOTALS + 2 && KMX_S_TOO_LONG > KMX_S_LEN_RANGE &&
              KMX_S_QUEUE > KMX_S_TOO_LONG, "d_scratch words overlap");
static_assert(KMX_Q_MARKED >= KMX_Q_HEADS * KMX_Q_HEAD_STRIDE && KMX_Q_GATE > KMX_Q_MARKED && KMX_Q_MASKS > KMX_Q_GATE &&
              KMX_Q_MARKED_OUT > KMX_Q_MASKS && KMX_Q_HOST > KMX_Q_MARKED_OUT && KMX_Q_RESULT > KMX_Q_HOST && KMX_Q_QUIET >= KMX_Q_RESULT + 4 &&
              KMX_Q_DONE >= KMX_Q_QUIET + KMX_Q_QUIET_WORDS && KMX_Q_SLOTS > KMX_Q_DONE, "queue block words overlap");
static_assert(KMX_Q_CLEAR_HEADS == 8u * KMX_Q_MARKED && KMX_Q_CLEAR_THROUGH_MARKED == 8u * KMX_Q_GATE, "a clear ends right behind its last word");
static_assert(8u * (KMX_S_QUEUE + KMX_Q_SLOTS + KMX_Q_SLOT_STRIDE * KMX_Q_N_SLOTS) <= KMX_SCRATCH_BYTES, "the queue block overruns d_scratch");
static_assert(KMX_PIN_SUMMARY >= KMX_PIN_READ + 2 && KMX_PIN_HOST_VIEW >= KMX_PIN_SUMMARY + 4 && 8u * (KMX_PIN_HOST_VIEW + 1) <= KMX_PIN_BYTES,
              "pinned host words overlap");

}  // namespace kmx
