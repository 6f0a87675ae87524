// kmx_internal.h -- host-side state shared by the translation units behind include/kmx.h
// (kmx_api.hip: entry points; kmx_comm.hip: the RCCL communicator).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/kmx.h"
#include "kmx_layout.h"

struct kmx_ctx {
    int device;
    hipStream_t stream;
    bool owns_stream;
    int n_cu;
    unsigned long long* h_pinned;   // eight pinned host words for read-backs on the context's own stream (kmx_layout.h, KMX_PIN_*)
    unsigned long long* d_scratch;  // KMX_SCRATCH_BYTES: the scratch words and the queue block (kmx_layout.h, KMX_S_* and KMX_Q_*)
    unsigned long long* h_pub;      // eight pinned host words the bit-sliced scan's last block can leave {token, marked reads, summary} in (kmx_canonical_reduce_host)
    uint32_t pub_token;             // the token of the last such launch (24 bits)
    bool queue_clean;               // the heads and KMX_Q_MARKED of the queue block are zero: only self-closing launches (kmx_layout.h) ran since the last clear
    unsigned long long dirty_desc;  // address of the dirty-tile flags as last written behind the queue heads
    uint8_t* d_flags;               // one byte per tile, all zero between calls
    size_t flags_bytes;
    // The work buffer: grow-only device memory that every call family lays its working set out in (the id streams of the partitioned
    // histogram, the segment plans of long reads, the arrays of the count, query and reads families, the chunk summaries of the FASTX
    // parses); a call's contents are dead when the call returns.  d_big, big_bytes and big_allocs are read and written only by the
    // acquire group at the top of kmx_api.hip (work_acquire), context creation / destruction and kmx_ctx_work_buffer_info.
    void* d_big;
    size_t big_bytes;
    unsigned long long big_allocs;  // how often the work buffer was (re)allocated (kmx_ctx_work_buffer_info)
    size_t big_limit;               // kmx_ctx_set_work_buffer_limit: 0 = automatic (an eighth of the device memory, at most half of what is free)
    // The FASTX count cache, the one thing in the work buffer that outlives a call: what the last counting pass of a parse was run on --
    // a second call on the same image with KMX_FASTX_SAME_TEXT reuses its chunk prefixes (they live in d_big) instead of summarising
    // the text again.  Written by the parse body (fastx_lines) alone; work_acquire clears fx_valid for every other taker of the buffer.
    const uint8_t* fx_text;
    uint64_t fx_bytes;
    uint32_t fx_fasta;
    uint32_t fx_entry;              // the line the chunk prefixes and totals were placed for: 0 = the reads, 2 = the quality lines (kmx_fastx_parse_quals)
    bool fx_valid;
    unsigned long long fx_totals[2];
    char last_error[256];
};

namespace kmx {
int fail_hip(kmx_ctx* ctx, hipError_t e, const char* where);

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};
}  // namespace kmx

#define KMX_HIP(ctx, expr)                                            \
    do {                                                              \
        hipError_t e__ = (expr);                                      \
        if (e__ != hipSuccess) return kmx::fail_hip(ctx, e__, #expr); \
    } while (0)
