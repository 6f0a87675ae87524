// kmx_api.hip -- the extern "C" boundary declared in include/kmx.h: argument checking,
// kernel selection and HIP error mapping.  No CPU compute path exists here: every entry
// point launches a gfx950 kernel or returns an error.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "kmx_internal.h"
#include "kmx_launch.h"

namespace kmx {
int fail_hip(kmx_ctx* ctx, hipError_t e, const char* where) {
    if (ctx) std::snprintf(ctx->last_error, sizeof ctx->last_error, "%s: %s", where, hipGetErrorString(e));
    return KMX_E_HIP;
}
}  // namespace kmx
using namespace kmx;   // (the launchers, kmx_launch.h, are called qualified; the layout's names, kmx_layout.h, are not)

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0u; }

// the words of d_scratch the calls address (kmx_layout.h)
unsigned long long* queue_of(kmx_ctx* ctx) { return ctx->d_scratch + KMX_S_QUEUE; }
unsigned long long* too_long_of(kmx_ctx* ctx) { return ctx->d_scratch + KMX_S_TOO_LONG; }
unsigned long long* first_bad_of(kmx_ctx* ctx) { return ctx->d_scratch + KMX_S_FIRST_BAD; }
uint32_t* gate_of(kmx_ctx* ctx) { return reinterpret_cast<uint32_t*>(queue_of(ctx) + KMX_Q_GATE); }

// Zero the first `bytes` of the context's queue block (KMX_Q_CLEAR_*) ahead of a launch that takes tickets.  The bit-sliced scans
// put back what they use (kmx_layout.h); every other user leaves its tickets behind.
hipError_t queue_clear(kmx_ctx* ctx, size_t bytes) {
    ctx->queue_clean = false;
    return hipMemsetAsync(queue_of(ctx), 0, bytes, ctx->stream);
}

// The uniform / ragged gate (kmx_canonical_reduce, kmx_canonical_reduce2): armed ahead of offsets_uniform_gate_kernel, which leaves
// its verdict in it; disarmed (verdict and length) behind the launches that read it, so it is never left armed.
hipError_t gate_arm(kmx_ctx* ctx) { return hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(gate_of(ctx)), 1, 1, ctx->stream); }
hipError_t gate_disarm(kmx_ctx* ctx) { return hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(gate_of(ctx)), 0, 2, ctx->stream); }

// The element-wise calls that report their first invalid / out-of-range element: KMX_S_FIRST_BAD is set to "none" (~0) ahead of
// the launch and read back, with a wait, into `h_bad` (a word of the caller's, or a pinned one) behind it.
hipError_t first_bad_reset(kmx_ctx* ctx) { return hipMemsetAsync(first_bad_of(ctx), 0xFF, 8, ctx->stream); }
int first_bad_read(kmx_ctx* ctx, unsigned long long* h_bad) {
    KMX_HIP(ctx, hipMemcpyAsync(h_bad, first_bad_of(ctx), 8, hipMemcpyDeviceToHost, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMX_OK;
}

// The bit-sliced scan blanks the reads that hold an invalid byte out of their tile and leaves their 64-bit mask (8 bytes
// per tile) for sweep_flagged_kernel (kmx_sweep.hip; kmx_bitslice_kernel.h, "reads with an invalid byte").  The masks are the context's
// own grow-only array, zeroed when it is allocated; the rolling kernel clears every mask it consumes, so it is all-zero
// again when a call ends and nothing has to be cleared per call.  Its address sits in the queue block (KMX_Q_MASKS), rewritten only
// when it changes.  No array: 0, and such tiles take the per-lane path as a whole, as they do for k without a bit-sliced kernel.
int prepare_dirty_flags(kmx_ctx* ctx, uint64_t n_reads, uint32_t k, bool any_k = false) {
    const uint64_t n_tiles = n_reads >> 6;
    uint8_t* buf = nullptr;
    if (n_tiles && (any_k || (k >= 9 && k <= 31) || (k >= 33 && k <= 64))) {   // the k with a bit-sliced kernel (any_k: the word-domain scan's histogram sinks mark too)
        if (8u * n_tiles > ctx->flags_bytes) {   // one 64-bit read mask per tile
            if (ctx->d_flags) {
                (void)hipStreamSynchronize(ctx->stream);
                (void)hipFree(ctx->d_flags);
                ctx->d_flags = nullptr;
                ctx->flags_bytes = 0;
            }
            const size_t want_bytes = 8u * (size_t)(n_tiles + n_tiles / 4u + 4096u);
            void* q = nullptr;
            // (cleared on the context's stream: a non-blocking stream is not ordered against the null stream hipMemset runs on)
            if (hipMalloc(&q, want_bytes) == hipSuccess && hipMemsetAsync(q, 0, want_bytes, ctx->stream) == hipSuccess) {
                ctx->d_flags = static_cast<uint8_t*>(q);
                ctx->flags_bytes = want_bytes;
            } else {
                (void)hipGetLastError();
                if (q) (void)hipFree(q);
            }
        }
        buf = 8u * n_tiles <= ctx->flags_bytes ? ctx->d_flags : nullptr;
        if (!buf) {   // one byte per 64 reads: if even that cannot be had, nothing else will work either
            std::snprintf(ctx->last_error, sizeof ctx->last_error, "kmx: no memory for %llu tile flags", (unsigned long long)n_tiles);
            return KMX_E_NOMEM;
        }
    }
    const unsigned long long want = (unsigned long long)reinterpret_cast<uintptr_t>(buf);
    if (want != ctx->dirty_desc) {
        ctx->dirty_desc = want;
        hipError_t e = hipMemcpyAsync(queue_of(ctx) + KMX_Q_MASKS, &ctx->dirty_desc, 8, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return fail_hip(ctx, e, "dirty-tile flags");
    }
    return KMX_OK;
}

// The queue block cleared through the gate, then the mask array for `n_reads` reads (prepare_dirty_flags): ahead of a tiled launch.
int queue_clear_marks(kmx_ctx* ctx, uint64_t n_reads, uint32_t k, bool any_k) {
    KMX_HIP(ctx, queue_clear(ctx, KMX_Q_CLEAR_THROUGH_GATE));
    return prepare_dirty_flags(ctx, n_reads, k, any_k);
}

// ---- the context's work buffer (kmx_internal.h).  Only this group, the context's creation and destruction and
// kmx_ctx_work_buffer_info touch d_big / big_bytes / big_allocs. ----
// A hold on the buffer: where it was, how large as a whole and which allocation it was when it was handed out.  A hold is not
// exclusive: count_impl and the reads forms of the queries lay their arrays out in the buffer and then call kmx_canonical_windows,
// which takes the start of the same buffer for its segment plan (count_plan_bytes) -- so whoever called out checks work_kept.
struct WorkHold {
    char* base = nullptr;
    size_t size = 0;
    unsigned long long allocs = 0;
    size_t reserved = 0;   // query_scratch: the bytes at the start that are the holder's arrays; the lookup's directory goes behind them
    bool kept(const kmx_ctx* ctx) const { return ctx->d_big == base && ctx->big_allocs == allocs; }
};

// The one place the buffer is handed out: grown on demand (hipFree / hipMalloc synchronise, so only when it must grow), kept until
// the context is destroyed; no base: no memory.  Whoever takes the buffer here has invalidated the FASTX count cache (fx_*, whose
// chunk prefixes live in the buffer); nothing else needs to.  `keep_fastx`: the FASTX parse itself, whose cache goes only when the
// buffer moves.
WorkHold work_acquire(kmx_ctx* ctx, size_t bytes, bool keep_fastx = false) {
    const bool grow = bytes > ctx->big_bytes;
    if (grow || !keep_fastx) ctx->fx_valid = false;
    if (grow) {
        if (ctx->d_big) {
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipFree(ctx->d_big);
            ctx->d_big = nullptr;
            ctx->big_bytes = 0;
        }
        void* q = nullptr;
        if (hipMalloc(&q, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return WorkHold{};
        }
        ctx->big_allocs += 1;
        ctx->d_big = q;
        ctx->big_bytes = bytes;
    }
    return WorkHold{static_cast<char*>(ctx->d_big), ctx->big_bytes, ctx->big_allocs};
}

// (a callee took a route that grew the work buffer under the arrays laid out in it: a bug, never expected)
int work_kept(kmx_ctx* ctx, const char* who, const WorkHold& hold) {
    if (hold.kept(ctx)) return KMX_OK;
    char msg[96];
    std::snprintf(msg, sizeof msg, "%s: work buffer moved", who);
    return fail_hip(ctx, hipErrorUnknown, msg);
}

// What the histogram launchers ask their scratch of (user = the context); nullptr => they fall back to the global-atomic kernel.
void* work_callback(void* user, size_t bytes) { return work_acquire(static_cast<kmx_ctx*>(user), bytes).base; }

// The segment arrays of the long-read paths (16-24 bytes per segment): inside the cap of kmx_ctx_set_work_buffer_limit, or not at
// all -- the call then takes the per-read kernels, as it does when the allocation fails.
void* capped_scratch(kmx_ctx* ctx, size_t bytes) {
    if (ctx->big_limit != 0 && bytes > ctx->big_limit) return nullptr;
    return work_acquire(ctx, bytes).base;
}

// The cap on the work buffer: an eighth of the device memory, at least 8 GiB (kmx_ctx_set_work_buffer_limit overrides), and at most
// half of what is free: fewer, larger chunks of reads per call (configs[4], 1.25e8 reads: 6 chunks at 8 GiB 19.3 ms, 2 at 36 GiB 18.6 ms)
// (`held`: the work buffer the context already owns -- it is not part of "free" any more, but it IS available: without adding
// it back a second call under memory pressure got a smaller budget than the buffer it holds, cut the reads into more chunks
// than the first call had, and timing depended on call order)
size_t work_budget(const kmx_ctx* ctx) {
    if (ctx->big_limit) return ctx->big_limit;
    const size_t held = ctx->big_bytes;
    size_t free_b = 0, total_b = 0;
    const bool have = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    size_t budget = (size_t)8 << 30;
    if (have && total_b / 8u > budget) budget = total_b / 8u;
    if (have && budget > (free_b + held) / 2) budget = (free_b + held) / 2;
    if (budget < held) budget = held;
    return budget;
}

bool reads_ok(const kmx_reads* r) {
    if (!r) return false;
    if (r->n_reads && !r->d_bases && (r->d_offsets || r->read_len)) return false;
    return true;
}

// ---- host-side restatement of the per-encoding tables of src/encoding/naive.rs ----
// rev_encoding (naive.rs:28-39)
u32 rev_encoding(u32 enc) {
    u32 rev = 0;
    rev ^= 0u << (6 - ((enc >> 6) * 2));
    rev ^= 1u << (6 - (((enc >> 4) & 3) * 2));
    rev ^= 2u << (6 - (((enc >> 2) & 3) * 2));
    rev ^= 3u << (6 - ((enc & 3) * 2));
    return rev & 0xFFu;
}
// complement (naive.rs:98-109) for the four codes, packed 2 bits each
u32 comp_lut_for(u32 enc) {
    const u32 rev = rev_encoding(enc);
    u32 lut = 0;
    for (u32 bits = 0; bits < 4; ++bits) {
        const u32 internal = (rev >> (6 - bits * 2)) & 3;
        const u32 comp_internal = (internal ^ 2u) & 3;
        lut |= ((enc >> (6 - comp_internal * 2)) & 3) << (2 * bits);
    }
    return lut;
}
// bits2nuc (naive.rs:88-95, INTERNAL2NUC :19) for the four codes, one letter per byte
u32 nuc_lut_for(u32 enc) {
    static const unsigned char internal2nuc[4] = {'A', 'C', 'T', 'G'};
    const u32 rev = rev_encoding(enc);
    u32 lut = 0;
    for (u32 bits = 0; bits < 4; ++bits) lut |= (u32)internal2nuc[(rev >> (6 - bits * 2)) & 3] << (8 * bits);
    return lut;
}
// the 24 discriminants of `enum Naive` (naive.rs:48-74) are exactly the bytes whose four 2-bit
// fields are a permutation of {0,1,2,3}
bool enc_ok(u32 enc) {
    if (enc > 0xFFu) return false;
    u32 seen = 0;
    for (int i = 0; i < 4; ++i) seen |= 1u << ((enc >> (2 * i)) & 3);
    return seen == 0xFu;
}

}  // namespace

extern "C" {

int kmx_version(void) { return KMX_VERSION; }

const char* kmx_strerror(int status) {
    switch (status) {
    case KMX_OK: return "ok";
    case KMX_E_ARG: return "invalid argument";
    case KMX_E_K_RANGE: return "k outside the supported range for this call";
    case KMX_E_HIP: return "HIP runtime error (see kmx_last_error)";
    case KMX_E_INVALID_BASE: return "byte is not one of ACGTacgt (reference: encode_binary panics)";
    case KMX_E_TOO_LONG: return "sequence longer than the k-mer storage (reference panics)";
    case KMX_E_NOMEM: return "out of memory";
    default: return "unknown kmx status";
    }
}

static int ctx_create_common(int device, hipStream_t stream, bool owns, kmx_ctx** out) {
    if (!out) return KMX_E_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return KMX_E_HIP;  // fail loudly: no GPU, no kmx
    if (device < 0 || device >= count) return KMX_E_ARG;
    kmx_ctx* c = new (std::nothrow) kmx_ctx();
    if (!c) return KMX_E_NOMEM;
    c->device = device;   // (every other member is zero: the context is value-initialised)
    c->stream = stream;
    c->owns_stream = owns;
    DeviceGuard g(device);
    hipDeviceProp_t prop;
    hipError_t e = g.ok ? hipGetDeviceProperties(&prop, device) : hipErrorInvalidDevice;
    if (e == hipSuccess && owns) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->d_scratch), KMX_SCRATCH_BYTES);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&c->h_pinned), KMX_PIN_BYTES, hipHostMallocDefault);
    // (the dirty-list descriptor behind the queue heads starts as "no list"; cleared on the context's own stream so that
    // the clear is ordered before every kernel the context launches)
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&c->h_pub), 64, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemsetAsync(c->d_scratch, 0, KMX_SCRATCH_BYTES, c->stream);
    if (e == hipSuccess) {
        // the pinned words as the device addresses them, left in the queue block once (kmx_device.h, KMX_Q_HOST)
        void* dev_view = nullptr;
        e = hipHostGetDevicePointer(&dev_view, c->h_pub, 0);
        if (e == hipSuccess) {
            for (int i = 0; i < 8; ++i) c->h_pub[i] = 0;
            c->h_pinned[KMX_PIN_HOST_VIEW] = (unsigned long long)reinterpret_cast<uintptr_t>(dev_view);
            e = hipMemcpyAsync(queue_of(c) + KMX_Q_HOST, c->h_pinned + KMX_PIN_HOST_VIEW, 8, hipMemcpyHostToDevice, c->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (c->d_scratch) (void)hipFree(c->d_scratch);
        if (c->h_pinned) (void)hipHostFree(c->h_pinned);
        if (c->h_pub) (void)hipHostFree(c->h_pub);
        if (owns && c->stream) (void)hipStreamDestroy(c->stream);
        delete c;
        return KMX_E_HIP;
    }
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    *out = c;
    return KMX_OK;
}

int kmx_ctx_create(int device, kmx_ctx** out) { return ctx_create_common(device, nullptr, true, out); }

int kmx_ctx_create_on_stream(int device, void* hip_stream, kmx_ctx** out) {
    return ctx_create_common(device, static_cast<hipStream_t>(hip_stream), false, out);
}

void kmx_ctx_destroy(kmx_ctx* ctx) {
    if (!ctx) return;
    DeviceGuard g(ctx->device);
    if (ctx->d_scratch) (void)hipFree(ctx->d_scratch);
    if (ctx->h_pinned) (void)hipHostFree(ctx->h_pinned);
    if (ctx->h_pub) (void)hipHostFree(ctx->h_pub);
    if (ctx->d_flags) (void)hipFree(ctx->d_flags);
    if (ctx->d_big) (void)hipFree(ctx->d_big);
    if (ctx->owns_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int kmx_ctx_synchronize(kmx_ctx* ctx) {
    if (!ctx) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    // the sticky flag of the scans: a ragged read of 2^31 bases or more was skipped (kmx.h "Limits").  Read back on the context's
    // own stream into pinned memory, ahead of the one wait: no blocking copy on the null stream (which would also synchronise
    // with every other blocking stream of the process)
    KMX_HIP(ctx, hipMemcpyAsync(ctx->h_pinned + KMX_PIN_READ, too_long_of(ctx), 8, hipMemcpyDeviceToHost, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const unsigned long long too_long = ctx->h_pinned[KMX_PIN_READ];
    if (too_long) {
        KMX_HIP(ctx, hipMemsetAsync(too_long_of(ctx), 0, 8, ctx->stream));
        KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::snprintf(ctx->last_error, sizeof ctx->last_error,
                      "a read of 2^31 bases or more was skipped by a scan since the last kmx_ctx_synchronize (cut such records into overlapping pieces)");
        return KMX_E_ARG;
    }
    return KMX_OK;
}

int kmx_ctx_device(const kmx_ctx* ctx) { return ctx ? ctx->device : -1; }

int kmx_ctx_set_work_buffer_limit(kmx_ctx* ctx, size_t bytes) {
    if (!ctx) return KMX_E_ARG;
    ctx->big_limit = bytes;
    return KMX_OK;
}

int kmx_ctx_work_buffer_info(const kmx_ctx* ctx, size_t* bytes_held, uint64_t* n_allocations) {
    if (!ctx) return KMX_E_ARG;
    if (bytes_held) *bytes_held = ctx->big_bytes;
    if (n_allocations) *n_allocations = ctx->big_allocs;
    return KMX_OK;
}

const char* kmx_last_error(const kmx_ctx* ctx) { return ctx ? ctx->last_error : "null ctx"; }

int kmx_malloc(kmx_ctx* ctx, size_t nbytes, void** d_out) {
    if (!ctx || !d_out) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    *d_out = nullptr;
    if (nbytes == 0) return KMX_OK;
    hipError_t e = hipMalloc(d_out, nbytes);
    if (e == hipErrorOutOfMemory) return KMX_E_NOMEM;
    KMX_HIP(ctx, e);
    return KMX_OK;
}

int kmx_free(kmx_ctx* ctx, void* d_ptr) {
    if (!ctx) return KMX_E_ARG;
    if (!d_ptr) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, hipFree(d_ptr));
    return KMX_OK;
}

int kmx_memcpy_h2d(kmx_ctx* ctx, void* d_dst, const void* h_src, size_t nbytes) {
    if (!ctx || (nbytes && (!d_dst || !h_src))) return KMX_E_ARG;
    if (!nbytes) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, hipMemcpyAsync(d_dst, h_src, nbytes, hipMemcpyHostToDevice, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMX_OK;
}

int kmx_memcpy_d2h(kmx_ctx* ctx, void* h_dst, const void* d_src, size_t nbytes) {
    if (!ctx || (nbytes && (!h_dst || !d_src))) return KMX_E_ARG;
    if (!nbytes) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, hipMemcpyAsync(h_dst, d_src, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMX_OK;
}

int kmx_memset(kmx_ctx* ctx, void* d_dst, int value, size_t nbytes) {
    if (!ctx || (nbytes && !d_dst)) return KMX_E_ARG;
    if (!nbytes) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, hipMemsetAsync(d_dst, value, nbytes, ctx->stream));
    return KMX_OK;
}

/* ------------------------------------------------------------ hot path ---- */

// The first and the last offset of a batch behind an offsets array, read back through the pinned words: one host round trip.
static int offsets_span(kmx_ctx* ctx, const kmx_reads* reads, uint64_t* first, uint64_t* last) {
    unsigned long long* const h = ctx->h_pinned + KMX_PIN_READ;
    KMX_HIP(ctx, hipMemcpyAsync(h, reads->d_offsets, 8, hipMemcpyDeviceToHost, ctx->stream));
    KMX_HIP(ctx, hipMemcpyAsync(h + 1, reads->d_offsets + reads->n_reads, 8, hipMemcpyDeviceToHost, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *first = h[0];
    *last = h[1];
    return KMX_OK;
}

// Long ragged reads (round 4): the reads of a batch behind an offsets array cut into overlapping segments of at most t_max windows
// on the device (kmx_segments.hip), in the context's work buffer.  Two host round trips: the first and the last offset (the
// arrays are sized from the number of bases), then the number of segments.  0: *starts / *ends / *n_seg are set (n_seg may be 0);
// -1: no scratch (the caller falls back); > 0: a status to return.
static int long_ragged_segments(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, uint32_t t_max, const uint64_t** starts, const uint64_t** ends,
                                uint64_t* n_seg, const uint64_t* win_offsets = nullptr, const uint64_t** wins = nullptr) {
    uint64_t o_first = 0, o_last = 0;
    if (int st = offsets_span(ctx, reads, &o_first, &o_last)) return st;
    if (!(o_last >= o_first && o_last - o_first < (1ull << 62))) return -1;
    const uint64_t cap = kmx::segments_capacity(reads->n_reads, o_last - o_first, t_max);
    void* scratch = capped_scratch(ctx, kmx::segments_scratch_bytes(reads->n_reads, cap, win_offsets != nullptr));
    if (!scratch) return -1;
    const uint64_t* d_total = nullptr;
    KMX_HIP(ctx, kmx::launch_segments_build(reads->d_offsets, reads->n_reads, k, t_max, cap, scratch, starts, ends, &d_total, too_long_of(ctx), ctx->stream,
                                            win_offsets, wins));
    // (the second and last round trip: how many segments there are -- the bound above is up to one per read too high)
    KMX_HIP(ctx, hipMemcpyAsync(ctx->h_pinned + KMX_PIN_READ, d_total, 8, hipMemcpyDeviceToHost, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_seg = ctx->h_pinned[KMX_PIN_READ];
    if (*n_seg > cap) return fail_hip(ctx, hipErrorUnknown, "segment count above its bound");
    if (wins != nullptr && *wins != nullptr && *n_seg != 0)     // the slot behind the last segment's windows: the batch's total
        KMX_HIP(ctx, hipMemcpyAsync(const_cast<uint64_t*>(*wins) + *n_seg, win_offsets + reads->n_reads, 8, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

// Uniform reads longer than a frame (round 4) as segments: as few per read as the 16-word frame allows (at most 257 - k windows),
// all of *T windows but the last.  Returns how many per read.
static uint32_t uniform_segments_per_read(uint32_t L, uint32_t k, uint32_t* T = nullptr) {
    const uint32_t W = L - k + 1u, J = (W + (257u - k) - 1u) / (257u - k);
    if (T) *T = (W + J - 1u) / J;
    return J;
}

// ... planned on the device in the context's work buffer (a start, an end and a first output slot per segment: 24 bytes against the
// ~1.8 KB a segment writes).  0: *starts / *ends / *wins / *n_seg are set; -1: no scratch (the caller falls back); > 0: a status.
static int uniform_long_segments(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, const uint64_t** starts, const uint64_t** ends,
                                 const uint64_t** wins, uint64_t* n_seg) {
    uint32_t T = 0;
    const uint32_t J = uniform_segments_per_read(reads->read_len, k, &T);
    void* scratch = capped_scratch(ctx, kmx::uniform_segments_scratch_bytes(reads->n_reads * J));
    if (!scratch) return -1;
    KMX_HIP(ctx, kmx::launch_uniform_segments_plan(reads->n_reads, reads->read_len, k, T, scratch, starts, ends, wins, n_seg, ctx->stream));
    return 0;
}

// The windows of reads above the frames (a length or a length bound of more than 256 bases; 16-byte aligned base) as segments of at
// most 257 - k windows: uniform reads planned, ragged ones cut (above).  0: the segments are set (n_seg may be 0); -1: not such
// reads, or no scratch (the caller falls back); > 0: a status to return.
static int long_segments(kmx_ctx* ctx, const kmx_reads* reads, const uint64_t* win_offsets, uint32_t k, const uint64_t** starts,
                         const uint64_t** ends, const uint64_t** wins, uint64_t* n_seg) {
    if (reads->read_len <= 256u || !aligned16(reads->d_bases)) return -1;
    if (reads->d_offsets) return win_offsets ? long_ragged_segments(ctx, reads, k, 257u - k, starts, ends, n_seg, win_offsets, wins) : -1;
    if (win_offsets || reads->n_reads >= (1ull << 40) || (uint64_t)reads->read_len * reads->n_reads >= (1ull << 62)) return -1;
    return uniform_long_segments(ctx, reads, k, starts, ends, wins, n_seg);
}

// Segments of long reads (long_segments) materialised by the tiled kernels as reads of their own (a bound of 256).
static int windows_segments(kmx_ctx* ctx, const kmx_reads* reads, const uint64_t* starts, const uint64_t* ends, const uint64_t* wins, uint64_t n_seg,
                            uint32_t k, uint64_t* d_fw, uint64_t* d_rc, uint64_t* d_canon, uint8_t* d_flags, bool* handled) {
    if (int st = queue_clear_marks(ctx, n_seg, k, k >= 2u /* (k = 1: no sweep behind the passes, so no marks) */)) return st;
    KMX_HIP(ctx, kmx::launch_windows_ragged(reads->d_bases, starts, wins, n_seg, 256u, k, d_fw, d_rc, d_canon, d_flags, queue_of(ctx), ctx->n_cu,
                                            ctx->stream, handled, ends));
    return KMX_OK;
}

static int windows2_segments(kmx_ctx* ctx, const kmx_reads* reads, const uint64_t* starts, const uint64_t* ends, const uint64_t* wins, uint64_t n_seg,
                             uint32_t k, uint64_t* d_fw2, uint64_t* d_rc2, uint64_t* d_canon2, uint8_t* d_flags, bool* handled) {
    kmx_reads segs = *reads;
    segs.d_offsets = starts;
    segs.n_reads = n_seg;
    segs.read_len = 256u;
    if (int st = queue_clear_marks(ctx, n_seg, k, true)) return st;
    KMX_HIP(ctx, kmx::launch_windows2_tiled_ragged(&segs, wins, k, d_fw2, d_rc2, d_canon2, d_flags, ctx->n_cu, ctx->stream, handled, too_long_of(ctx), ends,
                                                   queue_of(ctx)));
    return KMX_OK;
}

// The body of kmx_canonical_reduce.  `host_mode` (kmx_canonical_reduce_host): KMX_BS_PUBLISH | KMX_BS_NO_SWEEP | token << 8 for
// the launch that can end the call by itself -- uniform reads on the bit-sliced scan, no second kernel behind it; `*published`
// says whether that launch was made.
static int reduce_impl(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, uint32_t hasher, uint32_t hasher_k, uint32_t flags,
                       kmx_summary* d_out, uint32_t host_mode, bool* published) {
    if (published) *published = false;
    if (!ctx || !reads_ok(reads) || !d_out) return KMX_E_ARG;
    if (k < 1 || k > 31) return KMX_E_K_RANGE;  // MASK_TABLE[32]==0 (kmer.rs:617) breaks the reference's own rolling at 32
    if (hasher > KMX_HASH_IDENTITY) return KMX_E_ARG;
    if (hasher == KMX_HASH_LEX && (hasher_k < 1 || hasher_k > 32)) return KMX_E_K_RANGE;
    DeviceGuard g(ctx->device);
    if (reads->n_reads == 0) {
        KMX_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(kmx_summary), ctx->stream));
        return KMX_OK;
    }
    const bool want_sumfw = (flags & KMX_REDUCE_SUM_FW) != 0;
    // The tiled kernels fold LexHasher(k); the fold under LexHasher(hasher_k != k) or the identity hasher follows from it
    // (fix_hash_fold_kernel: every hasher offered is linear over GF(2)), so no hasher sends a call to the per-lane kernel.
    const bool want_fold = hasher != KMX_HASH_NONE;
    const bool fix_fold = want_fold && !(hasher == KMX_HASH_LEX && hasher_k == k);
    // Uniform reads on the bit-sliced scan (round 6): its last block STORES the summary and puts the queue block back as it found
    // it (kmx_layout.h), so neither `d_out` nor -- after a launch of that kind -- the queue block is cleared here: two fill kernels
    // and the gaps around them were 11 us of the 70 a batch of 1e5 reads took (profiles/r06_small_batches.txt).
    if (!reads->d_offsets) {
        bool handled = false;
        if (!ctx->queue_clean) KMX_HIP(ctx, queue_clear(ctx, KMX_Q_CLEAR_THROUGH_GATE));
        // (reads longer than a frame are scanned as segments: a mask word per 64 of THOSE)
        if (int st = prepare_dirty_flags(ctx, reads->n_reads * kmx::bitsliced_segments_per_read(reads->read_len, k), k)) return st;
        const bool alone = host_mode != 0u && !fix_fold && reads->read_len <= 256u;   // (segments: the sweep's geometry is the launcher's)
        const uint32_t mode = (want_sumfw ? 1u : 0u) | 2u /* KMX_BS_STORE */ | (alone ? host_mode : 0u);
        KMX_HIP(ctx, kmx::launch_scan_bitsliced(reads->d_bases, reads->n_reads, reads->read_len, k, want_fold, mode, d_out,
                                                queue_of(ctx), ctx->n_cu, ctx->stream, &handled));
        if (handled) {
            ctx->queue_clean = true;
            if (published) *published = alone;
            if (fix_fold) KMX_HIP(ctx, kmx::launch_fix_hash_fold(d_out, k, hasher, hasher_k, ctx->stream));
            return KMX_OK;
        }
    }
    KMX_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(kmx_summary), ctx->stream));
    {
        bool handled = false;
        KMX_HIP(ctx, queue_clear(ctx, KMX_Q_CLEAR_THROUGH_GATE));
        // Reads behind an offsets array with a length bound L that the uniform bit-sliced kernels take: most FASTQ is
        // untrimmed -- every read exactly L bases -- and the uniform kernel is ~1.4x the ragged one.  Decided on the device:
        // a small kernel checks offsets[i] == i*L, both scans are launched behind its verdict, the one it names runs.
        // (round 5: uniform at ANY length up to the bound -- the gate leaves the length it found for the uniform scan, which is laid out
        // for the bound; no bound = the 160-base frame the ragged launcher assumes as well)
        const uint32_t Lh = reads->read_len ? reads->read_len : 160u;
        // (only where BOTH bit-sliced launchers take the call: the ragged one needs a 16-byte aligned base -- with a misaligned
        // base the uniform scan used to be enqueued behind the gate and the generic kernel then counted the batch a second time)
        if (reads->d_offsets && !want_sumfw && k >= 9 && k <= 31 && Lh >= k && Lh <= 256 && reads->read_len <= 256 && aligned16(reads->d_bases)) {
            KMX_HIP(ctx, gate_arm(ctx));
            KMX_HIP(ctx, kmx::launch_offsets_uniform_gate(reads->d_offsets, reads->n_reads, Lh, k, gate_of(ctx), ctx->n_cu, ctx->stream));
            if (int st = prepare_dirty_flags(ctx, reads->n_reads, k)) return st;
            bool h_u = false, h_r = false;
            KMX_HIP(ctx, kmx::launch_scan_bitsliced(reads->d_bases, reads->n_reads, Lh, k, want_fold, 0u, d_out, queue_of(ctx),
                                                    ctx->n_cu, ctx->stream, &h_u));
            // (the uniform scan took tickets from the queue heads only if it ran; if it did not they are still zero)
            if (h_u)
                KMX_HIP(ctx, kmx::launch_scan_bitsliced_ragged(reads->d_bases, reads->d_offsets, reads->n_reads, Lh, k, want_fold, d_out,
                                                               queue_of(ctx), ctx->n_cu, ctx->stream, &h_r));
            KMX_HIP(ctx, gate_disarm(ctx));   // never left armed
            if (h_u && h_r) {
                if (fix_fold) KMX_HIP(ctx, kmx::launch_fix_hash_fold(d_out, k, hasher, hasher_k, ctx->stream));
                return KMX_OK;
            }
            if (h_u) {
                // The ragged launcher takes every aligned (k, L) the uniform one takes.  Should that ever stop being true, the uniform
                // scan is already enqueued behind the gate and nothing may run after it: fail loudly, never count twice.
                KMX_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(kmx_summary), ctx->stream));
                std::snprintf(ctx->last_error, sizeof ctx->last_error, "kmx: internal -- the ragged scan refused k=%u, L<=%u that the uniform scan accepted", k, Lh);
                return KMX_E_HIP;
            }
        }
        if (!handled && reads->d_offsets && reads->read_len > 256 && k >= 9 && k <= 31 && aligned16(reads->d_bases)) {
            // Long ragged reads (a length bound above the frames: PacBio / ONT reads, contigs), round 4: cut into overlapping
            // segments on the device (kmx_segments.hip) and scanned by the ragged bit-sliced kernel as reads of their own.  Two
            // host round trips: the first and the last offset (the segment arrays are sized from the number of bases), then the
            // number of segments.  No scratch -> the lane-per-read kernel below.
            const uint32_t t_max = 161u - k < 128u ? 161u - k : 128u;      // windows per segment: at most 4 per lane (the three-wave variant)
            const uint64_t *starts = nullptr, *ends = nullptr;
            uint64_t n_seg = 0;
            const int st = long_ragged_segments(ctx, reads, k, t_max, &starts, &ends, &n_seg);
            if (st > 0) return st;
            if (st == 0) {
                if (n_seg == 0) return KMX_OK;   // no read holds a window
                if (int st2 = prepare_dirty_flags(ctx, n_seg, k)) return st2;
                KMX_HIP(ctx, kmx::launch_scan_bitsliced_ragged(reads->d_bases, starts, n_seg, t_max + k - 1u, k, want_fold, d_out,
                                                               queue_of(ctx), ctx->n_cu, ctx->stream, &handled, want_sumfw, ends));
            }
        }
        if (!handled && reads->d_offsets) {   // ragged reads on the bit-sliced kernel (read_len = optional length bound)
            if (int st = prepare_dirty_flags(ctx, reads->n_reads, k)) return st;
            KMX_HIP(ctx, kmx::launch_scan_bitsliced_ragged(reads->d_bases, reads->d_offsets, reads->n_reads, reads->read_len, k,
                                                           want_fold, d_out, queue_of(ctx), ctx->n_cu, ctx->stream, &handled, want_sumfw));
        }
        // word-domain kernel: uniform reads of any (k, L) in its domain, and ragged reads (read_len = optional length bound)
        if (!handled)
            KMX_HIP(ctx, kmx::launch_scan_uniform(reads->d_bases, reads->n_reads, reads->read_len, k, want_fold, want_sumfw,
                                                  d_out, queue_of(ctx), ctx->n_cu, ctx->stream, &handled, reads->d_offsets));
        if (handled) {
            if (fix_fold) KMX_HIP(ctx, kmx::launch_fix_hash_fold(d_out, k, hasher, hasher_k, ctx->stream));
            return KMX_OK;
        }
    }
    KMX_HIP(ctx, kmx::launch_reduce_generic(reads, k, hasher, hasher_k, want_sumfw ? 1u : 0u, d_out, ctx->n_cu, ctx->stream, too_long_of(ctx)));
    return KMX_OK;
}

int kmx_canonical_reduce(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, uint32_t hasher, uint32_t hasher_k,
                         uint32_t flags, kmx_summary* d_out) {
    return reduce_impl(ctx, reads, k, hasher, hasher_k, flags, d_out, 0u, nullptr);
}

// The summary straight into host memory, the call returning when it is there (round 6; kmx.h).  Uniform reads of up to 256
// bases on the bit-sliced scan: ONE kernel launch -- its last block leaves {token, marked reads, summary} in the context's
// pinned words, which this thread watches -- and, only if the scan marked reads with an invalid byte, the sweep and a copy
// back.  Everything else: kmx_canonical_reduce into a summary of the context's own, a copy, a wait.
int kmx_canonical_reduce_host(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, uint32_t hasher, uint32_t hasher_k,
                              uint32_t flags, kmx_summary* h_out) {
    if (!ctx || !h_out) return KMX_E_ARG;
    kmx_summary* const d_res = reinterpret_cast<kmx_summary*>(queue_of(ctx) + KMX_Q_RESULT);   // (eight free words of the queue block)
    uint32_t token = (ctx->pub_token + 1u) & 0xFFFFFFu;
    if (token == 0u) token = 1u;                       // (the pinned word starts at 0)
    bool published = false;
    const int st = reduce_impl(ctx, reads, k, hasher, hasher_k, flags, d_res, 4u /* KMX_BS_PUBLISH */ | 8u /* KMX_BS_NO_SWEEP */ | (token << 8), &published);
    if (st != KMX_OK) return st;
    DeviceGuard g(ctx->device);
    if (published) {
        ctx->pub_token = token;
        volatile unsigned long long* const hp = ctx->h_pub;
        unsigned spins = 0, done_seen = 0;
        while (hp[0] != (unsigned long long)token) {
            if ((++spins & 0x3FFFu) == 0u) {           // (a launch that died never writes the token)
                const hipError_t q = hipStreamQuery(ctx->stream);
                if (q != hipErrorNotReady) {
                    if (q != hipSuccess) return fail_hip(ctx, q, "kmx_canonical_reduce_host");
                    if (++done_seen > 64u) {
                        std::snprintf(ctx->last_error, sizeof ctx->last_error, "kmx: internal -- the scan ended without publishing its summary");
                        return KMX_E_HIP;
                    }
                }
            }
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        if (hp[1] == 0ull) {                           // no read was marked: what the scan left is the answer
            h_out->n_valid = hp[2]; h_out->sum_canon = hp[3]; h_out->xor_hash = hp[4]; h_out->sum_fw = hp[5];
            return KMX_OK;
        }
        KMX_HIP(ctx, kmx::launch_sweep_uniform(reads->d_bases, reads->n_reads, reads->read_len, k, hasher != KMX_HASH_NONE,
                                               (flags & KMX_REDUCE_SUM_FW) != 0, d_res, queue_of(ctx), ctx->n_cu, ctx->stream));
    }
    KMX_HIP(ctx, hipMemcpyAsync(ctx->h_pinned + KMX_PIN_SUMMARY, d_res, sizeof(kmx_summary), hipMemcpyDeviceToHost, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const unsigned long long* const hs = ctx->h_pinned + KMX_PIN_SUMMARY;
    h_out->n_valid = hs[0]; h_out->sum_canon = hs[1]; h_out->xor_hash = hs[2]; h_out->sum_fw = hs[3];
    return KMX_OK;
}

int kmx_canonical_windows(kmx_ctx* ctx, const kmx_reads* reads, const uint64_t* d_win_offsets, uint32_t k,
                          uint64_t* d_fw, uint64_t* d_rc, uint64_t* d_canon, uint8_t* d_flags) {
    if (!ctx || !reads_ok(reads)) return KMX_E_ARG;
    if (k < 1 || k > 31) return KMX_E_K_RANGE;
    if (reads->d_offsets && !d_win_offsets) return KMX_E_ARG;
    if (reads->n_reads == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    if (!reads->d_offsets && !d_win_offsets) {   // uniform layout: fast word-domain kernel
        bool handled = false;
        // (the window sinks mark the reads of a tile with an invalid byte and the sweep behind the passes zeroes their spoiled slots: round 6)
        if (int st = queue_clear_marks(ctx, reads->n_reads, k, k >= 2u /* (k = 1: no sweep behind the passes, so no marks) */)) return st;
        KMX_HIP(ctx, kmx::launch_windows_uniform(reads->d_bases, reads->n_reads, reads->read_len, k, d_fw, d_rc, d_canon,
                                                 d_flags, queue_of(ctx), ctx->n_cu, ctx->stream, &handled));
        if (handled) return KMX_OK;
    }
    // Reads longer than a frame (round 4): segments of at most 257 - k windows, each a read of its own for the ragged materialise
    // kernels (kmx_segments.hip).  No scratch -> the kernels below.  (k = 1 is outside the tiled kernel's domain: nothing is planned)
    if (k >= 2) {
        const uint64_t *starts = nullptr, *ends = nullptr, *wins = nullptr;
        uint64_t n_seg = 0;
        const int st = long_segments(ctx, reads, d_win_offsets, k, &starts, &ends, &wins, &n_seg);
        if (st > 0) return st;
        if (st == 0) {
            if (n_seg == 0) return KMX_OK;      // no read holds a window
            bool handled = false;
            if (int st2 = windows_segments(ctx, reads, starts, ends, wins, n_seg, k, d_fw, d_rc, d_canon, d_flags, &handled)) return st2;
            if (handled) return KMX_OK;
        }
    }
    if (reads->d_offsets && d_win_offsets) {     // ragged reads: the tiled word-domain kernel (read_len = optional length bound)
        bool handled = false;
        if (int st = queue_clear_marks(ctx, reads->n_reads, k, k >= 2u /* (k = 1: no sweep behind the passes, so no marks) */)) return st;
        KMX_HIP(ctx, kmx::launch_windows_ragged(reads->d_bases, reads->d_offsets, d_win_offsets, reads->n_reads, reads->read_len, k,
                                                d_fw, d_rc, d_canon, d_flags, queue_of(ctx), ctx->n_cu, ctx->stream, &handled));
        if (handled) return KMX_OK;
    }
    KMX_HIP(ctx, kmx::launch_windows_generic(reads, d_win_offsets, k, d_fw, d_rc, d_canon, d_flags, ctx->n_cu, ctx->stream, too_long_of(ctx)));
    return KMX_OK;
}

// Exact counting (kmx_count_canonical): the windows' canonical words and flags through kmx_canonical_windows -- every route it
// takes, the segment plan of long reads included -- into the context's work buffer, then the partition / leaf sort of
// kmx_count.hip.  The work buffer is laid out up front, before any kernel runs: [segment plan of long reads][ragged: window
// offsets][canon 8 B/window][flags 1 B/window][count area: keys 8 B/window, keep 1 B/window, level arrays].  The plan sits at the
// buffer's start, where the routes of kmx_canonical_windows ask for it (capped_scratch), so it never overlaps the arrays behind it.
static size_t count_plan_bytes(const kmx_reads* reads, uint32_t k, uint64_t n_bases) {
    if (k < 2u || reads->read_len <= 256u || !aligned16(reads->d_bases)) return 0;
    if (!reads->d_offsets) return kmx::uniform_segments_scratch_bytes(reads->n_reads * uniform_segments_per_read(reads->read_len, k));
    return kmx::segments_scratch_bytes(reads->n_reads, kmx::segments_capacity(reads->n_reads, n_bases, 257u - k), true);
}

// The windows kmx_count_canonical(2) and the reads forms of the queries size their arrays for: exact for uniform reads (*n_bound = 0: no
// window), the number of bases -- a bound, also in *n_bases -- for ragged ones.
static int query_window_bound(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, uint64_t* n_bound, uint64_t* n_bases, uint64_t* first = nullptr) {
    *n_bound = *n_bases = 0;
    if (reads->d_offsets) {
        uint64_t o_first = 0, o_last = 0;
        if (int st = offsets_span(ctx, reads, &o_first, &o_last)) return st;
        if (first) *first = o_first;   // (ragged reads: where the batch's bases start)
        if (o_last < o_first) return KMX_E_ARG;
        if (o_last - o_first >= (1ull << 40)) return KMX_E_NOMEM;
        *n_bases = *n_bound = o_last - o_first;
        return KMX_OK;
    }
    if (reads->read_len < k) return KMX_OK;
    const uint64_t w = reads->read_len - k + 1u;
    if (reads->n_reads > (1ull << 40) / w) return KMX_E_NOMEM;
    *n_bound = reads->n_reads * w;
    return KMX_OK;
}

// The work buffer of a count-family call, `bytes` of working set: refused above the cap (kmx_ctx_set_work_buffer_limit, or what
// the device has to spare), grown if need be, and the call's to overwrite.  `hold`, where asked for: for work_kept behind a nested use.
static int work_area(kmx_ctx* ctx, const char* who, size_t bytes, void** area, WorkHold* hold = nullptr) {
    const size_t budget = work_budget(ctx);
    if (bytes > budget) {
        std::snprintf(ctx->last_error, sizeof ctx->last_error, "%s: %zu bytes of working set above the work buffer's cap of %zu", who, bytes,
                      budget);
        return KMX_E_NOMEM;
    }
    const WorkHold h = work_acquire(ctx, bytes);
    if (!(*area = h.base)) {
        std::snprintf(ctx->last_error, sizeof ctx->last_error, "%s: no memory for %zu bytes of working set", who, bytes);
        return KMX_E_NOMEM;
    }
    if (hold) *hold = h;
    return KMX_OK;
}

// A result of n_out entries (`what` they are, for the message) for arrays of max_out: KMX_E_NOMEM when it is larger than the room.
static int room_for(kmx_ctx* ctx, const char* who, uint64_t n_out, const char* what, uint64_t max_out) {
    if (n_out <= max_out) return KMX_OK;
    std::snprintf(ctx->last_error, sizeof ctx->last_error, "%s: %llu %s, room for %llu", who, (unsigned long long)n_out, what,
                  (unsigned long long)max_out);
    return KMX_E_NOMEM;
}

// What the one-word and the two-word counter differ in: the words of a key and the windows call that fills canon / flags.
struct CountKind {
    const char* who;
    uint32_t words;
    int (*windows)(kmx_ctx*, const kmx_reads*, const uint64_t*, uint32_t, uint64_t*, uint64_t*, uint64_t*, uint8_t*);
};

// A counting sketch as the calls take it (kmx.h): 64 << log2_blocks bytes, 64-byte aligned.
struct Sketch {
    const uint8_t* cells;
    uint32_t log2_blocks;
    uint64_t seed;
};
static bool sketch_ok(const void* d_sketch, uint32_t log2_blocks, bool needed) {
    return log2_blocks <= 32u && (reinterpret_cast<uintptr_t>(d_sketch) & 63u) == 0 && (d_sketch != nullptr || !needed);
}
// The filter step of kmx_count_canonical_min(2): the windows whose estimate in `sketch` is below min_est lose KMX_WIN_VALID.
struct CountFilter {
    Sketch sketch;
    uint32_t min_est;
};

// The front half kmx_count_canonical(2) and kmx_sketch_add(2) share: sizing, cap, work buffer, window offsets, windows.  The work
// buffer, laid out up front: [segment plan of long reads][ragged: window offsets][canon 8 (16) B/window][flags 1 B/window][the caller's
// area: area_bytes(words, windows), none without it].
struct WindowsFront {
    char* base = nullptr;        // the work buffer
    uint64_t n_win = 0;          // the windows there are; 0 = none, and no kernel wrote canon / flags
    uint64_t* canon = nullptr;   // one key per window
    uint8_t* flags = nullptr;    // one byte per window
    size_t area_at = 0;          // where the caller's area starts
};
static int windows_front(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, const CountKind& kind, size_t (*area_bytes)(uint32_t, uint64_t),
                         WindowsFront* f) {
    uint64_t n_bound = 0, n_bases = 0;
    if (int st = query_window_bound(ctx, reads, k, &n_bound, &n_bases)) return st;
    if (n_bound == 0) return KMX_OK;   // no window
    const size_t plan = align256(count_plan_bytes(reads, k, n_bases));
    const size_t wo_bytes = reads->d_offsets ? align256(kmx::win_offsets_bytes(reads->n_reads)) : 0;
    const size_t canon_at = plan + wo_bytes, flags_at = canon_at + align256(8u * kind.words * n_bound), area_at = flags_at + align256(n_bound);
    const size_t bytes = area_at + (area_bytes ? area_bytes(kind.words, n_bound) : 0u);
    void* buf = nullptr;
    WorkHold hold;
    if (int st = work_area(ctx, kind.who, bytes, &buf, &hold)) return st;
    char* const base = hold.base;
    uint64_t n_win = n_bound;
    uint64_t* wo = nullptr;
    if (reads->d_offsets) {
        KMX_HIP(ctx, kmx::launch_count_win_offsets(reads->d_offsets, reads->n_reads, k, base + plan, &wo, ctx->h_pinned, &n_win, ctx->stream));
        if (n_win > n_bound) {
            char msg[96];
            std::snprintf(msg, sizeof msg, "%s: window count above its bound", kind.who);
            return fail_hip(ctx, hipErrorUnknown, msg);
        }
        if (n_win == 0) return KMX_OK;
    }
    uint64_t* canon = reinterpret_cast<uint64_t*>(base + canon_at);
    uint8_t* flags = reinterpret_cast<uint8_t*>(base + flags_at);
    if (int st = kind.windows(ctx, reads, wo, k, nullptr, nullptr, canon, flags)) return st;
    if (int st = work_kept(ctx, kind.who, hold)) return st;
    *f = WindowsFront{base, n_win, canon, flags, area_at};
    return KMX_OK;
}

// The body of kmx_count_canonical(2) and kmx_count_canonical_min(2) behind their argument checks: the windows (windows_front), the
// filter step where there is one, sort, emit.
static int count_impl(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, const CountKind& kind, uint64_t* d_kmers, uint64_t* d_counts,
                      uint64_t max_distinct, uint64_t* h_n_distinct, const CountFilter* filter = nullptr) {
    *h_n_distinct = 0;
    if (reads->n_reads == 0) return KMX_OK;
    if (filter && filter->min_est > 255u) return KMX_OK;   // (no estimate is above 255: the empty table)
    DeviceGuard g(ctx->device);
    WindowsFront f;
    if (int st = windows_front(ctx, reads, k, kind, kmx::count_area_bytes, &f)) return st;
    if (f.n_win == 0) return KMX_OK;
    if (filter && filter->min_est > 0u)
        KMX_HIP(ctx, kmx::launch_sketch_filter(kind.words, f.canon, f.flags, f.n_win, filter->sketch.cells, filter->sketch.log2_blocks,
                                               filter->sketch.seed, filter->min_est, ctx->n_cu, ctx->stream));
    uint64_t n_valid = 0, n_distinct = 0;
    bool bad = false;
    // (the count area is laid out for the n_win windows there are, inside the bytes reserved for the bound on them)
    void* area = f.base + f.area_at;
    KMX_HIP(ctx, kmx::launch_count_sort(kind.words, f.canon, f.flags, f.n_win, k, area, ctx->h_pinned, &n_valid, &n_distinct, &bad, ctx->stream));
    if (bad) {
        char msg[96];
        std::snprintf(msg, sizeof msg, "%s: partition arrays above their bounds", kind.who);
        return fail_hip(ctx, hipErrorUnknown, msg);
    }
    *h_n_distinct = n_distinct;
    if (!d_kmers || n_distinct == 0) return KMX_OK;
    if (int st = room_for(ctx, kind.who, n_distinct, "distinct k-mers", max_distinct)) return st;
    KMX_HIP(ctx, kmx::launch_count_emit(kind.words, f.canon, f.n_win, n_valid, area, d_kmers, d_counts, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMX_OK;
}

int kmx_count_canonical(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, uint64_t* d_kmers, uint64_t* d_counts, uint64_t max_distinct,
                        uint64_t* h_n_distinct) {
    if (!ctx || !reads_ok(reads) || !h_n_distinct || ((d_kmers == nullptr) != (d_counts == nullptr))) return KMX_E_ARG;
    if (k < 1 || k > 31) return KMX_E_K_RANGE;
    static const CountKind kind{"kmx_count_canonical", 1u, kmx_canonical_windows};
    return count_impl(ctx, reads, k, kind, d_kmers, d_counts, max_distinct, h_n_distinct);
}

// (two-word keys are read and written as 16-byte elements: the caller's key arrays must be 16-byte aligned)
int kmx_count_canonical2(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, uint64_t* d_kmers2, uint64_t* d_counts, uint64_t max_distinct,
                         uint64_t* h_n_distinct) {
    if (!ctx || !reads_ok(reads) || !h_n_distinct || ((d_kmers2 == nullptr) != (d_counts == nullptr)) || !aligned16(d_kmers2)) return KMX_E_ARG;
    if (k < 33 || k > 64) return KMX_E_K_RANGE;
    static const CountKind kind{"kmx_count_canonical2", 2u, kmx_canonical_windows2};
    return count_impl(ctx, reads, k, kind, d_kmers2, d_counts, max_distinct, h_n_distinct);
}

int kmx_count_canonical_min(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, const uint8_t* d_sketch, uint32_t log2_blocks, uint64_t seed,
                            uint32_t min_est, uint64_t* d_kmers, uint64_t* d_counts, uint64_t max_distinct, uint64_t* h_n_distinct) {
    if (!ctx || !reads_ok(reads) || !h_n_distinct || ((d_kmers == nullptr) != (d_counts == nullptr))) return KMX_E_ARG;
    if (!sketch_ok(d_sketch, log2_blocks, reads->n_reads != 0)) return KMX_E_ARG;
    if (k < 1 || k > 31) return KMX_E_K_RANGE;
    static const CountKind kind{"kmx_count_canonical_min", 1u, kmx_canonical_windows};
    const CountFilter filter{{d_sketch, log2_blocks, seed}, min_est};
    return count_impl(ctx, reads, k, kind, d_kmers, d_counts, max_distinct, h_n_distinct, &filter);
}

int kmx_count_canonical_min2(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, const uint8_t* d_sketch, uint32_t log2_blocks, uint64_t seed,
                             uint32_t min_est, uint64_t* d_kmers2, uint64_t* d_counts, uint64_t max_distinct, uint64_t* h_n_distinct) {
    if (!ctx || !reads_ok(reads) || !h_n_distinct || ((d_kmers2 == nullptr) != (d_counts == nullptr)) || !aligned16(d_kmers2)) return KMX_E_ARG;
    if (!sketch_ok(d_sketch, log2_blocks, reads->n_reads != 0)) return KMX_E_ARG;
    if (k < 33 || k > 64) return KMX_E_K_RANGE;
    static const CountKind kind{"kmx_count_canonical_min2", 2u, kmx_canonical_windows2};
    const CountFilter filter{{d_sketch, log2_blocks, seed}, min_est};
    return count_impl(ctx, reads, k, kind, d_kmers2, d_counts, max_distinct, h_n_distinct, &filter);
}

static int merge_impl(kmx_ctx* ctx, const char* who, uint32_t words, const uint64_t* d_kmers_a, const uint64_t* d_counts_a, uint64_t n_a,
                      const uint64_t* d_kmers_b, const uint64_t* d_counts_b, uint64_t n_b, uint64_t* d_kmers_out, uint64_t* d_counts_out,
                      uint64_t max_out, uint64_t* h_n_out) {
    if (!ctx || !h_n_out || ((d_kmers_out == nullptr) != (d_counts_out == nullptr))) return KMX_E_ARG;
    if ((n_a && (!d_kmers_a || !d_counts_a)) || (n_b && (!d_kmers_b || !d_counts_b))) return KMX_E_ARG;
    if (n_a > (1ull << 40) || n_b > (1ull << 40)) return KMX_E_ARG;
    *h_n_out = 0;
    const uint64_t n = n_a + n_b;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    void* area = nullptr;
    if (int st = work_area(ctx, who, kmx::count_merge_bytes(words, n), &area)) return st;
    uint64_t n_out = 0;
    KMX_HIP(ctx, kmx::launch_count_merge(words, d_kmers_a, d_counts_a, n_a, d_kmers_b, d_counts_b, n_b, area, ctx->h_pinned, &n_out, ctx->stream));
    *h_n_out = n_out;
    if (!d_kmers_out) return KMX_OK;
    if (int st = room_for(ctx, who, n_out, "distinct k-mers", max_out)) return st;
    KMX_HIP(ctx, kmx::launch_count_merge_emit(words, n, area, d_kmers_out, d_counts_out, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMX_OK;
}

int kmx_count_merge(kmx_ctx* ctx, const uint64_t* d_kmers_a, const uint64_t* d_counts_a, uint64_t n_a, const uint64_t* d_kmers_b,
                    const uint64_t* d_counts_b, uint64_t n_b, uint64_t* d_kmers_out, uint64_t* d_counts_out, uint64_t max_out, uint64_t* h_n_out) {
    return merge_impl(ctx, "kmx_count_merge", 1u, d_kmers_a, d_counts_a, n_a, d_kmers_b, d_counts_b, n_b, d_kmers_out, d_counts_out, max_out, h_n_out);
}

int kmx_count_merge2(kmx_ctx* ctx, const uint64_t* d_kmers2_a, const uint64_t* d_counts_a, uint64_t n_a, const uint64_t* d_kmers2_b,
                     const uint64_t* d_counts_b, uint64_t n_b, uint64_t* d_kmers2_out, uint64_t* d_counts_out, uint64_t max_out, uint64_t* h_n_out) {
    if (!aligned16(d_kmers2_a) || !aligned16(d_kmers2_b) || !aligned16(d_kmers2_out)) return KMX_E_ARG;
    return merge_impl(ctx, "kmx_count_merge2", 2u, d_kmers2_a, d_counts_a, n_a, d_kmers2_b, d_counts_b, n_b, d_kmers2_out, d_counts_out, max_out, h_n_out);
}

// ---- queries on a count table (kmx_count_query.hip) ----
// What the one-word and the two-word queries differ in: the words of a key, the domain of k, the windows call of the reads form.
struct QueryKind {
    const char* who;
    uint32_t words, k_min, k_max;
    int (*windows)(kmx_ctx*, const kmx_reads*, const uint64_t*, uint32_t, uint64_t*, uint64_t*, uint64_t*, uint8_t*);
};
static const QueryKind kQuery1{"kmx_count_lookup", 1u, 1u, 31u, kmx_canonical_windows};
static const QueryKind kQuery2{"kmx_count_lookup2", 2u, 33u, 64u, kmx_canonical_windows2};

// Where the directory of a search for n_query keys among n goes (*p: its prefix bits): into the work buffer when the byte counts say
// it pays (count_lookup_wants_dir) and it fits under the cap, nullptr otherwise -- the plain search, which needs no work buffer.
// `hold`: the caller's, whose first `reserved` bytes stay its own (the reads forms keep their flags / canonical words there) -- the
// directory goes behind them if the buffer as a whole has the room (query_scratch asked for it with the rest, or could not); none: the
// buffer is taken here.
static void* lookup_dir(kmx_ctx* ctx, const WorkHold* hold, uint32_t words, uint64_t n, uint32_t k, uint64_t n_query, uint32_t* p) {
    const size_t dir_bytes = kmx::count_lookup_dir_bytes(n, k, p), reserved = hold ? hold->reserved : 0;
    if (dir_bytes == 0 || !kmx::count_lookup_wants_dir(n, n_query, words) || reserved + dir_bytes > work_budget(ctx)) return nullptr;
    if (!hold) return work_acquire(ctx, dir_bytes).base;
    return reserved + dir_bytes <= hold->size ? hold->base + reserved : nullptr;
}

// The lookup behind its argument checks, with its directory (lookup_dir) or without: never KMX_E_NOMEM from here.  *dir_out / *p_out,
// where asked for: the directory that was built and its prefix bits, nullptr = the plain search ran.
static int lookup_run(kmx_ctx* ctx, const QueryKind& kind, const uint64_t* d_kmers, const uint64_t* d_counts, uint64_t n, uint32_t k,
                      const uint64_t* d_query, const uint8_t* d_query_flags, uint64_t n_query, uint64_t* d_out, const WorkHold* hold,
                      const void** dir_out = nullptr, uint32_t* p_out = nullptr) {
    if (dir_out) *dir_out = nullptr;
    if (p_out) *p_out = 0;
    if (n_query == 0) return KMX_OK;
    if (n == 0) {
        KMX_HIP(ctx, hipMemsetAsync(d_out, 0, 8u * n_query, ctx->stream));
        return KMX_OK;
    }
    uint32_t p = 0;
    void* const dir = lookup_dir(ctx, hold, kind.words, n, k, n_query, &p);
    KMX_HIP(ctx, kmx::launch_count_lookup(kind.words, d_kmers, d_counts, n, k, d_query, d_query_flags, n_query, d_out, dir, p, ctx->stream));
    if (dir_out) *dir_out = dir;   // (it stays what it is until the work buffer is used again)
    if (p_out) *p_out = p;
    return KMX_OK;
}

static int lookup_impl(kmx_ctx* ctx, const QueryKind& kind, const uint64_t* d_kmers, const uint64_t* d_counts, uint64_t n, uint32_t k,
                       const uint64_t* d_query, const uint8_t* d_query_flags, uint64_t n_query, uint64_t* d_out) {
    if (!ctx || (n && !d_kmers) || (n_query && (!d_query || !d_out)) || n > (1ull << 40) || n_query > (1ull << 40)) return KMX_E_ARG;
    if (kind.words == 2u && (!aligned16(d_kmers) || !aligned16(d_query))) return KMX_E_ARG;
    if (k < kind.k_min || k > kind.k_max) return KMX_E_K_RANGE;
    DeviceGuard g(ctx->device);
    return lookup_run(ctx, kind, d_kmers, d_counts, n, k, d_query, d_query_flags, n_query, d_out, nullptr);
}

int kmx_count_lookup(kmx_ctx* ctx, const uint64_t* d_kmers, const uint64_t* d_counts, uint64_t n, uint32_t k, const uint64_t* d_query,
                     const uint8_t* d_query_flags, uint64_t n_query, uint64_t* d_out) {
    return lookup_impl(ctx, kQuery1, d_kmers, d_counts, n, k, d_query, d_query_flags, n_query, d_out);
}

int kmx_count_lookup2(kmx_ctx* ctx, const uint64_t* d_kmers2, const uint64_t* d_counts, uint64_t n, uint32_t k, const uint64_t* d_query2,
                      const uint8_t* d_query_flags, uint64_t n_query, uint64_t* d_out) {
    return lookup_impl(ctx, kQuery2, d_kmers2, d_counts, n, k, d_query2, d_query_flags, n_query, d_out);
}

// ---- the reads forms of the queries: kmx_count_lookup_reads(2) and kmx_count_read_stats(2) ----
// Their work buffer: `reserved` bytes for the caller's arrays, refused above the cap, and room for the lookup's directory behind them
// when it pays for n_query windows and fits (asked for with the rest, so the buffer does not move between the windows call and the
// lookup; left out, never refused).
static int query_scratch(kmx_ctx* ctx, const char* who, uint32_t words, size_t reserved, uint64_t n, uint32_t k, uint64_t n_query, WorkHold* hold) {
    const size_t budget = work_budget(ctx);
    if (reserved > budget) {
        std::snprintf(ctx->last_error, sizeof ctx->last_error, "%s: %zu bytes of working set above the work buffer's cap of %zu", who, reserved, budget);
        return KMX_E_NOMEM;
    }
    uint32_t p = 0;
    const size_t dir_bytes = n ? kmx::count_lookup_dir_bytes(n, k, &p) : 0;
    const bool with_dir = dir_bytes != 0 && kmx::count_lookup_wants_dir(n, n_query, words) && reserved + dir_bytes <= budget;
    *hold = work_acquire(ctx, reserved + (with_dir ? dir_bytes : 0));
    if (!hold->base && with_dir) *hold = work_acquire(ctx, reserved);
    if (!hold->base) {
        std::snprintf(ctx->last_error, sizeof ctx->last_error, "%s: no memory for %zu bytes of working set", who, reserved);
        return KMX_E_NOMEM;
    }
    hold->reserved = reserved;
    return KMX_OK;
}

// The windows the arrays of a reads form are sized for (query_window_bound) and the windows there are in the caller's slot layout
// (*n_win; 0 = none): ragged reads by the last of their d_win_offsets, which comes back to the host.
static int caller_windows(kmx_ctx* ctx, const kmx_reads* reads, const uint64_t* d_win_offsets, uint32_t k, uint64_t* n_bound, uint64_t* n_bases,
                          uint64_t* n_win) {
    *n_win = 0;
    if (int st = query_window_bound(ctx, reads, k, n_bound, n_bases)) return st;
    if (reads->d_offsets) {
        KMX_HIP(ctx, hipMemcpyAsync(ctx->h_pinned + KMX_PIN_READ, d_win_offsets + reads->n_reads, 8, hipMemcpyDeviceToHost, ctx->stream));
        KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *n_win = ctx->h_pinned[KMX_PIN_READ];
        if (*n_win > *n_bound) return KMX_E_ARG;   // (more windows than bases: not this batch's window offsets)
        return KMX_OK;
    }
    if (*n_bound == 0) return KMX_OK;   // no window
    if (d_win_offsets) {   // (uniform reads in slots of the caller's: kmx_canonical_windows serves them, so they are served)
        KMX_HIP(ctx, hipMemcpyAsync(ctx->h_pinned + KMX_PIN_READ, d_win_offsets + reads->n_reads, 8, hipMemcpyDeviceToHost, ctx->stream));
        KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->h_pinned[KMX_PIN_READ] != *n_bound) return KMX_E_ARG;
    }
    *n_win = *n_bound;
    return KMX_OK;
}

// kmx_count_lookup_reads(2) = kmx_canonical_windows(2) followed by the lookup kernel.  The work buffer is laid out up front, as
// count_impl lays its arrays out: [segment plan of long reads][two-word keys: canon 16 B/window][flags 1 B/window][directory, when
// it pays and fits].  One-word keys: the windows call writes its canonical words into d_out and they are looked up in place.
static int lookup_reads_impl(kmx_ctx* ctx, const QueryKind& kind, const kmx_reads* reads, const uint64_t* d_win_offsets, uint32_t k,
                             const uint64_t* d_kmers, const uint64_t* d_counts, uint64_t n, uint64_t* d_out) {
    if (!ctx || !reads_ok(reads) || (n && !d_kmers) || n > (1ull << 40)) return KMX_E_ARG;
    if (kind.words == 2u && !aligned16(d_kmers)) return KMX_E_ARG;
    if (k < kind.k_min || k > kind.k_max) return KMX_E_K_RANGE;
    if (reads->d_offsets && !d_win_offsets) return KMX_E_ARG;
    if (reads->n_reads == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    uint64_t n_bound = 0, n_bases = 0, n_win = 0;
    if (int st = caller_windows(ctx, reads, d_win_offsets, k, &n_bound, &n_bases, &n_win)) return st;
    if (n_win == 0) return KMX_OK;
    if (!d_out) return KMX_E_ARG;
    const size_t plan = align256(count_plan_bytes(reads, k, n_bases));
    const size_t canon_at = plan, flags_at = canon_at + (kind.words == 2u ? align256(16u * n_bound) : 0u), reserved = flags_at + align256(n_bound);
    char who[48];
    std::snprintf(who, sizeof who, "%s_reads", kind.who);
    WorkHold hold;
    if (int st = query_scratch(ctx, who, kind.words, reserved, n, k, n_win, &hold)) return st;
    char* const base = hold.base;
    uint64_t* canon = kind.words == 2u ? reinterpret_cast<uint64_t*>(base + canon_at) : d_out;
    uint8_t* flags = reinterpret_cast<uint8_t*>(base + flags_at);
    if (int st = kind.windows(ctx, reads, d_win_offsets, k, nullptr, nullptr, canon, flags)) return st;
    if (int st = work_kept(ctx, who, hold)) return st;
    return lookup_run(ctx, kind, d_kmers, d_counts, n, k, canon, flags, n_win, d_out, &hold);
}

int kmx_count_lookup_reads(kmx_ctx* ctx, const kmx_reads* reads, const uint64_t* d_win_offsets, uint32_t k, const uint64_t* d_kmers,
                           const uint64_t* d_counts, uint64_t n, uint64_t* d_out) {
    return lookup_reads_impl(ctx, kQuery1, reads, d_win_offsets, k, d_kmers, d_counts, n, d_out);
}

int kmx_count_lookup_reads2(kmx_ctx* ctx, const kmx_reads* reads, const uint64_t* d_win_offsets, uint32_t k, const uint64_t* d_kmers2,
                            const uint64_t* d_counts, uint64_t n, uint64_t* d_out) {
    return lookup_reads_impl(ctx, kQuery2, reads, d_win_offsets, k, d_kmers2, d_counts, n, d_out);
}

// ---- the counting sketch (kmx_sketch.hip) ----
static const CountKind kSketchAdd1{"kmx_sketch_add", 1u, kmx_canonical_windows};
static const CountKind kSketchAdd2{"kmx_sketch_add2", 2u, kmx_canonical_windows2};

static int sketch_add_words_impl(kmx_ctx* ctx, uint32_t words, const uint64_t* d_words, const uint64_t* d_weights, uint64_t n, uint8_t* d_sketch,
                                 uint32_t log2_blocks, uint64_t seed) {
    if (!ctx || (n && !d_words) || n > (1ull << 40) || !sketch_ok(d_sketch, log2_blocks, n != 0)) return KMX_E_ARG;
    if (words == 2u && !aligned16(d_words)) return KMX_E_ARG;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_sketch_add(words, d_words, d_weights, nullptr, n, d_sketch, log2_blocks, seed, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_sketch_add_words(kmx_ctx* ctx, const uint64_t* d_words, const uint64_t* d_weights, uint64_t n, uint8_t* d_sketch, uint32_t log2_blocks,
                         uint64_t seed) {
    return sketch_add_words_impl(ctx, 1u, d_words, d_weights, n, d_sketch, log2_blocks, seed);
}

int kmx_sketch_add_words2(kmx_ctx* ctx, const uint64_t* d_words2, const uint64_t* d_weights, uint64_t n, uint8_t* d_sketch, uint32_t log2_blocks,
                          uint64_t seed) {
    return sketch_add_words_impl(ctx, 2u, d_words2, d_weights, n, d_sketch, log2_blocks, seed);
}

// kmx_sketch_add(2) = the windows of the batch as the counter makes them (windows_front), then the add kernel over (canon, flags).
static int sketch_add_impl(kmx_ctx* ctx, const CountKind& kind, uint32_t k_min, uint32_t k_max, const kmx_reads* reads, uint32_t k,
                           uint8_t* d_sketch, uint32_t log2_blocks, uint64_t seed) {
    if (!ctx || !reads_ok(reads) || !sketch_ok(d_sketch, log2_blocks, reads->n_reads != 0)) return KMX_E_ARG;
    if (k < k_min || k > k_max) return KMX_E_K_RANGE;
    if (reads->n_reads == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    WindowsFront f;
    if (int st = windows_front(ctx, reads, k, kind, nullptr, &f)) return st;
    KMX_HIP(ctx, kmx::launch_sketch_add(kind.words, f.canon, nullptr, f.flags, f.n_win, d_sketch, log2_blocks, seed, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_sketch_add(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, uint8_t* d_sketch, uint32_t log2_blocks, uint64_t seed) {
    return sketch_add_impl(ctx, kSketchAdd1, 1u, 31u, reads, k, d_sketch, log2_blocks, seed);
}

int kmx_sketch_add2(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, uint8_t* d_sketch, uint32_t log2_blocks, uint64_t seed) {
    return sketch_add_impl(ctx, kSketchAdd2, 33u, 64u, reads, k, d_sketch, log2_blocks, seed);
}

static int sketch_lookup_impl(kmx_ctx* ctx, uint32_t words, const uint64_t* d_words, uint64_t n, const uint8_t* d_sketch, uint32_t log2_blocks,
                              uint64_t seed, uint8_t* d_est) {
    if (!ctx || (n && (!d_words || !d_est)) || n > (1ull << 40) || !sketch_ok(d_sketch, log2_blocks, n != 0)) return KMX_E_ARG;
    if (words == 2u && !aligned16(d_words)) return KMX_E_ARG;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_sketch_lookup(words, d_words, nullptr, n, d_sketch, log2_blocks, seed, d_est, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_sketch_lookup(kmx_ctx* ctx, const uint64_t* d_words, uint64_t n, const uint8_t* d_sketch, uint32_t log2_blocks, uint64_t seed,
                      uint8_t* d_est) {
    return sketch_lookup_impl(ctx, 1u, d_words, n, d_sketch, log2_blocks, seed, d_est);
}

int kmx_sketch_lookup2(kmx_ctx* ctx, const uint64_t* d_words2, uint64_t n, const uint8_t* d_sketch, uint32_t log2_blocks, uint64_t seed,
                       uint8_t* d_est) {
    return sketch_lookup_impl(ctx, 2u, d_words2, n, d_sketch, log2_blocks, seed, d_est);
}

// kmx_sketch_lookup_reads(2) = kmx_canonical_windows(2) into the work buffer -- [segment plan of long reads][canon 8 (16) B/window]
// [flags 1 B/window] -- followed by the lookup kernel, in the caller's slot layout as kmx_count_lookup_reads(2).
static int sketch_lookup_reads_impl(kmx_ctx* ctx, const QueryKind& kind, const char* who, const kmx_reads* reads, const uint64_t* d_win_offsets,
                                    uint32_t k, const uint8_t* d_sketch, uint32_t log2_blocks, uint64_t seed, uint8_t* d_est) {
    if (!ctx || !reads_ok(reads) || !sketch_ok(d_sketch, log2_blocks, reads->n_reads != 0)) return KMX_E_ARG;
    if (k < kind.k_min || k > kind.k_max) return KMX_E_K_RANGE;
    if (reads->d_offsets && !d_win_offsets) return KMX_E_ARG;
    if (reads->n_reads == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    uint64_t n_bound = 0, n_bases = 0, n_win = 0;
    if (int st = caller_windows(ctx, reads, d_win_offsets, k, &n_bound, &n_bases, &n_win)) return st;
    if (n_win == 0) return KMX_OK;
    if (!d_est) return KMX_E_ARG;
    const size_t plan = align256(count_plan_bytes(reads, k, n_bases));
    const size_t canon_at = plan, flags_at = canon_at + align256(8u * kind.words * n_bound), bytes = flags_at + align256(n_bound);
    void* buf = nullptr;
    WorkHold hold;
    if (int st = work_area(ctx, who, bytes, &buf, &hold)) return st;
    uint64_t* canon = reinterpret_cast<uint64_t*>(hold.base + canon_at);
    uint8_t* flags = reinterpret_cast<uint8_t*>(hold.base + flags_at);
    if (int st = kind.windows(ctx, reads, d_win_offsets, k, nullptr, nullptr, canon, flags)) return st;
    if (int st = work_kept(ctx, who, hold)) return st;
    KMX_HIP(ctx, kmx::launch_sketch_lookup(kind.words, canon, flags, n_win, d_sketch, log2_blocks, seed, d_est, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_sketch_lookup_reads(kmx_ctx* ctx, const kmx_reads* reads, const uint64_t* d_win_offsets, uint32_t k, const uint8_t* d_sketch,
                            uint32_t log2_blocks, uint64_t seed, uint8_t* d_est) {
    return sketch_lookup_reads_impl(ctx, kQuery1, "kmx_sketch_lookup_reads", reads, d_win_offsets, k, d_sketch, log2_blocks, seed, d_est);
}

int kmx_sketch_lookup_reads2(kmx_ctx* ctx, const kmx_reads* reads, const uint64_t* d_win_offsets, uint32_t k, const uint8_t* d_sketch,
                             uint32_t log2_blocks, uint64_t seed, uint8_t* d_est) {
    return sketch_lookup_reads_impl(ctx, kQuery2, "kmx_sketch_lookup_reads2", reads, d_win_offsets, k, d_sketch, log2_blocks, seed, d_est);
}

int kmx_sketch_merge(kmx_ctx* ctx, const uint8_t* d_a, const uint8_t* d_b, uint32_t log2_blocks, uint8_t* d_out) {
    if (!ctx || !sketch_ok(d_a, log2_blocks, true) || !sketch_ok(d_b, log2_blocks, true) || !sketch_ok(d_out, log2_blocks, true)) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_sketch_merge(d_a, d_b, log2_blocks, d_out, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_sketch_stats(kmx_ctx* ctx, const uint8_t* d_sketch, uint32_t log2_blocks, uint64_t* d_hist) {
    if (!ctx || !sketch_ok(d_sketch, log2_blocks, true) || !d_hist) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_sketch_stats(d_sketch, log2_blocks, d_hist, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

// ---- the distinct-key estimator (kmx_hll.hip) ----
// HyperLogLog registers as the calls take them (kmx.h): 1 << log2_regs bytes, 16-byte aligned, 4 <= log2_regs <= 24.
static bool hll_ok(const void* d_regs, uint32_t log2_regs, bool needed) {
    return log2_regs >= 4u && log2_regs <= 24u && (reinterpret_cast<uintptr_t>(d_regs) & 15u) == 0 && (d_regs != nullptr || !needed);
}
static const CountKind kHllAdd1{"kmx_hll_add", 1u, kmx_canonical_windows};
static const CountKind kHllAdd2{"kmx_hll_add2", 2u, kmx_canonical_windows2};

static int hll_add_words_impl(kmx_ctx* ctx, uint32_t words, const uint64_t* d_words, uint64_t n, uint8_t* d_regs, uint32_t log2_regs, uint64_t seed) {
    if (!ctx || (n && !d_words) || n > (1ull << 40) || !hll_ok(d_regs, log2_regs, n != 0)) return KMX_E_ARG;
    if (words == 2u && !aligned16(d_words)) return KMX_E_ARG;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_hll_add(words, d_words, nullptr, n, d_regs, log2_regs, seed, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_hll_add_words(kmx_ctx* ctx, const uint64_t* d_words, uint64_t n, uint8_t* d_regs, uint32_t log2_regs, uint64_t seed) {
    return hll_add_words_impl(ctx, 1u, d_words, n, d_regs, log2_regs, seed);
}

int kmx_hll_add_words2(kmx_ctx* ctx, const uint64_t* d_words2, uint64_t n, uint8_t* d_regs, uint32_t log2_regs, uint64_t seed) {
    return hll_add_words_impl(ctx, 2u, d_words2, n, d_regs, log2_regs, seed);
}

// kmx_hll_add(2) = the windows of the batch as the counter makes them (windows_front), then the add kernel over (canon, flags):
// kmx_sketch_add(2) with the other kernel behind it.
static int hll_add_impl(kmx_ctx* ctx, const CountKind& kind, uint32_t k_min, uint32_t k_max, const kmx_reads* reads, uint32_t k, uint8_t* d_regs,
                        uint32_t log2_regs, uint64_t seed) {
    if (!ctx || !reads_ok(reads) || !hll_ok(d_regs, log2_regs, reads->n_reads != 0)) return KMX_E_ARG;
    if (k < k_min || k > k_max) return KMX_E_K_RANGE;
    if (reads->n_reads == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    WindowsFront f;
    if (int st = windows_front(ctx, reads, k, kind, nullptr, &f)) return st;
    KMX_HIP(ctx, kmx::launch_hll_add(kind.words, f.canon, f.flags, f.n_win, d_regs, log2_regs, seed, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_hll_add(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, uint8_t* d_regs, uint32_t log2_regs, uint64_t seed) {
    return hll_add_impl(ctx, kHllAdd1, 1u, 31u, reads, k, d_regs, log2_regs, seed);
}

int kmx_hll_add2(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, uint8_t* d_regs, uint32_t log2_regs, uint64_t seed) {
    return hll_add_impl(ctx, kHllAdd2, 33u, 64u, reads, k, d_regs, log2_regs, seed);
}

int kmx_hll_merge(kmx_ctx* ctx, const uint8_t* d_a, const uint8_t* d_b, uint32_t log2_regs, uint8_t* d_out) {
    if (!ctx || !hll_ok(d_a, log2_regs, true) || !hll_ok(d_b, log2_regs, true) || !hll_ok(d_out, log2_regs, true)) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_hll_merge(d_a, d_b, log2_regs, d_out, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_hll_stats(kmx_ctx* ctx, const uint8_t* d_a, const uint8_t* d_b, uint32_t log2_regs, uint64_t* d_hist) {
    if (!ctx || !hll_ok(d_a, log2_regs, true) || !hll_ok(d_b, log2_regs, false) || !d_hist) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_hll_stats(d_a, d_b, log2_regs, d_hist, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

// The front half the per-read calls share (kmx_count_read_stats(2), kmx_count_read_paths(2), kmx_count_correct_reads(2), kmx_count_read_colors(2)):
// kmx_canonical_windows(2) and the lookup kernel, which leave one u64 answer (the count, or whatever `d_values` holds per entry) and one
// flag byte per window.  The work buffer, laid out up front: [segment plan of long reads][ragged reads: window offsets][two-word keys:
// canon 16 B/window][answers 8 B/window][flags 1 B/window][`extra` bytes of the caller's][directory, when it pays and fits].  One-word
// keys: the windows call writes its canonical words into the answers array and they are looked up in place.
struct ReadsFront {
    char* base = nullptr;          // the work buffer
    uint64_t n_win = 0;            // the windows there are; 0 = none, and nothing ran
    uint64_t* wo = nullptr;        // ragged reads: the window offsets, made on the device
    uint64_t* answers = nullptr;   // one u64 per window
    uint8_t* flags = nullptr;      // one byte per window
    size_t area_at = 0;            // where the caller's `extra` bytes start
    const void* dir = nullptr;     // the directory the lookup built (prefix bits p), nullptr = it searched plainly
    uint32_t p = 0;
};
// n_bound / n_bases: query_window_bound's, n_bound != 0.  KMX_E_NOMEM above the cap before any kernel runs.
static int reads_front(kmx_ctx* ctx, const QueryKind& kind, const char* who, const kmx_reads* reads, uint32_t k, const uint64_t* d_kmers,
                       const uint64_t* d_values, uint64_t n, uint64_t n_bound, uint64_t n_bases, size_t extra, ReadsFront* f) {
    const size_t plan = align256(count_plan_bytes(reads, k, n_bases));
    const size_t wo_bytes = reads->d_offsets ? align256(kmx::win_offsets_bytes(reads->n_reads)) : 0;
    const size_t canon_at = plan + wo_bytes, answers_at = canon_at + (kind.words == 2u ? align256(16u * n_bound) : 0u);
    const size_t flags_at = answers_at + align256(8u * n_bound), area_at = flags_at + align256(n_bound);
    const size_t reserved = area_at + extra;
    WorkHold hold;
    if (int st = query_scratch(ctx, who, kind.words, reserved, n, k, n_bound, &hold)) return st;
    char* const base = hold.base;
    uint64_t n_win = n_bound;
    uint64_t* wo = nullptr;
    if (reads->d_offsets) {
        KMX_HIP(ctx, kmx::launch_count_win_offsets(reads->d_offsets, reads->n_reads, k, base + plan, &wo, ctx->h_pinned, &n_win, ctx->stream));
        if (n_win > n_bound) {
            char msg[96];
            std::snprintf(msg, sizeof msg, "%s: window count above its bound", who);
            return fail_hip(ctx, hipErrorUnknown, msg);
        }
        if (n_win == 0) return KMX_OK;
    }
    uint64_t* answers = reinterpret_cast<uint64_t*>(base + answers_at);
    uint64_t* canon = kind.words == 2u ? reinterpret_cast<uint64_t*>(base + canon_at) : answers;
    uint8_t* flags = reinterpret_cast<uint8_t*>(base + flags_at);
    if (int st = kind.windows(ctx, reads, wo, k, nullptr, nullptr, canon, flags)) return st;
    if (int st = work_kept(ctx, who, hold)) return st;
    if (int st = lookup_run(ctx, kind, d_kmers, d_values, n, k, canon, flags, n_win, answers, &hold, &f->dir, &f->p)) return st;
    f->base = base;
    f->wo = wo;
    f->answers = answers;
    f->flags = flags;
    f->area_at = area_at;
    f->n_win = n_win;
    return KMX_OK;
}

// kmx_count_read_stats(2) = reads_front and the per-read reduction of kmx_count_read_stats.hip over its answers.
static int read_stats_impl(kmx_ctx* ctx, const QueryKind& kind, const kmx_reads* reads, uint32_t k, const uint64_t* d_kmers,
                           const uint64_t* d_counts, uint64_t n, uint64_t solid_min, uint64_t* d_stats) {
    if (!ctx || !reads_ok(reads) || (n && !d_kmers) || n > (1ull << 40)) return KMX_E_ARG;
    if (kind.words == 2u && !aligned16(d_kmers)) return KMX_E_ARG;
    if (k < kind.k_min || k > kind.k_max) return KMX_E_K_RANGE;
    if (reads->n_reads == 0) return KMX_OK;
    if (!d_stats) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    const char* who = kind.words == 2u ? "kmx_count_read_stats2" : "kmx_count_read_stats";
    const size_t stats_bytes = 8u * KMX_RS_WORDS * reads->n_reads;
    uint64_t n_bound = 0, n_bases = 0;
    if (int st = query_window_bound(ctx, reads, k, &n_bound, &n_bases)) return st;
    ReadsFront f;
    if (n_bound != 0)
        if (int st = reads_front(ctx, kind, who, reads, k, d_kmers, d_counts, n, n_bound, n_bases, 0, &f)) return st;
    if (f.n_win == 0) {   // no window in the batch: every row is eight zeros
        KMX_HIP(ctx, hipMemsetAsync(d_stats, 0, stats_bytes, ctx->stream));
        return KMX_OK;
    }
    // uniform reads: the windows of a read; ragged reads: the most a read within the bound has (0 = no bound given)
    const uint32_t w = reads->read_len >= k ? reads->read_len - k + 1u : 0u;
    KMX_HIP(ctx, kmx::launch_count_read_stats(f.answers, f.flags, f.wo, reads->n_reads, w, solid_min, d_stats, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_count_read_stats(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, const uint64_t* d_kmers, const uint64_t* d_counts, uint64_t n,
                         uint64_t solid_min, uint64_t* d_stats) {
    return read_stats_impl(ctx, kQuery1, reads, k, d_kmers, d_counts, n, solid_min, d_stats);
}

int kmx_count_read_stats2(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, const uint64_t* d_kmers2, const uint64_t* d_counts, uint64_t n,
                          uint64_t solid_min, uint64_t* d_stats) {
    return read_stats_impl(ctx, kQuery2, reads, k, d_kmers2, d_counts, n, solid_min, d_stats);
}

// kmx_count_correct_reads(2) = reads_front, a copy of the reads into the output, and the decision kernel of kmx_count_correct.hip, which
// stores the corrected bytes over the copy and a row per read.  Nothing is written before the work buffer is granted.
static int correct_reads_impl(kmx_ctx* ctx, const QueryKind& kind, const kmx_reads* reads, uint32_t k, const uint64_t* d_kmers,
                              const uint64_t* d_counts, uint64_t n, uint64_t solid_min, uint32_t min_cover, uint8_t* d_out_bases,
                              uint64_t* d_fixes) {
    if (!ctx || !reads_ok(reads) || (n && !d_kmers) || n > (1ull << 40)) return KMX_E_ARG;
    if (kind.words == 2u && !aligned16(d_kmers)) return KMX_E_ARG;
    if (k < kind.k_min || k > kind.k_max) return KMX_E_K_RANGE;
    if (min_cover < 1u || min_cover > k) return KMX_E_ARG;
    if (reads->n_reads == 0) return KMX_OK;
    if (!d_out_bases) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    const char* who = kind.words == 2u ? "kmx_count_correct_reads2" : "kmx_count_correct_reads";
    uint64_t n_bound = 0, n_bases = 0, first = 0;
    if (int st = query_window_bound(ctx, reads, k, &n_bound, &n_bases, &first)) return st;
    // the bytes that are written: as many, and as far into the output, as the reads take of d_bases
    uint64_t n_bytes = n_bases;
    if (!reads->d_offsets) {
        if (reads->read_len && reads->n_reads > (1ull << 62) / reads->read_len) return KMX_E_ARG;
        n_bytes = reads->n_reads * reads->read_len;
    }
    const uintptr_t in_at = reinterpret_cast<uintptr_t>(reads->d_bases) + first, out_at = reinterpret_cast<uintptr_t>(d_out_bases) + first;
    if (n_bytes && in_at < out_at + n_bytes && out_at < in_at + n_bytes) return KMX_E_ARG;   // (decisions are against the original bytes)
    ReadsFront f;
    if (n_bound != 0)
        if (int st = reads_front(ctx, kind, who, reads, k, d_kmers, d_counts, n, n_bound, n_bases, 0, &f)) return st;
    if (n_bytes) KMX_HIP(ctx, hipMemcpyAsync(d_out_bases + first, reads->d_bases + first, n_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    if (f.n_win == 0) {   // no window in the batch: the copy, and every row is four zeros
        if (d_fixes) KMX_HIP(ctx, hipMemsetAsync(d_fixes, 0, 8u * KMX_CR_WORDS * reads->n_reads, ctx->stream));
        return KMX_OK;
    }
    KMX_HIP(ctx, kmx::launch_count_correct(kind.words, reads->d_bases, d_out_bases, reads->d_offsets, f.wo, reads->n_reads, reads->read_len, f.answers,
                                           f.flags, d_kmers, d_counts, n, k, f.dir, f.p, solid_min, min_cover, d_fixes, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_count_correct_reads(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, const uint64_t* d_kmers, const uint64_t* d_counts, uint64_t n,
                            uint64_t solid_min, uint32_t min_cover, uint8_t* d_out_bases, uint64_t* d_fixes) {
    return correct_reads_impl(ctx, kQuery1, reads, k, d_kmers, d_counts, n, solid_min, min_cover, d_out_bases, d_fixes);
}

int kmx_count_correct_reads2(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, const uint64_t* d_kmers2, const uint64_t* d_counts, uint64_t n,
                             uint64_t solid_min, uint32_t min_cover, uint8_t* d_out_bases, uint64_t* d_fixes) {
    return correct_reads_impl(ctx, kQuery2, reads, k, d_kmers2, d_counts, n, solid_min, min_cover, d_out_bases, d_fixes);
}

// kmx_count_read_colors(2) = reads_front -- with the masks as the values -- and the per-read reduction of kmx_count_color.hip.
static int read_colors_impl(kmx_ctx* ctx, const QueryKind& kind, const kmx_reads* reads, uint32_t k, const uint64_t* d_kmers,
                            const uint64_t* d_colors, uint64_t n, uint32_t n_colors, uint32_t thr_num, uint32_t thr_den, uint64_t* d_rows,
                            uint32_t* d_hits) {
    if (!ctx || !reads_ok(reads) || (n && (!d_kmers || !d_colors)) || n > (1ull << 40)) return KMX_E_ARG;
    if (kind.words == 2u && !aligned16(d_kmers)) return KMX_E_ARG;
    if (k < kind.k_min || k > kind.k_max) return KMX_E_K_RANGE;
    if (n_colors < 1u || n_colors > 64u || thr_den < 1u || thr_num > thr_den) return KMX_E_ARG;
    if (reads->n_reads == 0) return KMX_OK;
    if (!d_rows) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    const char* who = kind.words == 2u ? "kmx_count_read_colors2" : "kmx_count_read_colors";
    uint64_t n_bound = 0, n_bases = 0;
    if (int st = query_window_bound(ctx, reads, k, &n_bound, &n_bases)) return st;
    ReadsFront f;
    if (n_bound != 0)
        if (int st = reads_front(ctx, kind, who, reads, k, d_kmers, d_colors, n, n_bound, n_bases, 0, &f)) return st;
    if (f.n_win == 0) {   // no window in the batch: every row and every hit count is zero
        KMX_HIP(ctx, hipMemsetAsync(d_rows, 0, 8u * KMX_RC_WORDS * reads->n_reads, ctx->stream));
        if (d_hits) KMX_HIP(ctx, hipMemsetAsync(d_hits, 0, 4u * n_colors * reads->n_reads, ctx->stream));
        return KMX_OK;
    }
    const uint32_t w = reads->read_len >= k ? reads->read_len - k + 1u : 0u;   // (uniform reads: the windows of a read)
    KMX_HIP(ctx, kmx::launch_count_read_colors(f.answers, f.flags, f.wo, reads->n_reads, w, n_colors, thr_num, thr_den, d_rows, d_hits, ctx->n_cu,
                                               ctx->stream));
    return KMX_OK;
}

int kmx_count_read_colors(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, const uint64_t* d_kmers, const uint64_t* d_colors, uint64_t n,
                          uint32_t n_colors, uint32_t thr_num, uint32_t thr_den, uint64_t* d_rows, uint32_t* d_hits) {
    return read_colors_impl(ctx, kQuery1, reads, k, d_kmers, d_colors, n, n_colors, thr_num, thr_den, d_rows, d_hits);
}

int kmx_count_read_colors2(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, const uint64_t* d_kmers2, const uint64_t* d_colors, uint64_t n,
                           uint32_t n_colors, uint32_t thr_num, uint32_t thr_den, uint64_t* d_rows, uint32_t* d_hits) {
    return read_colors_impl(ctx, kQuery2, reads, k, d_kmers2, d_colors, n, n_colors, thr_num, thr_den, d_rows, d_hits);
}

int kmx_count_color_matrix(kmx_ctx* ctx, const uint64_t* d_colors, uint64_t n, uint32_t n_colors, uint64_t* d_matrix, uint64_t* d_spectrum) {
    if (!ctx || !d_matrix || n_colors < 1u || n_colors > 64u || (n && !d_colors) || n > (1ull << 40)) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    void* area = nullptr;   // the blocks' partial results (n == 0: none, the summing kernel writes the zeros)
    if (n != 0)
        if (int st = work_area(ctx, "kmx_count_color_matrix", kmx::count_color_matrix_bytes(n, n_colors, ctx->n_cu), &area)) return st;
    KMX_HIP(ctx, kmx::launch_count_color_matrix(d_colors, n, n_colors, area, d_matrix, d_spectrum, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_count_spectrum(kmx_ctx* ctx, const uint64_t* d_counts, uint64_t n, uint64_t n_bins, uint64_t* d_spectrum) {
    if (!ctx || !d_spectrum || n_bins < 2 || (n && !d_counts) || n > (1ull << 40)) return KMX_E_ARG;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_count_spectrum(d_counts, n, n_bins, d_spectrum, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

static int filter_impl(kmx_ctx* ctx, const char* who, uint32_t words, const uint64_t* d_kmers, const uint64_t* d_counts, uint64_t n,
                       uint64_t min_count, uint64_t max_count, uint64_t* d_kmers_out, uint64_t* d_counts_out, uint64_t max_out, uint64_t* h_n_out) {
    if (!ctx || !h_n_out || ((d_kmers_out == nullptr) != (d_counts_out == nullptr))) return KMX_E_ARG;
    if ((n && (!d_kmers || !d_counts)) || n > (1ull << 38)) return KMX_E_ARG;   // (the mark pass is one grid of a thread per entry)
    if (words == 2u && (!aligned16(d_kmers) || !aligned16(d_kmers_out))) return KMX_E_ARG;
    *h_n_out = 0;
    if (n == 0 || min_count > max_count) return KMX_OK;
    DeviceGuard g(ctx->device);
    void* area = nullptr;
    if (int st = work_area(ctx, who, kmx::count_filter_bytes(n), &area)) return st;
    uint64_t n_out = 0;
    KMX_HIP(ctx, kmx::launch_count_filter_mark(d_counts, n, min_count, max_count, area, ctx->h_pinned, &n_out, ctx->stream));
    *h_n_out = n_out;
    if (!d_kmers_out || n_out == 0) return KMX_OK;
    if (int st = room_for(ctx, who, n_out, "entries kept", max_out)) return st;
    KMX_HIP(ctx, kmx::launch_count_filter_emit(words, d_kmers, d_counts, n, area, d_kmers_out, d_counts_out, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMX_OK;
}

int kmx_count_filter(kmx_ctx* ctx, const uint64_t* d_kmers, const uint64_t* d_counts, uint64_t n, uint64_t min_count, uint64_t max_count,
                     uint64_t* d_kmers_out, uint64_t* d_counts_out, uint64_t max_out, uint64_t* h_n_out) {
    return filter_impl(ctx, "kmx_count_filter", 1u, d_kmers, d_counts, n, min_count, max_count, d_kmers_out, d_counts_out, max_out, h_n_out);
}

int kmx_count_filter2(kmx_ctx* ctx, const uint64_t* d_kmers2, const uint64_t* d_counts, uint64_t n, uint64_t min_count, uint64_t max_count,
                      uint64_t* d_kmers2_out, uint64_t* d_counts_out, uint64_t max_out, uint64_t* h_n_out) {
    return filter_impl(ctx, "kmx_count_filter2", 2u, d_kmers2, d_counts, n, min_count, max_count, d_kmers2_out, d_counts_out, max_out, h_n_out);
}

// ---- a count table as the node set of a de Bruijn graph (kmx_count_graph.hip) ----
// One body for both key widths.  8 * n neighbour words are asked of n keys, so the directory is built whenever the lookup would build
// one for that many queries (n above one line of keys, n < 2^32) and it fits under the cap; otherwise the plain search, which needs no
// work buffer: never KMX_E_NOMEM from here.
static int adjacency_impl(kmx_ctx* ctx, const QueryKind& kind, const uint64_t* d_kmers, const uint64_t* d_counts, uint64_t n, uint32_t k,
                          uint64_t min_count, uint8_t* d_edges, uint8_t* d_flips, uint64_t* d_nbr) {
    if (!ctx || (n && (!d_kmers || !d_edges)) || n > (1ull << 40)) return KMX_E_ARG;
    if (kind.words == 2u && !aligned16(d_kmers)) return KMX_E_ARG;
    if (k < (kind.words == 1u ? 2u : kind.k_min) || k > kind.k_max) return KMX_E_K_RANGE;   // (a word of one base has no overlap to share)
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    uint32_t p = 0;
    void* const dir = lookup_dir(ctx, nullptr, kind.words, n, k, 8u * n, &p);
    KMX_HIP(ctx, kmx::launch_count_adjacency(kind.words, d_kmers, d_counts, n, k, min_count, d_edges, d_flips, d_nbr, dir, p, ctx->stream));
    return KMX_OK;
}

int kmx_count_adjacency(kmx_ctx* ctx, const uint64_t* d_kmers, const uint64_t* d_counts, uint64_t n, uint32_t k, uint64_t min_count,
                        uint8_t* d_edges, uint8_t* d_flips, uint64_t* d_nbr) {
    return adjacency_impl(ctx, kQuery1, d_kmers, d_counts, n, k, min_count, d_edges, d_flips, d_nbr);
}

int kmx_count_adjacency2(kmx_ctx* ctx, const uint64_t* d_kmers2, const uint64_t* d_counts, uint64_t n, uint32_t k, uint64_t min_count,
                         uint8_t* d_edges, uint8_t* d_flips, uint64_t* d_nbr) {
    return adjacency_impl(ctx, kQuery2, d_kmers2, d_counts, n, k, min_count, d_edges, d_flips, d_nbr);
}

int kmx_count_edge_histogram(kmx_ctx* ctx, const uint8_t* d_edges, uint64_t n, uint64_t* d_hist) {
    if (!ctx || !d_hist || (n && !d_edges) || n > (1ull << 40)) return KMX_E_ARG;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_count_edge_histogram(d_edges, n, d_hist, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_count_unitig_ends(kmx_ctx* ctx, const uint8_t* d_edges, const uint8_t* d_flips, const uint64_t* d_nbr, uint64_t n, uint8_t* d_ends) {
    if (!ctx || (n && (!d_edges || !d_flips || !d_nbr || !d_ends)) || n > (1ull << 40)) return KMX_E_ARG;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_count_unitig_ends(d_edges, d_flips, d_nbr, n, d_ends, ctx->stream));
    return KMX_OK;
}

// ---- the unitigs of that graph (kmx_count_unitigs.hip) ----
// One body for both key widths.  The keys are read at even k only (the palindromes), so they may be NULL at odd k.
static int unitigs_impl(kmx_ctx* ctx, const QueryKind& kind, const char* who, const uint64_t* d_kmers, const uint64_t* d_counts, uint64_t n, uint32_t k,
                        uint64_t min_count, const uint8_t* d_edges, const uint8_t* d_flips, const uint64_t* d_nbr, uint64_t* d_nodes, uint64_t* d_offsets,
                        uint8_t* d_circular, uint64_t* d_count_sums, uint64_t* h_n_unitigs, uint64_t* h_n_nodes) {
    if (!ctx || !h_n_unitigs || !h_n_nodes || n > (1ull << 40)) return KMX_E_ARG;
    if (n && (!d_edges || !d_flips || !d_nbr || !d_nodes || !d_offsets)) return KMX_E_ARG;
    if (kind.words == 2u && !aligned16(d_kmers)) return KMX_E_ARG;
    if (k < (kind.words == 1u ? 2u : kind.k_min) || k > kind.k_max) return KMX_E_K_RANGE;
    if (n && (k & 1u) == 0u && !d_kmers) return KMX_E_ARG;
    *h_n_unitigs = *h_n_nodes = 0;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    void* area = nullptr;
    if (int st = work_area(ctx, who, kmx::count_unitigs_bytes(n), &area)) return st;
    uint64_t n_unitigs = 0, n_nodes = 0;
    uint32_t rounds = 0;
    bool bad = false;
    KMX_HIP(ctx, kmx::launch_count_unitigs(kind.words, d_kmers, d_counts, n, k, min_count, d_edges, d_flips, d_nbr, d_nodes, d_offsets, d_circular,
                                           d_count_sums, area, ctx->h_pinned, &n_unitigs, &n_nodes, &rounds, &bad, ctx->stream));
    if (bad) {
        char msg[96];
        std::snprintf(msg, sizeof msg, "%s: ranking did not end", who);
        return fail_hip(ctx, hipErrorUnknown, msg);
    }
    *h_n_unitigs = n_unitigs;
    *h_n_nodes = n_nodes;
    return KMX_OK;
}

int kmx_count_unitigs(kmx_ctx* ctx, const uint64_t* d_kmers, const uint64_t* d_counts, uint64_t n, uint32_t k, uint64_t min_count,
                      const uint8_t* d_edges, const uint8_t* d_flips, const uint64_t* d_nbr, uint64_t* d_nodes, uint64_t* d_offsets,
                      uint8_t* d_circular, uint64_t* d_count_sums, uint64_t* h_n_unitigs, uint64_t* h_n_nodes) {
    return unitigs_impl(ctx, kQuery1, "kmx_count_unitigs", d_kmers, d_counts, n, k, min_count, d_edges, d_flips, d_nbr, d_nodes, d_offsets, d_circular,
                        d_count_sums, h_n_unitigs, h_n_nodes);
}

int kmx_count_unitigs2(kmx_ctx* ctx, const uint64_t* d_kmers2, const uint64_t* d_counts, uint64_t n, uint32_t k, uint64_t min_count,
                       const uint8_t* d_edges, const uint8_t* d_flips, const uint64_t* d_nbr, uint64_t* d_nodes, uint64_t* d_offsets,
                       uint8_t* d_circular, uint64_t* d_count_sums, uint64_t* h_n_unitigs, uint64_t* h_n_nodes) {
    return unitigs_impl(ctx, kQuery2, "kmx_count_unitigs2", d_kmers2, d_counts, n, k, min_count, d_edges, d_flips, d_nbr, d_nodes, d_offsets, d_circular,
                        d_count_sums, h_n_unitigs, h_n_nodes);
}

static int unitig_sequences_impl(kmx_ctx* ctx, const QueryKind& kind, const uint64_t* d_kmers, uint64_t n, uint32_t k, const uint64_t* d_nodes,
                                 const uint64_t* d_offsets, uint64_t n_unitigs, uint8_t* d_seq) {
    if (!ctx || n > (1ull << 40) || n_unitigs > n) return KMX_E_ARG;
    if (n_unitigs && (!d_kmers || !d_nodes || !d_offsets || !d_seq)) return KMX_E_ARG;
    if (kind.words == 2u && !aligned16(d_kmers)) return KMX_E_ARG;
    if (k < (kind.words == 1u ? 2u : kind.k_min) || k > kind.k_max) return KMX_E_K_RANGE;
    if (n_unitigs == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_count_unitig_sequences(kind.words, d_kmers, n, k, d_nodes, d_offsets, n_unitigs, d_seq, ctx->stream));
    return KMX_OK;
}

int kmx_count_unitig_sequences(kmx_ctx* ctx, const uint64_t* d_kmers, uint64_t n, uint32_t k, const uint64_t* d_nodes, const uint64_t* d_offsets,
                               uint64_t n_unitigs, uint8_t* d_seq) {
    return unitig_sequences_impl(ctx, kQuery1, d_kmers, n, k, d_nodes, d_offsets, n_unitigs, d_seq);
}

int kmx_count_unitig_sequences2(kmx_ctx* ctx, const uint64_t* d_kmers2, uint64_t n, uint32_t k, const uint64_t* d_nodes, const uint64_t* d_offsets,
                                uint64_t n_unitigs, uint8_t* d_seq) {
    return unitig_sequences_impl(ctx, kQuery2, d_kmers2, n, k, d_nodes, d_offsets, n_unitigs, d_seq);
}

// ---- reads threaded through the unitigs (kmx_count_paths.hip) ----
int kmx_count_unitig_index(kmx_ctx* ctx, const uint64_t* d_nodes, const uint64_t* d_offsets, uint64_t n_unitigs, uint64_t n, uint64_t* d_place) {
    if (!ctx || n > (1ull << 40) || n_unitigs > (1ull << 40)) return KMX_E_ARG;
    if (n == 0) return KMX_OK;
    if (!d_place || (n_unitigs && (!d_nodes || !d_offsets))) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_count_unitig_index(d_nodes, d_offsets, n_unitigs, n, d_place, ctx->stream));
    return KMX_OK;
}

// kmx_count_read_paths(2) = reads_front -- the windows call and the lookup kernel, with the places as the counts -- and the segment
// kernels of kmx_count_paths.hip over its answers; the ballots, counts and partials of the segment kernels are its `extra` bytes.
static int read_paths_impl(kmx_ctx* ctx, const QueryKind& kind, const kmx_reads* reads, uint32_t k, const uint64_t* d_kmers, uint64_t n,
                           const uint64_t* d_place, const uint64_t* d_offsets, uint64_t n_unitigs, uint64_t* d_path_offsets, uint64_t* d_segments,
                           uint64_t max_segments, uint64_t* h_n_segments) {
    if (!ctx || !reads_ok(reads) || !h_n_segments || n > (1ull << 40) || n_unitigs > (1ull << 40)) return KMX_E_ARG;
    if ((n && (!d_kmers || !d_place)) || (n_unitigs && !d_offsets) || ((d_path_offsets == nullptr) != (d_segments == nullptr))) return KMX_E_ARG;
    if (kind.words == 2u && !aligned16(d_kmers)) return KMX_E_ARG;
    if (k < (kind.words == 1u ? 2u : kind.k_min) || k > kind.k_max) return KMX_E_K_RANGE;
    *h_n_segments = 0;
    if (reads->n_reads == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    const char* who = kind.words == 2u ? "kmx_count_read_paths2" : "kmx_count_read_paths";
    const size_t offsets_bytes = 8u * (reads->n_reads + 1u);
    uint64_t n_bound = 0, n_bases = 0;
    if (int st = query_window_bound(ctx, reads, k, &n_bound, &n_bases)) return st;
    if (n_bound == 0 || n == 0 || n_unitigs == 0) {   // no window, or nothing to lie on: no segment, every offset 0
        if (d_path_offsets) KMX_HIP(ctx, hipMemsetAsync(d_path_offsets, 0, offsets_bytes, ctx->stream));
        return KMX_OK;
    }
    ReadsFront f;
    if (int st = reads_front(ctx, kind, who, reads, k, d_kmers, d_place, n, n_bound, n_bases, kmx::count_paths_bytes(n_bound), &f)) return st;
    if (f.n_win == 0) {
        if (d_path_offsets) KMX_HIP(ctx, hipMemsetAsync(d_path_offsets, 0, offsets_bytes, ctx->stream));
        return KMX_OK;
    }
    const uint64_t n_win = f.n_win;
    const uint64_t *places = f.answers, *wo = f.wo;
    uint8_t* flags = f.flags;
    char* base = f.base;
    const size_t area_at = f.area_at;
    const uint32_t w = reads->read_len >= k ? reads->read_len - k + 1u : 0u;   // (uniform reads: the windows of a read)
    uint64_t n_segments = 0;
    KMX_HIP(ctx, kmx::launch_count_paths_mark(places, flags, wo, reads->n_reads, w, n_win, d_offsets, n_unitigs, base + area_at, ctx->h_pinned,
                                              &n_segments, ctx->stream));
    *h_n_segments = n_segments;
    if (!d_path_offsets) return KMX_OK;
    const int room = room_for(ctx, who, n_segments, "segments", max_segments);   // (the offsets are written all the same: they say how to batch)
    KMX_HIP(ctx, kmx::launch_count_paths_emit(places, flags, wo, reads->n_reads, w, n_win, d_offsets, n_unitigs, base + area_at, d_path_offsets,
                                              room == KMX_OK ? d_segments : nullptr, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return room;
}

int kmx_count_read_paths(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, const uint64_t* d_kmers, uint64_t n, const uint64_t* d_place,
                         const uint64_t* d_offsets, uint64_t n_unitigs, uint64_t* d_path_offsets, uint64_t* d_segments, uint64_t max_segments,
                         uint64_t* h_n_segments) {
    return read_paths_impl(ctx, kQuery1, reads, k, d_kmers, n, d_place, d_offsets, n_unitigs, d_path_offsets, d_segments, max_segments, h_n_segments);
}

int kmx_count_read_paths2(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, const uint64_t* d_kmers2, uint64_t n, const uint64_t* d_place,
                          const uint64_t* d_offsets, uint64_t n_unitigs, uint64_t* d_path_offsets, uint64_t* d_segments, uint64_t max_segments,
                          uint64_t* h_n_segments) {
    return read_paths_impl(ctx, kQuery2, reads, k, d_kmers2, n, d_place, d_offsets, n_unitigs, d_path_offsets, d_segments, max_segments, h_n_segments);
}

// ---- the unitigs as a graph, and a table cut down by unitig (kmx_count_links.hip) ----
int kmx_count_unitig_links(kmx_ctx* ctx, const uint8_t* d_edges, const uint8_t* d_flips, const uint64_t* d_nbr, uint64_t n, const uint64_t* d_nodes,
                           const uint64_t* d_offsets, uint64_t n_unitigs, const uint64_t* d_place, uint64_t* d_link_offsets, uint64_t* d_links,
                           uint64_t max_links, uint64_t* h_n_links) {
    if (!ctx || !h_n_links || n > (1ull << 40) || n_unitigs > (1ull << 40)) return KMX_E_ARG;
    if ((d_link_offsets == nullptr) != (d_links == nullptr)) return KMX_E_ARG;
    if (n_unitigs && (!d_nodes || !d_offsets || (n && (!d_edges || !d_flips || !d_nbr || !d_place)))) return KMX_E_ARG;
    *h_n_links = 0;
    if (n_unitigs == 0 && (n == 0 || !d_link_offsets)) return KMX_OK;
    DeviceGuard g(ctx->device);
    if (n_unitigs == 0) {   // the single offset 0
        KMX_HIP(ctx, hipMemsetAsync(d_link_offsets, 0, 8u, ctx->stream));
        KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return KMX_OK;
    }
    const char* who = "kmx_count_unitig_links";
    void* area = nullptr;
    if (int st = work_area(ctx, who, kmx::count_links_bytes(n_unitigs), &area)) return st;
    uint64_t n_links = 0;
    KMX_HIP(ctx, kmx::launch_count_links_count(d_edges, d_flips, d_nbr, n, d_nodes, d_offsets, n_unitigs, d_place, area, ctx->h_pinned, &n_links,
                                               ctx->stream));
    *h_n_links = n_links;
    if (!d_link_offsets) return KMX_OK;
    const int room = room_for(ctx, who, n_links, "links", max_links);   // (the offsets are written all the same, as the read paths' are)
    KMX_HIP(ctx, kmx::launch_count_links_emit(d_edges, d_flips, d_nbr, n, d_nodes, d_offsets, n_unitigs, d_place, area, n_links, d_link_offsets,
                                              room == KMX_OK ? d_links : nullptr, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return room;
}

// One body for both key widths: the filter's -- its area, its emit -- behind another mark.
static int unitig_select_impl(kmx_ctx* ctx, const char* who, uint32_t words, const uint64_t* d_kmers, const uint64_t* d_counts, uint64_t n,
                              const uint64_t* d_place, const uint64_t* d_offsets, uint64_t n_unitigs, const uint8_t* d_keep, uint64_t* d_kmers_out,
                              uint64_t* d_counts_out, uint64_t max_out, uint64_t* h_n_out) {
    if (!ctx || !h_n_out || ((d_kmers_out == nullptr) != (d_counts_out == nullptr))) return KMX_E_ARG;
    if ((n && (!d_kmers || !d_counts || !d_place)) || n > (1ull << 38)) return KMX_E_ARG;   // (the mark pass is one grid of a thread per entry)
    if ((n_unitigs && (!d_offsets || !d_keep)) || n_unitigs > (1ull << 40)) return KMX_E_ARG;
    if (words == 2u && (!aligned16(d_kmers) || !aligned16(d_kmers_out))) return KMX_E_ARG;
    *h_n_out = 0;
    if (n == 0 || n_unitigs == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    void* area = nullptr;
    if (int st = work_area(ctx, who, kmx::count_filter_bytes(n), &area)) return st;
    uint64_t n_out = 0;
    KMX_HIP(ctx, kmx::launch_count_select_mark(d_place, n, d_offsets, n_unitigs, d_keep, area, ctx->h_pinned, &n_out, ctx->stream));
    *h_n_out = n_out;
    if (!d_kmers_out || n_out == 0) return KMX_OK;
    if (int st = room_for(ctx, who, n_out, "entries kept", max_out)) return st;
    KMX_HIP(ctx, kmx::launch_count_filter_emit(words, d_kmers, d_counts, n, area, d_kmers_out, d_counts_out, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMX_OK;
}

int kmx_count_unitig_select(kmx_ctx* ctx, const uint64_t* d_kmers, const uint64_t* d_counts, uint64_t n, const uint64_t* d_place,
                            const uint64_t* d_offsets, uint64_t n_unitigs, const uint8_t* d_keep, uint64_t* d_kmers_out, uint64_t* d_counts_out,
                            uint64_t max_out, uint64_t* h_n_out) {
    return unitig_select_impl(ctx, "kmx_count_unitig_select", 1u, d_kmers, d_counts, n, d_place, d_offsets, n_unitigs, d_keep, d_kmers_out, d_counts_out,
                              max_out, h_n_out);
}

int kmx_count_unitig_select2(kmx_ctx* ctx, const uint64_t* d_kmers2, const uint64_t* d_counts, uint64_t n, const uint64_t* d_place,
                             const uint64_t* d_offsets, uint64_t n_unitigs, const uint8_t* d_keep, uint64_t* d_kmers2_out, uint64_t* d_counts_out,
                             uint64_t max_out, uint64_t* h_n_out) {
    return unitig_select_impl(ctx, "kmx_count_unitig_select2", 2u, d_kmers2, d_counts, n, d_place, d_offsets, n_unitigs, d_keep, d_kmers2_out,
                              d_counts_out, max_out, h_n_out);
}

// ---- which unitigs to drop: tips, bubble branches, islands (kmx_count_clean.hip) ----
int kmx_count_unitig_clean(kmx_ctx* ctx, const uint64_t* d_offsets, const uint8_t* d_circular, const uint64_t* d_count_sums, uint64_t n_unitigs,
                           const uint64_t* d_link_offsets, const uint64_t* d_links, uint64_t n_links, uint64_t tip_max_nodes, uint32_t tip_num,
                           uint32_t tip_den, uint64_t bubble_max_nodes, uint64_t bubble_max_diff, uint64_t island_max_nodes, uint8_t* d_keep,
                           uint8_t* d_reason) {
    if (!ctx || n_unitigs > (1ull << 40) || n_links > (1ull << 43)) return KMX_E_ARG;   // (four links per oriented unitig)
    if (tip_num > tip_den || tip_num > 65535u || tip_den > 65535u || (tip_den == 0u && tip_max_nodes > 0u)) return KMX_E_ARG;
    if (n_unitigs == 0) return KMX_OK;
    if (!d_keep || !d_offsets || !d_link_offsets || (n_links && !d_links)) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_count_unitig_clean(d_offsets, d_circular, d_count_sums, n_unitigs, d_link_offsets, d_links, n_links, tip_max_nodes, tip_num,
                                                tip_den, bubble_max_nodes, bubble_max_diff, island_max_nodes, d_keep, d_reason, ctx->stream));
    return KMX_OK;
}

// ---- which unitigs hang together (kmx_count_components.hip) ----
int kmx_count_unitig_components(kmx_ctx* ctx, const uint64_t* d_offsets, const uint64_t* d_count_sums, uint64_t n_unitigs,
                                const uint64_t* d_link_offsets, const uint64_t* d_links, uint64_t n_links, const uint8_t* d_mask, uint64_t* d_labels,
                                uint64_t* d_ids, uint64_t* d_components, uint64_t max_components, uint64_t* h_n_components, uint32_t* h_rounds) {
    if (!ctx || !h_n_components || n_unitigs > (1ull << 40) || n_links > (1ull << 43)) return KMX_E_ARG;   // (four links per oriented unitig)
    if (n_unitigs && (!d_labels || !d_link_offsets)) return KMX_E_ARG;
    if (n_links && !d_links) return KMX_E_ARG;
    *h_n_components = 0;
    if (h_rounds) *h_rounds = 0;
    if (n_unitigs == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    const char* who = "kmx_count_unitig_components";
    const bool own_rank = d_components && !d_ids;
    void* area = nullptr;
    if (int st = work_area(ctx, who, kmx::count_components_bytes(n_unitigs, own_rank), &area)) return st;
    uint64_t n_components = 0;
    uint32_t rounds = 0;
    bool bad = false;
    KMX_HIP(ctx, kmx::launch_count_components_label(d_link_offsets, d_links, n_links, d_mask, n_unitigs, d_labels, area, own_rank, ctx->h_pinned,
                                                    &n_components, &rounds, &bad, ctx->stream));
    if (bad) {
        char msg[96];
        std::snprintf(msg, sizeof msg, "%s: the rounds did not end", who);
        return fail_hip(ctx, hipErrorUnknown, msg);
    }
    *h_n_components = n_components;
    if (h_rounds) *h_rounds = rounds;
    const int room = d_components ? room_for(ctx, who, n_components, "components", max_components) : KMX_OK;   // (labels and ids all the same)
    uint64_t* records = room == KMX_OK ? d_components : nullptr;
    if (d_ids || records) {
        KMX_HIP(ctx, kmx::launch_count_components_emit(d_labels, n_unitigs, d_offsets, d_count_sums, area, own_rank, d_ids, records, n_components,
                                                       ctx->stream));
        KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return room;
}

// ---- which links the reads walk, and an adjacency without chosen links (kmx_count_link_support.hip) ----
int kmx_count_link_support(kmx_ctx* ctx, const uint64_t* d_segments, uint64_t n_segments, const uint64_t* d_offsets, uint64_t n_unitigs,
                           const uint64_t* d_link_offsets, const uint64_t* d_links, uint64_t n_links, uint64_t* d_support, uint64_t* d_summary) {
    if (!ctx || !d_summary || n_segments > (1ull << 40) || n_unitigs > (1ull << 40) || n_links > (1ull << 43)) return KMX_E_ARG;
    if ((n_segments && !d_segments) || (n_links && (!d_links || !d_support)) || (n_unitigs && (!d_offsets || !d_link_offsets))) return KMX_E_ARG;
    if (n_segments < 2) return KMX_OK;   // (no pair of segments)
    DeviceGuard g(ctx->device);
    // (n_unitigs == 0: every junction names a unitig at or above U and is unlinked; neither offsets array is read)
    KMX_HIP(ctx, kmx::launch_count_link_support(d_segments, n_segments, d_offsets, n_unitigs, d_link_offsets, d_links, n_links, d_support, d_summary,
                                                ctx->stream));
    return KMX_OK;
}

int kmx_count_adjacency_cut(kmx_ctx* ctx, const uint8_t* d_edges, const uint8_t* d_flips, const uint64_t* d_nbr, uint64_t n, const uint64_t* d_nodes,
                            const uint64_t* d_offsets, uint64_t n_unitigs, const uint64_t* d_place, const uint64_t* d_link_offsets, uint64_t n_links,
                            const uint8_t* d_cut, uint8_t* d_edges_out) {
    if (!ctx || n > (1ull << 40) || n_unitigs > (1ull << 40) || n_links > (1ull << 43)) return KMX_E_ARG;
    if (n == 0) return KMX_OK;
    if (!d_edges || !d_edges_out) return KMX_E_ARG;
    if (d_edges_out < d_edges + n && d_edges < d_edges_out + n) return KMX_E_ARG;   // (the bits are re-derived from the input while the output is cut)
    if (n_unitigs && n_links && (!d_flips || !d_nbr || !d_nodes || !d_offsets || !d_place || !d_link_offsets || !d_cut)) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_count_adjacency_cut(d_edges, d_flips, d_nbr, n, d_nodes, d_offsets, n_unitigs, d_place, d_link_offsets, n_links, d_cut,
                                                 d_edges_out, ctx->stream));
    return KMX_OK;
}

// ---- what the kmx_reads_* calls share on the host ----
namespace {
// the size of a batch the calls accept (behind reads_ok): at most 2^40 reads and, of uniform reads, at most 2^62 bases
bool reads_batch_ok(const kmx_reads* reads) {
    if (reads->n_reads > (1ull << 40)) return false;
    return reads->d_offsets || !reads->read_len || reads->n_reads <= (1ull << 62) / reads->read_len;
}
struct Range {   // device bytes, for "the bytes a call reads against the bytes it writes"; an empty range overlaps nothing
    uintptr_t at;
    uint64_t bytes;
    bool overlaps(const Range& o) const { return bytes && o.bytes && at < o.at + o.bytes && o.at < at + bytes; }
    static Range of_bytes(const void* base, uint64_t n) { return Range{reinterpret_cast<uintptr_t>(base), base ? n : 0u}; }
    static Range of_words(const void* base, uint64_t n_words) { return of_bytes(base, 8u * n_words); }
    // the bytes at `base` that a batch spans: from its first to its last offset (both from the device), or n_reads uniform reads
    static Range of_batch(const void* base, const uint64_t* d_offsets, uint64_t n_reads, uint32_t read_len, uint64_t first, uint64_t last) {
        if (!base) return Range{0, 0};
        if (d_offsets) return Range{reinterpret_cast<uintptr_t>(base) + first, last >= first ? last - first : 0};
        return of_bytes(base, n_reads * (uint64_t)read_len);
    }
};
}  // namespace

// ---- a new batch of reads from an old one (kmx_reads_edit.hip) ----
// What kmx_reads_select and kmx_reads_gather share behind their argument checks (e.n_rows > 0): the work buffer, the plan's count,
// the room and overlap checks, the emit.  n_out may be nullptr (gather: every row is an output read).
static int reads_edit_impl(kmx_ctx* ctx, const char* who, const kmx::ReadsEdit& e, uint8_t* d_out_bases, uint64_t* d_out_offsets,
                           uint64_t* d_out_index, uint64_t max_reads, uint64_t max_bases, uint64_t* h_n_reads, uint64_t* h_n_bases) {
    DeviceGuard g(ctx->device);
    void* area = nullptr;
    if (int st = work_area(ctx, who, kmx::reads_edit_bytes(e.n_rows), &area)) return st;
    uint64_t h[4] = {0, 0, 0, 0};   // output reads, output bases, the batch's first and last offset
    KMX_HIP(ctx, kmx::launch_reads_edit_count(e, area, ctx->h_pinned, h, ctx->stream));
    if (h_n_reads) *h_n_reads = h[0];
    *h_n_bases = h[1];
    if (!d_out_bases) return KMX_OK;
    if (int st = room_for(ctx, who, h[0], "reads kept", max_reads)) return st;
    if (int st = room_for(ctx, who, h[1], "bases kept", max_bases)) return st;
    if (h[1] >= (1ull << 44)) {   // (the copy is one grid of a block per 16 KiB)
        std::snprintf(ctx->last_error, sizeof ctx->last_error, "%s: %llu bases in one batch", who, (unsigned long long)h[1]);
        return KMX_E_NOMEM;
    }
    // the bytes the source batch spans against the bytes that are written
    if (Range::of_batch(e.bases, e.offsets, e.n_reads, e.read_len, h[2], h[3]).overlaps(Range::of_bytes(d_out_bases, h[1]))) return KMX_E_ARG;
    KMX_HIP(ctx, kmx::launch_reads_edit_emit(e, area, h[0], h[1], d_out_bases, d_out_offsets, d_out_index, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMX_OK;
}

int kmx_reads_select(kmx_ctx* ctx, const kmx_reads* reads, const uint8_t* d_keep, const uint64_t* d_span, uint64_t span_stride, uint32_t span_k,
                     uint64_t min_len, uint8_t* d_out_bases, uint64_t* d_out_offsets, uint64_t* d_out_index, uint64_t max_reads, uint64_t max_bases,
                     uint64_t* h_n_reads, uint64_t* h_n_bases) {
    if (!ctx || !reads_ok(reads) || !h_n_reads || !h_n_bases || ((d_out_bases == nullptr) != (d_out_offsets == nullptr))) return KMX_E_ARG;
    if ((d_span && span_stride == 0) || !reads_batch_ok(reads)) return KMX_E_ARG;
    *h_n_reads = *h_n_bases = 0;
    if (reads->n_reads == 0) return KMX_OK;
    const kmx::ReadsEdit e{reads->d_bases, reads->d_offsets, reads->n_reads, reads->read_len, d_keep, d_span, span_stride, span_k, min_len, nullptr,
                           reads->n_reads};
    return reads_edit_impl(ctx, "kmx_reads_select", e, d_out_bases, d_out_offsets, d_out_index, max_reads, max_bases, h_n_reads, h_n_bases);
}

int kmx_reads_gather(kmx_ctx* ctx, const kmx_reads* reads, const uint64_t* d_index, uint64_t n_index, const uint64_t* d_span, uint64_t span_stride,
                     uint32_t span_k, uint8_t* d_out_bases, uint64_t* d_out_offsets, uint64_t max_bases, uint64_t* h_n_bases) {
    if (!ctx || !reads_ok(reads) || !h_n_bases || ((d_out_bases == nullptr) != (d_out_offsets == nullptr))) return KMX_E_ARG;
    if ((d_span && span_stride == 0) || !reads_batch_ok(reads) || n_index > (1ull << 32) || (n_index && !d_index)) return KMX_E_ARG;
    *h_n_bases = 0;
    if (n_index == 0) return KMX_OK;
    const kmx::ReadsEdit e{reads->d_bases, reads->d_offsets, reads->n_reads, reads->read_len, nullptr, d_span, span_stride, span_k, 0u, d_index, n_index};
    return reads_edit_impl(ctx, "kmx_reads_gather", e, d_out_bases, d_out_offsets, nullptr, n_index, max_bases, nullptr, h_n_bases);
}

// ---- set algebra and comparison of two count tables (kmx_count_setop.hip) ----
// The checks the six calls share, and the work buffer for n_a + n_b > 0 entries (*area).
static int setop_area(kmx_ctx* ctx, const char* who, uint32_t words, const uint64_t* d_kmers_a, uint64_t n_a, const uint64_t* d_kmers_b, uint64_t n_b,
                      void** area) {
    if ((n_a && !d_kmers_a) || (n_b && !d_kmers_b) || n_a > (1ull << 40) || n_b > (1ull << 40)) return KMX_E_ARG;
    if (words == 2u && (!aligned16(d_kmers_a) || !aligned16(d_kmers_b))) return KMX_E_ARG;
    *area = nullptr;
    if (n_a + n_b == 0) return KMX_OK;
    return work_area(ctx, who, kmx::count_setop_bytes(n_a + n_b), area);
}

static int setop_impl(kmx_ctx* ctx, const char* who, uint32_t words, uint32_t op, uint32_t rule, const uint64_t* d_kmers_a, const uint64_t* d_counts_a,
                      uint64_t n_a, const uint64_t* d_kmers_b, const uint64_t* d_counts_b, uint64_t n_b, uint64_t* d_kmers_out, uint64_t* d_counts_out,
                      uint64_t max_out, uint64_t* h_n_out) {
    if (!ctx || !h_n_out || ((d_kmers_out == nullptr) != (d_counts_out == nullptr))) return KMX_E_ARG;
    if (op > KMX_SETOP_COUNTER_SUBTRACT || rule > KMX_RULE_RIGHT) return KMX_E_ARG;
    const bool ruled = op == KMX_SETOP_INTERSECT || op == KMX_SETOP_UNION;
    if (!ruled && rule != 0u) return KMX_E_ARG;
    // the count arrays the operation reads
    const bool reads_a = !(op == KMX_SETOP_INTERSECT && rule == KMX_RULE_RIGHT);
    const bool reads_b = !(op == KMX_SETOP_SUBTRACT || (op == KMX_SETOP_INTERSECT && rule == KMX_RULE_LEFT));
    if ((n_a && reads_a && !d_counts_a) || (n_b && reads_b && !d_counts_b)) return KMX_E_ARG;
    if (words == 2u && !aligned16(d_kmers_out)) return KMX_E_ARG;
    *h_n_out = 0;
    DeviceGuard g(ctx->device);
    void* area = nullptr;
    if (int st = setop_area(ctx, who, words, d_kmers_a, n_a, d_kmers_b, n_b, &area)) return st;
    if (!area) return KMX_OK;   // (both tables empty)
    uint64_t n_out = 0;
    KMX_HIP(ctx, kmx::launch_count_setop(words, op, d_kmers_a, d_counts_a, n_a, d_kmers_b, d_counts_b, n_b, area, ctx->h_pinned, &n_out, ctx->stream));
    *h_n_out = n_out;
    if (!d_kmers_out || n_out == 0) return KMX_OK;
    if (int st = room_for(ctx, who, n_out, "k-mers in the result", max_out)) return st;
    KMX_HIP(ctx, kmx::launch_count_setop_emit(words, op, rule, d_kmers_a, d_counts_a, n_a, d_kmers_b, d_counts_b, n_b, area, d_kmers_out, d_counts_out,
                                              ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMX_OK;
}

int kmx_count_setop(kmx_ctx* ctx, uint32_t op, uint32_t rule, const uint64_t* d_kmers_a, const uint64_t* d_counts_a, uint64_t n_a,
                    const uint64_t* d_kmers_b, const uint64_t* d_counts_b, uint64_t n_b, uint64_t* d_kmers_out, uint64_t* d_counts_out, uint64_t max_out,
                    uint64_t* h_n_out) {
    return setop_impl(ctx, "kmx_count_setop", 1u, op, rule, d_kmers_a, d_counts_a, n_a, d_kmers_b, d_counts_b, n_b, d_kmers_out, d_counts_out, max_out,
                      h_n_out);
}

int kmx_count_setop2(kmx_ctx* ctx, uint32_t op, uint32_t rule, const uint64_t* d_kmers2_a, const uint64_t* d_counts_a, uint64_t n_a,
                     const uint64_t* d_kmers2_b, const uint64_t* d_counts_b, uint64_t n_b, uint64_t* d_kmers2_out, uint64_t* d_counts_out,
                     uint64_t max_out, uint64_t* h_n_out) {
    return setop_impl(ctx, "kmx_count_setop2", 2u, op, rule, d_kmers2_a, d_counts_a, n_a, d_kmers2_b, d_counts_b, n_b, d_kmers2_out, d_counts_out,
                      max_out, h_n_out);
}

static int compare_impl(kmx_ctx* ctx, const char* who, uint32_t words, const uint64_t* d_kmers_a, const uint64_t* d_counts_a, uint64_t n_a,
                        const uint64_t* d_kmers_b, const uint64_t* d_counts_b, uint64_t n_b, void* h_out) {
    if (!ctx || !h_out) return KMX_E_ARG;
    // counts of both tables, or of neither (an empty table has none to give)
    const bool with_counts = d_counts_a != nullptr || d_counts_b != nullptr;
    if (with_counts && ((n_a && !d_counts_a) || (n_b && !d_counts_b))) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    void* area = nullptr;
    if (int st = setop_area(ctx, who, words, d_kmers_a, n_a, d_kmers_b, n_b, &area)) return st;
    uint64_t rec[6] = {0, 0, 0, 0, 0, 0};   // n_both, sum_a, sum_b, sum_a_both, sum_b_both, sum_min
    if (area)
        KMX_HIP(ctx, kmx::launch_count_compare(words, d_kmers_a, with_counts ? d_counts_a : nullptr, n_a, d_kmers_b, with_counts ? d_counts_b : nullptr,
                                               n_b, area, ctx->h_pinned, rec, ctx->stream));
    kmx_table_compare* out = static_cast<kmx_table_compare*>(h_out);
    out->n_both = rec[0];
    out->n_only_a = n_a - rec[0];
    out->n_only_b = n_b - rec[0];
    out->sum_a = rec[1];
    out->sum_b = rec[2];
    out->sum_a_both = rec[3];
    out->sum_b_both = rec[4];
    out->sum_min = rec[5];
    out->sum_max = rec[1] + rec[2] - rec[5];   // (per key max + min = count_a + count_b; all of it mod 2^64)
    return KMX_OK;
}

int kmx_count_compare(kmx_ctx* ctx, const uint64_t* d_kmers_a, const uint64_t* d_counts_a, uint64_t n_a, const uint64_t* d_kmers_b,
                      const uint64_t* d_counts_b, uint64_t n_b, void* h_out) {
    return compare_impl(ctx, "kmx_count_compare", 1u, d_kmers_a, d_counts_a, n_a, d_kmers_b, d_counts_b, n_b, h_out);
}

int kmx_count_compare2(kmx_ctx* ctx, const uint64_t* d_kmers2_a, const uint64_t* d_counts_a, uint64_t n_a, const uint64_t* d_kmers2_b,
                       const uint64_t* d_counts_b, uint64_t n_b, void* h_out) {
    return compare_impl(ctx, "kmx_count_compare2", 2u, d_kmers2_a, d_counts_a, n_a, d_kmers2_b, d_counts_b, n_b, h_out);
}

int kmx_canonical_reduce2(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, uint32_t with_hash, kmx_summary2* d_out) {
    if (!ctx || !reads_ok(reads) || !d_out) return KMX_E_ARG;
    if (k < 33 || k > 64) return KMX_E_K_RANGE;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(kmx_summary2), ctx->stream));
    if (reads->n_reads == 0) return KMX_OK;
    if (!reads->d_offsets) {
        bool handled = false;
        if (int st = queue_clear_marks(ctx, reads->n_reads * kmx::bitsliced_segments_per_read(reads->read_len, k), k, false)) return st;
        KMX_HIP(ctx, kmx::launch_scan_bitsliced2(reads->d_bases, reads->n_reads, reads->read_len, k, with_hash != 0, d_out,
                                                 queue_of(ctx), ctx->n_cu, ctx->stream, &handled));
        if (handled) return KMX_OK;
    }
    // Reads behind an offsets array (what kmx_fastx_parse hands over), 16-byte aligned base: the tiled kernels.  With a length bound
    // the uniform two-word kernel takes, "is every read exactly that long" (untrimmed FASTQ) is decided on the device as
    // kmx_canonical_reduce does it: a small kernel checks offsets[i] == i*L, the uniform scan and the ragged one (the 10-word frame:
    // the reads themselves with a bound of at most 160 or none, segments of them above) are both launched behind its verdict, exactly one counts.
    const uint32_t Lh = reads->read_len;
    if (reads->d_offsets && aligned16(reads->d_bases)) {
        KMX_HIP(ctx, queue_clear(ctx, KMX_Q_CLEAR_THROUGH_GATE));
        // A bound above the 10-word frame (161...: 250-base reads, long reads): the ragged kernel scans SEGMENTS of at most 161 - k
        // windows, cut on the device as kmx_canonical_reduce does for long reads (two host round trips) -- first of all, so that the
        // masks of the dirty reads are sized once for whichever kernel will run.
        const uint64_t *starts = nullptr, *ends = nullptr;
        uint64_t n_seg = 0;
        bool segmented = false;
        bool cut = Lh > 160;
        if (cut && Lh <= 256) {
            // (a bound the uniform kernel takes: if the batch holds exactly n_reads * bound bases it is, almost certainly, untrimmed --
            // the gate below will say so for sure -- and the segments would be built for nothing: 16 bytes of offsets tell.  Should
            // the gate disagree, the lane-per-read kernel counts.)
            // (round 6: at ANY one length up to the bound -- 150-base reads handed over with a bound of 250 paid the segment cut, three host
            // round trips and a second set of marks, for the uniform kernel to run in the end: the gate passes every uniform length)
            uint64_t o_first = 0, o_last = 0;
            if (int st = offsets_span(ctx, reads, &o_first, &o_last)) return st;
            if (o_first == 0 && o_last % reads->n_reads == 0 && o_last / reads->n_reads >= k && o_last / reads->n_reads <= Lh) cut = false;
        }
        if (cut) {
            const int st = long_ragged_segments(ctx, reads, k, 161u - k, &starts, &ends, &n_seg);
            if (st > 0) return st;
            segmented = st == 0;
            if (segmented && n_seg == 0) return KMX_OK;      // no read holds a window
        }
        if (int st = prepare_dirty_flags(ctx, segmented && n_seg > reads->n_reads ? n_seg : reads->n_reads, k)) return st;
        bool h_u = false, h_r = false;
        const uint32_t Lg = Lh ? Lh : 160u;   // (round 5: the gate passes reads that are uniform at ANY length up to the bound; no bound = the 160-base frame)
        if (Lg >= k && Lg <= 256) {
            KMX_HIP(ctx, gate_arm(ctx));
            KMX_HIP(ctx, kmx::launch_offsets_uniform_gate(reads->d_offsets, reads->n_reads, Lg, k, gate_of(ctx), ctx->n_cu, ctx->stream));
            KMX_HIP(ctx, kmx::launch_scan_bitsliced2(reads->d_bases, reads->n_reads, Lg, k, with_hash != 0, d_out, queue_of(ctx),
                                                     ctx->n_cu, ctx->stream, &h_u));
            // (not launched: the verdict must not keep the other kernel from running)
            if (!h_u) KMX_HIP(ctx, gate_disarm(ctx));
        }
        if (segmented)
            KMX_HIP(ctx, kmx::launch_scan_bitsliced2_ragged(reads->d_bases, starts, n_seg, 160u, k, with_hash != 0, d_out, queue_of(ctx), ctx->n_cu,
                                                            ctx->stream, &h_r, ends));
        else if (Lh <= 160)
            KMX_HIP(ctx, kmx::launch_scan_bitsliced2_ragged(reads->d_bases, reads->d_offsets, reads->n_reads, Lh, k, with_hash != 0, d_out,
                                                            queue_of(ctx), ctx->n_cu, ctx->stream, &h_r));
        if (!h_r) KMX_HIP(ctx, kmx::launch_reduce2_generic(reads, k, with_hash, d_out, ctx->n_cu, ctx->stream, too_long_of(ctx), h_u ? gate_of(ctx) : nullptr));
        if (h_u) KMX_HIP(ctx, gate_disarm(ctx));   // never left armed
        return KMX_OK;
    }
    KMX_HIP(ctx, kmx::launch_reduce2_generic(reads, k, with_hash, d_out, ctx->n_cu, ctx->stream, too_long_of(ctx), nullptr));
    return KMX_OK;
}

int kmx_canonical_windows2(kmx_ctx* ctx, const kmx_reads* reads, const uint64_t* d_win_offsets, uint32_t k,
                           uint64_t* d_fw2, uint64_t* d_rc2, uint64_t* d_canon2, uint8_t* d_flags) {
    if (!ctx || !reads_ok(reads)) return KMX_E_ARG;
    if (k < 33 || k > 64) return KMX_E_K_RANGE;
    if (reads->d_offsets && !d_win_offsets) return KMX_E_ARG;
    if (reads->n_reads == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    bool handled = false;   // uniform reads of up to 256 bases in the dense layout (slot r*W + p): the tiled kernel (kmx_generic.hip)
    if (!reads->d_offsets && !d_win_offsets) {   // (a caller's win_offsets for uniform reads are honoured by the lane-per-read kernel, as kmx_canonical_windows does)
        // (a tile with an invalid byte stays on the tiled path: its reads are marked, the sweep behind the passes zeroes the spoiled slots -- round 6)
        if (int st = queue_clear_marks(ctx, reads->n_reads, k, true)) return st;
        KMX_HIP(ctx, kmx::launch_windows2_tiled(reads, k, d_fw2, d_rc2, d_canon2, d_flags, ctx->n_cu, ctx->stream, &handled, queue_of(ctx)));
    }
    if (!handled) {   // reads longer than a frame (round 4): segments, as kmx_canonical_windows takes them
        const uint64_t *starts = nullptr, *ends = nullptr, *wins = nullptr;
        uint64_t n_seg = 0;
        const int st = long_segments(ctx, reads, d_win_offsets, k, &starts, &ends, &wins, &n_seg);
        if (st > 0) return st;
        if (st == 0) {
            if (n_seg == 0) return KMX_OK;
            if (int st2 = windows2_segments(ctx, reads, starts, ends, wins, n_seg, k, d_fw2, d_rc2, d_canon2, d_flags, &handled)) return st2;
        }
    }
    if (!handled && reads->d_offsets && d_win_offsets) {   // ragged reads (round 4): tiled too; read_len = optional length bound
        if (int st = queue_clear_marks(ctx, reads->n_reads, k, true)) return st;
        KMX_HIP(ctx, kmx::launch_windows2_tiled_ragged(reads, d_win_offsets, k, d_fw2, d_rc2, d_canon2, d_flags, ctx->n_cu, ctx->stream, &handled,
                                                       too_long_of(ctx), nullptr, queue_of(ctx)));
    }
    if (handled) return KMX_OK;
    KMX_HIP(ctx, kmx::launch_windows2_generic(reads, d_win_offsets, k, d_fw2, d_rc2, d_canon2, d_flags, ctx->n_cu, ctx->stream, too_long_of(ctx)));
    return KMX_OK;
}

int kmx_histogram(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, uint32_t hasher, uint32_t hasher_k,
                  uint32_t log2_buckets, uint64_t* d_counts) {
    if (!ctx || !reads_ok(reads) || !d_counts) return KMX_E_ARG;
    if (k < 1 || k > 31) return KMX_E_K_RANGE;
    if (hasher > KMX_HASH_IDENTITY || log2_buckets > 30) return KMX_E_ARG;
    if (hasher == KMX_HASH_LEX && (hasher_k < 1 || hasher_k > 32)) return KMX_E_K_RANGE;
    if (reads->n_reads == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    {
        bool handled = false;
        KMX_HIP(ctx, queue_clear(ctx, KMX_Q_CLEAR_THROUGH_GATE));
        // (the histogram sinks mark the reads of a dirty tile like the bit-sliced scan does; without the array they roll such tiles, exactly)
        if (k >= 2 && k <= 31) {
            if (int st = prepare_dirty_flags(ctx, reads->n_reads, k, true)) return st;
        }
        KMX_HIP(ctx, kmx::launch_hist_uniform(reads->d_bases, reads->n_reads, reads->read_len, k, hasher, hasher_k,
                                              log2_buckets, d_counts, queue_of(ctx), ctx->n_cu, ctx->stream, &handled,
                                              &work_callback, ctx, work_budget(ctx), reads->d_offsets));
        if (handled) return KMX_OK;
    }
    KMX_HIP(ctx, kmx::launch_histogram_generic(reads, k, hasher, hasher_k, log2_buckets, d_counts, ctx->n_cu, ctx->stream, too_long_of(ctx)));
    return KMX_OK;
}

int kmx_gen_reads(kmx_ctx* ctx, uint64_t seed, uint64_t first_byte, uint8_t* d_out, uint64_t nbytes) {
    if (!ctx || (nbytes && !d_out)) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_gen_reads(seed, first_byte, d_out, nbytes, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

/* -------------------------------------------------------- element-wise ---- */

int kmx_kmers_from_bytes(kmx_ctx* ctx, const uint8_t* d_seqs, uint64_t n, uint32_t k, uint64_t* d_words,
                         uint64_t* h_first_bad) {
    if (!ctx || (n && (!d_seqs || !d_words))) return KMX_E_ARG;
    if (k > 32) return KMX_E_TOO_LONG;  // kmer.rs:236-238
    if (k < 1) return KMX_E_K_RANGE;
    if (h_first_bad) *h_first_bad = ~0ull;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, first_bad_reset(ctx));
    KMX_HIP(ctx, kmx::launch_kmers_from_bytes(d_seqs, n, k, d_words, first_bad_of(ctx), ctx->n_cu, ctx->stream));
    unsigned long long bad = 0;
    if (int st = first_bad_read(ctx, &bad)) return st;
    if (bad != ~0ull) {
        if (h_first_bad) *h_first_bad = bad;
        return KMX_E_INVALID_BASE;
    }
    return KMX_OK;
}

int kmx_revcomp_words(kmx_ctx* ctx, const uint64_t* d_in, uint64_t n, uint32_t k, uint64_t* d_out) {
    if (!ctx || (n && (!d_in || !d_out))) return KMX_E_ARG;
    if (k < 1 || k > 32) return KMX_E_K_RANGE;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_revcomp_words(d_in, n, k, d_out, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_canonical_words(kmx_ctx* ctx, const uint64_t* d_in, uint64_t n, uint32_t k, uint64_t* d_canon,
                        uint8_t* d_is_canonical) {
    if (!ctx || (n && !d_in)) return KMX_E_ARG;
    if (k < 1 || k > 32) return KMX_E_K_RANGE;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_canonical_words(d_in, n, k, d_canon, d_is_canonical, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_hash_words(kmx_ctx* ctx, const uint64_t* d_in, uint64_t n, uint32_t hasher, uint32_t hasher_k, uint64_t* d_out) {
    if (!ctx || (n && (!d_in || !d_out))) return KMX_E_ARG;
    if (hasher != KMX_HASH_LEX && hasher != KMX_HASH_IDENTITY) return KMX_E_ARG;
    if (hasher == KMX_HASH_LEX && (hasher_k < 1 || hasher_k > 32)) return KMX_E_K_RANGE;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_hash_words(d_in, n, hasher, hasher_k, d_out, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_hash_words_sip13(kmx_ctx* ctx, const uint64_t* d_in, uint64_t n, uint64_t key0, uint64_t key1, uint64_t* d_out) {
    if (!ctx || (n && (!d_in || !d_out))) return KMX_E_ARG;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_hash_words_sip13(d_in, n, key0, key1, d_out, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_match_words(kmx_ctx* ctx, const uint64_t* d_fw, const uint64_t* d_rc, const uint64_t* d_other, uint64_t n,
                    uint8_t* d_out) {
    if (!ctx || (n && (!d_fw || !d_rc || !d_other || !d_out))) return KMX_E_ARG;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_match_words(d_fw, d_rc, d_other, n, d_out, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

static int ck_shift(kmx_ctx* ctx, bool append, uint64_t* d_fw, uint64_t* d_rc, const uint8_t* d_bases, uint64_t n,
                    uint32_t k, uint8_t* d_dropped) {
    if (!ctx || (n && (!d_fw || !d_rc || !d_bases))) return KMX_E_ARG;
    if (k < 1 || k > 31) return KMX_E_K_RANGE;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_ck_shift(append, d_fw, d_rc, d_bases, n, k, d_dropped, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_ck_append_bases(kmx_ctx* ctx, uint64_t* d_fw, uint64_t* d_rc, const uint8_t* d_bases, uint64_t n, uint32_t k,
                        uint8_t* d_dropped) {
    return ck_shift(ctx, true, d_fw, d_rc, d_bases, n, k, d_dropped);
}

int kmx_ck_prepend_bases(kmx_ctx* ctx, uint64_t* d_fw, uint64_t* d_rc, const uint8_t* d_bases, uint64_t n, uint32_t k,
                         uint8_t* d_dropped) {
    return ck_shift(ctx, false, d_fw, d_rc, d_bases, n, k, d_dropped);
}

int kmx_encode_kmers(kmx_ctx* ctx, const uint8_t* d_seqs, uint64_t n, uint32_t seq_len, uint8_t enc_byte,
                     uint32_t words_per_kmer, uint64_t* d_words) {
    if (!ctx || (n && ((seq_len && !d_seqs) || !d_words))) return KMX_E_ARG;
    if (!enc_ok(enc_byte) || words_per_kmer < 1 || words_per_kmer > 4) return KMX_E_ARG;
    if (seq_len > 32u * words_per_kmer) return KMX_E_TOO_LONG;  // bit_field set_bits would panic
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_encode_kmers(d_seqs, n, seq_len, enc_byte, words_per_kmer, d_words, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_encode_windows(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, uint8_t enc_byte, uint32_t words_per_kmer,
                       uint64_t* d_words) {
    if (!ctx || !reads_ok(reads) || reads->d_offsets) return KMX_E_ARG;
    if (!enc_ok(enc_byte) || words_per_kmer < 1 || words_per_kmer > 4) return KMX_E_ARG;
    if (k < 1) return KMX_E_K_RANGE;
    if (k > 32u * words_per_kmer) return KMX_E_TOO_LONG;
    if (reads->n_reads == 0 || reads->read_len < k) return KMX_OK;
    if (!d_words) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_encode_windows(reads->d_bases, reads->n_reads, reads->read_len, k, enc_byte, words_per_kmer,
                                            d_words, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_encoding_rev_comp(kmx_ctx* ctx, const uint64_t* d_in, uint64_t n, uint32_t K, uint8_t enc_byte,
                          uint32_t words_per_kmer, uint64_t* d_out) {
    if (!ctx || (n && (!d_in || !d_out))) return KMX_E_ARG;
    if (!enc_ok(enc_byte) || words_per_kmer < 1 || words_per_kmer > 4) return KMX_E_ARG;
    if (K < 2 || K > 32u * words_per_kmer) return KMX_E_K_RANGE;  // K=1 underflows usize in the reference (naive.rs:140,150)
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_encoding_rev_comp(d_in, n, K, comp_lut_for(enc_byte), words_per_kmer, d_out, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_encoding_decode(kmx_ctx* ctx, const uint64_t* d_in, uint64_t n, uint8_t enc_byte, uint32_t words_per_kmer,
                        uint8_t* d_seqs) {
    if (!ctx || (n && (!d_in || !d_seqs))) return KMX_E_ARG;
    if (!enc_ok(enc_byte) || words_per_kmer < 1 || words_per_kmer > 4) return KMX_E_ARG;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_encoding_decode(d_in, n, nuc_lut_for(enc_byte), words_per_kmer, d_seqs, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

/* ------------------------------------------------ decode / display (f3) ---- */

int kmx_sub_kmer_words(kmx_ctx* ctx, const uint64_t* d_words, uint64_t n, uint32_t k, uint32_t pos, uint32_t width,
                       uint64_t* d_out) {
    if (!ctx || (n && (!d_words || !d_out))) return KMX_E_ARG;
    if (k < 1 || k > 32) return KMX_E_K_RANGE;
    if (!(pos < k) || !(pos + width <= k)) return KMX_E_ARG;   // the reference's two asserts (kmer.rs:157-158)
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_sub_kmer_words(d_words, n, pos, width, d_out, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_kmers_to_strings(kmx_ctx* ctx, const uint64_t* d_words, uint64_t n, uint32_t k, uint8_t* d_out) {
    if (!ctx || (n && k && (!d_words || !d_out))) return KMX_E_ARG;
    if (k > 32) return KMX_E_K_RANGE;
    if (n == 0 || k == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_kmers_to_bytes(d_words, n, k, false, d_out, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_bitmers_to_bytes(kmx_ctx* ctx, const uint64_t* d_mers, uint64_t n, uint32_t len, uint8_t* d_out) {
    if (!ctx || (n && len && (!d_mers || !d_out))) return KMX_E_ARG;
    if (len > 32) return KMX_E_K_RANGE;
    if (n == 0 || len == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_kmers_to_bytes(d_mers, n, len, true, d_out, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

/* ------------------------------------------------ Encoding<P, B>, any utils::Data P ---- */

static int p_shape_ok(uint32_t word_bits, uint32_t words_per_kmer, uint32_t* nb) {
    if (word_bits != 8 && word_bits != 16 && word_bits != 32 && word_bits != 64 && word_bits != 128) return KMX_E_ARG;
    if (words_per_kmer < 1) return KMX_E_ARG;
    const uint64_t bytes = (uint64_t)(word_bits / 8u) * words_per_kmer;
    if (bytes > 64) return KMX_E_ARG;
    *nb = (uint32_t)bytes;
    return KMX_OK;
}

int kmx_encode_kmers_p(kmx_ctx* ctx, const uint8_t* d_seqs, uint64_t n, uint32_t seq_len, uint8_t enc_byte, uint32_t word_bits,
                       uint32_t words_per_kmer, void* d_arrays) {
    uint32_t nb = 0;
    if (!ctx || (n && ((seq_len && !d_seqs) || !d_arrays))) return KMX_E_ARG;
    if (!enc_ok(enc_byte)) return KMX_E_ARG;
    if (int st = p_shape_ok(word_bits, words_per_kmer, &nb)) return st;
    if (seq_len > 4u * nb) return KMX_E_TOO_LONG;   // bit_field set_bits would panic (naive.rs:120)
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_encode_kmers_bytes(d_seqs, n, seq_len, enc_byte, nb, static_cast<uint8_t*>(d_arrays), ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_encoding_rev_comp_p(kmx_ctx* ctx, const void* d_in, uint64_t n, uint32_t K, uint8_t enc_byte, uint32_t word_bits,
                            uint32_t words_per_kmer, void* d_out) {
    uint32_t nb = 0;
    if (!ctx || (n && (!d_in || !d_out))) return KMX_E_ARG;
    if (!enc_ok(enc_byte)) return KMX_E_ARG;
    if (int st = p_shape_ok(word_bits, words_per_kmer, &nb)) return st;
    if (K < 2 || K > 4u * nb) return KMX_E_K_RANGE;   // K=1 underflows usize in the reference (naive.rs:140,150)
    if (n == 0) return KMX_OK;
    if (d_in == d_out) return KMX_E_ARG;              // base i reads base K-1-i of the input
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_encoding_rev_comp_bytes(static_cast<const uint8_t*>(d_in), n, K, comp_lut_for(enc_byte), nb,
                                                     static_cast<uint8_t*>(d_out), ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_encoding_decode_p(kmx_ctx* ctx, const void* d_in, uint64_t n, uint8_t enc_byte, uint32_t word_bits,
                          uint32_t words_per_kmer, uint8_t* d_seqs) {
    uint32_t nb = 0;
    if (!ctx || (n && (!d_in || !d_seqs))) return KMX_E_ARG;
    if (!enc_ok(enc_byte)) return KMX_E_ARG;
    if (int st = p_shape_ok(word_bits, words_per_kmer, &nb)) return st;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_encoding_decode_bytes(static_cast<const uint8_t*>(d_in), n * (uint64_t)nb, nuc_lut_for(enc_byte), d_seqs,
                                                   ctx->n_cu, ctx->stream));
    return KMX_OK;
}

/* ------------------------------------------------ measurement helper ---- */

int kmx_calib_stream_read(kmx_ctx* ctx, const uint8_t* d_buf, uint64_t nbytes, uint64_t* d_out) {
    if (!ctx || !d_out || (nbytes && !d_buf)) return KMX_E_ARG;
    if (!aligned16(d_buf)) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, hipMemsetAsync(d_out, 0, 8, ctx->stream));
    if (nbytes < 16) return KMX_OK;
    KMX_HIP(ctx, kmx::launch_calib_stream_read(d_buf, nbytes, reinterpret_cast<unsigned long long*>(d_out), ctx->n_cu, ctx->stream));
    return KMX_OK;
}

/* ------------------------------------------------------------- SeqVector ---- */

int kmx_seqvec_push_chars(kmx_ctx* ctx, uint64_t* d_words, uint64_t n_bases_before, const uint8_t* d_bytes, uint64_t n,
                          uint64_t* h_first_bad) {
    if (!ctx || (n && (!d_words || !d_bytes))) return KMX_E_ARG;
    if (h_first_bad) *h_first_bad = ~0ull;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, first_bad_reset(ctx));
    KMX_HIP(ctx, kmx::launch_seqvec_push(d_words, n_bases_before, d_bytes, n, first_bad_of(ctx), ctx->n_cu, ctx->stream));
    unsigned long long bad = 0;
    if (int st = first_bad_read(ctx, &bad)) return st;
    if (bad != ~0ull) {
        if (h_first_bad) *h_first_bad = bad;
        return KMX_E_INVALID_BASE;
    }
    return KMX_OK;
}

int kmx_seqvec_to_bytes(kmx_ctx* ctx, const uint64_t* d_words, uint64_t n_bases, uint8_t* d_bytes) {
    if (!ctx || (n_bases && (!d_words || !d_bytes))) return KMX_E_ARG;
    if (n_bases == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_seqvec_to_bytes(d_words, n_bases, d_bytes, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_seqvec_get_kmers(kmx_ctx* ctx, const uint64_t* d_words, uint64_t n_bases, const uint64_t* d_pos, uint64_t n,
                         uint32_t k, uint64_t* d_out) {
    if (!ctx || (n && (!d_words || !d_pos || !d_out))) return KMX_E_ARG;
    if (k < 1 || k > 32) return KMX_E_K_RANGE;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, first_bad_reset(ctx));
    KMX_HIP(ctx, kmx::launch_seqvec_get_kmers(d_words, n_bases, d_pos, n, k, d_out, first_bad_of(ctx), ctx->n_cu, ctx->stream));
    unsigned long long bad = 0;
    if (int st = first_bad_read(ctx, &bad)) return st;
    if (bad != ~0ull) {
        std::snprintf(ctx->last_error, sizeof ctx->last_error, "kmx_seqvec_get_kmers: element %llu lies outside the vector", bad);
        return KMX_E_ARG;
    }
    return KMX_OK;
}

int kmx_seqvec_iter_kmers(kmx_ctx* ctx, const uint64_t* d_words, uint64_t n_bases, uint64_t start, uint64_t end, uint32_t k,
                          uint64_t* d_out) {
    if (!ctx || start > end || end > n_bases) return KMX_E_ARG;
    if (k < 1 || k > 32) return KMX_E_K_RANGE;
    if (end - start < k) return KMX_OK;   // the reference's `len - k + 1` underflows here; an empty iteration is the only sane answer
    if (!d_words || !d_out) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_seqvec_iter_kmers(d_words, n_bases, start, end - start - k + 1u, k, d_out, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_seqvec_canonical_reduce(kmx_ctx* ctx, const uint64_t* d_words, uint64_t n_reads, uint32_t read_len, uint32_t k,
                                uint32_t hasher, uint32_t hasher_k, uint32_t flags, kmx_summary* d_out) {
    if (!ctx || !d_out || (n_reads && !d_words)) return KMX_E_ARG;
    if (k < 1 || k > 31) return KMX_E_K_RANGE;   // rolling with MASK_TABLE[32] == 0 is unusable (kmer.rs:617)
    if (hasher > KMX_HASH_IDENTITY) return KMX_E_ARG;
    if (hasher == KMX_HASH_LEX && (hasher_k < 1 || hasher_k > 32)) return KMX_E_K_RANGE;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(kmx_summary), ctx->stream));
    if (n_reads == 0 || read_len < k) return KMX_OK;
    const bool want_hash = hasher != KMX_HASH_NONE, want_sumfw = (flags & KMX_REDUCE_SUM_FW) != 0;
    const bool fix_fold = want_hash && !(hasher == KMX_HASH_LEX && hasher_k == k);   // (as in kmx_canonical_reduce)
    bool handled = false;
    KMX_HIP(ctx, queue_clear(ctx, KMX_Q_CLEAR_HEADS));
    KMX_HIP(ctx, kmx::launch_scan_bitsliced_packed(d_words, n_reads, read_len, k, want_hash, want_sumfw, d_out,
                                                   queue_of(ctx), ctx->n_cu, ctx->stream, &handled));
    if (!handled)
        KMX_HIP(ctx, kmx::launch_reduce_packed_generic(d_words, n_reads, read_len, k, want_hash, want_sumfw, d_out, ctx->n_cu, ctx->stream));
    if (fix_fold) KMX_HIP(ctx, kmx::launch_fix_hash_fold(d_out, k, hasher, hasher_k, ctx->stream));
    return KMX_OK;
}

/* ------------------------------------------------------------- minimizers ---- */

static int mm_hasher_ok(uint32_t hasher, uint32_t hasher_k) {
    if (hasher == KMX_HASH_IDENTITY) return KMX_OK;
    if (hasher != KMX_HASH_LEX) return KMX_E_ARG;
    return (hasher_k >= 1 && hasher_k <= 32) ? KMX_OK : KMX_E_K_RANGE;
}

int kmx_minimizer_words(kmx_ctx* ctx, const uint64_t* d_words, uint64_t n, uint32_t k, uint32_t width, uint32_t hasher,
                        uint32_t hasher_k, uint64_t* d_mmer, uint32_t* d_offset) {
    if (!ctx || (n && (!d_words || !d_mmer || !d_offset))) return KMX_E_ARG;
    if (k < 1 || k > 32 || width < 1 || width > k) return KMX_E_K_RANGE;   // sub_kmer_word asserts pos + width <= k
    if (int st = mm_hasher_ok(hasher, hasher_k)) return st;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_minimizer_words(d_words, n, k, width, hasher, hasher_k, d_mmer, d_offset, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_seqvec_minimizers(kmx_ctx* ctx, const uint64_t* d_words, uint64_t n_reads, uint32_t read_len, uint32_t k, uint32_t w,
                          uint32_t hasher, uint32_t hasher_k, uint64_t* d_word, uint32_t* d_pos) {
    if (!ctx || (n_reads && (!d_words || !d_word || !d_pos))) return KMX_E_ARG;
    if (k < 1 || w < 1 || w > k || w > 32) return KMX_E_K_RANGE;
    if (read_len < k) return KMX_E_ARG;   // SeqVecMinimizerIter::new: assert!(sv.len() >= k)
    if (int st = mm_hasher_ok(hasher, hasher_k)) return st;
    if (n_reads == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_seqvec_minimizers(d_words, n_reads, read_len, k, w, hasher, hasher_k, d_word, d_pos, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

// The argument checks of kmx_minimizers and kmx_minimizers_sip13, in their order (`hasher_st`: what the hasher's own check said,
// which counts after the k range).  -1: go on; anything else is the status to return.
static int minimizers_args(const kmx_ctx* ctx, const kmx_reads* reads, const uint64_t* d_win_offsets, uint32_t k, uint32_t w, int hasher_st,
                           const uint64_t* d_word, const uint32_t* d_pos, uint64_t* h_first_bad) {
    if (!ctx || !reads_ok(reads)) return KMX_E_ARG;
    if (k < 1 || w < 1 || w > k || w > 32) return KMX_E_K_RANGE;
    if (hasher_st != KMX_OK) return hasher_st;
    if (h_first_bad) *h_first_bad = ~0ull;
    if (reads->n_reads == 0) return KMX_OK;
    if (!d_word || !d_pos) return KMX_E_ARG;
    if (reads->d_offsets && !d_win_offsets) return KMX_E_ARG;
    if (!reads->d_offsets && reads->read_len < k) return KMX_E_ARG;   // SeqVecMinimizerIter::new: assert!(sv.len() >= k) (a ragged read shorter than k owns no slot)
    return -1;
}

int kmx_minimizers(kmx_ctx* ctx, const kmx_reads* reads, const uint64_t* d_win_offsets, uint32_t k, uint32_t w, uint32_t hasher,
                   uint32_t hasher_k, uint64_t* d_word, uint32_t* d_pos, uint64_t* h_first_bad) {
    const int args = minimizers_args(ctx, reads, d_win_offsets, k, w, mm_hasher_ok(hasher, hasher_k), d_word, d_pos, h_first_bad);
    if (args >= 0) return args;
    DeviceGuard g(ctx->device);
    uint64_t total_bytes = reads->n_reads * (uint64_t)reads->read_len;
    uint32_t bound = reads->read_len;
    if (reads->d_offsets) {
        // the batch's last byte and its longest read (the bound of kmx_reads is a hint; the key of the sliding minimum holds 8 bits
        // of position): one host round trip
        uint32_t lo = 0, hi = 0;
        if (int st = kmx_reads_length_range(ctx, reads->d_offsets, reads->n_reads, &lo, &hi)) return st;
        KMX_HIP(ctx, hipMemcpyAsync(ctx->h_pinned + KMX_PIN_READ, reads->d_offsets + reads->n_reads, 8, hipMemcpyDeviceToHost, ctx->stream));
        KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        total_bytes = ctx->h_pinned[KMX_PIN_READ];
        bound = hi;
        if (hi < k) return KMX_OK;      // no read holds a k-mer
    }
    KMX_HIP(ctx, first_bad_reset(ctx));
    bool tiled = false;
    KMX_HIP(ctx, kmx::launch_minimizers_reads(reads->d_bases, total_bytes, reads->d_offsets, d_win_offsets, reads->n_reads, reads->read_len, bound, k, w,
                                              hasher, hasher_k, d_word, d_pos, first_bad_of(ctx), ctx->n_cu, ctx->stream, &tiled));
    if (!h_first_bad) return KMX_OK;
    if (int st = first_bad_read(ctx, ctx->h_pinned + KMX_PIN_READ)) return st;
    if (ctx->h_pinned[KMX_PIN_READ] != ~0ull) {
        *h_first_bad = ctx->h_pinned[KMX_PIN_READ];
        return KMX_E_INVALID_BASE;
    }
    return KMX_OK;
}

/* ------------------------------------------------- SipHash-1-3 (std's DefaultHasher / RandomState) ---- */
// The counterparts of kmx_canonical_reduce, kmx_histogram and the three minimizer calls with the hash SipHash-1-3(key0, key1; the
// word's 8 little-endian bytes) -- kmx_hash_words_sip13's.  Same domains, layouts, slots, codes and synchronisation as the
// counterpart; the kernels are their own (the Lex / identity instantiations are untouched).

int kmx_canonical_reduce_sip13(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, uint64_t key0, uint64_t key1, uint32_t flags,
                               kmx_summary* d_out) {
    if (!ctx || !reads_ok(reads) || !d_out) return KMX_E_ARG;
    if (k < 1 || k > 31) return KMX_E_K_RANGE;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(kmx_summary), ctx->stream));
    if (reads->n_reads == 0) return KMX_OK;
    const bool want_sumfw = (flags & KMX_REDUCE_SUM_FW) != 0;
    // (the ticket heads are cleared unconditionally: this scan does not put them back, and a captured graph must hold the clear)
    KMX_HIP(ctx, queue_clear(ctx, KMX_Q_CLEAR_THROUGH_GATE));
    bool handled = false;
    KMX_HIP(ctx, kmx::launch_scan_reduce_sip(reads->d_bases, reads->n_reads, reads->read_len, k, key0, key1, want_sumfw, d_out,
                                             queue_of(ctx), ctx->n_cu, ctx->stream, &handled, reads->d_offsets));
    if (handled) return KMX_OK;
    // k = 1, reads above 256 bases, a misaligned ragged d_bases: a lane per read
    KMX_HIP(ctx, kmx::launch_reduce_generic_sip(reads, k, key0, key1, want_sumfw ? 1u : 0u, d_out, ctx->n_cu, ctx->stream, too_long_of(ctx)));
    return KMX_OK;
}

int kmx_histogram_sip13(kmx_ctx* ctx, const kmx_reads* reads, uint32_t k, uint64_t key0, uint64_t key1, uint32_t log2_buckets,
                        uint64_t* d_counts) {
    if (!ctx || !reads_ok(reads) || !d_counts) return KMX_E_ARG;
    if (k < 1 || k > 31) return KMX_E_K_RANGE;
    if (log2_buckets > 30) return KMX_E_ARG;
    if (reads->n_reads == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, queue_clear(ctx, KMX_Q_CLEAR_THROUGH_GATE));
    bool handled = false;
    // the routes of kmx_histogram (LDS tables, one- and two-level partitions, device atomics) with the SipHash sinks
    KMX_HIP(ctx, kmx::launch_hist_uniform(reads->d_bases, reads->n_reads, reads->read_len, k, kmx::KMX_HASH_SIP13_INTERNAL, 0u, log2_buckets,
                                          d_counts, queue_of(ctx), ctx->n_cu, ctx->stream, &handled, &work_callback, ctx,
                                          work_budget(ctx), reads->d_offsets, key0, key1));
    if (handled) return KMX_OK;
    KMX_HIP(ctx, kmx::launch_histogram_generic_sip(reads, k, key0, key1, log2_buckets, d_counts, ctx->n_cu, ctx->stream, too_long_of(ctx)));
    return KMX_OK;
}

int kmx_minimizer_words_sip13(kmx_ctx* ctx, const uint64_t* d_words, uint64_t n, uint32_t k, uint32_t width, uint64_t key0,
                              uint64_t key1, uint64_t* d_mmer, uint32_t* d_offset) {
    if (!ctx || (n && (!d_words || !d_mmer || !d_offset))) return KMX_E_ARG;
    if (k < 1 || k > 32 || width < 1 || width > k) return KMX_E_K_RANGE;   // sub_kmer_word asserts pos + width <= k
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_minimizer_words_sip(d_words, n, k, width, key0, key1, d_mmer, d_offset, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_seqvec_minimizers_sip13(kmx_ctx* ctx, const uint64_t* d_words, uint64_t n_reads, uint32_t read_len, uint32_t k, uint32_t w,
                                uint64_t key0, uint64_t key1, uint64_t* d_word, uint32_t* d_pos) {
    if (!ctx || (n_reads && (!d_words || !d_word || !d_pos))) return KMX_E_ARG;
    if (k < 1 || w < 1 || w > k || w > 32) return KMX_E_K_RANGE;
    if (read_len < k) return KMX_E_ARG;   // SeqVecMinimizerIter::new: assert!(sv.len() >= k)
    if (n_reads == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_seqvec_minimizers_sip(d_words, n_reads, read_len, k, w, key0, key1, d_word, d_pos, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_minimizers_sip13(kmx_ctx* ctx, const kmx_reads* reads, const uint64_t* d_win_offsets, uint32_t k, uint32_t w, uint64_t key0,
                         uint64_t key1, uint64_t* d_word, uint32_t* d_pos, uint64_t* h_first_bad) {
    const int args = minimizers_args(ctx, reads, d_win_offsets, k, w, KMX_OK, d_word, d_pos, h_first_bad);
    if (args >= 0) return args;
    DeviceGuard g(ctx->device);
    if (reads->d_offsets) {
        // as kmx_minimizers: a batch without a read of k bases returns here (one host round trip for its longest read)
        uint32_t lo = 0, hi = 0;
        if (int st = kmx_reads_length_range(ctx, reads->d_offsets, reads->n_reads, &lo, &hi)) return st;
        if (hi < k) return KMX_OK;
    }
    KMX_HIP(ctx, first_bad_reset(ctx));
    KMX_HIP(ctx, kmx::launch_minimizers_reads_sip(reads->d_bases, reads->d_offsets, d_win_offsets, reads->n_reads, reads->read_len, k, w, key0,
                                                  key1, d_word, d_pos, first_bad_of(ctx), ctx->n_cu, ctx->stream));
    if (!h_first_bad) return KMX_OK;
    if (int st = first_bad_read(ctx, ctx->h_pinned + KMX_PIN_READ)) return st;
    if (ctx->h_pinned[KMX_PIN_READ] != ~0ull) {
        *h_first_bad = ctx->h_pinned[KMX_PIN_READ];
        return KMX_E_INVALID_BASE;
    }
    return KMX_OK;
}

// ---- FASTQ / FASTA text parsed on the device (kmx_fastx.hip) ----
// What the three parse calls differ in.  The lines of a FASTQ record are selected by the line the machine is entered on: passes 2 and 3
// take line 1 (entry 0: the reads), line 3 (entry 2: the quality lines) or line 0 (entry 1: the names).
struct FastxCall {
    const char* who;
    const char* what;    // the lines, for the messages
    uint32_t entry;
    bool fasta_too;      // FASTA is taken as well, and KMX_FASTX_AUTO tells the two apart by the first byte; otherwise FASTQ only
    bool any_entry;      // KMX_FASTX_SAME_TEXT may keep pass 1 of a count made for another entry and rerun pass 2 alone
};
static const FastxCall kFastxReads{"kmx_fastx_parse", "reads", 0u, true, false};
static const FastxCall kFastxQuals{"kmx_fastx_parse_quals", "quality lines", 2u, false, true};
static const FastxCall kFastxNames{"kmx_fastx_parse_names", "names", 1u, false, true};

// The one body of the parse calls: the argument checks (behind them *h_reset = ~0, if given), the count and -- with room -- the launch
// of pass 3, which is left running: *emitted says so.  What the context remembers of a count (fx_*, written here and nowhere else) is
// shared by the three calls: the chunk summaries of pass 1 do not depend on the entry line, the chunk prefixes and totals of pass 2 do
// (fx_entry).  They live in the work buffer, so they are as good as fx_valid, which work_acquire clears for every other taker.
static int fastx_lines(kmx_ctx* ctx, const FastxCall& call, const uint8_t* d_text, uint64_t n_bytes, uint32_t format, uint8_t* d_out,
                       uint64_t* d_ooffsets, uint64_t max_reads, uint64_t* h_n_reads, uint64_t* h_n_bytes, uint64_t* h_reset, uint64_t* n_lines,
                       bool* emitted) {
    *emitted = false;
    const bool same_text = (format & KMX_FASTX_SAME_TEXT) != 0u;
    format &= ~KMX_FASTX_SAME_TEXT;
    if (!ctx || format > (call.fasta_too ? KMX_FASTX_FASTA : KMX_FASTX_FASTQ) || (n_bytes && !d_text) || (!d_out != !d_ooffsets)) return KMX_E_ARG;
    if (!aligned16(d_text)) return KMX_E_ARG;
    if (h_n_reads) *h_n_reads = 0;
    if (h_n_bytes) *h_n_bytes = 0;
    if (h_reset) *h_reset = ~0ull;
    DeviceGuard g(ctx->device);
    if (n_bytes == 0) {
        if (d_ooffsets) {
            KMX_HIP(ctx, hipMemsetAsync(d_ooffsets, 0, 8, ctx->stream));
            KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        return KMX_OK;
    }
    if (!call.fasta_too) format = KMX_FASTX_FASTQ;
    // (the emit call of a counts-then-emit pair: the counting call looked at the first byte and settled the format)
    const bool known = same_text && ctx->fx_valid && ctx->fx_text == d_text && ctx->fx_bytes == n_bytes &&
                       (format == KMX_FASTX_AUTO || ctx->fx_fasta == (format == KMX_FASTX_FASTA ? 1u : 0u)) &&
                       (call.any_entry || ctx->fx_entry == call.entry);
    if (known) {
        format = ctx->fx_fasta ? KMX_FASTX_FASTA : KMX_FASTX_FASTQ;
    } else {
        uint8_t first = 0;
        KMX_HIP(ctx, hipMemcpyAsync(&first, d_text, 1, hipMemcpyDeviceToHost, ctx->stream));
        KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (format == KMX_FASTX_AUTO) format = first == '@' ? KMX_FASTX_FASTQ : first == '>' ? KMX_FASTX_FASTA : 3u;
        if (format == 3u || first != (format == KMX_FASTX_FASTQ ? '@' : '>')) {
            std::snprintf(ctx->last_error, sizeof ctx->last_error, "%s: the text starts with byte 0x%02x, not with '@' (FASTQ)%s", call.who, first,
                          call.fasta_too ? " or '>' (FASTA)" : "");
            return KMX_E_ARG;
        }
    }
    const bool fasta = format == KMX_FASTX_FASTA;
    void* scratch = work_acquire(ctx, kmx::fastx_scratch_bytes(n_bytes), true).base;
    if (!scratch) return KMX_E_NOMEM;
    unsigned long long* d_totals = ctx->d_scratch + KMX_S_FASTX_TOTALS;
    unsigned long long totals[2] = {0, 0};
    const bool summaries = known && ctx->fx_valid;   // the work buffer did not move: pass 1 of the earlier count of this text is still in it
    if (summaries && ctx->fx_entry == call.entry) {
        // ... and so are the chunk prefixes of its pass 2, its totals in d_scratch[KMX_S_FASTX_TOTALS]
        totals[0] = ctx->fx_totals[0];
        totals[1] = ctx->fx_totals[1];
    } else {
        ctx->fx_valid = false;
        KMX_HIP(ctx, kmx::launch_fastx_count(d_text, n_bytes, fasta, scratch, d_totals, ctx->stream, call.entry, !summaries));
        KMX_HIP(ctx, hipMemcpyAsync(totals, d_totals, 16, hipMemcpyDeviceToHost, ctx->stream));
        KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->fx_text = d_text;
        ctx->fx_bytes = n_bytes;
        ctx->fx_fasta = fasta ? 1u : 0u;
        ctx->fx_entry = call.entry;
        ctx->fx_totals[0] = totals[0];
        ctx->fx_totals[1] = totals[1];
        ctx->fx_valid = true;
    }
    if (h_n_reads) *h_n_reads = totals[0];
    if (h_n_bytes) *h_n_bytes = totals[1];
    *n_lines = totals[0];
    if (!d_out) return KMX_OK;
    if (int st = room_for(ctx, call.who, totals[0], call.what, max_reads)) return st;
    KMX_HIP(ctx, kmx::launch_fastx_emit(d_text, n_bytes, fasta, scratch, d_totals, d_out, d_ooffsets, ctx->stream, call.entry));
    *emitted = true;
    return KMX_OK;
}

// ... and the wait for pass 3, where nothing else follows it.
static int fastx_lines_wait(kmx_ctx* ctx, const FastxCall& call, const uint8_t* d_text, uint64_t n_bytes, uint32_t format, uint8_t* d_out,
                            uint64_t* d_ooffsets, uint64_t max_reads, uint64_t* h_n_reads, uint64_t* h_n_bytes) {
    uint64_t n_lines = 0;
    bool emitted = false;
    const int st = fastx_lines(ctx, call, d_text, n_bytes, format, d_out, d_ooffsets, max_reads, h_n_reads, h_n_bytes, nullptr, &n_lines, &emitted);
    if (st != KMX_OK || !emitted) return st;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMX_OK;
}

int kmx_fastx_parse(kmx_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, uint32_t format, uint8_t* d_bases,
                    uint64_t* d_offsets, uint64_t max_reads, uint64_t* h_n_reads, uint64_t* h_n_bases) {
    return fastx_lines_wait(ctx, kFastxReads, d_text, n_bytes, format, d_bases, d_offsets, max_reads, h_n_reads, h_n_bases);
}

int kmx_fastx_parse_quals(kmx_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, uint32_t format, uint8_t* d_quals, uint64_t* d_qoffsets,
                          uint64_t max_reads, const uint64_t* d_read_offsets, uint64_t* h_n_reads, uint64_t* h_n_bytes, uint64_t* h_first_mismatch) {
    uint64_t n_lines = 0;
    bool emitted = false;
    const int st = fastx_lines(ctx, kFastxQuals, d_text, n_bytes, format, d_quals, d_qoffsets, max_reads, h_n_reads, h_n_bytes, h_first_mismatch,
                               &n_lines, &emitted);
    if (st != KMX_OK || !emitted) return st;
    DeviceGuard g(ctx->device);
    if (d_read_offsets && h_first_mismatch && n_lines) {
        KMX_HIP(ctx, first_bad_reset(ctx));
        KMX_HIP(ctx, kmx::launch_fastx_length_mismatch(d_qoffsets, d_read_offsets, n_lines, first_bad_of(ctx), ctx->n_cu, ctx->stream));
        if (int st2 = first_bad_read(ctx, ctx->h_pinned + KMX_PIN_READ)) return st2;
        *h_first_mismatch = ctx->h_pinned[KMX_PIN_READ];
        return KMX_OK;
    }
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMX_OK;
}

int kmx_fastx_parse_names(kmx_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, uint32_t format, uint8_t* d_names, uint64_t* d_noffsets,
                          uint64_t max_reads, uint64_t* h_n_names, uint64_t* h_n_bytes) {
    return fastx_lines_wait(ctx, kFastxNames, d_text, n_bytes, format, d_names, d_noffsets, max_reads, h_n_names, h_n_bytes);
}

// ---- BGZF-compressed images (kmx_bgzf.hip) ----
int kmx_bgzf_index(kmx_ctx* ctx, const uint8_t* d_file, uint64_t n_bytes, uint64_t* d_block_offsets, uint64_t* d_text_offsets, uint64_t max_blocks,
                   uint64_t* h_info) {
    const char* who = "kmx_bgzf_index";
    if (!ctx || !h_info || (n_bytes && !d_file) || (!d_block_offsets != !d_text_offsets)) return KMX_E_ARG;
    h_info[0] = h_info[1] = h_info[3] = 0;
    h_info[2] = n_bytes;
    DeviceGuard g(ctx->device);
    uint64_t n_blocks = 0, n_text = 0, end = 0, last_start = 0;
    uint32_t n_cand = 0;
    void* area = nullptr;
    if (n_bytes) {
        uint8_t head[18] = {0};
        if (n_bytes >= sizeof head) {
            KMX_HIP(ctx, hipMemcpyAsync(head, d_file, sizeof head, hipMemcpyDeviceToHost, ctx->stream));
            KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        static const uint8_t kAt[10] = {0, 1, 2, 3, 10, 11, 12, 13, 14, 15}, kIs[10] = {0x1f, 0x8b, 8, 4, 6, 0, 'B', 'C', 2, 0};
        bool is = n_bytes >= sizeof head;
        for (int i = 0; i < 10; ++i) is = is && head[kAt[i]] == kIs[i];
        if (!is) {
            std::snprintf(ctx->last_error, sizeof ctx->last_error,
                          "%s: the image does not begin with a BGZF block header (plain gzip and plain text are not BGZF; bgzip writes it)", who);
            return KMX_E_ARG;
        }
        // the counting pass in the small front of the layout, then -- the candidates known -- the whole; a buffer that moved in between
        // has lost the counts
        WorkHold first;
        if (int st = work_area(ctx, who, kmx::bgzf_index_units_bytes(n_bytes), &area, &first)) return st;
        unsigned long long cand = 0;
        for (int pass = 0; pass < 2; ++pass) {
            KMX_HIP(ctx, kmx::launch_bgzf_count_candidates(d_file, n_bytes, area, ctx->n_cu, ctx->stream));
            KMX_HIP(ctx, hipMemcpyAsync(&cand, static_cast<unsigned long long*>(area) + 2, 8, hipMemcpyDeviceToHost, ctx->stream));
            KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (pass == 1) break;
            if (cand >= 0xFFFFFFF0ull) {
                std::snprintf(ctx->last_error, sizeof ctx->last_error, "%s: %llu header patterns in the image", who, cand);
                return KMX_E_NOMEM;
            }
            WorkHold whole;
            if (int st = work_area(ctx, who, kmx::bgzf_index_scratch_bytes(n_bytes, cand), &area, &whole)) return st;
            if (whole.base == first.base && whole.allocs == first.allocs) break;
        }
        n_cand = (uint32_t)cand;
        if (n_cand) {
            unsigned long long stats[6] = {0, 0, 0, 0, 0, 0};
            KMX_HIP(ctx, kmx::launch_bgzf_chain(d_file, n_bytes, area, n_cand, ctx->n_cu, ctx->stream));
            KMX_HIP(ctx, hipMemcpyAsync(stats, area, sizeof stats, hipMemcpyDeviceToHost, ctx->stream));
            KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
            n_text = stats[0];
            end = stats[1];
            n_blocks = stats[3];
            last_start = stats[5];
        }
        if (n_blocks && end >= 28u) {
            static const uint8_t kEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            uint8_t tail[28];
            KMX_HIP(ctx, hipMemcpyAsync(tail, d_file + end - 28u, sizeof tail, hipMemcpyDeviceToHost, ctx->stream));
            KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
            h_info[3] = end - last_start == 28u && std::memcmp(tail, kEof, sizeof tail) == 0 ? 1u : 0u;
        }
    }
    h_info[0] = n_blocks;
    h_info[1] = n_text;
    h_info[2] = n_bytes - end;
    if (!d_block_offsets) return KMX_OK;
    if (int st = room_for(ctx, who, n_blocks, "blocks", max_blocks)) return st;
    if (n_blocks == 0) {
        KMX_HIP(ctx, hipMemsetAsync(d_block_offsets, 0, 8, ctx->stream));
        KMX_HIP(ctx, hipMemsetAsync(d_text_offsets, 0, 8, ctx->stream));
    } else {
        KMX_HIP(ctx, kmx::launch_bgzf_write_index(d_file, n_bytes, area, n_cand, n_blocks, end, d_block_offsets, d_text_offsets, ctx->n_cu, ctx->stream));
    }
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMX_OK;
}

int kmx_bgzf_inflate(kmx_ctx* ctx, const uint8_t* d_file, uint64_t n_bytes, const uint64_t* d_block_offsets, const uint64_t* d_text_offsets,
                     uint64_t n_blocks, uint32_t flags, uint8_t* d_text, uint64_t text_capacity, uint32_t* d_status, uint64_t* h_first_bad) {
    const char* who = "kmx_bgzf_inflate";
    if (!ctx || (flags & ~(uint32_t)KMX_BGZF_NO_CRC) || (n_blocks && (!d_file || !d_block_offsets || !d_text_offsets)) || !aligned16(d_text) ||
        n_blocks > (1ull << 32))
        return KMX_E_ARG;
    if (h_first_bad) *h_first_bad = ~0ull;
    if (n_blocks == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    uint64_t t0 = 0, t1 = 0;
    KMX_HIP(ctx, hipMemcpyAsync(&t0, d_text_offsets, 8, hipMemcpyDeviceToHost, ctx->stream));
    KMX_HIP(ctx, hipMemcpyAsync(&t1, d_text_offsets + n_blocks, 8, hipMemcpyDeviceToHost, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (t1 < t0) return KMX_E_ARG;
    const uint64_t span = t1 - t0;
    if (int st = room_for(ctx, who, span, "bytes of text", text_capacity)) return st;
    if (span && !d_text) return KMX_E_ARG;
    uint32_t* status = d_status;
    if (!status) {
        void* area = nullptr;
        if (int st = work_area(ctx, who, (size_t)n_blocks * 4u, &area)) return st;
        status = static_cast<uint32_t*>(area);
    }
    KMX_HIP(ctx, first_bad_reset(ctx));
    KMX_HIP(ctx, kmx::launch_bgzf_inflate(d_file, n_bytes, d_block_offsets, d_text_offsets, n_blocks, span, d_text, status, first_bad_of(ctx),
                                          (flags & KMX_BGZF_NO_CRC) == 0u, ctx->stream));
    if (int st = first_bad_read(ctx, ctx->h_pinned + KMX_PIN_READ)) return st;
    const unsigned long long bad = ctx->h_pinned[KMX_PIN_READ];
    if (h_first_bad) *h_first_bad = bad;
    if (bad == ~0ull) return KMX_OK;
    uint32_t why = 0;
    KMX_HIP(ctx, hipMemcpyAsync(&why, status + bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::snprintf(ctx->last_error, sizeof ctx->last_error, "%s: block %llu is not sound (KMX_BGZF_ST_* reason %u)", who, bad, why);
    return KMX_E_ARG;
}

// ---- a text compressed to BGZF (kmx_bgzf.hip) ----
uint64_t kmx_bgzf_deflate_bound(uint64_t n_bytes, uint32_t block_bytes) {
    if (block_bytes > 65280u) return 0;
    const uint64_t bb = block_bytes ? block_bytes : 65280u;
    const uint64_t whole = n_bytes / bb, rest = n_bytes % bb;      // per piece: header and footer, and zlib's level-0 stored form
    return n_bytes + whole * (bb < 32768u ? 31u : 36u) + (rest ? (rest < 32768u ? 31u : 36u) : 0u) + 28u;
}

int kmx_bgzf_deflate(kmx_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, uint32_t block_bytes, uint32_t flags, uint8_t* d_file,
                     uint64_t file_capacity, uint64_t* d_block_offsets, uint64_t* h_info) {
    const char* who = "kmx_bgzf_deflate";
    if (!ctx || !h_info || (flags & ~(uint32_t)KMX_BGZF_DEFLATE_STORED) || (n_bytes && !d_text) || n_bytes >= (1ull << 44) || block_bytes > 65280u)
        return KMX_E_ARG;
    const uint32_t bb = block_bytes ? block_bytes : 65280u;
    const uint64_t pieces = (n_bytes + bb - 1u) / bb;
    h_info[0] = pieces + 1u;
    h_info[1] = h_info[2] = 0;
    h_info[3] = n_bytes;
    DeviceGuard g(ctx->device);
    // the per-piece words, and as many slots behind them as the cap holds: all pieces, or chunks of them
    const uint32_t slot = (flags & KMX_BGZF_DEFLATE_STORED) || pieces == 0 ? 0u : kmx::bgzf_deflate_slot_bytes(bb);   // (no text: the marker alone)
    const size_t meta = kmx::bgzf_deflate_meta_bytes(pieces), budget = work_budget(ctx);
    uint64_t chunk = pieces;
    if (slot && pieces && meta < budget && (budget - meta) / slot < pieces) chunk = (budget - meta) / slot;
    void* area = nullptr;
    if (int st = work_area(ctx, who, meta + (size_t)(chunk ? chunk : 1u) * slot, &area)) return st;   // (not one slot under the cap: refused here)
    KMX_HIP(ctx, hipMemsetAsync(area, 0, 256, ctx->stream));
    for (uint64_t b0 = 0; b0 < pieces; b0 += chunk)
        KMX_HIP(ctx, kmx::launch_bgzf_deflate_blocks(d_text, n_bytes, bb, pieces, b0, b0 + chunk < pieces ? b0 + chunk : pieces, slot, true, area, ctx->n_cu,
                                                     ctx->stream));
    KMX_HIP(ctx, kmx::launch_bgzf_deflate_offsets(pieces, area, ctx->stream));
    unsigned long long stats[2] = {0, 0};
    KMX_HIP(ctx, hipMemcpyAsync(stats, area, sizeof stats, hipMemcpyDeviceToHost, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    h_info[1] = stats[0];
    h_info[2] = stats[1];
    if (d_file) {
        if (int st = room_for(ctx, who, stats[0], "bytes of image", file_capacity)) return st;
        if (chunk >= pieces) {
            KMX_HIP(ctx, kmx::launch_bgzf_deflate_copy(d_text, n_bytes, bb, pieces, 0, 0, pieces + 1u, slot, area, stats[0], d_file, ctx->n_cu, ctx->stream));
        } else {
            // the slots held a chunk at a time and the size had to be known before the first byte: every chunk coded again, then written
            for (uint64_t b0 = 0; b0 < pieces; b0 += chunk) {
                const uint64_t b1 = b0 + chunk < pieces ? b0 + chunk : pieces;
                KMX_HIP(ctx, kmx::launch_bgzf_deflate_blocks(d_text, n_bytes, bb, pieces, b0, b1, slot, false, area, ctx->n_cu, ctx->stream));
                KMX_HIP(ctx, kmx::launch_bgzf_deflate_copy(d_text, n_bytes, bb, pieces, b0, b0, b1 == pieces ? pieces + 1u : b1, slot, area,
                                                           (b1 - b0 + 1u) * (bb + 31ull), d_file, ctx->n_cu, ctx->stream));
            }
        }
    }
    if (d_block_offsets)
        KMX_HIP(ctx, hipMemcpyAsync(d_block_offsets, kmx::bgzf_deflate_offsets(area), (size_t)(pieces + 2u) * 8u, hipMemcpyDeviceToDevice, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMX_OK;
}

// ---- a batch laid out as a FASTQ / FASTA image (kmx_fastx_format.hip) ----
int kmx_fastx_format(kmx_ctx* ctx, const kmx_reads* reads, const uint8_t* d_quals, const kmx_reads* names, uint32_t name_skip, uint64_t name_base,
                     uint32_t format, uint32_t line_width, uint32_t qual_fill, uint8_t* d_text, uint64_t* d_rec_offsets, uint64_t max_bytes,
                     uint64_t* h_n_bytes) {
    const char* who = "kmx_fastx_format";
    if (!ctx || !reads_ok(reads) || !h_n_bytes || !reads_batch_ok(reads)) return KMX_E_ARG;
    if (format != KMX_FASTX_FASTQ && format != KMX_FASTX_FASTA) return KMX_E_ARG;
    const bool fastq = format == KMX_FASTX_FASTQ;
    if (fastq && (line_width != 0u || (!d_quals && qual_fill > 255u))) return KMX_E_ARG;
    if (names && (!reads_ok(names) || !reads_batch_ok(names) || names->n_reads != reads->n_reads)) return KMX_E_ARG;
    *h_n_bytes = 0;
    const uint64_t n = reads->n_reads;
    if (n == 0) return KMX_OK;
    const kmx::FastxFormat f{reads->d_bases, reads->d_offsets, n, reads->read_len, fastq ? d_quals : nullptr, names ? names->d_bases : nullptr,
                             names ? names->d_offsets : nullptr, names ? names->read_len : 0u, name_skip, name_base, line_width, qual_fill & 255u,
                             names != nullptr, fastq};
    DeviceGuard g(ctx->device);
    const bool own_offsets = !d_rec_offsets;
    void* area = nullptr;
    if (int st = work_area(ctx, who, kmx::fastx_format_bytes(n, own_offsets), &area)) return st;
    uint64_t h[6] = {0, 0, 0, 0, 0, 0};   // records, bytes of the image, the first and last offset of the reads and of the names
    KMX_HIP(ctx, kmx::launch_fastx_format_count(f, area, own_offsets, ctx->h_pinned, h, ctx->stream));
    *h_n_bytes = h[1];
    if (!d_text && !d_rec_offsets) return KMX_OK;
    if (d_text) {
        if (int st = room_for(ctx, who, h[1], "bytes", max_bytes)) return st;
        if (h[1] >= (1ull << 44)) {   // (the copy is one grid of a block per 64 KiB)
            std::snprintf(ctx->last_error, sizeof ctx->last_error, "%s: %llu bytes in one image", who, (unsigned long long)h[1]);
            return KMX_E_NOMEM;
        }
        // the bytes the three sources span, and the record offsets, against the bytes that are written
        const Range out = Range::of_bytes(d_text, h[1]);
        if (Range::of_batch(f.bases, f.offsets, n, f.read_len, h[2], h[3]).overlaps(out)) return KMX_E_ARG;
        if (Range::of_batch(f.quals, f.offsets, n, f.read_len, h[2], h[3]).overlaps(out)) return KMX_E_ARG;
        if (names && Range::of_batch(f.names, f.name_offsets, n, f.name_len, h[4], h[5]).overlaps(out)) return KMX_E_ARG;
        if (Range::of_words(d_rec_offsets, n + 1u).overlaps(out)) return KMX_E_ARG;
    }
    KMX_HIP(ctx, kmx::launch_fastx_format_emit(f, area, own_offsets, d_rec_offsets, h[1], d_text, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMX_OK;
}

// ---- the masked copies of a batch (kmx_reads_quality, kmx_reads_complexity) ----
// The bytes the batch spans (ragged: its first and last offset, one round trip) against the bytes of d_masked that are written:
// KMX_E_ARG unless d_masked is d_bases itself (in place) or clear of the bases, and clear of `d_also` -- bytes laid out as the
// bases are, which the call reads on a dword grid of their own (the quality bytes; nullptr: there are none).
static int masked_copy_ok(kmx_ctx* ctx, const kmx_reads* reads, const uint8_t* d_masked, const uint8_t* d_also) {
    uint64_t first = 0, last = 0;
    if (reads->d_offsets)
        if (int st = offsets_span(ctx, reads, &first, &last)) return st;
    auto spanned = [&](const void* base) { return Range::of_batch(base, reads->d_offsets, reads->n_reads, reads->read_len, first, last); };
    const Range m = spanned(d_masked);
    if (d_masked != reads->d_bases && m.overlaps(spanned(reads->d_bases))) return KMX_E_ARG;
    if (m.overlaps(spanned(d_also))) return KMX_E_ARG;
    return KMX_OK;
}

// ---- the quality bytes of a batch acted on (kmx_reads_quality.hip) ----
int kmx_reads_quality(kmx_ctx* ctx, const kmx_reads* reads, const uint8_t* d_quals, uint32_t phred_base, uint32_t min_q, uint32_t trim_q, uint32_t k,
                      const uint64_t* d_weights, uint8_t* d_masked, uint64_t* d_rows) {
    if (!ctx || !reads_ok(reads) || phred_base > 255u || min_q > 255u || trim_q > 255u || (!d_masked && !d_rows)) return KMX_E_ARG;
    if (!reads_batch_ok(reads)) return KMX_E_ARG;
    if (reads->n_reads == 0) return KMX_OK;
    const bool bytes = reads->d_offsets || reads->read_len;   // (uniform reads of no bases: rows of zeros, nothing is read)
    if (bytes && !d_quals) return KMX_E_ARG;
    DeviceGuard g(ctx->device);
    if (bytes && d_masked)
        if (int st = masked_copy_ok(ctx, reads, d_masked, d_quals)) return st;
    const kmx::ReadsQuality a{reads->d_bases, reads->d_offsets, reads->n_reads, reads->read_len, d_quals, phred_base, min_q, trim_q, k, d_weights,
                              d_masked, d_rows};
    KMX_HIP(ctx, kmx::launch_reads_quality(a, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

// ---- adapter read-through (kmx_reads_adapter.hip) ----
namespace {
// what both calls refuse in a batch and in the thresholds
bool adapter_args_ok(const kmx_reads* reads, uint32_t min_overlap, uint32_t err_num, uint32_t err_den) {
    if (!reads_ok(reads) || min_overlap == 0u || err_den == 0u || err_num > err_den) return false;
    return reads_batch_ok(reads);
}
}  // namespace

int kmx_reads_adapter(kmx_ctx* ctx, const kmx_reads* reads, const uint8_t* h_adapters, const uint32_t* h_adapter_lens, uint32_t n_adapters,
                      uint32_t min_overlap, uint32_t err_num, uint32_t err_den, uint64_t* d_rows) {
    if (!ctx || !d_rows || !h_adapters || !h_adapter_lens || !adapter_args_ok(reads, min_overlap, err_num, err_den)) return KMX_E_ARG;
    if (n_adapters < 1u || n_adapters > KMX_RA_MAX_ADAPTERS) return KMX_E_ARG;
    kmx::ReadsAdapter a{};
    a.bases = reads->d_bases;
    a.offsets = reads->d_offsets;
    a.n_reads = reads->n_reads;
    a.read_len = reads->read_len;
    a.n_adapters = n_adapters;
    a.min_overlap = min_overlap;
    a.err_num = err_num;
    a.err_den = err_den;
    a.rows = d_rows;
    const uint8_t* s = h_adapters;
    for (uint32_t i = 0; i < n_adapters; ++i) {
        const uint32_t len = h_adapter_lens[i];
        if (len < 1u || len > KMX_RA_MAX_ADAPTER_LEN) return KMX_E_ARG;
        a.len[i] = len;
        for (uint32_t j = 0; j < len; ++j) {
            const uint32_t b = s[j], u = b & 0xDFu;
            if (u == 'N') continue;   // a wildcard: no bit of care
            if (u != 'A' && u != 'C' && u != 'G' && u != 'T') return KMX_E_ARG;
            const uint32_t c = (b >> 1) & 3u;   // the code of kmx_reads_adapter.hip
            a.lo[i] |= (uint64_t)(c & 1u) << j;
            a.hi[i] |= (uint64_t)(c >> 1) << j;
            a.care[i] |= 1ull << j;
        }
        s += len;
    }
    if (reads->n_reads == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    KMX_HIP(ctx, kmx::launch_reads_adapter(a, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

int kmx_reads_pair_overlap(kmx_ctx* ctx, const kmx_reads* reads1, const kmx_reads* reads2, uint32_t min_overlap, uint32_t max_mism, uint32_t err_num,
                           uint32_t err_den, uint64_t* d_rows) {
    if (!ctx || !d_rows || !adapter_args_ok(reads1, min_overlap, err_num, err_den) || !adapter_args_ok(reads2, min_overlap, err_num, err_den))
        return KMX_E_ARG;
    if (reads1->n_reads != reads2->n_reads) return KMX_E_ARG;
    if (reads1->n_reads == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    const kmx::ReadsPairOverlap a{reads1->d_bases, reads2->d_bases, reads1->d_offsets, reads2->d_offsets, reads1->n_reads, reads1->read_len,
                                  reads2->read_len, min_overlap, max_mism, err_num, err_den, d_rows};
    KMX_HIP(ctx, kmx::launch_reads_pair_overlap(a, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

// ---- poly-X ends, composition and DUST windows (kmx_reads_complexity.hip) ----
int kmx_reads_complexity(kmx_ctx* ctx, const kmx_reads* reads, uint32_t tail_bases, uint32_t head_bases, uint32_t min_len, uint32_t err_num,
                         uint32_t err_den, uint32_t penalty, uint32_t dust_max, uint8_t* d_masked, uint64_t* d_rows) {
    if (!ctx || !reads_ok(reads) || (!d_masked && !d_rows) || tail_bases > 15u || head_bases > 15u) return KMX_E_ARG;
    if (err_den == 0u || err_num > err_den || penalty > 255u || (min_len == 0u && (tail_bases | head_bases))) return KMX_E_ARG;
    if (!reads_batch_ok(reads)) return KMX_E_ARG;
    if (reads->n_reads == 0) return KMX_OK;
    const bool bytes = reads->d_offsets || reads->read_len;   // (uniform reads of no bases: rows of zeros, nothing is read)
    DeviceGuard g(ctx->device);
    if (bytes && d_masked)
        if (int st = masked_copy_ok(ctx, reads, d_masked, nullptr)) return st;
    const kmx::ReadsComplexity a{reads->d_bases, reads->d_offsets, reads->n_reads, reads->read_len, tail_bases, head_bases, min_len, err_num, err_den,
                                 penalty, dust_max, d_masked, d_rows};
    KMX_HIP(ctx, kmx::launch_reads_complexity(a, ctx->n_cu, ctx->stream));
    return KMX_OK;
}

// ---- overlapping mate pairs merged into consensus reads (kmx_reads_merge.hip) ----
int kmx_reads_pair_merge(kmx_ctx* ctx, const kmx_reads* reads1, const kmx_reads* reads2, const uint8_t* d_quals1, const uint8_t* d_quals2,
                         const uint64_t* d_insert, uint64_t insert_stride, uint32_t phred_base, uint32_t q_cap, uint8_t* d_out_bases,
                         uint8_t* d_out_quals, uint64_t* d_out_offsets, uint64_t* d_rows, uint64_t max_bases, uint64_t* h_n_merged,
                         uint64_t* h_n_bases) {
    const char* who = "kmx_reads_pair_merge";
    if (!ctx || !reads_ok(reads1) || !reads_ok(reads2) || !h_n_merged || !h_n_bases) return KMX_E_ARG;
    *h_n_merged = *h_n_bases = 0;
    const uint64_t n = reads1->n_reads;
    if (n != reads2->n_reads || !reads_batch_ok(reads1) || !reads_batch_ok(reads2) || (uint64_t)phred_base + q_cap > 255u) return KMX_E_ARG;
    if ((d_quals1 == nullptr) != (d_quals2 == nullptr) || (d_out_quals && !d_quals1)) return KMX_E_ARG;
    if ((d_out_bases == nullptr) != (d_out_offsets == nullptr) || (d_out_quals && !d_out_bases)) return KMX_E_ARG;
    if (n && (!d_insert || insert_stride == 0 || (n - 1u) > ((1ull << 60) - 1u) / insert_stride)) return KMX_E_ARG;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    void* area = nullptr;
    if (int st = work_area(ctx, who, kmx::reads_merge_bytes(n), &area)) return st;
    const kmx::ReadsPairMerge a{reads1->d_bases, reads2->d_bases, reads1->d_offsets, reads2->d_offsets, d_quals1, d_quals2, d_insert, insert_stride, n,
                                reads1->read_len, reads2->read_len, phred_base, q_cap, d_out_bases, d_out_quals, d_out_offsets, d_rows};
    uint64_t h[6] = {0, 0, 0, 0, 0, 0};   // merged pairs, merged bases, the first and last offset of batch 1, of batch 2
    KMX_HIP(ctx, kmx::launch_reads_merge_count(a, area, ctx->h_pinned, h, ctx->stream));
    *h_n_merged = h[0];
    *h_n_bases = h[1];
    if (!d_out_bases && !d_rows) return KMX_OK;
    if (d_out_bases)
        if (int st = room_for(ctx, who, h[1], "bases merged", max_bases)) return st;
    // the bytes the inputs span against the bytes that are written
    auto batch = [&](const void* base, const kmx_reads* r, uint64_t first, uint64_t last) {
        return Range::of_batch(base, r->d_offsets, n, r->read_len, first, last);
    };
    const Range in[] = {batch(reads1->d_bases, reads1, h[2], h[3]), batch(reads2->d_bases, reads2, h[4], h[5]), batch(d_quals1, reads1, h[2], h[3]),
                        batch(d_quals2, reads2, h[4], h[5]), Range::of_words(reads1->d_offsets, n + 1u), Range::of_words(reads2->d_offsets, n + 1u),
                        Range::of_words(d_insert, (n - 1u) * insert_stride + 1u)};
    const Range out[] = {Range::of_bytes(d_out_bases, h[1]), Range::of_bytes(d_out_quals, h[1]), Range::of_words(d_out_offsets, n + 1u),
                         Range::of_words(d_rows, KMX_RM_WORDS * n)};
    for (const Range& o : out)
        for (const Range& i : in)
            if (o.overlaps(i)) return KMX_E_ARG;
    KMX_HIP(ctx, kmx::launch_reads_merge_emit(a, area, ctx->n_cu, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMX_OK;
}

// ---- duplicate reads and read pairs (kmx_reads_dedup.hip) ----
int kmx_reads_dedup(kmx_ctx* ctx, const kmx_reads* reads, const kmx_reads* mates, uint32_t flags, uint32_t hash_bits, const uint64_t* d_score,
                    uint64_t score_stride, uint64_t* d_rows, uint8_t* d_keep, uint64_t* h_summary) {
    const char* who = "kmx_reads_dedup";
    if (!ctx || !reads_ok(reads) || (mates && !reads_ok(mates)) || !d_rows || !h_summary) return KMX_E_ARG;
    for (uint32_t w = 0; w < KMX_DD_SUMMARY_WORDS; ++w) h_summary[w] = 0;
    const uint64_t n = reads->n_reads;
    if ((mates && mates->n_reads != n) || !reads_batch_ok(reads) || (mates && !reads_batch_ok(mates))) return KMX_E_ARG;
    if ((flags & ~KMX_DD_STRAND) != 0u || hash_bits < 1u || hash_bits > 64u) return KMX_E_ARG;
    if (n >= (1ull << 32)) return KMX_E_ARG;   // (the index shares a word with the score)
    if (d_score && (score_stride == 0 || (n && (n - 1u) > ((1ull << 60) - 1u) / score_stride))) return KMX_E_ARG;
    if (n == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    void* area = nullptr;
    if (int st = work_area(ctx, who, kmx::reads_dedup_bytes(n, ctx->n_cu), &area)) return st;
    const kmx::ReadsDedup a{reads->d_bases, mates ? mates->d_bases : nullptr, reads->d_offsets, mates ? mates->d_offsets : nullptr, n, reads->read_len,
                            mates ? mates->read_len : 0u, mates ? 1u : 0u, flags & KMX_DD_STRAND, hash_bits, d_score, score_stride, d_rows, d_keep};
    bool bad = false;
    KMX_HIP(ctx, kmx::launch_reads_dedup(a, area, ctx->h_pinned, h_summary, &bad, ctx->n_cu, ctx->stream));
    if (bad) return fail_hip(ctx, hipErrorUnknown, "kmx_reads_dedup: the sort did not return every record once");
    return KMX_OK;
}

int kmx_reads_length_range(kmx_ctx* ctx, const uint64_t* d_offsets, uint64_t n_reads, uint32_t* h_min_len, uint32_t* h_max_len) {
    if (!ctx || (n_reads && !d_offsets)) return KMX_E_ARG;
    if (h_min_len) *h_min_len = 0;
    if (h_max_len) *h_max_len = 0;
    if (n_reads == 0) return KMX_OK;
    DeviceGuard g(ctx->device);
    uint32_t* d_out = reinterpret_cast<uint32_t*>(ctx->d_scratch + KMX_S_LEN_RANGE);
    const uint32_t init[2] = {0xFFFFFFFFu, 0u};
    uint32_t got[2] = {0, 0};
    KMX_HIP(ctx, hipMemcpyAsync(d_out, init, 8, hipMemcpyHostToDevice, ctx->stream));
    KMX_HIP(ctx, kmx::launch_length_range(d_offsets, n_reads, d_out, ctx->n_cu, ctx->stream));
    KMX_HIP(ctx, hipMemcpyAsync(got, d_out, 8, hipMemcpyDeviceToHost, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_min_len) *h_min_len = got[0];
    if (h_max_len) *h_max_len = got[1];
    if (got[1] >= 0x80000000u) {   // (lengths are clamped to 32 bits by the kernel: anything from 2^31 up lands here)
        std::snprintf(ctx->last_error, sizeof ctx->last_error, "kmx_reads_length_range: a read of 2^31 bases or more (the scans skip such reads)");
        return KMX_E_ARG;
    }
    return KMX_OK;
}

}  // extern "C"
