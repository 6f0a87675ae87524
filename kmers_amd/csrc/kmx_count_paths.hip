// kmx_count_paths.hip -- reads threaded through the unitigs of a count table (kmx_count_unitig_index, kmx_count_read_paths(2)).
//
// Index.  place[i] = ((p + 1) << 3) | (last << 2) | (first << 1) | o for the entry i that d_nodes[p] names, 0 for an entry no node
// names: the array is zeroed, a lane per node position writes the place of an interior node, a lane per unitig writes those of its
// first and last node (whole words, after the first kernel: nothing is read back and or-ed).  Indices only: no key width here.
//
// Paths.  What kmx_count_lookup_reads(2) leaves with the places as the counts -- one u64 place and one flag byte per window, 0 for
// a window that is invalid, absent or in no unitig -- is cut into SEGMENTS, maximal runs of consecutive windows of one read that
// walk one unitig in one direction (kmx.h has the rule).  Key width plays no part here either.  Three kernels over the flat window
// array, no LDS, no atomics, no block-wide step:
//   mark   a wave per RANGE of 4096 windows, 64 windows (a GROUP) per step.  A lane holds the state of its window, takes its
//          predecessor's from the lane below (lane 0 loads it) and decides "continues its predecessor"; the ballot of that answers
//          "is continued by its successor" for lanes 0 .. 62, lane 63 loads the window behind the group.  HEAD = mapped and does
//          not continue, TAIL = mapped and is not continued.  Per group: the two ballots (8 bytes each) and the number of heads in
//          the range before the group (4 bytes); per range: its number of heads.
//   scan   the family's scan_single_kernel over the ranges' head counts: the slot of a range's first head, and the total.
//   emit   a lane per window, at work only where its bit in the group's head ballot is set: slot = range + group + the heads
//          below it in the ballot.  It finds its tail in the tail ballots (its own group's bits at or above it, then word by word:
//          64 windows per load, so the 120 windows of a short read cost two or three loads), reads its place, searches d_offsets
//          once for the unitig (and the window offsets for the read, ragged reads) and writes the record's four words.
//          Heads and tails alternate, so the first tail at or behind a head is its own.
//   offsets  a lane per read: the slot of the first head at or behind its first window, from the same three arrays.
// Where a read starts: uniform reads at the multiples of W, from the group's own division; ragged reads carry bit 7 of the flag
// byte of their first window, set by a lane per read over the window offsets before `mark` (the flags live in the work buffer and
// are the call's to change; bits 0 and 1 are what the windows call wrote).  A read start never continues anything, in every route
// of the windows call: the slots of consecutive reads are adjacent, with no invalid slot between them.
// Every record is written by exactly one lane and depends on the inputs only: repeated calls give identical bytes.
#include "kmx_count_common.h"

namespace kmx {

namespace {

constexpr u32 PATH_RANGE = 64u * 64u;   // windows per wave of the mark kernel, and per scanned partial
constexpr uint8_t WIN_READ_START = 0x80u;   // (work-buffer flags only) the first window of a ragged read

// ---------------------------------------------------------------- the index
__global__ void __launch_bounds__(CT) unitig_index_nodes_kernel(const u64* __restrict__ nodes, const u64* __restrict__ offsets, u64 n_unitigs, u64 n,
                                                                u64* __restrict__ place) {
    const u64 n_nodes = offsets[n_unitigs];   // (known on the device only: the grid is sized from n and strides)
    for (u64 p = (u64)blockIdx.x * CT + threadIdx.x; p < n_nodes; p += (u64)gridDim.x * CT) {
        const u64 v = nodes[p], i = v >> 1;
        if (i < n) place[i] = ((p + 1u) << 3) | (v & 1u);
    }
}

__global__ void __launch_bounds__(CT) unitig_index_ends_kernel(const u64* __restrict__ nodes, const u64* __restrict__ offsets, u64 n_unitigs, u64 n,
                                                               u64* __restrict__ place) {
    const u64 u = (u64)blockIdx.x * CT + threadIdx.x;
    if (u >= n_unitigs) return;
    const u64 n_nodes = offsets[n_unitigs];
    const u64 a = offsets[u], b = offsets[u + 1u];
    if (a >= b || b > n_nodes) return;   // (an empty unitig, or offsets that do not ascend)
    const u64 vf = nodes[a], vl = nodes[b - 1u];
    if (b - a == 1u) {
        if ((vf >> 1) < n) place[vf >> 1] = ((a + 1u) << 3) | 6u | (vf & 1u);
        return;
    }
    if ((vf >> 1) < n) place[vf >> 1] = ((a + 1u) << 3) | 2u | (vf & 1u);
    if ((vl >> 1) < n) place[vl >> 1] = (b << 3) | 4u | (vl & 1u);
}

// ---------------------------------------------------------------- the paths
// a window as the continuation rule sees it: x = its place if it is MAPPED (valid, in the table, in a unitig whose node list holds
// its position), else 0; s = the read's strand there
struct Win {
    u64 x;
    u32 s;
};

__device__ __forceinline__ Win load_win(const u64* __restrict__ places, const uint8_t* __restrict__ flags, u64 j, u64 n_win, u64 n_nodes, u32* flag) {
    Win w{0u, 0u};
    *flag = 0u;
    if (j >= n_win) return w;
    const u32 f = flags[j];
    const u64 x = places[j];
    *flag = f;
    w.s = (f & KMX_WIN_FW_CANONICAL) != 0u ? 0u : 1u;
    if ((f & KMX_WIN_VALID) != 0u && (x >> 3) != 0u && (x >> 3) - 1u < n_nodes) w.x = x;
    return w;
}

// does window b (not the first of its read) continue window a, the one before it?
__device__ __forceinline__ bool continues(const Win& a, const Win& b) {
    if (a.x == 0u || b.x == 0u) return false;
    const u32 da = a.s ^ (u32)(a.x & 1u), db = b.s ^ (u32)(b.x & 1u);
    if (da != db) return false;
    const u64 pa = a.x >> 3, pb = b.x >> 3;
    return da == 0u ? pb == pa + 1u && (b.x & 2u) == 0u : pb + 1u == pa && (b.x & 4u) == 0u;
}

// position within its read of the window `off` (0 .. 64) behind one at position rem < W of a uniform read of W windows
__device__ __forceinline__ u64 pos_in_read(u64 rem, u32 off, u32 W) {
    const u64 pos = rem + off;
    if (W > 64u) return pos >= W ? pos - W : pos;
    return (u32)pos % W;
}

__global__ void __launch_bounds__(CT) path_read_starts_kernel(const u64* __restrict__ wo, u64 n_reads, u64 n_win, uint8_t* __restrict__ flags) {
    const u64 r = (u64)blockIdx.x * CT + threadIdx.x;
    if (r >= n_reads) return;
    const u64 a = wo[r];
    if (wo[r + 1u] > a && a < n_win) flags[a] |= WIN_READ_START;   // (one read per byte: nobody else writes it)
}

// W != 0: uniform reads of W windows.  W == 0: ragged reads, starts marked in the flags.
__global__ void __launch_bounds__(CT) path_mark_kernel(const u64* __restrict__ places, const uint8_t* __restrict__ flags, u64 n_win, u32 W,
                                                       const u64* __restrict__ unitig_offsets, u64 n_unitigs, u64* __restrict__ heads,
                                                       u64* __restrict__ tails, u32* __restrict__ sub, u64* __restrict__ partial) {
    const u32 lane = threadIdx.x & 63u;
    const u64 range = (u64)blockIdx.x * (CT / 64u) + (threadIdx.x >> 6);
    const u64 j0 = range * PATH_RANGE;
    if (j0 >= n_win) return;
    const u64 n_nodes = unitig_offsets[n_unitigs];
    u64 rem = W != 0u ? j0 % W : 0u;
    u32 run = 0;
    for (u32 step = 0; step < 64u; ++step) {
        const u64 base = j0 + (u64)step * 64u;
        if (base >= n_win) break;   // (uniform over the wave)
        const u64 j = base + lane;
        u32 f, fx;
        const Win cur = load_win(places, flags, j, n_win, n_nodes, &f);
        Win prev;
        prev.x = __shfl_up(cur.x, 1);
        prev.s = __shfl_up(cur.s, 1);
        if (lane == 0u) prev = base != 0u ? load_win(places, flags, base - 1u, n_win, n_nodes, &fx) : Win{0u, 0u};
        const bool start = W != 0u ? pos_in_read(rem, lane, W) == 0u : (f & WIN_READ_START) != 0u;
        const bool cont = !start && continues(prev, cur);
        const u64 cb = __ballot(cont);
        bool cont_next = ((cb >> 1) >> lane & 1ull) != 0u;
        if (lane == 63u) {   // the window behind the group: is it this read's, and does it continue this one?
            const Win nxt = load_win(places, flags, j + 1u, n_win, n_nodes, &fx);
            const bool nstart = W != 0u ? pos_in_read(rem, 64u, W) == 0u : (fx & WIN_READ_START) != 0u;
            cont_next = !nstart && continues(cur, nxt);
        }
        const u64 hb = __ballot(cur.x != 0u && !cont), tb = __ballot(cur.x != 0u && !cont_next);
        if (lane == 0u) {
            const u64 g = base >> 6;
            heads[g] = hb;
            tails[g] = tb;
            sub[g] = run;
        }
        run += (u32)__popcll(hb);
        if (W != 0u) rem = pos_in_read(rem, 64u, W);
    }
    if (lane == 0u) partial[range] = run;
}

// heads in front of window j (j < n_win)
__device__ __forceinline__ u64 heads_before(const u64* __restrict__ heads, const u32* __restrict__ sub, const u64* __restrict__ partial, u64 j) {
    const u64 g = j >> 6;
    return partial[g >> 6] + sub[g] + (u64)__popcll(heads[g] & ((1ull << (j & 63u)) - 1ull));
}

// the largest i in [0, n) with a[i] <= x (0 if there is none); n >= 1; reads a[1 .. n) only
__device__ __forceinline__ u64 last_at_or_below(const u64* __restrict__ a, u64 n, u64 x) {
    u64 lo = 0, hi = n;
    while (hi - lo > 1u) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(CT) path_emit_kernel(const u64* __restrict__ places, const uint8_t* __restrict__ flags, u64 n_win, u32 W,
                                                       const u64* __restrict__ wo, u64 n_reads, const u64* __restrict__ unitig_offsets, u64 n_unitigs,
                                                       const u64* __restrict__ heads, const u64* __restrict__ tails, const u32* __restrict__ sub,
                                                       const u64* __restrict__ partial, u64* __restrict__ segments) {
    const u64 j = (u64)blockIdx.x * CT + threadIdx.x;
    if (j >= n_win) return;
    const u32 lane = threadIdx.x & 63u;
    const u64 g = j >> 6, n_groups = ceil_div(n_win, 64u);
    const u64 hb = heads[g];
    if ((hb >> lane & 1ull) == 0u) return;
    const u64 slot = partial[g >> 6] + sub[g] + (u64)__popcll(hb & ((1ull << lane) - 1ull));
    // its tail: the first one at or behind it
    u64 tb = tails[g] & (~0ull << lane), gt = g;
    while (tb == 0u && gt + 1u < n_groups) tb = tails[++gt];
    const u64 jt = tb != 0u ? gt * 64u + (u64)(__ffsll((long long)tb) - 1) : n_win - 1u;   // (a head always has one)
    const u64 x = places[j];
    const u32 d = ((flags[j] & KMX_WIN_FW_CANONICAL) != 0u ? 0u : 1u) ^ (u32)(x & 1u);
    const u64 p = (x >> 3) - 1u;
    const u64 u = last_at_or_below(unitig_offsets, n_unitigs, p);
    u64 r, start;
    if (W != 0u) {
        r = j / W;
        start = j - r * W;
    } else {
        r = last_at_or_below(wo, n_reads, j);   // (an empty read shares its offset with the next one: the last read at or below j holds it)
        start = j - wo[r];
    }
    u64* rec = segments + KMX_PATH_WORDS * slot;
    rec[KMX_PATH_READ] = r;
    rec[KMX_PATH_SPAN] = ((jt - j + 1u) << 32) | (start & 0xFFFFFFFFull);
    rec[KMX_PATH_UNITIG] = u;
    rec[KMX_PATH_POS] = ((p - unitig_offsets[u]) << 1) | d;
}

// path_offsets[r] = the segments in front of read r, r = 0 .. n_reads (first: the reads' first windows, nullptr = uniform reads)
__global__ void __launch_bounds__(CT) path_offsets_kernel(const u64* __restrict__ first, u64 n_reads, u32 W, u64 n_win, const u64* __restrict__ heads,
                                                          const u32* __restrict__ sub, const u64* __restrict__ partial, u64 n_ranges,
                                                          u64* __restrict__ path_offsets) {
    const u64 r = (u64)blockIdx.x * CT + threadIdx.x;
    if (r > n_reads) return;
    const u64 j = r == n_reads ? n_win : first != nullptr ? first[r] : r * W;
    path_offsets[r] = j < n_win ? heads_before(heads, sub, partial, j) : partial[n_ranges];
}

struct PathArea {
    u64 *heads, *tails, *partial;
    u32* sub;
    u64 n_groups, n_ranges;
};
PathArea path_area(void* area, u64 n_win) {
    PathArea a;
    a.n_groups = ceil_div(n_win, 64u);
    a.n_ranges = ceil_div(n_win, PATH_RANGE);
    char* b = static_cast<char*>(area);
    a.heads = reinterpret_cast<u64*>(b);
    a.tails = reinterpret_cast<u64*>(b += align256(8u * a.n_groups));
    a.sub = reinterpret_cast<u32*>(b += align256(8u * a.n_groups));
    a.partial = reinterpret_cast<u64*>(b + align256(4u * a.n_groups));
    return a;
}

}  // namespace

hipError_t launch_count_unitig_index(const u64* nodes, const u64* offsets, u64 n_unitigs, u64 n, u64* place, hipStream_t st) {
    hipError_t e = hipMemsetAsync(place, 0, 8u * n, st);
    if (e != hipSuccess || n_unitigs == 0) return e;
    const u64 nb = ceil_div(n, CT);   // (a unitig's nodes are entries: about n positions; the kernel strides over however many there are)
    hipLaunchKernelGGL(unitig_index_nodes_kernel, dim3((unsigned)(nb < (1u << 20) ? nb : (1u << 20))), dim3(CT), 0, st, nodes, offsets, n_unitigs, n, place);
    hipLaunchKernelGGL(unitig_index_ends_kernel, dim3((unsigned)ceil_div(n_unitigs, CT)), dim3(CT), 0, st, nodes, offsets, n_unitigs, n, place);
    return hipGetLastError();
}

// the paths' own arrays for n_win windows: two ballots and a count per 64 windows, a partial per 4096 (+ the total, + one spare)
size_t count_paths_bytes(u64 n_win) {
    const u64 g = ceil_div(n_win, 64u);
    return 2u * align256(8u * g) + align256(4u * g) + align256(8u * (ceil_div(n_win, PATH_RANGE) + 2u));
}

// places / flags: one u64 and one byte per window, as launch_count_lookup leaves them with the places as the counts.  win_offsets ==
// nullptr: uniform reads of W windows each (W >= 1); otherwise ragged reads (their flags get the read-start marks).  n_win >= 1,
// n_unitigs >= 1.  Synchronous: *h_segments = the number of segments.
hipError_t launch_count_paths_mark(const u64* places, uint8_t* flags, const u64* win_offsets, u64 n_reads, u32 W, u64 n_win, const u64* unitig_offsets,
                                   u64 n_unitigs, void* area, unsigned long long* h_pinned, u64* h_segments, hipStream_t st) {
    const PathArea a = path_area(area, n_win);
    if (win_offsets) hipLaunchKernelGGL(path_read_starts_kernel, dim3((unsigned)ceil_div(n_reads, CT)), dim3(CT), 0, st, win_offsets, n_reads, n_win, flags);
    hipLaunchKernelGGL(path_mark_kernel, dim3((unsigned)ceil_div(a.n_ranges, CT / 64u)), dim3(CT), 0, st, places, flags, n_win, win_offsets ? 0u : W,
                       unitig_offsets, n_unitigs, a.heads, a.tails, a.sub, a.partial);
    hipLaunchKernelGGL(scan_single_kernel, dim3(1), dim3(CT), 0, st, a.partial, a.n_ranges, a.partial + a.n_ranges);
    return read_back(h_pinned, a.partial + a.n_ranges, 1u, h_segments, st);
}

// after launch_count_paths_mark on the same arrays; segments may be nullptr (the offsets only)
hipError_t launch_count_paths_emit(const u64* places, const uint8_t* flags, const u64* win_offsets, u64 n_reads, u32 W, u64 n_win,
                                   const u64* unitig_offsets, u64 n_unitigs, const void* area, u64* path_offsets, u64* segments, hipStream_t st) {
    const PathArea a = path_area(const_cast<void*>(area), n_win);
    const u32 w = win_offsets ? 0u : W;
    hipLaunchKernelGGL(path_offsets_kernel, dim3((unsigned)ceil_div(n_reads + 1u, CT)), dim3(CT), 0, st, win_offsets, n_reads, w, n_win, a.heads, a.sub,
                       a.partial, a.n_ranges, path_offsets);
    if (segments)
        hipLaunchKernelGGL(path_emit_kernel, dim3((unsigned)ceil_div(n_win, CT)), dim3(CT), 0, st, places, flags, n_win, w, win_offsets, n_reads,
                           unitig_offsets, n_unitigs, a.heads, a.tails, a.sub, a.partial, segments);
    return hipGetLastError();
}

}  // namespace kmx
