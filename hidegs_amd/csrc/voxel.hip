// voxel.hip -- voxel grid over a point cloud (include/hidegs_voxel.h): group the rows that share a cell, then
// reduce rows per group.
//
// Grouping (hidegs_voxel_group), every step a launch, no host read:
//   1. voxel_bounds / voxel_frame: the origin -- the caller's, or the minimum over the eligible rows (partials
//      of up to kBoundBlocks workgroups, one finishing workgroup); the frame kernel also clears the counter;
//   2. voxel_keys: key[i] = cx << 42 | cy << 21 | cz of a candidate row, kNoKey (bit 63) of every other row,
//      and the count of eligible rows that are out of range (a ballot per wave, one integer add per wave);
//   3. the stable radix sort (sort_pairs_u64) of (key, row) over all 64 bits: the candidates come first,
//      ascending by (key, row), the other rows last;
//   4. voxel_heads (1 where a candidate's key differs from the key before it) and the library's inclusive
//      scan: rank[j] = 1 + the group of sorted position j;
//   5. voxel_assign: order, group_of, starts, and info[0..2] by the one thread that sees the last candidate;
//   6. voxel_flags: first_flags, and info[3] by an integer maximum (per workgroup, then one atomic).
//
// Reduction (hidegs_voxel_reduce_rows), three size classes, decided per group on the device from starts:
//   small   n <= kSmallMax: voxel_reduce_small, one lane per (group, column), the rows added one by one;
//           consecutive lanes read consecutive columns of one row.  FIRST of every group is written here too;
//   medium  kSmallMax < n <= kChunk: voxel_reduce_wave, one wave per group.  L = the power of two at or above
//           min(width, 64) lanes share a row (64 / L rows in flight), every lane adds its rows of its column,
//           then a fixed xor tree over the lanes of a column;
//   large   n > kChunk: the group is cut into chunks of kChunk rows.  voxel_reduce_chunk gives a workgroup to
//           every chunk (L lanes per row, 256 / L rows in flight, the tree, then the four waves in order) and
//           stores the chunk's partial in scratch; voxel_reduce_finish adds a group's partials as a chunk adds
//           its rows (L threads per partial, every thread its partials in chunk order, the tree, the waves).
// Finding the chunks needs no work list: the grid has one workgroup per window of kChunk positions of `order`,
// and a window holds the start of at most two chunks -- one of the large group that covers the window's first
// position (chunks start kChunk apart) and chunk 0 of a large group that starts inside it (a second one would
// have to end inside the window too).  They take partial slots 2 * window and 2 * window + 1.  Likewise at
// most one large group starts in a window, and that window's workgroup of the finishing launch owns it.
// What a lane adds, and in which order, depends on the group's size and the field's width alone.
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/hidegs_voxel.h"
#include "common.h"

namespace hidegs {

// The inclusive scan of primitives.hip, as hidegs_inclusive_scan_u32 calls it.
size_t inclusive_scan_scratch(long long n);
int inclusive_scan_u32(void* scratch, size_t scratch_bytes, const uint32_t* in, uint32_t* out, long long n,
                       hipStream_t stream);

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;  // 4
constexpr long long kVoxelMax = 0x7fffffffLL;
constexpr int kBoundBlocks = 1024;          // partial minima of the origin
constexpr uint64_t kNoKey = 1ull << 63;     // every row that is no candidate: sorts behind every key
constexpr float kCellLimit = 2097152.f;     // 2^21 cells per axis
constexpr int kMaxFields = 8;               // fields per launch set
constexpr uint32_t kSmallMax = 32;          // rows of a small group
constexpr uint32_t kChunk = 512;            // rows of a chunk, and of the largest medium group
constexpr int kGridCap = 8192;              // workgroups of a launch over the groups: 32 per CU, the rest by stride

__device__ __forceinline__ bool eligible(const float* __restrict__ pts, const uint8_t* __restrict__ among, long long i,
                                         float (&v)[3])
{
    if (among && among[i] == 0) return false;
    v[0] = pts[3 * i], v[1] = pts[3 * i + 1], v[2] = pts[3 * i + 2];
    return finite3(v[0], v[1], v[2]);
}

// ---- grouping: origin ---------------------------------------------------------------------------------
// Thread a < 3 of the workgroup returns the minimum of lo[a] over its threads.
__device__ __forceinline__ float block_min3(float (&lo)[3], float (*s)[3])
{
#pragma unroll
    for (int a = 0; a < 3; a++) lo[a] = wave_min(lo[a]);
    if (lane_id() == 0)
        for (int a = 0; a < 3; a++) s[threadIdx.x / kWave][a] = lo[a];
    __syncthreads();
    float l = INFINITY;
    if (threadIdx.x < 3)
        for (int w = 0; w < kWaves; w++) l = fminf(l, s[w][threadIdx.x]);
    return l;
}

__global__ __launch_bounds__(kBlock) void voxel_bounds_kernel(const float* __restrict__ pts,
                                                              const uint8_t* __restrict__ among, long long P,
                                                              float* __restrict__ partials)
{
    __shared__ float s[kWaves][3];
    float lo[3] = {INFINITY, INFINITY, INFINITY};
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long long)gridDim.x * kBlock) {
        float v[3];
        if (!eligible(pts, among, i, v)) continue;
#pragma unroll
        for (int a = 0; a < 3; a++) lo[a] = fminf(lo[a], v[a]);
    }
    const float l = block_min3(lo, s);
    if (threadIdx.x < 3) partials[blockIdx.x * 3 + threadIdx.x] = l;
}

// One workgroup: frame = {origin, cell}, the origin given or the minimum of the partials (+0.0 for a zero,
// 0 with no eligible row: a minimum of finite values is below +inf).  Clears the out-of-range counter.
__global__ __launch_bounds__(kBlock) void voxel_frame_kernel(const float* __restrict__ origin,
                                                             const float* __restrict__ partials, int nparts, float cell,
                                                             float* __restrict__ frame, uint32_t* __restrict__ counter)
{
    __shared__ float s[kWaves][3];
    float lo[3] = {INFINITY, INFINITY, INFINITY};
    if (!origin)
        for (int b = threadIdx.x; b < nparts; b += kBlock)
            for (int a = 0; a < 3; a++) lo[a] = fminf(lo[a], partials[b * 3 + a]);
    const float l = block_min3(lo, s);
    if (threadIdx.x < 3) frame[threadIdx.x] = origin ? origin[threadIdx.x] : (l < INFINITY ? l + 0.0f : 0.0f);
    if (threadIdx.x == 3) {
        frame[3] = cell;
        *counter = 0u;
    }
}

// ---- grouping: keys, heads, outputs -------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void voxel_keys_kernel(const float* __restrict__ pts, const uint8_t* __restrict__ among,
                                                            long long P, const float* __restrict__ frame, float inv,
                                                            uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                            uint32_t* __restrict__ counter)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    bool out_of_range = false;
    if (i < P) {
        float v[3];
        uint64_t key = kNoKey;
        if (eligible(pts, among, i, v)) {
            bool in = true;
            uint64_t k = 0;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const float t = (v[a] - frame[a]) * inv;
                in = in && t >= 0.f && t < kCellLimit;
                k = (k << 21) | (uint64_t)(uint32_t)floorf(in ? t : 0.f);
            }
            if (in) key = k;
            out_of_range = !in;
        }
        keys[i] = key;
        vals[i] = (uint32_t)i;
    }
    const uint64_t b = __ballot(out_of_range);
    if (b && lane_id() == 0) atomicAdd(counter, (uint32_t)__popcll(b));
}

__global__ __launch_bounds__(kBlock) void voxel_heads_kernel(const uint64_t* __restrict__ keys_sorted, long long P,
                                                             uint32_t* __restrict__ heads)
{
    const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (j >= P) return;
    const uint64_t k = keys_sorted[j];
    heads[j] = (k < kNoKey && (j == 0 || keys_sorted[j - 1] != k)) ? 1u : 0u;
}

// rank[j] = the heads at and before j.  Sorted position j of a candidate belongs to group rank[j] - 1, and is
// its head iff rank[j] != rank[j - 1].
__global__ __launch_bounds__(kBlock) void voxel_assign_kernel(const uint64_t* __restrict__ keys_sorted,
                                                              const uint32_t* __restrict__ rows_sorted,
                                                              const uint32_t* __restrict__ rank, long long P,
                                                              const uint32_t* __restrict__ counter,
                                                              int32_t* __restrict__ group_of, uint32_t* __restrict__ order,
                                                              uint32_t* __restrict__ starts, uint32_t* __restrict__ info)
{
    const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (j >= P) return;
    const uint32_t row = rows_sorted[j];
    if (keys_sorted[j] >= kNoKey) {
        group_of[row] = -1;
        if (j == 0) {  // no candidate at all
            starts[0] = 0u;
            info[0] = 0u, info[1] = 0u, info[2] = *counter, info[3] = 0u;
        }
        return;
    }
    const uint32_t r = rank[j];
    order[j] = row;
    group_of[row] = (int32_t)(r - 1);
    if (j == 0 || rank[j - 1] != r) starts[r - 1] = (uint32_t)j;
    if (j == P - 1 || keys_sorted[j + 1] >= kNoKey) {  // the last candidate: G = r, m = j + 1
        starts[r] = (uint32_t)(j + 1);
        info[0] = r, info[1] = (uint32_t)(j + 1), info[2] = *counter, info[3] = 0u;  // info[3]: voxel_flags
    }
}

__global__ __launch_bounds__(kBlock) void voxel_flags_kernel(const uint64_t* __restrict__ keys_sorted,
                                                             const uint32_t* __restrict__ rows_sorted,
                                                             const uint32_t* __restrict__ rank, long long P,
                                                             const uint32_t* __restrict__ starts,
                                                             uint8_t* __restrict__ first_flags, uint32_t* __restrict__ info)
{
    __shared__ uint32_t s_max[kWaves];
    const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
    uint32_t size = 0;
    if (j < P) {
        bool head = false;
        if (keys_sorted[j] < kNoKey) {
            const uint32_t r = rank[j];
            head = j == 0 || rank[j - 1] != r;
            if (head) size = starts[r] - starts[r - 1];
        }
        if (first_flags) first_flags[rows_sorted[j]] = head ? 1 : 0;
    }
    size = wave_max_u32(size);
    if (lane_id() == 0) s_max[threadIdx.x / kWave] = size;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; w++) size = s_max[w] > size ? s_max[w] : size;
        if (size) atomicMax(&info[3], size);
    }
}

struct GroupLayout {
    uint64_t *keys, *keys_sorted;
    uint32_t *vals, *vals_sorted, *rank;
    void *sort_tmp, *scan_tmp;
    size_t sort_bytes, scan_bytes;
    float* partials;
    uint32_t* counter;
    size_t total;
};

GroupLayout group_layout(void* base, long long P)
{
    GroupLayout l;
    Carver c(base);
    l.keys = c.take<uint64_t>(P);
    l.keys_sorted = c.take<uint64_t>(P);
    l.vals = c.take<uint32_t>(P);
    l.vals_sorted = c.take<uint32_t>(P);
    l.rank = c.take<uint32_t>(P);
    l.sort_bytes = sort_u64_scratch(P);
    l.sort_tmp = c.take<char>(l.sort_bytes);
    l.scan_bytes = inclusive_scan_scratch(P);
    l.scan_tmp = c.take<char>(l.scan_bytes);
    l.partials = c.take<float>(kBoundBlocks * 3);
    l.counter = c.take<uint32_t>(1);
    l.total = c.used;
    return l;
}

// ---- reduction ----------------------------------------------------------------------------------------
struct Field {
    const float* src;
    float* out;
    uint32_t n_rows;  // rows at and past it are skipped (<= 2^31: order holds u32 rows below 2^31)
    uint32_t width;
    int op;
};

struct Batch {
    Field f[kMaxFields];
};

struct Groups {
    const uint32_t* order;
    const uint32_t* starts;
    const uint32_t* info;
    const float* weights;
    uint32_t P;
    uint32_t max_groups;
};

// G and m as the launches may use them: whatever info holds, no position past P and no group past P is read.
struct Counts {
    uint32_t G, m, ng;  // ng = min(G, max_groups): the groups that are written
};

__device__ __forceinline__ Counts load_counts(const Groups& gr)
{
    Counts c;
    c.m = min(gr.info[1], gr.P);
    c.G = min(gr.info[0], c.m);
    c.ng = min(c.G, gr.max_groups);
    return c;
}

// Group g < G is order[a .. e), kept inside [0, m] whatever starts holds.
__device__ __forceinline__ void group_span(const Groups& gr, const Counts& c, uint32_t g, uint32_t& a, uint32_t& e)
{
    e = min(gr.starts[g + 1], c.m);
    a = min(gr.starts[g], e);
}

struct Acc {
    float v;       // the sum, the minimum or the maximum
    float ws;      // the sum of the weights
    uint32_t cnt;  // rows that were not skipped
};

__device__ __forceinline__ Acc acc_init(int op)
{
    Acc a;
    a.v = (op == HIDEGS_VOXEL_MIN || op == HIDEGS_VOXEL_MAX) ? __uint_as_float(0x7fc00000u) : 0.f;
    a.ws = 0.f;
    a.cnt = 0u;
    return a;
}

__device__ __forceinline__ Acc acc_merge(const Acc& a, const Acc& b, int op)
{
    Acc r;
    if (op == HIDEGS_VOXEL_MIN)
        r.v = fminf(a.v, b.v);  // fminf / fmaxf return the number where one side is a NaN
    else if (op == HIDEGS_VOXEL_MAX)
        r.v = fmaxf(a.v, b.v);
    else
        r.v = a.v + b.v;
    r.ws = a.ws + b.ws;
    r.cnt = a.cnt + b.cnt;
    return r;
}

__device__ __forceinline__ float acc_result(const Acc& a, int op, bool weighted)
{
    if (op == HIDEGS_VOXEL_MEAN) return a.v / (weighted ? a.ws : (float)a.cnt);
    return a.v;
}

// One row's contribution.
__device__ __forceinline__ Acc acc_row(float x, float wt, bool weighted)
{
    Acc b;
    b.v = weighted ? x * wt : x;
    b.ws = wt;
    b.cnt = 1u;
    return b;
}

// Positions first, first + step, ... of order[.. end) at column c, added one after the other; four rows are
// loaded at a time so that their latencies overlap.  `load` is false for a lane beyond the field's width: it
// walks the same rows and keeps no value.
__device__ __forceinline__ Acc reduce_rows(const Groups& gr, const Field& f, uint32_t first, uint32_t end, uint32_t step,
                                           uint32_t c, bool load)
{
    constexpr int kInFlight = 4;
    Acc a = acc_init(f.op);
    const bool weighted = gr.weights && f.op <= HIDEGS_VOXEL_MEAN;
    uint32_t j = first;
    for (; j < end && end - j > (kInFlight - 1) * step; j += kInFlight * step) {
        uint32_t row[kInFlight];
        float x[kInFlight], wt[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; u++) row[u] = gr.order[j + u * step];
#pragma unroll
        for (int u = 0; u < kInFlight; u++) {
            const bool ok = row[u] < f.n_rows;
            x[u] = (ok && load) ? f.src[(size_t)row[u] * f.width + c] : 0.f;
            wt[u] = (ok && gr.weights) ? gr.weights[row[u]] : 1.f;
        }
#pragma unroll
        for (int u = 0; u < kInFlight; u++)
            if (row[u] < f.n_rows) a = acc_merge(a, acc_row(x[u], wt[u], weighted), f.op);
    }
    for (; j < end; j += step) {
        const uint32_t row = gr.order[j];
        if (row >= f.n_rows) continue;
        const float x = load ? f.src[(size_t)row * f.width + c] : 0.f;
        a = acc_merge(a, acc_row(x, gr.weights ? gr.weights[row] : 1.f, weighted), f.op);
    }
    return a;
}

// The lanes of a wave that hold one column (lane & (L - 1) equal) merged by a fixed xor tree, widest step
// first; every lane ends with the same bits (the merges commute).  All 64 lanes must be active.
__device__ __forceinline__ Acc wave_merge_columns(Acc a, uint32_t L, int op)
{
#pragma unroll
    for (uint32_t mask = kWave / 2; mask >= 1; mask >>= 1) {
        if (mask >= L) {  // wave-uniform
            Acc b;
            b.v = __shfl_xor(a.v, (int)mask, kWave);
            b.ws = __shfl_xor(a.ws, (int)mask, kWave);
            b.cnt = __shfl_xor(a.cnt, (int)mask, kWave);
            a = acc_merge(a, b, op);
        }
    }
    return a;
}

// Lanes that share a row: the power of two at or above min(width, 64).
__device__ __forceinline__ uint32_t lanes_per_row(uint32_t width)
{
    uint32_t L = 1;
    while (L < width && L < (uint32_t)kWave) L <<= 1;
    return L;
}

// The first row of order[a .. e) that the field holds, or 0xffffffff.
__device__ __forceinline__ uint32_t first_row(const Groups& gr, const Field& f, uint32_t a, uint32_t e)
{
    for (uint32_t j = a; j < e; j++) {
        const uint32_t row = gr.order[j];
        if (row < f.n_rows) return row;
    }
    return 0xffffffffu;
}

// Small groups, and FIRST of every group.  A workgroup holds gpb = max(1, 256 / width) groups at a time, thread
// t column t % width of group t / width; a field wider than the workgroup has its columns strided.
__global__ __launch_bounds__(kBlock) void voxel_reduce_small_kernel(Groups gr, Batch bt)
{
    const Field f = bt.f[blockIdx.y];
    const Counts cn = load_counts(gr);
    const uint32_t w = f.width;
    const uint32_t gpb = w < (uint32_t)kBlock ? kBlock / w : 1u;
    const uint32_t gl = threadIdx.x / w, c0 = threadIdx.x % w;  // gl == 0 where w >= 256
    if (gl >= gpb) return;
    const bool weighted = gr.weights != nullptr;
    for (unsigned long long gb = blockIdx.x; gb * gpb < cn.ng; gb += gridDim.x) {
        const unsigned long long g64 = gb * gpb + gl;
        if (g64 >= cn.ng) continue;
        const uint32_t g = (uint32_t)g64;
        uint32_t a, e;
        group_span(gr, cn, g, a, e);
        if (f.op == HIDEGS_VOXEL_FIRST) {
            const uint32_t row = first_row(gr, f, a, e);
            for (uint32_t c = c0; c < w; c += kBlock)
                f.out[(size_t)g * w + c] = row != 0xffffffffu ? f.src[(size_t)row * w + c] : 0.f;
        } else if (e - a <= kSmallMax) {
            for (uint32_t c = c0; c < w; c += kBlock)
                f.out[(size_t)g * w + c] = acc_result(reduce_rows(gr, f, a, e, 1u, c, true), f.op, weighted);
        }
    }
}

// Medium groups: one wave per group, the waves striding over the groups (consecutive groups, which are of
// like size where the cloud is dense, go to different waves).
__global__ __launch_bounds__(kBlock) void voxel_reduce_wave_kernel(Groups gr, Batch bt)
{
    const Field f = bt.f[blockIdx.y];
    if (f.op == HIDEGS_VOXEL_FIRST) return;
    const Counts cn = load_counts(gr);
    const uint32_t w = f.width, L = lanes_per_row(w), R = kWave / L;
    const uint32_t lane = lane_id(), slot = lane / L, cl = lane & (L - 1);
    const bool weighted = gr.weights != nullptr;
    for (unsigned long long g64 = (unsigned long long)blockIdx.x * kWaves + threadIdx.x / kWave; g64 < cn.ng;
         g64 += (unsigned long long)gridDim.x * kWaves) {  // wave-uniform
        const uint32_t g = (uint32_t)g64;
        uint32_t a, e;
        group_span(gr, cn, g, a, e);
        if (e - a <= kSmallMax || e - a > kChunk) continue;
        for (uint32_t cb = 0; cb < w; cb += L) {
            const uint32_t c = cb + cl;
            Acc acc = reduce_rows(gr, f, a + slot, e, R, c, c < w);
            acc = wave_merge_columns(acc, L, f.op);
            if (slot == 0 && c < w) f.out[(size_t)g * w + c] = acc_result(acc, f.op, weighted);
        }
    }
}

// Largest g < G with starts[g] <= p (starts[0] = 0; G >= 1).
__device__ __forceinline__ uint32_t find_group(const uint32_t* __restrict__ starts, uint32_t G, uint32_t p)
{
    uint32_t lo = 0, hi = G;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (starts[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// The partial of (slot, field i of the set): stride floats -- width values, the weight sum, the row count.
__device__ __forceinline__ size_t partial_at(uint32_t stride, uint32_t slot, int i)
{
    return ((size_t)slot * kMaxFields + i) * stride;
}

// The accumulators of the workgroup's threads that hold one column (threadIdx.x & (L - 1) equal): the tree
// inside each wave, then the four waves in order.  The result is valid in wave 0's lanes below L.
__device__ __forceinline__ Acc block_merge_columns(Acc acc, uint32_t L, int op, Acc (*s_acc)[kWave])
{
    const uint32_t wave = threadIdx.x / kWave, lane = lane_id();
    acc = wave_merge_columns(acc, L, op);
    s_acc[wave][lane] = acc;
    __syncthreads();
    Acc t = s_acc[0][lane];
    if (wave == 0)
        for (int v = 1; v < kWaves; v++) t = acc_merge(t, s_acc[v][lane], op);
    __syncthreads();  // s_acc is reused
    return t;
}

// Large groups: the chunks that start in this workgroup's window of kChunk positions.
__global__ __launch_bounds__(kBlock) void voxel_reduce_chunk_kernel(Groups gr, Batch bt, float* __restrict__ partials,
                                                                    uint32_t stride)
{
    __shared__ Acc s_acc[kWaves][kWave];
    const Field f = bt.f[blockIdx.y];
    if (f.op == HIDEGS_VOXEL_FIRST) return;
    const Counts cn = load_counts(gr);
    const uint32_t p0 = blockIdx.x * kChunk;
    if (p0 >= cn.m || cn.ng == 0) return;
    const uint32_t p1 = min(p0 + kChunk, cn.m) - 1;
    const uint32_t gA = find_group(gr.starts, cn.G, p0), gB = find_group(gr.starts, cn.G, p1);
    const uint32_t w = f.width, L = lanes_per_row(w), R = kBlock / L;
    const uint32_t slot = threadIdx.x / L, cl = threadIdx.x & (L - 1);
    for (uint32_t which = 0; which < 2; which++) {  // everything below is workgroup-uniform up to the merge
        const uint32_t g = which ? gB : gA;
        if ((which && gB == gA) || g >= cn.ng) continue;
        uint32_t a, e;
        group_span(gr, cn, g, a, e);
        if (e - a <= kChunk) continue;
        uint32_t s;
        if (which == 0) {  // the group covers p0: its chunk that starts at or after p0
            if (a > p0) continue;
            s = a + (p0 - a + kChunk - 1) / kChunk * kChunk;
        } else {  // the group starts inside the window: its chunk 0
            if (a <= p0) continue;
            s = a;
        }
        if (s > p1 || s >= e) continue;
        const uint32_t end = min(s + kChunk, e);
        float* part = partials + partial_at(stride, 2 * blockIdx.x + which, blockIdx.y);
        for (uint32_t cb = 0; cb < w; cb += L) {
            const uint32_t c = cb + cl;
            const Acc t = block_merge_columns(reduce_rows(gr, f, s + slot, end, R, c, c < w), L, f.op, s_acc);
            if (threadIdx.x < L) {  // wave 0, lane == cl
                if (c < w) part[c] = t.v;
                if (c == 0) {
                    part[w] = t.ws;
                    part[w + 1] = __uint_as_float(t.cnt);
                }
            }
        }
    }
}

// The large group that starts in this workgroup's window, if any.  Its partials are added as its rows were:
// L threads share a chunk, 256 / L chunks are in flight, every thread adds its chunks in chunk order, then the
// tree and the four waves in order.
__global__ __launch_bounds__(kBlock) void voxel_reduce_finish_kernel(Groups gr, Batch bt,
                                                                     const float* __restrict__ partials, uint32_t stride)
{
    __shared__ Acc s_acc[kWaves][kWave];
    const Field f = bt.f[blockIdx.y];
    if (f.op == HIDEGS_VOXEL_FIRST) return;
    const Counts cn = load_counts(gr);
    const uint32_t p0 = blockIdx.x * kChunk;
    if (p0 >= cn.m || cn.ng == 0) return;
    const uint32_t p1 = min(p0 + kChunk, cn.m) - 1;
    const uint32_t g = find_group(gr.starts, cn.G, p1);
    if (g >= cn.ng) return;
    uint32_t a, e;
    group_span(gr, cn, g, a, e);
    if (a < p0 || a > p1 || e - a <= kChunk) return;  // workgroup-uniform, like everything above
    const uint32_t w = f.width, nchunks = (e - a + kChunk - 1) / kChunk;
    const uint32_t L = lanes_per_row(w), R = kBlock / L;
    const uint32_t slot = threadIdx.x / L, cl = threadIdx.x & (L - 1);
    const bool weighted = gr.weights != nullptr;
    // chunk k starts at position a + k * kChunk, in window (a + k * kChunk) / kChunk; it has slot 1 there only as
    // chunk 0 of a group that starts inside the window
    const uint32_t win0 = a / kChunk, odd0 = a % kChunk != 0 ? 1u : 0u;
    for (uint32_t cb = 0; cb < w; cb += L) {
        const uint32_t c = cb + cl;
        Acc acc = acc_init(f.op);
        for (uint32_t k = slot; k < nchunks; k += R) {
            const uint32_t pslot = k == 0 ? 2 * win0 + odd0 : 2 * ((a + k * kChunk) / kChunk);
            const float* part = partials + partial_at(stride, pslot, blockIdx.y);
            Acc b;
            b.v = c < w ? part[c] : 0.f;
            b.ws = part[w];
            b.cnt = __float_as_uint(part[w + 1]);
            acc = acc_merge(acc, b, f.op);
        }
        const Acc t = block_merge_columns(acc, L, f.op, s_acc);
        if (threadIdx.x < L && c < w) f.out[(size_t)g * w + c] = acc_result(t, f.op, weighted);
    }
}

long long windows_of(long long P) { return (P + kChunk - 1) / kChunk; }

size_t reduce_scratch(long long P, int max_width)
{
    return align_up((size_t)2 * windows_of(P) * kMaxFields * ((size_t)max_width + 2) * sizeof(float));
}

bool in_range(long long n) { return n >= 0 && n <= kVoxelMax; }

int grid_of(long long blocks) { return (int)std::min<long long>(std::max<long long>(blocks, 1), kGridCap); }

}  // namespace
}  // namespace hidegs

extern "C" size_t hidegs_voxel_group_scratch_bytes(long long P)
{
    return P > 0 && hidegs::in_range(P) ? hidegs::group_layout(nullptr, P).total : 0;
}

extern "C" int hidegs_voxel_group(void* scratch, size_t scratch_bytes, const float* points, const unsigned char* among,
                                  long long P, float cell, const float* origin, int32_t* group_of, uint32_t* order,
                                  uint32_t* starts, unsigned char* first_flags, float* frame, uint32_t* info,
                                  void* stream)
{
    using namespace hidegs;
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_voxel_group", s)) return rc;
    if (!in_range(P)) return fail(HIDEGS_E_ARG, "voxel_group: P must be in [0, 2^31)");
    if (!(cell > 0.f) || !(cell < INFINITY)) return fail(HIDEGS_E_ARG, "voxel_group: cell must be finite and > 0");
    const float inv = 1.0f / cell;
    if (!(inv < INFINITY)) return fail(HIDEGS_E_ARG, "voxel_group: cell is so small that 1 / cell overflows");
    if (!starts) return fail(HIDEGS_E_ARG, "voxel_group: NULL starts");
    if (!frame) return fail(HIDEGS_E_ARG, "voxel_group: NULL frame");
    if (!info) return fail(HIDEGS_E_ARG, "voxel_group: NULL info");
    if (P > 0) {
        if (!points) return fail(HIDEGS_E_ARG, "voxel_group: NULL points");
        if (!group_of) return fail(HIDEGS_E_ARG, "voxel_group: NULL group_of");
        if (!order) return fail(HIDEGS_E_ARG, "voxel_group: NULL order");
        if (!scratch || scratch_bytes < group_layout(nullptr, P).total)
            return fail(HIDEGS_E_ARG, "voxel_group: scratch NULL or too small");
    }
    const GroupLayout l = group_layout(scratch, P);
    const int nb = (int)((P + kBlock - 1) / kBlock);
    const int nbound = origin || P == 0 ? 0 : std::min(kBoundBlocks, nb);
    if (nbound)
        HIDEGS_LAUNCH("voxel_bounds", voxel_bounds_kernel, dim3(nbound), dim3(kBlock), 0, s, points, among, P, l.partials);
    if (P == 0) {  // frame, and info = {0, 0, 0, 0}, starts[0] = 0
        if (hipMemsetAsync(info, 0, 4 * sizeof(uint32_t), s) != hipSuccess ||
            hipMemsetAsync(starts, 0, sizeof(uint32_t), s) != hipSuccess)
            return fail(HIDEGS_E_HIP, "voxel_group: clearing info failed");
        HIDEGS_LAUNCH("voxel_frame", voxel_frame_kernel, dim3(1), dim3(kBlock), 0, s, origin, (const float*)nullptr, 0, cell,
                      frame, info + 2);
        return check_launch("voxel_group", s, 0);
    }
    HIDEGS_LAUNCH("voxel_frame", voxel_frame_kernel, dim3(1), dim3(kBlock), 0, s, origin, (const float*)l.partials, nbound,
                  cell, frame, l.counter);
    HIDEGS_LAUNCH("voxel_keys", voxel_keys_kernel, dim3(nb), dim3(kBlock), 0, s, points, among, P, (const float*)frame, inv,
                  l.keys, l.vals, l.counter);
    if (int rc = sort_pairs_u64(l.sort_tmp, l.sort_bytes, l.keys, l.keys_sorted, l.vals, l.vals_sorted, P, 0, 64, s))
        return rc;
    HIDEGS_LAUNCH("voxel_heads", voxel_heads_kernel, dim3(nb), dim3(kBlock), 0, s, (const uint64_t*)l.keys_sorted, P, l.rank);
    if (int rc = inclusive_scan_u32(l.scan_tmp, l.scan_bytes, l.rank, l.rank, P, s)) return rc;
    HIDEGS_LAUNCH("voxel_assign", voxel_assign_kernel, dim3(nb), dim3(kBlock), 0, s, (const uint64_t*)l.keys_sorted,
                  (const uint32_t*)l.vals_sorted, (const uint32_t*)l.rank, P, (const uint32_t*)l.counter, group_of, order,
                  starts, info);
    HIDEGS_LAUNCH("voxel_flags", voxel_flags_kernel, dim3(nb), dim3(kBlock), 0, s, (const uint64_t*)l.keys_sorted,
                  (const uint32_t*)l.vals_sorted, (const uint32_t*)l.rank, P, (const uint32_t*)starts, first_flags, info);
    return check_launch("voxel_group", s, 0);
}

extern "C" size_t hidegs_voxel_reduce_scratch_bytes(long long P, long long max_groups, int max_width)
{
    (void)max_groups;  // the partials are per window of the cloud, not per group
    return P > 0 && hidegs::in_range(P) && max_width >= 1 ? hidegs::reduce_scratch(P, max_width) : 0;
}

extern "C" int hidegs_voxel_reduce_rows(void* scratch, size_t scratch_bytes, const hidegs_voxel_field* fields, int nfields,
                                        const uint32_t* order, const uint32_t* starts, const uint32_t* info, long long P,
                                        long long max_groups, const float* weights, void* stream)
{
    using namespace hidegs;
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_voxel_reduce_rows", s)) return rc;
    if (!in_range(P)) return fail(HIDEGS_E_ARG, "voxel_reduce_rows: P must be in [0, 2^31)");
    if (max_groups < 0) return fail(HIDEGS_E_ARG, "voxel_reduce_rows: negative max_groups");
    if (nfields < 0) return fail(HIDEGS_E_ARG, "voxel_reduce_rows: negative field count");
    if (nfields > 0 && !fields) return fail(HIDEGS_E_ARG, "voxel_reduce_rows: NULL field list");
    int max_width = 1;
    for (int i = 0; i < nfields; i++) {
        const hidegs_voxel_field& f = fields[i];
        const std::string who = "voxel_reduce_rows: field " + std::to_string(i);
        if (f.width < 1) return fail(HIDEGS_E_ARG, who + ": width must be >= 1");
        if (f.op < HIDEGS_VOXEL_SUM || f.op > HIDEGS_VOXEL_FIRST) return fail(HIDEGS_E_ARG, who + ": unknown op");
        if (f.n_rows < 0) return fail(HIDEGS_E_ARG, who + ": negative n_rows");
        max_width = std::max(max_width, f.width);
    }
    if (P == 0 || nfields == 0 || max_groups == 0) return 0;
    for (int i = 0; i < nfields; i++) {
        const std::string who = "voxel_reduce_rows: field " + std::to_string(i);
        if (fields[i].n_rows > 0 && !fields[i].src) return fail(HIDEGS_E_ARG, who + ": NULL src");
        if (!fields[i].out) return fail(HIDEGS_E_ARG, who + ": NULL out");
    }
    if (!order) return fail(HIDEGS_E_ARG, "voxel_reduce_rows: NULL order");
    if (!starts) return fail(HIDEGS_E_ARG, "voxel_reduce_rows: NULL starts");
    if (!info) return fail(HIDEGS_E_ARG, "voxel_reduce_rows: NULL info");
    if (!scratch || scratch_bytes < reduce_scratch(P, max_width))
        return fail(HIDEGS_E_ARG, "voxel_reduce_rows: scratch NULL or too small");
    const long long ng = std::min(max_groups, P);  // there are at most P groups
    const Groups gr{order, starts, info, weights, (uint32_t)P, (uint32_t)ng};
    const uint32_t stride = (uint32_t)max_width + 2;
    float* partials = static_cast<float*>(scratch);
    for (int i0 = 0; i0 < nfields; i0 += kMaxFields) {  // kMaxFields per launch set
        const int count = std::min(kMaxFields, nfields - i0);
        Batch bt = {};
        long long small_blocks = 1;
        for (int i = 0; i < count; i++) {
            const hidegs_voxel_field& f = fields[i0 + i];
            const long long rows = weights ? std::min(f.n_rows, P) : f.n_rows;
            bt.f[i] = Field{f.src, f.out, (uint32_t)std::min<long long>(rows, 1ll << 31), (uint32_t)f.width, f.op};
            const long long gpb = f.width < kBlock ? kBlock / f.width : 1;
            small_blocks = std::max(small_blocks, (ng + gpb - 1) / gpb);
        }
        HIDEGS_LAUNCH("voxel_reduce_small", voxel_reduce_small_kernel, dim3(grid_of(small_blocks), count), dim3(kBlock), 0, s,
                      gr, bt);
        if (P > kSmallMax)  // no larger group otherwise
            HIDEGS_LAUNCH("voxel_reduce_wave", voxel_reduce_wave_kernel, dim3(grid_of((ng + kWaves - 1) / kWaves), count),
                          dim3(kBlock), 0, s, gr, bt);
        if (P > kChunk) {
            const dim3 grid((unsigned)windows_of(P), count);
            HIDEGS_LAUNCH("voxel_reduce_chunk", voxel_reduce_chunk_kernel, grid, dim3(kBlock), 0, s, gr, bt, partials, stride);
            HIDEGS_LAUNCH("voxel_reduce_finish", voxel_reduce_finish_kernel, grid, dim3(kBlock), 0, s, gr, bt,
                          (const float*)partials, stride);
        }
    }
    return check_launch("voxel_reduce_rows", s, 0);
}
