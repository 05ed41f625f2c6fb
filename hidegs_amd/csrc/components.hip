// components.hip -- connected components over neighbour lists (include/hidegs_components.h): the forest's begin,
// the two linking kernels that read lists, and finish.  find and unite are union_find.h's, shared with the fused
// walk of nearest_components.h; the rule and its termination argument are stated there and in the header.
//
//   components_begin   one lane per row: parent[i] = i or -1.
//   components_table   one lane per table entry (Q * k of them, 64-bit, striding past the grid cap): neighbouring
//                      lanes read neighbouring words, and a row's k entries sit in k lanes of one or two waves.
//   components_lists   one wave per 64 consecutive lists.  A lane walks the first kLaneEntries entries of its own
//                      list; what a list holds beyond that is served by the whole wave, 64 entries per round, list
//                      after list (a ballot names them, v_readlane hands their span on).  Short lists, the common
//                      case of a radius search, cost no idle lanes, and no list of any length is walked by one
//                      lane.  It needs no scratch and no second launch, which a list of long lists would.
//   components_flatten one lane per row: parent[i] = its root, or -1; clears the row's counter.
//   components_count   one lane per row: the counter of the row's label goes up.  The lanes of a wave that share
//                      a label issue one add of their number (a ballot per distinct label of the wave), so one
//                      giant component costs one atomic per wave, not 64 on one address.  Also the root flags,
//                      and C and the number of nodes by one atomic each per wave.
//   components_sizes   one lane per row: size_out, and the largest (size, lowest label) by one 64-bit integer
//                      maximum per wave.
//   components_ids     one lane per row: ids_out from the scan of the root flags; one thread writes info_out.
// Integer atomics only; no workgroup waits on another; capped launches stride past their caps.
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/hidegs_components.h"
#include "common.h"
#include "union_find.h"

namespace hidegs {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;  // 4
constexpr long long kComponentsMax = 0x7fffffffLL;
constexpr int kGridCap = 8192;           // workgroups at most: 32 per CU, then by stride
constexpr uint32_t kLaneEntries = 16;    // entries of its own list that a lane walks before the wave takes over

__global__ __launch_bounds__(kBlock) void components_begin_kernel(int32_t* __restrict__ parent, uint32_t N,
                                                                  const unsigned char* __restrict__ among)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < N;
         i += (unsigned long long)gridDim.x * kBlock)
        parent[i] = !among || among[i] ? (int32_t)i : -1;
}

// The edge {s, r} where both are rows; unite skips it where either is no node.
__device__ __forceinline__ void link(int32_t* __restrict__ parent, uint32_t N, int32_t s, int32_t r)
{
    if ((uint32_t)s < N && (uint32_t)r < N) uf_unite(parent, s, r);  // a negative row is above every N
}

__global__ __launch_bounds__(kBlock) void components_table_kernel(int32_t* __restrict__ parent, uint32_t N,
                                                                  const int32_t* __restrict__ sources,
                                                                  const int32_t* __restrict__ table, uint32_t Q, uint32_t k)
{
    const unsigned long long total = (unsigned long long)Q * k;
    for (unsigned long long e = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; e < total;
         e += (unsigned long long)gridDim.x * kBlock) {
        const uint32_t j = (uint32_t)(e / k);
        link(parent, N, sources ? sources[j] : (int32_t)j, table[e]);
    }
}

__global__ __launch_bounds__(kBlock) void components_lists_kernel(int32_t* __restrict__ parent, uint32_t N,
                                                                  const int32_t* __restrict__ sources,
                                                                  const int32_t* __restrict__ starts,
                                                                  const int32_t* __restrict__ rows, uint32_t capacity, uint32_t Q)
{
    const uint32_t lane = (uint32_t)lane_id();
    for (unsigned long long base = ((unsigned long long)blockIdx.x * kWaves + threadIdx.x / kWave) * kWave; base < Q;
         base += (unsigned long long)gridDim.x * kBlock) {  // wave-uniform
        const unsigned long long j = base + lane;
        int32_t s = -1, a = 0;
        uint32_t L = 0;
        if (j < Q) {
            s = sources ? sources[j] : (int32_t)j;
            a = max(starts[j], 0);
            const int32_t e = min(starts[j + 1], (int32_t)capacity);  // nothing at or past capacity is inside
            L = e > a && (uint32_t)s < N ? (uint32_t)(e - a) : 0u;
        }
        for (uint32_t i = 0; i < min(L, kLaneEntries); i++) link(parent, N, s, rows[a + i]);
        uint64_t longer = __ballot(L > kLaneEntries);
        while (longer) {  // wave-uniform
            const int l = __builtin_ctzll(longer);
            longer &= longer - 1;
            const int32_t sl = __builtin_amdgcn_readlane(s, l), al = __builtin_amdgcn_readlane(a, l);
            const uint32_t Ll = (uint32_t)__builtin_amdgcn_readlane((int)L, l);
            for (uint32_t i = kLaneEntries + lane; i < Ll; i += kWave) link(parent, N, sl, rows[al + i]);
        }
    }
}

__global__ __launch_bounds__(kBlock) void components_flatten_kernel(int32_t* __restrict__ parent, uint32_t N,
                                                                    uint32_t* __restrict__ cnt)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < N;
         i += (unsigned long long)gridDim.x * kBlock) {
        int32_t seen, label = -1;
        if (uf_load(parent + i) >= 0) label = uf_find<true>(parent, (int32_t)i, seen);
        __hip_atomic_store(parent + i, label, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cnt[i] = 0;
    }
}

// counters: {C, the number of nodes}, cleared by the call.  flags may be NULL.
__global__ __launch_bounds__(kBlock) void components_count_kernel(const int32_t* __restrict__ parent, uint32_t N,
                                                                  uint32_t* __restrict__ cnt, uint32_t* __restrict__ flags,
                                                                  uint32_t* __restrict__ counters)
{
    const int lane = lane_id();
    uint32_t roots = 0, nodes = 0;
    for (unsigned long long base = (unsigned long long)blockIdx.x * kBlock; base < N;
         base += (unsigned long long)gridDim.x * kBlock) {  // workgroup-uniform
        const unsigned long long i = base + threadIdx.x;
        const int32_t label = i < N ? parent[i] : -1;
        const bool node = (uint32_t)label < N, root = node && (uint32_t)label == i;
        if (flags && i < N) flags[i] = root;
        uint64_t left = __ballot(node);
        nodes += (uint32_t)__popcll(left);
        roots += (uint32_t)__popcll(__ballot(root));
        while (left) {  // one add per distinct label of the wave
            const int lead = __builtin_ctzll(left);
            const int32_t ll = __builtin_amdgcn_readlane(label, lead);
            const uint64_t same = __ballot(node && label == ll);
            if (lane == lead) atomicAdd(cnt + ll, (uint32_t)__popcll(same));
            left &= ~same;
        }
    }
    if (lane == 0 && nodes) {
        atomicAdd(counters, roots);
        atomicAdd(counters + 1, nodes);
    }
}

// best: (size << 32 | ~label) of the largest component, the lowest label among equals; cleared by the call.
__global__ __launch_bounds__(kBlock) void components_sizes_kernel(const int32_t* __restrict__ parent, uint32_t N,
                                                                  const uint32_t* __restrict__ cnt, int32_t* __restrict__ size_out,
                                                                  unsigned long long* __restrict__ best)
{
    unsigned long long mine = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < N;
         i += (unsigned long long)gridDim.x * kBlock) {
        const int32_t label = parent[i];
        const uint32_t size = (uint32_t)label < N ? cnt[label] : 0u;
        if (size_out) size_out[i] = (int32_t)size;
        if ((uint32_t)label == i) mine = max(mine, ((unsigned long long)size << 32) | (0xffffffffu - (uint32_t)label));
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mine = max(mine, (unsigned long long)__shfl_xor(mine, m, kWave));
    if (lane_id() == 0 && mine) atomicMax(best, mine);
}

// rank: the inclusive scan of the root flags, or NULL with ids_out.
__global__ __launch_bounds__(kBlock) void components_ids_kernel(const int32_t* __restrict__ parent, uint32_t N,
                                                                const uint32_t* __restrict__ rank, int32_t* __restrict__ ids_out,
                                                                const unsigned long long* __restrict__ best,
                                                                const uint32_t* __restrict__ counters, int32_t* __restrict__ info_out)
{
    if (ids_out)
        for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < N;
             i += (unsigned long long)gridDim.x * kBlock) {
            const int32_t label = parent[i];
            ids_out[i] = (uint32_t)label < N ? (int32_t)(rank[label] - 1u) : -1;
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long b = *best;
        info_out[0] = (int32_t)counters[0];
        info_out[1] = (int32_t)counters[1];
        info_out[2] = (int32_t)(uint32_t)(b >> 32);
        info_out[3] = b ? (int32_t)(0xffffffffu - (uint32_t)b) : 0;
    }
}

bool in_range(long long n) { return n >= 0 && n <= kComponentsMax; }

bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && pa < pb + nb && pb < pa + na;
}

int row_grid(unsigned long long n) { return (int)std::min<unsigned long long>((n + kBlock - 1) / kBlock, kGridCap); }

struct FinishLayout {
    uint32_t *cnt, *flags;
    unsigned long long* best;  // then the two counters: 16 bytes, cleared together
    void* scan_tmp;
    size_t scan_bytes, total;
};

FinishLayout finish_layout(void* base, long long N)
{
    FinishLayout l;
    Carver c(base);
    l.cnt = c.take<uint32_t>((size_t)N);
    l.flags = c.take<uint32_t>((size_t)N);
    l.best = c.take<unsigned long long>(2);
    l.scan_bytes = hidegs_scan_scratch_bytes(N);
    l.scan_tmp = c.take<char>(l.scan_bytes);
    l.total = c.used;
    return l;
}

// The checks that the two list forms share; `who` names the entry point.
int check_add(const std::string& who, const int32_t* parent, long long N, const int32_t* sources, long long Q)
{
    if (!in_range(N)) return fail(HIDEGS_E_ARG, who + ": N must be in [0, 2^31)");
    if (!in_range(Q)) return fail(HIDEGS_E_ARG, who + ": Q must be in [0, 2^31)");
    if (!sources && Q > N) return fail(HIDEGS_E_ARG, who + ": Q must not exceed N without sources");
    if (Q == 0) return 0;
    if (N > 0 && !parent) return fail(HIDEGS_E_ARG, who + ": NULL parent");
    if (overlap(parent, (size_t)N * 4, sources, (size_t)Q * 4)) return fail(HIDEGS_E_ARG, who + ": sources overlaps parent");
    return 0;
}

}  // namespace
}  // namespace hidegs

extern "C" int hidegs_components_begin(int32_t* parent, long long N, const unsigned char* among, void* stream)
{
    using namespace hidegs;
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_components_begin", s)) return rc;
    if (!in_range(N)) return fail(HIDEGS_E_ARG, "components_begin: N must be in [0, 2^31)");
    if (N == 0) return 0;
    if (!parent) return fail(HIDEGS_E_ARG, "components_begin: NULL parent");
    if (overlap(parent, (size_t)N * 4, among, (size_t)N)) return fail(HIDEGS_E_ARG, "components_begin: among overlaps parent");
    HIDEGS_LAUNCH("components_begin", components_begin_kernel, dim3(row_grid(N)), dim3(kBlock), 0, s, parent, (uint32_t)N, among);
    return check_launch("components_begin", s, 0);
}

extern "C" int hidegs_components_add_table(int32_t* parent, long long N, const int32_t* sources, const int32_t* table,
                                           long long Q, int k, void* stream)
{
    using namespace hidegs;
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_components_add_table", s)) return rc;
    if (k < 1) return fail(HIDEGS_E_ARG, "components_add_table: k must be >= 1");
    if (int rc = check_add("components_add_table", parent, N, sources, Q)) return rc;
    if (Q == 0) return 0;
    if (!table) return fail(HIDEGS_E_ARG, "components_add_table: NULL table");
    if (overlap(parent, (size_t)N * 4, table, (size_t)Q * k * 4))
        return fail(HIDEGS_E_ARG, "components_add_table: table overlaps parent");
    if (N == 0) return 0;  // no row, no edge
    HIDEGS_LAUNCH("components_table", components_table_kernel, dim3(row_grid((unsigned long long)Q * k)), dim3(kBlock), 0, s, parent,
                  (uint32_t)N, sources, table, (uint32_t)Q, (uint32_t)k);
    return check_launch("components_add_table", s, 0);
}

extern "C" int hidegs_components_add_lists(int32_t* parent, long long N, const int32_t* sources, const int32_t* starts,
                                           const int32_t* rows, long long capacity, long long Q, void* stream)
{
    using namespace hidegs;
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_components_add_lists", s)) return rc;
    if (!in_range(capacity)) return fail(HIDEGS_E_ARG, "components_add_lists: capacity must be in [0, 2^31)");
    if (int rc = check_add("components_add_lists", parent, N, sources, Q)) return rc;
    if (Q == 0) return 0;
    if (!starts) return fail(HIDEGS_E_ARG, "components_add_lists: NULL starts");
    if (capacity > 0 && !rows) return fail(HIDEGS_E_ARG, "components_add_lists: NULL rows");
    if (overlap(parent, (size_t)N * 4, starts, (size_t)(Q + 1) * 4))
        return fail(HIDEGS_E_ARG, "components_add_lists: starts overlaps parent");
    if (overlap(parent, (size_t)N * 4, rows, (size_t)capacity * 4))
        return fail(HIDEGS_E_ARG, "components_add_lists: rows overlaps parent");
    if (N == 0 || capacity == 0) return 0;  // no row or no entry: no edge
    HIDEGS_LAUNCH("components_lists", components_lists_kernel, dim3(row_grid(Q)), dim3(kBlock), 0, s, parent, (uint32_t)N, sources,
                  starts, rows, (uint32_t)capacity, (uint32_t)Q);
    return check_launch("components_add_lists", s, 0);
}

extern "C" size_t hidegs_components_finish_scratch_bytes(long long N)
{
    return N > 0 && hidegs::in_range(N) ? hidegs::finish_layout(nullptr, N).total : 0;
}

extern "C" int hidegs_components_finish(void* scratch, size_t scratch_bytes, int32_t* parent, long long N, int32_t* size_out,
                                        int32_t* ids_out, int32_t* info_out, void* stream)
{
    using namespace hidegs;
    const std::string who = "components_finish: ";
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_components_finish", s)) return rc;
    if (!in_range(N)) return fail(HIDEGS_E_ARG, who + "N must be in [0, 2^31)");
    if (!info_out) return fail(HIDEGS_E_ARG, who + "NULL info_out");
    if (N > 0) {
        if (!parent) return fail(HIDEGS_E_ARG, who + "NULL parent");
        if (!scratch || !aligned16(scratch) || scratch_bytes < finish_layout(nullptr, N).total)
            return fail(HIDEGS_E_ARG, who + "scratch buffer NULL, not 16-byte aligned or too small");
    } else {
        scratch = nullptr, scratch_bytes = 0;  // not used
    }
    const size_t rows = (size_t)N * 4;
    struct {
        const void* p;
        size_t n;
        const char* name;
    } const outs[3] = {{size_out, rows, "size_out"}, {ids_out, rows, "ids_out"}, {info_out, 16, "info_out"}},
            ins[2] = {{parent, rows, "parent"}, {scratch, scratch_bytes, "scratch"}};
    for (const auto& out : outs)
        for (const auto& in : ins)
            if (overlap(out.p, out.n, in.p, in.n)) return fail(HIDEGS_E_ARG, who + out.name + " overlaps " + in.name);
    for (int a = 0; a < 3; a++)
        for (int b = a + 1; b < 3; b++)
            if (overlap(outs[a].p, outs[a].n, outs[b].p, outs[b].n))
                return fail(HIDEGS_E_ARG, who + outs[b].name + " overlaps " + outs[a].name);
    if (overlap(parent, rows, scratch, scratch_bytes)) return fail(HIDEGS_E_ARG, who + "scratch overlaps parent");
    if (N == 0) {
        if (hipMemsetAsync(info_out, 0, 16, s) != hipSuccess) return fail(HIDEGS_E_HIP, who + "clearing info_out failed");
        return check_launch("components_finish", s, 0);
    }
    const FinishLayout l = finish_layout(scratch, N);
    uint32_t* counters = reinterpret_cast<uint32_t*>(l.best + 1);
    if (hipMemsetAsync(l.best, 0, 16, s) != hipSuccess) return fail(HIDEGS_E_HIP, who + "clearing the counters failed");
    const dim3 grid(row_grid(N)), block(kBlock);
    const uint32_t n = (uint32_t)N;
    uint32_t* flags = ids_out ? l.flags : nullptr;
    HIDEGS_LAUNCH("components_flatten", components_flatten_kernel, grid, block, 0, s, parent, n, l.cnt);
    HIDEGS_LAUNCH("components_count", components_count_kernel, grid, block, 0, s, (const int32_t*)parent, n, l.cnt, flags, counters);
    HIDEGS_LAUNCH("components_sizes", components_sizes_kernel, grid, block, 0, s, (const int32_t*)parent, n, (const uint32_t*)l.cnt,
                  size_out, l.best);
    if (ids_out)
        if (int rc = hidegs_inclusive_scan_u32(l.scan_tmp, l.scan_bytes, flags, flags, N, stream)) return rc;
    HIDEGS_LAUNCH("components_ids", components_ids_kernel, ids_out ? grid : dim3(1), block, 0, s, (const int32_t*)parent, n,
                  (const uint32_t*)flags, ids_out, (const unsigned long long*)l.best, (const uint32_t*)counters, info_out);
    return check_launch("components_finish", s, 0);
}
