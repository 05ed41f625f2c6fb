// neighbor_reduce.hip -- per-row fields reduced over neighbour lists (include/hidegs_neighbor_reduce.h).
//
// The rule is that of moments.hip: a list is cut into blocks of kSum = 64 positions, a block's partial is a
// sequential sum from +0.0f, a total is block 0's partial plus the partials of the later blocks in block order.
// The work is a gather of whole rows, so the lanes are dealt by the width of the rows:
//   a group of G lanes shares one list, G = 1 where every field of the launch is at most kNarrow floats wide and
//   otherwise the power of two at or above min(widest field, 64), at least 8.  Lane g of the group takes the
//   columns g, g + G, ... of every row, so a row is read as contiguous lines; a wave holds 64 / G lists side by
//   side and every group walks its own list in the rule's order.  With G = 1 the lane reads the whole row in one
//   dwordx2/x3/x4 load.  A group reads G entries' indices and weights in one coalesced load and hands them round
//   (ds_bpermute); kInFlight entries' rows are loaded before their additions.  A one-lane group loads
//   kInFlightNarrow entries at a time, a whole chunk's indices and weights unpredicated so that the loads merge.
// Two kernels per G:
//   nreduce_group  one group per list, for lists of up to kGroupBlocks blocks, the groups striding over the
//                  queries.  A longer list is appended to the long list in scratch -- one ballot and one integer
//                  atomic per wave on a counter that the call clears -- and left alone;
//   nreduce_wave   one wave per long list over a fixed grid, the waves striding over the long list.  In a round
//                  the wave's 64 / G groups sum 64 / G consecutive blocks, one each, and every group then adds
//                  the round's partials in block order: the rule's order exactly.
// A table of more than kGroupBlocks * 64 columns has only long lists: nreduce_wave alone over every query.
// Up to kMaxFields fields share a launch: a list is walked once per field and per kColumns * G columns of it; the
// indices and weights of the later walks come from the cache.  count is one walk of the indices alone.
// There is no floating-point atomic and no workgroup waits on another; capped launches stride past their caps.
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/hidegs_neighbor_reduce.h"
#include "common.h"
#include "neighbor_sum.h"

namespace hidegs {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;  // 4
constexpr long long kReduceMax = 0x7fffffffLL;
constexpr int kMaxFields = 8;          // fields per launch set
constexpr uint32_t kGroupBlocks = 4;   // blocks of the longest list that one group sums
constexpr int kGroupGridCap = 8192;    // workgroups of nreduce_group: 32 per CU, then by stride
constexpr int kWaveGrid = 2048;        // workgroups of nreduce_wave: 8 per CU
constexpr int kNarrow = 4;             // floats of the widest row that one lane reads whole
constexpr int kColumns = 4;            // columns of a row that a lane of a group holds in one walk
constexpr int kInFlight = 4;           // entries of a group whose row loads are issued together
constexpr int kInFlightNarrow = 8;     // the same for the one-lane groups of narrow rows
constexpr int kInFlightWave = 2;       // and for the lanes of nreduce_wave with narrow rows, whose uniform values fill the SGPRs

struct Field {
    const float* src;
    float* out;
    uint32_t width;
    int op;
};

struct Fields {
    Field f[kMaxFields];
    int n;
};

struct Lists {
    const int32_t* table;  // (Q, k), or NULL: the list form
    const int32_t* starts;
    const int32_t* rows;
    const float* weights;        // (P) or NULL
    const float* entry_weights;  // laid out like the entries, or NULL
    uint32_t k, capacity, Q, P;
};

// The entries of query j < Q: positions at .. at + L of the table or of rows.  Nothing at or past capacity is
// inside it, whatever starts holds.
__device__ __forceinline__ void list_span(const Lists& ls, uint32_t j, size_t& at, uint32_t& L)
{
    if (ls.table) {
        at = (size_t)j * ls.k;
        L = ls.k;
    } else {
        const int32_t a = max(ls.starts[j], 0), e = min(ls.starts[j + 1], (int32_t)ls.capacity);
        at = (size_t)a;
        L = e > a ? (uint32_t)(e - a) : 0u;
    }
}

__device__ __forceinline__ const int32_t* entries(const Lists& ls) { return ls.table ? ls.table : ls.rows; }

// One entry as its lane loads it: the row, or -1 for an invalid one, and its weight.
template <bool kSumOp>
__device__ __forceinline__ void load_entry(const Lists& ls, const int32_t* __restrict__ ent, const float* __restrict__ ew,
                                           uint32_t i, uint32_t n, int32_t& r, float& w)
{
    r = i < n ? ent[i] : -1;
    if ((uint32_t)r >= ls.P) r = -1;  // a negative row is above every P
    w = 1.f;
    if (kSumOp && r >= 0) {
        if (ls.weights) w = ls.weights[r];
        if (ew) w = ls.weights ? w * ew[i] : ew[i];
    }
}

template <bool kSumOp>
__device__ __forceinline__ float start_value()
{
    return kSumOp ? 0.f : __uint_as_float(0x7fc00000u);  // fminf / fmaxf return the number where one side is a NaN
}

template <bool kSumOp>
__device__ __forceinline__ float combine(float acc, float w, float x, int op)
{
    if (kSumOp) return fmaf(w, x, acc);
    return op == HIDEGS_NEIGHBOR_MIN ? fminf(acc, x) : fmaxf(acc, x);
}

template <bool kSumOp>
__device__ __forceinline__ float join(float a, float b, int op)
{
    if (kSumOp) return a + b;
    return op == HIDEGS_NEIGHBOR_MIN ? fminf(a, b) : fmaxf(a, b);
}

// The partial of the n <= 64 entries ent[0 .. n) for the C columns c0 + g + c * G of the field, by the group of G
// lanes whose lane g this is: from the start value, the valid entries in ascending position.  W: the weights' sum.
template <int G, int C, bool kSumOp, int kNarrowLoads = kInFlightNarrow>
__device__ __forceinline__ void block_partial(const Lists& ls, const Field& fd, uint32_t c0, const int32_t* __restrict__ ent,
                                              const float* __restrict__ ew, uint32_t n, uint32_t g, float (&acc)[C], float& W)
{
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = start_value<kSumOp>();
    W = 0.f;
    if constexpr (G == 1) {  // the lane's own entries, the whole row of each in one load
        for (uint32_t i = 0; i < n; i += kNarrowLoads) {
            int32_t r[kNarrowLoads];
            float w[kNarrowLoads], x[kNarrowLoads][C];
            const bool weighted = kSumOp && ew;
            if (i + kNarrowLoads <= n) {  // whole: loads that can be merged
#pragma unroll
                for (int u = 0; u < kNarrowLoads; u++) r[u] = ent[i + u];
#pragma unroll
                for (int u = 0; u < kNarrowLoads; u++) w[u] = weighted ? ew[i + u] : 1.f;
            } else {
#pragma unroll
                for (int u = 0; u < kNarrowLoads; u++) r[u] = i + u < n ? ent[i + u] : -1;
#pragma unroll
                for (int u = 0; u < kNarrowLoads; u++) w[u] = weighted && i + u < n ? ew[i + u] : 1.f;
            }
#pragma unroll
            for (int u = 0; u < kNarrowLoads; u++) {
                if ((uint32_t)r[u] >= ls.P) r[u] = -1;  // a negative row is above every P; its weight is not used
                if (kSumOp && ls.weights && r[u] >= 0) w[u] = ew ? ls.weights[r[u]] * w[u] : ls.weights[r[u]];
            }
#pragma unroll
            for (int u = 0; u < kNarrowLoads; u++) {
                const float* __restrict__ p = fd.src + (size_t)(r[u] < 0 ? 0 : r[u]) * C;
#pragma unroll
                for (int c = 0; c < C; c++) x[u][c] = r[u] >= 0 ? p[c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kNarrowLoads; u++) {
                if (r[u] < 0) continue;
#pragma unroll
                for (int c = 0; c < C; c++) acc[c] = combine<kSumOp>(acc[c], w[u], x[u][c], fd.op);
                if (kSumOp) W = W + w[u];
            }
        }
    } else {
        static_assert(G % kInFlight == 0, "a group hands its entries round kInFlight at a time");
        for (uint32_t i = 0; i < n; i += G) {  // G entries: one coalesced load, then handed round
            int32_t mine;
            float wmine;
            load_entry<kSumOp>(ls, ent, ew, i + g, n, mine, wmine);
            const uint32_t m = min((uint32_t)G, n - i);  // the same in every lane of the group
            for (uint32_t u0 = 0; u0 < m; u0 += kInFlight) {
                int32_t r[kInFlight];
                float w[kInFlight], x[kInFlight][C];
#pragma unroll
                for (int u = 0; u < kInFlight; u++) {
                    r[u] = __shfl(mine, (int)(u0 + u), G);
                    w[u] = __shfl(wmine, (int)(u0 + u), G);
                }
#pragma unroll
                for (int u = 0; u < kInFlight; u++) {
                    const float* __restrict__ p = fd.src + (size_t)(r[u] < 0 ? 0 : r[u]) * fd.width;
#pragma unroll
                    for (int c = 0; c < C; c++) {
                        const uint32_t col = c0 + g + c * G;
                        x[u][c] = (r[u] >= 0 && col < fd.width) ? p[col] : 0.f;
                    }
                }
#pragma unroll
                for (int u = 0; u < kInFlight; u++) {
                    if (r[u] < 0) continue;  // the same in every lane of the group
#pragma unroll
                    for (int c = 0; c < C; c++) acc[c] = combine<kSumOp>(acc[c], w[u], x[u][c], fd.op);
                    if (kSumOp) W = W + w[u];
                }
            }
        }
    }
}

// What the lane writes of its C columns of query j.
template <int G, int C>
__device__ __forceinline__ void write_columns(const Field& fd, uint32_t j, uint32_t c0, uint32_t g, const float (&tot)[C], float W)
{
    float* __restrict__ o = fd.out + (size_t)j * fd.width;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const uint32_t col = G == 1 ? (uint32_t)c : c0 + g + c * G;
        if (col < fd.width) o[col] = fd.op == HIDEGS_NEIGHBOR_MEAN ? tot[c] / W : tot[c];
    }
}

// One group, the whole list: block 0's partial, then the later blocks' in block order.
template <int G, int C, bool kSumOp>
__device__ __forceinline__ void group_columns(const Lists& ls, const Field& fd, uint32_t c0, uint32_t j, size_t at, uint32_t L,
                                              uint32_t g)
{
    const int32_t* __restrict__ ent = entries(ls) + at;
    const float* __restrict__ ew = ls.entry_weights ? ls.entry_weights + at : nullptr;
    float tot[C], W = 0.f;
#pragma unroll
    for (int c = 0; c < C; c++) tot[c] = start_value<kSumOp>();
    for (uint32_t b = 0; b * kSum < L; b++) {
        float part[C], Wp;
        block_partial<G, C, kSumOp>(ls, fd, c0, ent + b * kSum, ew ? ew + b * kSum : nullptr, min(kSum, L - b * kSum), g, part, Wp);
#pragma unroll
        for (int c = 0; c < C; c++) tot[c] = b == 0 ? part[c] : join<kSumOp>(tot[c], part[c], fd.op);
        W = b == 0 ? Wp : W + Wp;
    }
    write_columns<G, C>(fd, j, c0, g, tot, W);
}

// One wave, the whole list (j, at and L wave-uniform): group q of the wave's 64 / G sums block b0 + q of a round,
// then every group adds the round's partials in block order.  Group 0 writes.
template <int G, int C, bool kSumOp>
__device__ __forceinline__ void wave_columns(const Lists& ls, const Field& fd, uint32_t c0, uint32_t j, size_t at, uint32_t L)
{
    constexpr uint32_t kGroups = kWave / G;
    const int32_t* __restrict__ ent = entries(ls) + at;
    const float* __restrict__ ew = ls.entry_weights ? ls.entry_weights + at : nullptr;
    const uint32_t nb = (L + kSum - 1) / kSum, lane = lane_id(), q = lane / G, g = lane % G;
    float tot[C], W = 0.f;
#pragma unroll
    for (int c = 0; c < C; c++) tot[c] = start_value<kSumOp>();
    for (uint32_t b0 = 0; b0 < nb; b0 += kGroups) {  // wave-uniform
        float part[C], Wp = 0.f;
#pragma unroll
        for (int c = 0; c < C; c++) part[c] = start_value<kSumOp>();
        const uint32_t b = b0 + q;
        if (b < nb)
            block_partial<G, C, kSumOp, kInFlightWave>(ls, fd, c0, ent + (size_t)b * kSum, ew ? ew + (size_t)b * kSum : nullptr,
                                        min(kSum, L - b * kSum), g, part, Wp);
        const uint32_t groups = min(kGroups, nb - b0);
        for (uint32_t s = 0; s < groups; s++) {
            const bool first = b0 == 0 && s == 0;
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float v = kGroups == 1 ? part[c] : __shfl(part[c], (int)(s * G + g), kWave);
                tot[c] = first ? v : join<kSumOp>(tot[c], v, fd.op);
            }
            if (kSumOp) {
                const float v = kGroups == 1 ? Wp : __shfl(Wp, (int)(s * G + g), kWave);
                W = first ? v : W + v;
            }
        }
    }
    if (q == 0) write_columns<G, C>(fd, j, c0, g, tot, W);
}

// Every field of the launch for one list: kWhole = false by the group of G lanes whose lane g this is, kWhole =
// true by the wave.
template <int G, bool kWhole, int C, bool kSumOp>
__device__ __forceinline__ void columns(const Lists& ls, const Field& fd, uint32_t c0, uint32_t j, size_t at, uint32_t L, uint32_t g)
{
    if constexpr (kWhole)
        wave_columns<G, C, kSumOp>(ls, fd, c0, j, at, L);
    else
        group_columns<G, C, kSumOp>(ls, fd, c0, j, at, L, g);
}

template <int G, bool kWhole, int C>
__device__ __forceinline__ void columns_op(const Lists& ls, const Field& fd, uint32_t c0, uint32_t j, size_t at, uint32_t L,
                                           uint32_t g)
{
    if (fd.op <= HIDEGS_NEIGHBOR_MEAN)
        columns<G, kWhole, C, true>(ls, fd, c0, j, at, L, g);
    else
        columns<G, kWhole, C, false>(ls, fd, c0, j, at, L, g);
}

template <int G, bool kWhole>
__device__ __forceinline__ void reduce_list(const Lists& ls, const Fields& fs, uint32_t j, size_t at, uint32_t L, uint32_t g)
{
    for (int i = 0; i < fs.n; i++) {  // uniform
        const Field fd = fs.f[i];
        if constexpr (G == 1) {  // every width of the launch is at most kNarrow
            switch (fd.width) {
            case 1: columns_op<1, kWhole, 1>(ls, fd, 0, j, at, L, 0); break;
            case 2: columns_op<1, kWhole, 2>(ls, fd, 0, j, at, L, 0); break;
            case 3: columns_op<1, kWhole, 3>(ls, fd, 0, j, at, L, 0); break;
            default: columns_op<1, kWhole, 4>(ls, fd, 0, j, at, L, 0); break;
            }
        } else {
            for (uint32_t c0 = 0; c0 < fd.width;) {
                if (fd.width - c0 <= (uint32_t)G) {
                    columns_op<G, kWhole, 1>(ls, fd, c0, j, at, L, g);
                    c0 += G;
                } else {
                    columns_op<G, kWhole, kColumns>(ls, fd, c0, j, at, L, g);
                    c0 += kColumns * G;
                }
            }
        }
    }
}

// The valid entries of the list, counted by the n lanes (a power of two, aligned) of which this is lane g.
__device__ __forceinline__ uint32_t count_valid(const Lists& ls, size_t at, uint32_t L, uint32_t g, uint32_t n)
{
    const int32_t* __restrict__ ent = entries(ls) + at;
    uint32_t c = 0;
    for (uint32_t i = g; i < L; i += n) c += (uint32_t)ent[i] < ls.P;
    for (uint32_t m = 1; m < n; m <<= 1) c += __shfl_xor(c, (int)m, kWave);
    return c;
}

template <int G>
__global__ __launch_bounds__(kBlock) void nreduce_group_kernel(Lists ls, Fields fs, int32_t* __restrict__ count,
                                                               uint32_t* __restrict__ long_list, uint32_t* __restrict__ long_count,
                                                               int append)
{
    constexpr int kLists = kBlock / G;  // lists of a workgroup
    const uint32_t g = threadIdx.x % G;
    for (unsigned long long base = (unsigned long long)blockIdx.x * kLists; base < ls.Q;
         base += (unsigned long long)gridDim.x * kLists) {  // workgroup-uniform
        const unsigned long long j64 = base + threadIdx.x / G;
        const bool active = j64 < ls.Q;
        const uint32_t j = (uint32_t)j64;
        size_t at = 0;
        uint32_t L = 0;
        if (active) list_span(ls, j, at, L);
        const bool is_long = L > kGroupBlocks * kSum;
        if (append) {  // the long lists of this wave: one atomic, then every list its own slot
            const uint32_t slot = wave_append(is_long && g == 0, long_count);
            if (is_long && g == 0) long_list[slot] = j;
        }
        if (!active || is_long) continue;
        if (count) {
            const uint32_t c = count_valid(ls, at, L, g, G);
            if (g == 0) count[j] = (int32_t)c;
        }
        reduce_list<G, false>(ls, fs, j, at, L, g);
    }
}

// long_list == NULL: every query of the call is a long list (a wide table).
template <int G>
__global__ __launch_bounds__(kBlock) void nreduce_wave_kernel(Lists ls, Fields fs, int32_t* __restrict__ count,
                                                              const uint32_t* __restrict__ long_list,
                                                              const uint32_t* __restrict__ long_count)
{
    const uint32_t n = long_list ? min(*long_count, ls.Q) : ls.Q;
    // wave-uniform; n < 2^31 and the stride is at most kWaveGrid * kWaves, so 32 bits hold i
    for (uint32_t i = blockIdx.x * kWaves + threadIdx.x / kWave; i < n; i += gridDim.x * kWaves) {
        uint32_t j = long_list ? long_list[i] : (uint32_t)i;
        j = (uint32_t)__builtin_amdgcn_readfirstlane((int)j);
        if (j >= ls.Q) continue;
        size_t at;
        uint32_t L;
        list_span(ls, j, at, L);  // wave-uniform, like j
        if (count) {
            const uint32_t c = count_valid(ls, at, L, lane_id(), kWave);
            if (lane_id() == 0) count[j] = (int32_t)c;
        }
        reduce_list<G, true>(ls, fs, j, at, L, 0);
    }
}

bool in_range(long long n) { return n >= 0 && n <= kReduceMax; }

size_t lists_scratch(long long Q) { return align_up((size_t)Q * sizeof(uint32_t)) + align_up(sizeof(uint32_t)); }

// The lanes of a group for fields of at most `width` floats.
int group_lanes(int width)
{
    if (width <= kNarrow) return 1;
    int G = 8;
    while (G < kWave && G < width) G *= 2;
    return G;
}

int group_grid(long long Q, int G)
{
    const long long lists = kBlock / G;
    return (int)std::min<long long>((Q + lists - 1) / lists, kGroupGridCap);
}

int wave_grid(long long lists) { return (int)std::max<long long>(1, std::min<long long>((lists + kWaves - 1) / kWaves, kWaveGrid)); }

template <int G>
void launch_set(const Lists& ls, const Fields& fs, int32_t* count, uint32_t* long_list, uint32_t* long_count, bool append,
                long long long_lists, hipStream_t s)
{
    const bool wide_table = ls.table && ls.k > kGroupBlocks * kSum;
    if (!wide_table)
        HIDEGS_LAUNCH("nreduce_group", nreduce_group_kernel<G>, dim3(group_grid(ls.Q, G)), dim3(kBlock), 0, s, ls, fs, count,
                      long_list, long_count, append ? 1 : 0);
    if (wide_table)
        HIDEGS_LAUNCH("nreduce_wave", nreduce_wave_kernel<G>, dim3(wave_grid(ls.Q)), dim3(kBlock), 0, s, ls, fs, count,
                      (const uint32_t*)nullptr, (const uint32_t*)nullptr);
    else if (long_lists > 0)
        HIDEGS_LAUNCH("nreduce_wave", nreduce_wave_kernel<G>, dim3(wave_grid(long_lists)), dim3(kBlock), 0, s, ls, fs, count,
                      (const uint32_t*)long_list, (const uint32_t*)long_count);
}

// The checks that the two forms share, in the order of the header; `who` names the entry point.  `run` is false
// where the call has nothing to do.
int check_common(const std::string& who, const hidegs_neighbor_field* fields, int nfields, long long P, long long Q,
                 const int32_t* count, bool& run)
{
    run = false;
    if (!in_range(P)) return fail(HIDEGS_E_ARG, who + ": P must be in [0, 2^31)");
    if (!in_range(Q)) return fail(HIDEGS_E_ARG, who + ": Q must be in [0, 2^31)");
    if (nfields < 0) return fail(HIDEGS_E_ARG, who + ": negative field count");
    if (Q == 0) return 0;
    if (nfields > 0 && !fields) return fail(HIDEGS_E_ARG, who + ": NULL field list");
    for (int i = 0; i < nfields; i++) {
        const std::string what = who + ": field " + std::to_string(i);
        if (fields[i].width < 1) return fail(HIDEGS_E_ARG, what + ": width must be >= 1");
        if (fields[i].op < HIDEGS_NEIGHBOR_SUM || fields[i].op > HIDEGS_NEIGHBOR_MAX)
            return fail(HIDEGS_E_ARG, what + ": op is not one of HIDEGS_NEIGHBOR_*");
        if (P > 0 && !fields[i].src) return fail(HIDEGS_E_ARG, what + ": NULL src");
        if (!fields[i].out) return fail(HIDEGS_E_ARG, what + ": NULL out");
    }
    run = nfields > 0 || count;
    return 0;
}

// One set of launches per kMaxFields fields, the narrow fields (one lane per list) apart from the wider ones.
// The first set writes count and, in the list form, appends the long lists that every set then reads.
int run_sets(const char* who, Lists ls, const hidegs_neighbor_field* fields, int nfields, int32_t* count, uint32_t* long_list,
             uint32_t* long_count, long long long_lists, hipStream_t s)
{
    bool first = true;
    for (int narrow = 1; narrow >= 0; narrow--) {
        Fields fs;
        fs.n = 0;
        int widest = 1;
        for (int i = 0; i <= nfields; i++) {
            if (i < nfields) {
                if ((fields[i].width <= kNarrow) != (narrow == 1)) continue;
                fs.f[fs.n++] = Field{fields[i].src, fields[i].out, (uint32_t)fields[i].width, fields[i].op};
                widest = std::max(widest, fields[i].width);
            }
            const bool last = i == nfields;
            // count alone where the call has no field
            if (fs.n == kMaxFields || (last && (fs.n > 0 || (first && narrow == 0 && count)))) {
                int32_t* c = first ? count : nullptr;
                const bool append = first && long_list;
                switch (group_lanes(widest)) {
                case 1: launch_set<1>(ls, fs, c, long_list, long_count, append, long_lists, s); break;
                case 8: launch_set<8>(ls, fs, c, long_list, long_count, append, long_lists, s); break;
                case 16: launch_set<16>(ls, fs, c, long_list, long_count, append, long_lists, s); break;
                case 32: launch_set<32>(ls, fs, c, long_list, long_count, append, long_lists, s); break;
                default: launch_set<64>(ls, fs, c, long_list, long_count, append, long_lists, s); break;
                }
                first = false;
                fs.n = 0;
                widest = 1;
            }
        }
    }
    return check_launch(who, s, 0);
}

}  // namespace
}  // namespace hidegs

extern "C" size_t hidegs_neighbor_reduce_scratch_bytes(long long Q, int max_width)
{
    (void)max_width;  // the long list alone: no partial leaves its wave
    return Q > 0 && hidegs::in_range(Q) ? hidegs::lists_scratch(Q) : 0;
}

extern "C" int hidegs_neighbor_reduce_table(void* scratch, size_t scratch_bytes, const hidegs_neighbor_field* fields, int nfields,
                                            long long P, const float* weights, const int32_t* table, const float* entry_weights,
                                            long long Q, int k, int32_t* count, void* stream)
{
    using namespace hidegs;
    (void)scratch, (void)scratch_bytes;  // the table form needs none
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_neighbor_reduce_table", s)) return rc;
    if (k < 1) return fail(HIDEGS_E_ARG, "neighbor_reduce_table: k must be >= 1");
    bool run;
    if (int rc = check_common("neighbor_reduce_table", fields, nfields, P, Q, count, run)) return rc;
    if (!run) return 0;
    if (!table) return fail(HIDEGS_E_ARG, "neighbor_reduce_table: NULL table");
    const Lists ls{table, nullptr, nullptr, weights, entry_weights, (uint32_t)k, 0u, (uint32_t)Q, (uint32_t)P};
    return run_sets("neighbor_reduce_table", ls, fields, nfields, count, nullptr, nullptr, 0, s);
}

extern "C" int hidegs_neighbor_reduce_lists(void* scratch, size_t scratch_bytes, const hidegs_neighbor_field* fields, int nfields,
                                            long long P, const float* weights, const int32_t* starts, const int32_t* rows,
                                            const float* entry_weights, long long capacity, long long Q, int32_t* count,
                                            void* stream)
{
    using namespace hidegs;
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_neighbor_reduce_lists", s)) return rc;
    if (!in_range(capacity)) return fail(HIDEGS_E_ARG, "neighbor_reduce_lists: capacity must be in [0, 2^31)");
    bool run;
    if (int rc = check_common("neighbor_reduce_lists", fields, nfields, P, Q, count, run)) return rc;
    if (!run) return 0;
    if (!starts) return fail(HIDEGS_E_ARG, "neighbor_reduce_lists: NULL starts");
    if (capacity > 0 && !rows) return fail(HIDEGS_E_ARG, "neighbor_reduce_lists: NULL rows");
    if (!scratch || scratch_bytes < lists_scratch(Q))
        return fail(HIDEGS_E_ARG, "neighbor_reduce_lists: scratch NULL or too small");
    Carver carve(scratch);
    uint32_t* long_list = carve.take<uint32_t>((size_t)Q);
    uint32_t* long_count = carve.take<uint32_t>(1);
    if (hipMemsetAsync(long_count, 0, sizeof(uint32_t), s) != hipSuccess)
        return fail(HIDEGS_E_HIP, "neighbor_reduce_lists: clearing the long-list counter failed");
    const Lists ls{nullptr, starts, rows, weights, entry_weights, 0u, (uint32_t)capacity, (uint32_t)Q, (uint32_t)P};
    const long long long_lists = std::min(Q, capacity / (long long)(kGroupBlocks * kSum));  // no more can be long
    return run_sets("neighbor_reduce_lists", ls, fields, nfields, count, long_list, long_count, long_lists, s);
}
