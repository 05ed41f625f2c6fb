// nearest.hip -- nearest-point index (include/hidegs_nearest.h): built once over a (P,3) cloud, then asked for
// the nearest point of arbitrary query positions.  Exact: the candidate minimising (bits(d), row index).
//
// Build (the structure distCUDA2 searches, knn.hip, kept in a caller-owned buffer: the constants, the distance,
// the lower bounds, the keys and the build kernels but the gather are morton_tree.h's, shared with that file):
//   1. bounding box over the finite rows (grid-stride partials + one finishing workgroup), no host read;
//   2. 48-bit Morton keys (16 bits per axis), kept below the largest, which the rows with a non-finite
//      coordinate take alone: they sort strictly last;
//   3. stable radix sort (sort_pairs_u64);
//   4. gather into float4 {x, y, z, bits(row)}; a non-candidate row is stored as three NaNs, so its distance
//      is a NaN, whose bits are above +inf's: it can never win and it widens no box;
//   5. leaf AABBs over kLeaf = 64 consecutive sorted points, super-box AABBs over kFan = 64 leaves, and each
//      leaf's first key.  The frame (box origin and scale) is kept in the index for the queries' keys.
//
// Query:
//   1. key the queries in the index's frame (clamped into the box) and sort (key, j): the 64 queries of a
//      wave are neighbours in space.  The order is for coherence only; results go to position j.
//   2. phase 1, one wave per 64 sorted queries: every lane's best is seeded from the leaf where the wave's
//      median key falls and its two Morton neighbours (candidates broadcast by v_readlane); super-boxes and
//      then leaves are tested against the wave's query AABB and the largest lane bound; the passing leaves
//      are listed in LDS and evaluated with each lane's own bound as the fine filter.
//   3. a wave whose list would grow past kBailout leaves, or whose first and last key lie more than kSpanBail
//      leaves apart to begin with, hands its queries to the hard list (one atomic counter); phase 2, a
//      second launch, searches each with one wave: lanes over candidates, a wave min.
//
// A lane's best is one u64, bits(d) << 32 | row, kept by an unsigned min: the contract's order itself.
// Exactness: every lower bound is the distance's own monotone expression applied to componentwise smaller
// gaps, and a box or point is skipped only when its bound is strictly above an upper bound of the best
// distance of every query it is skipped for -- an equal bound may hide an equal distance at a lower row.
// Seeds, ordering and the bail-out change the speed only.  All distances and bounds are non-negative
// floats (or +inf), so they are compared as unsigned integers.
//
// Two further queries on the same index are stages of this file, included below inside its namespace: the k
// nearest (nearest_k.h) and the count and the k nearest within a radius (nearest_within.h).  Neither adds to
// the build or to the scratch layout.  What the three share is written once, here: phase 1 is lane_walk, a
// template over what a lane keeps (its searcher: LaneBest here, LaneK and LaneWithin there), and every entry
// point begins with begin_query (argument checks, the empty cloud, the query keys and their sort).  Phase 2 of
// the two list queries is one walk of their own (nearest_k.h's hard_list_walk).
#include <float.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/hidegs_nearest.h"
#include "../../include/hidegs_nearest_k.h"
#include "../../include/hidegs_nearest_within.h"
#include "../../include/hidegs_nearest_lists.h"
#include "../../include/hidegs_components.h"
#include "common.h"
#include "morton_tree.h"
#include "union_find.h"

namespace hidegs {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;  // 4
constexpr int kListCap = 256;           // candidate leaves buffered per wave
constexpr int kBailout = 256;           // candidate leaves after which a wave hands its queries to phase 2
constexpr int kSpanBail = 16;           // leaves between a wave's first and last key above which it does so unseeded
constexpr int kHardGrid = 4096;         // workgroups of phase 2 at most
constexpr long long kNearestMax = 0x7fffffffLL;
constexpr uint32_t kInfBits = 0x7f800000u;
static_assert(kBailout <= kListCap, "the list holds every leaf of a wave that does not bail");

// A row with a non-finite coordinate is no candidate: out of every box, sorted strictly last (morton_tree.h).
struct NearestTree {
    static constexpr bool kNonFiniteLast = true;
};

struct Counters {
    uint32_t hard;  // queries sent to phase 2: the first word of the query scratch
};

inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

__device__ __forceinline__ uint64_t pack(float d, float row_bits)
{
    return ((uint64_t)__float_as_uint(d) << 32) | __float_as_uint(row_bits);
}

// Upper bound of a best's distance, as bits: +inf while nothing (or only an overflowed distance) was found.
__device__ __forceinline__ uint32_t bound_bits(uint64_t best) { return min((uint32_t)(best >> 32), kInfBits); }

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v)
{
    const uint32_t hi = (uint32_t)(v >> 32);
    const uint32_t mh = wave_min_u32(hi);
    const uint32_t ml = wave_min_u32(hi == mh ? (uint32_t)v : 0xffffffffu);
    return ((uint64_t)mh << 32) | ml;
}

// Bits of morton_tree.h's lower bounds: what the searches compare.
__device__ __forceinline__ uint32_t point_lb_bits(const Box& b, float4 q) { return __float_as_uint(box_point_lb(b, q)); }
__device__ __forceinline__ uint32_t box_lb_bits(const Box& b, float4 qlo, float4 qhi)
{
    return __float_as_uint(box_box_lb(b, qlo, qhi));
}

// Key of a query position: morton_tree.h's, kept below kLastKey like every candidate's.  The non-candidate rows
// alone have that key, so they sort strictly last, behind every candidate, and no query's key -- one beyond the
// box's far corner included -- falls into a leaf that holds only them (find_leaf then seeds from the last leaf
// with a candidate).
__device__ __forceinline__ uint64_t query_key(float x, float y, float z, const float* __restrict__ frame)
{
    return min(morton_key(x, y, z, frame), kLastKey - 1);
}

// ---- build: gather ------------------------------------------------------------------------------------
// Sorted point j = row order[j] as {x, y, z, bits(row)}; a non-candidate row is stored as three NaNs.  Wave w of
// block b holds leaf 4b + w and writes its box and first key.
__global__ __launch_bounds__(kBlock) void nearest_gather_kernel(const float* __restrict__ pts, const uint32_t* __restrict__ order,
                                                                const uint64_t* __restrict__ keys_sorted, long long P,
                                                                float4* __restrict__ sp, long long nleaves,
                                                                Box* __restrict__ leaves, uint64_t* __restrict__ leaf_keys)
{
    const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
    const float nan = __uint_as_float(0x7fc00000u);
    float4 p = make_float4(nan, nan, nan, 0.f);
    bool valid = false;
    if (j < P) {
        const uint32_t i = order[j];
        if (i < (uint32_t)P) {  // a permutation of [0, P) by construction
            const float x = pts[3ll * i], y = pts[3ll * i + 1], z = pts[3ll * i + 2];
            valid = finite3(x, y, z);
            if (valid) p = make_float4(x, y, z, 0.f);
            p.w = __uint_as_float(i);
        }
        sp[j] = p;
    }
    const long long L = j / kLeaf;  // wave-uniform
    if (L >= nleaves) return;       // whole wave
    const float lo[3] = {wave_min(valid ? p.x : FLT_MAX), wave_min(valid ? p.y : FLT_MAX), wave_min(valid ? p.z : FLT_MAX)};
    const float hi[3] = {wave_max(valid ? p.x : -FLT_MAX), wave_max(valid ? p.y : -FLT_MAX), wave_max(valid ? p.z : -FLT_MAX)};
    if (lane_id() == 0) {
        leaves[L] = Box{make_float4(lo[0], lo[1], lo[2], 0.f), make_float4(hi[0], hi[1], hi[2], 0.f)};
        leaf_keys[L] = keys_sorted[j];  // lane 0 of a leaf below nleaves: j < P
    }
}

// ---- query --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void nearest_query_keys_kernel(const float* __restrict__ queries, long long Q,
                                                                    const float* __restrict__ frame,
                                                                    uint64_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (j >= Q) return;
    keys[j] = query_key(queries[3 * j], queries[3 * j + 1], queries[3 * j + 2], frame);
    vals[j] = (uint32_t)j;
}

__global__ __launch_bounds__(kBlock) void nearest_none_kernel(long long Q, int32_t* __restrict__ idx_out,
                                                              float* __restrict__ dist2_out)
{
    const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (j >= Q) return;
    idx_out[j] = -1;
    dist2_out[j] = INFINITY;
}

struct IndexView {
    const float* frame;
    const float4* sp;
    const Box* leaves;
    const Box* supers;
    const uint64_t* leaf_keys;
    long long P, nleaves;
    int nsuper;
};

// The last leaf whose first key is <= key (leaf 0 if none), by a 64-ary search: wave-uniform arguments and
// result, every lane active.  The range at least halves per round.
__device__ __forceinline__ long long find_leaf(const uint64_t* __restrict__ leaf_keys, long long nleaves, uint64_t key,
                                               int lane)
{
    long long lo = 0, n = nleaves;
    while (n > 1) {
        const long long step = (n + kWave - 1) / kWave;
        const long long i = lo + lane * step;
        const bool le = i < lo + n && leaf_keys[i] <= key;
        const int cnt = __popcll(__ballot(le));  // the keys ascend: lanes 0 .. cnt - 1
        const long long nlo = lo + (long long)max(cnt - 1, 0) * step;
        n = min(step, lo + n - nlo);
        lo = nlo;
    }
    return lo;
}

// Appends the sorted position `s` of every lane with `flag` to the hard list (phase 2's input): one atomic per
// wave.  A query is appended once at most, so the list holds at most Q entries.
__device__ __forceinline__ void push_hard(bool flag, long long s, uint32_t* __restrict__ hard,
                                          Counters* __restrict__ counters)
{
    const uint32_t at = wave_append(flag, &counters->hard);
    if (flag) hard[at] = (uint32_t)s;
}

// The point held by lane c of `pt`, broadcast to every lane.
__device__ __forceinline__ float4 lane_point(float4 pt, int c)
{
    return make_float4(uniform_lane(pt.x, c), uniform_lane(pt.y, c), uniform_lane(pt.z, c), uniform_lane(pt.w, c));
}

__device__ __forceinline__ void store_result(uint64_t best, long long j, int32_t* __restrict__ idx_out,
                                             float* __restrict__ dist2_out)
{
    const uint32_t d = (uint32_t)(best >> 32);
    const bool none = d > kInfBits;  // nothing found, or only NaN distances (non-candidate rows)
    idx_out[j] = none ? -1 : (int32_t)(uint32_t)best;
    dist2_out[j] = none ? INFINITY : __uint_as_float(d);
}

// Phase 1 for every query of this file: one wave per 64 sorted queries, one lane per query.  What a lane keeps
// of the candidates it meets is its searcher, a struct in registers whose members are all inlined:
//   bool load(long long j)                    reads query j's own arguments; false: it can have no answer
//   void reset()                              nothing met yet
//   void eval(float4 q, float4 c)             meets candidate c {x, y, z, bits(row)}
//   uint32_t bound(bool active, bool& live)   bits of an upper bound of every distance that can still change
//                                             the lane's answer; live: one can (active, for all but the radius)
//   void store(long long j), store_none(long long j)
//   kUnrollSeed                               the form of the seed loop, measured per searcher
//   kCanFinish                                whether an active lane can stop being live
// The walk is the same for all: every branch around a ballot, a readlane, a readfirstlane or the wave barrier
// is wave-uniform, and no lane returns alone before the last of them.
template <class Searcher>
__device__ __forceinline__ void lane_walk(Searcher& sr, const IndexView& ix, const float* __restrict__ queries, long long Q,
                                          const uint64_t* __restrict__ qkeys, const uint32_t* __restrict__ qorder,
                                          uint32_t* __restrict__ hard, Counters* __restrict__ counters)
{
    __shared__ uint32_t s_list[kWaves][kListCap];
    const int wave = threadIdx.x / kWave;
    const int lane = lane_id();
    const long long base = ((long long)blockIdx.x * kWaves + wave) * kWave;
    if (base >= Q) return;  // whole wave; no workgroup barrier below

    const long long s = base + lane;
    long long j = 0;
    bool inq = s < Q;
    if (inq) {
        j = qorder[s];
        inq = j < Q;  // a permutation of [0, Q) by construction
    }
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    bool reach = false;
    if (inq) {
        q = make_float4(queries[3 * j], queries[3 * j + 1], queries[3 * j + 2], 0.f);
        reach = sr.load(j);
    }
    const bool active = inq && reach && finite3(q.x, q.y, q.z);
    if (inq && !active) sr.store_none(j);
    if (!__ballot(active)) return;

    const long long P = ix.P, nleaves = ix.nleaves;
    // A wave whose keys span many leaves (few queries against a large cloud) would seed, walk and then bail out:
    // its queries go to phase 2 at once, which seeds each from its own leaf.
    {
        const long long lf = find_leaf(ix.leaf_keys, nleaves, qkeys[base], lane);
        const long long ll = find_leaf(ix.leaf_keys, nleaves, qkeys[min(base + kWave - 1, Q - 1)], lane);
        if (ll - lf > kSpanBail) {
            push_hard(active, s, hard, counters);
            return;
        }
    }
    sr.reset();
    // seed: the leaf of the wave's median key and its two Morton neighbours, every point against every lane
    const long long Ls = find_leaf(ix.leaf_keys, nleaves, qkeys[min(base + kWave / 2, Q - 1)], lane);
    for (long long C = max(Ls - 1, 0ll); C <= min(Ls + 1, nleaves - 1); C++) {
        const float4 pt = ix.sp[min(C * kLeaf + lane, P - 1)];
        const int nc = (int)min((long long)kLeaf, P - C * kLeaf);  // wave-uniform
        if constexpr (Searcher::kUnrollSeed) {
#pragma unroll 16
            for (int c = 0; c < kLeaf; c++)
                if (c < nc) sr.eval(q, lane_point(pt, c));
        } else {
            for (int c = 0; c < nc; c++) sr.eval(q, lane_point(pt, c));
        }
    }

    // the wave's query AABB and the largest bound of its live lanes: the coarse filter
    const float4 qlo = make_float4(wave_min(active ? q.x : FLT_MAX), wave_min(active ? q.y : FLT_MAX),
                                   wave_min(active ? q.z : FLT_MAX), 0.f);
    const float4 qhi = make_float4(wave_max(active ? q.x : -FLT_MAX), wave_max(active ? q.y : -FLT_MAX),
                                   wave_max(active ? q.z : -FLT_MAX), 0.f);
    bool live;
    uint32_t ub = sr.bound(active, live);
    ub = wave_max_u32(live ? ub : 0u);

    uint32_t* list = s_list[wave];
    int nlist = 0;
    bool bail = false;
    // every lane finished by its seed: no walk (the ballot is left out where live is active, which some lane is)
    const int nsuper = !Searcher::kCanFinish || __ballot(live) ? ix.nsuper : 0;
    for (int s0 = 0; s0 < nsuper && !bail; s0 += kWave) {  // one super-box per lane
        const int sidx = s0 + lane;
        bool pass = false;
        if (sidx < nsuper) pass = box_lb_bits(ix.supers[sidx], qlo, qhi) <= ub;
        uint64_t smask = __ballot(pass);
        while (smask) {
            const int S = s0 + __builtin_ctzll(smask);
            smask &= smask - 1;
            const long long l = (long long)S * kFan + lane;
            bool lpass = false;
            if (l < nleaves && (l < Ls - 1 || l > Ls + 1))  // those three were the seed
                lpass = box_lb_bits(ix.leaves[l], qlo, qhi) <= ub;
            const uint64_t lm = __ballot(lpass);
            const int cnt = __popcll(lm);
            if (cnt == 0) continue;
            if (nlist + cnt > kBailout) {
                bail = true;
                break;
            }
            if (lpass) list[nlist + __popcll(lm & lanes_below(lane))] = (uint32_t)l;
            nlist += cnt;
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (bail) {
        // The wave's queries are spread too far for one coarse filter (queries far outside the cloud, on both
        // sides of a Morton jump, or with a large radius): phase 2 searches each again from nothing, with its
        // own seed and bound.
        push_hard(active, s, hard, counters);
        return;
    }

    for (int i = 0; i < nlist; i++) {
        const long long C = (long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)list[i]);
        const Box lb = ix.leaves[C];  // wave-uniform address
        // fine filter: some live lane's own bound reaches the leaf
        const uint32_t bound = sr.bound(active, live);
        if (!__ballot(live && point_lb_bits(lb, q) <= bound)) continue;
        const float4 pt = ix.sp[min(C * kLeaf + lane, P - 1)];
        const int nc = (int)min((long long)kLeaf, P - C * kLeaf);
        // a point is evaluated if it is a candidate within the largest live bound of the query AABB
        uint64_t pm = __ballot(lane < nc && pt.x == pt.x && point_lb_bits(Box{qlo, qhi}, pt) <= ub);
        while (pm) {
            const int c = __builtin_ctzll(pm);
            pm &= pm - 1;
            sr.eval(q, lane_point(pt, c));
        }
        const uint32_t after = sr.bound(active, live);
        ub = wave_max_u32(live ? after : 0u);
    }
    if (active) sr.store(j);
}

// The searcher of the nearest point: one u64 kept by an unsigned min.
struct LaneBest {
    static constexpr bool kUnrollSeed = true, kCanFinish = false;
    int32_t* idx_out;
    float* dist2_out;
    uint64_t best = ~0ull;

    __device__ __forceinline__ bool load(long long) { return true; }
    __device__ __forceinline__ void reset() { best = ~0ull; }
    __device__ __forceinline__ void eval(float4 q, float4 c) { best = min(best, pack(sqdist(q, c), c.w)); }
    __device__ __forceinline__ uint32_t bound(bool active, bool& live) const
    {
        live = active;
        return bound_bits(best);
    }
    __device__ __forceinline__ void store(long long j) const { store_result(best, j, idx_out, dist2_out); }
    __device__ __forceinline__ void store_none(long long j) const { store_result(~0ull, j, idx_out, dist2_out); }
};

__global__ __launch_bounds__(kBlock) void nearest_wave_kernel(IndexView ix, const float* __restrict__ queries, long long Q,
                                                              const uint64_t* __restrict__ qkeys, const uint32_t* __restrict__ qorder,
                                                              int32_t* __restrict__ idx_out, float* __restrict__ dist2_out,
                                                              uint32_t* __restrict__ hard, Counters* __restrict__ counters)
{
    LaneBest sr{idx_out, dist2_out};
    lane_walk(sr, ix, queries, Q, qkeys, qorder, hard, counters);
}

// ---- query: one wave per query of the hard list -------------------------------------------------------
// Phase 2 of the nearest point: lane c holds candidate c of a leaf and keeps a minimum of its own, reduced once
// per super-box (the list queries' insertion, nearest_k.h, is another search: DESIGN.md has the measurement).
__global__ __launch_bounds__(kBlock) void nearest_hard_kernel(IndexView ix, const float* __restrict__ queries, long long Q,
                                                              const uint64_t* __restrict__ qkeys, const uint32_t* __restrict__ qorder,
                                                              int32_t* __restrict__ idx_out, float* __restrict__ dist2_out,
                                                              const uint32_t* __restrict__ hard, const Counters* __restrict__ counters)
{
    const int lane = lane_id();
    const long long P = ix.P, nleaves = ix.nleaves;
    const uint32_t nhard = min(counters->hard, (uint32_t)Q);
    const uint32_t nw = gridDim.x * kWaves;
    for (uint32_t h = blockIdx.x * kWaves + threadIdx.x / kWave; h < nhard; h += nw) {
        const long long s = hard[h];
        if (s >= Q) continue;  // written by phase 1: below Q by construction
        const long long j = qorder[s];
        if (j >= Q) continue;
        const float4 q = make_float4(queries[3 * j], queries[3 * j + 1], queries[3 * j + 2], 0.f);
        const long long L = find_leaf(ix.leaf_keys, nleaves, qkeys[s], lane);
        uint64_t mine = ~0ull;
        for (long long C = max(L - 1, 0ll); C <= min(L + 1, nleaves - 1); C++) {
            const long long c = C * kLeaf + lane;
            if (c < P) {
                const float4 pt = ix.sp[c];
                mine = min(mine, pack(sqdist(q, pt), pt.w));
            }
        }
        uint64_t best = wave_min_u64(mine);
        for (int s0 = 0; s0 < ix.nsuper; s0 += kWave) {  // one super-box per lane
            const int sidx = s0 + lane;
            bool pass = false;
            if (sidx < ix.nsuper) pass = point_lb_bits(ix.supers[sidx], q) <= bound_bits(best);
            uint64_t smask = __ballot(pass);
            while (smask) {
                const int S = s0 + __builtin_ctzll(smask);
                smask &= smask - 1;
                const long long l = (long long)S * kFan + lane;
                bool lpass = false;
                if (l < nleaves && (l < L - 1 || l > L + 1)) lpass = point_lb_bits(ix.leaves[l], q) <= bound_bits(best);
                uint64_t lmask = __ballot(lpass);
                if (!lmask) continue;
                while (lmask) {
                    const long long c = ((long long)S * kFan + __builtin_ctzll(lmask)) * kLeaf + lane;
                    lmask &= lmask - 1;
                    if (c < P) {
                        const float4 pt = ix.sp[c];
                        mine = min(mine, pack(sqdist(q, pt), pt.w));
                    }
                }
                best = wave_min_u64(mine);
            }
        }
        if (lane == 0) store_result(best, j, idx_out, dist2_out);
    }
}

// ---- layouts ------------------------------------------------------------------------------------------
struct IndexLayout {
    float* frame;
    float4* sp;
    Box *leaves, *supers;
    uint64_t* leaf_keys;
    long long nleaves;
    int nsuper;
    size_t total;
};

IndexLayout index_layout(void* base, long long P)
{
    IndexLayout l;
    l.nleaves = ceil_div(P, kLeaf);
    l.nsuper = (int)ceil_div(l.nleaves, kFan);
    Carver c(base);
    l.frame = c.take<float>(8);
    l.sp = c.take<float4>(P);
    l.leaves = c.take<Box>(l.nleaves);
    l.supers = c.take<Box>(l.nsuper);
    l.leaf_keys = c.take<uint64_t>(l.nleaves);
    l.total = c.used;
    return l;
}

struct BuildLayout {
    SortLayout sort;  // both calls sort n (key, row) pairs
    float* partials;
    size_t total;
};

BuildLayout build_layout(void* base, long long P)
{
    BuildLayout l;
    Carver c(base);
    sort_layout(c, P, l.sort);
    l.partials = c.take<float>(kBoundBlocks * 6);
    l.total = c.used;
    return l;
}

struct QueryLayout {
    Counters* counters;  // first: the header documents the word
    SortLayout sort;
    uint32_t* hard;
    size_t total;
};

QueryLayout query_layout(void* base, long long Q)
{
    QueryLayout l;
    Carver c(base);
    l.counters = c.take<Counters>(1);
    sort_layout(c, Q, l.sort);
    l.hard = c.take<uint32_t>(Q);
    l.total = c.used;
    return l;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && pa < pb + nb && pb < pa + na;
}

bool in_range(long long n) { return n >= 0 && n <= kNearestMax; }

// A caller's buffer as the argument checks name it.  `required`: NULL is an error, reported as "NULL <name>"
// followed by this text.
struct Span {
    const void* p;
    size_t n;
    const char* name;
    const char* required = nullptr;
};

// A query whose arguments passed, keyed and sorted: what its kernels are launched with.
struct QueryCall {
    int rc = 0;  // of a call that is over: an error, or nothing left to do
    hipStream_t s;
    unsigned nb;  // workgroups of a thread per query; in a lane kernel, of a wave per 64 sorted queries
    IndexView ix;
    QueryLayout l;
};

// What every query of the index does before its own kernels, in the order the errors are documented in: the
// argument checks (`own_error`: the entry point's verdict on the arguments only it has, reported after k's), the
// answer of an empty cloud (launched by `none`), the query keys and their sort.  False: the call is over with
// c.rc.  No host synchronisation and no allocation: it runs under graph capture.
template <class None>
bool begin_query(QueryCall& c, const char* name, void* stream, const void* index, size_t index_bytes, long long P,
                 void* scratch, size_t scratch_bytes, const float* queries, long long Q, int k, int kmin, int kmax,
                 const char* own_error, std::initializer_list<Span> more_inputs, std::initializer_list<Span> outputs, None none)
{
    const std::string who = std::string(name) + ": ";
    const auto over = [&](int rc) {
        c.rc = rc;
        return false;
    };
    c.s = as_stream(stream);
    if (int rc = take_async_error(("hidegs_" + std::string(name)).c_str(), c.s)) return over(rc);
    if (k < kmin || k > kmax)
        return over(fail(HIDEGS_E_ARG, who + "k must be in [" + std::to_string(kmin) + ", " + std::to_string(kmax) + "]"));
    if (own_error) return over(fail(HIDEGS_E_ARG, who + own_error));
    if (!in_range(P)) return over(fail(HIDEGS_E_ARG, who + "P must be in [0, 2^31)"));
    if (!in_range(Q)) return over(fail(HIDEGS_E_ARG, who + "Q must be in [0, 2^31)"));
    if (Q == 0) return over(0);
    const std::initializer_list<Span> first = {{queries, (size_t)Q * 12, "queries", ""}};
    for (const auto& list : {first, more_inputs, outputs})
        for (const Span& b : list)
            if (b.required && !b.p) return over(fail(HIDEGS_E_ARG, who + "NULL " + b.name + b.required));
    if (P > 0) {
        if (!index || !aligned16(index) || index_bytes < index_layout(nullptr, P).total)
            return over(fail(HIDEGS_E_ARG, who + "index buffer NULL, not 16-byte aligned or too small for P"));
        if (!scratch || !aligned16(scratch) || scratch_bytes < query_layout(nullptr, Q).total)
            return over(fail(HIDEGS_E_ARG, who + "scratch buffer NULL, not 16-byte aligned or too small"));
    } else {
        index = nullptr, index_bytes = 0, scratch = nullptr, scratch_bytes = 0;  // not used
    }
    const std::initializer_list<Span> own = {{index, index_bytes, "the index"}, {scratch, scratch_bytes, "scratch"}};
    for (const auto& inputs : {first, more_inputs, own})
        for (const Span& in : inputs)
            for (const Span& out : outputs)
                if (overlap(out.p, out.n, in.p, in.n)) return over(fail(HIDEGS_E_ARG, who + out.name + " overlaps " + in.name));
    for (const Span* a = outputs.begin(); a != outputs.end(); a++)
        for (const Span* b = a + 1; b != outputs.end(); b++)
            if (overlap(a->p, a->n, b->p, b->n)) return over(fail(HIDEGS_E_ARG, who + b->name + " overlaps " + a->name));
    c.nb = (unsigned)ceil_div(Q, kBlock);
    if (P == 0) {
        none(c);
        return over(check_launch(name, c.s, 0));
    }
    const IndexLayout il = index_layout(const_cast<void*>(index), P);
    c.ix = IndexView{il.frame, il.sp, il.leaves, il.supers, il.leaf_keys, P, il.nleaves, il.nsuper};
    c.l = query_layout(scratch, Q);
    if (hipMemsetAsync(c.l.counters, 0, sizeof(Counters), c.s) != hipSuccess)
        return over(fail(HIDEGS_E_HIP, who + "clearing the counter failed"));
    HIDEGS_LAUNCH("nearest_query_keys", nearest_query_keys_kernel, dim3(c.nb), dim3(kBlock), 0, c.s, queries, Q, c.ix.frame,
                  c.l.sort.keys, c.l.sort.vals);
    if (int rc = sort_pairs_u64(c.l.sort.sort_tmp, c.l.sort.sort_bytes, c.l.sort.keys, c.l.sort.keys_sorted, c.l.sort.vals,
                                c.l.sort.vals_sorted, Q, 0, 3 * kMortonBits, c.s))
        return over(rc);
    return true;
}

// The grid of a wave-per-query launch: a wave per query up to kHardGrid workgroups, whose waves stride on.
dim3 hard_grid(long long Q) { return dim3(std::min<unsigned>(kHardGrid, (unsigned)ceil_div(Q, kWaves))); }

#include "nearest_k.h"
#include "nearest_within.h"
#include "nearest_lists.h"
#include "nearest_components.h"

}  // namespace
}  // namespace hidegs

extern "C" size_t hidegs_nearest_index_bytes(long long P)
{
    return P > 0 && hidegs::in_range(P) ? hidegs::index_layout(nullptr, P).total : 0;
}

extern "C" size_t hidegs_nearest_build_scratch_bytes(long long P)
{
    return P > 0 && hidegs::in_range(P) ? hidegs::build_layout(nullptr, P).total : 0;
}

extern "C" size_t hidegs_nearest_query_scratch_bytes(long long P, long long Q)
{
    return Q > 0 && hidegs::in_range(Q) && hidegs::in_range(P) ? hidegs::query_layout(nullptr, Q).total : 0;
}

extern "C" int hidegs_nearest_build(void* index, size_t index_bytes, void* scratch, size_t scratch_bytes,
                                    const float* points, long long P, void* stream)
{
    using namespace hidegs;
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_nearest_build", s)) return rc;
    if (!in_range(P)) return fail(HIDEGS_E_ARG, "nearest_build: P must be in [0, 2^31)");
    if (P == 0) return 0;
    if (!points) return fail(HIDEGS_E_ARG, "nearest_build: NULL points");
    if (!index || !aligned16(index) || index_bytes < index_layout(nullptr, P).total)
        return fail(HIDEGS_E_ARG, "nearest_build: index buffer NULL, not 16-byte aligned or too small");
    if (!scratch || !aligned16(scratch) || scratch_bytes < build_layout(nullptr, P).total)
        return fail(HIDEGS_E_ARG, "nearest_build: scratch buffer NULL, not 16-byte aligned or too small");
    if (overlap(index, index_bytes, points, (size_t)P * 12) || overlap(index, index_bytes, scratch, scratch_bytes))
        return fail(HIDEGS_E_ARG, "nearest_build: index overlaps points or scratch");
    const IndexLayout ix = index_layout(index, P);
    const BuildLayout b = build_layout(scratch, P);
    const int nb = (int)ceil_div(P, kBlock);
    const int nbound = std::min(kBoundBlocks, nb);
    HIDEGS_LAUNCH("nearest_bounds", tree_bounds_kernel<NearestTree>, dim3(nbound), dim3(kTreeBlock), 0, s, points, P, b.partials);
    HIDEGS_LAUNCH("nearest_frame", tree_frame_kernel<NearestTree>, dim3(1), dim3(kTreeBlock), 0, s, b.partials, nbound, ix.frame);
    HIDEGS_LAUNCH("nearest_point_keys", tree_point_keys_kernel<NearestTree>, dim3(nb), dim3(kTreeBlock), 0, s, points, P, ix.frame,
                  b.sort.keys, b.sort.vals);
    if (int rc = sort_pairs_u64(b.sort.sort_tmp, b.sort.sort_bytes, b.sort.keys, b.sort.keys_sorted, b.sort.vals,
                                b.sort.vals_sorted, P, 0, 3 * kMortonBits, s))
        return rc;
    HIDEGS_LAUNCH("nearest_gather", nearest_gather_kernel, dim3(nb), dim3(kBlock), 0, s, points, b.sort.vals_sorted,
                  b.sort.keys_sorted, P, ix.sp, ix.nleaves, ix.leaves, ix.leaf_keys);
    HIDEGS_LAUNCH("nearest_super", tree_super_kernel<NearestTree>, dim3((unsigned)ceil_div(ix.nsuper, kTreeWaves)), dim3(kTreeBlock), 0, s,
                  ix.leaves, ix.nleaves, ix.nsuper, ix.supers);
    return check_launch("nearest_build", s, 0);
}

extern "C" int hidegs_nearest_query(const void* index, size_t index_bytes, long long P, void* scratch,
                                    size_t scratch_bytes, const float* queries, long long Q, int32_t* idx_out,
                                    float* dist2_out, void* stream)
{
    using namespace hidegs;
    const size_t out_bytes = (size_t)Q * 4;
    QueryCall c;
    if (!begin_query(c, "nearest_query", stream, index, index_bytes, P, scratch, scratch_bytes, queries, Q, 1, 1, 1, nullptr, {},
                     {{idx_out, out_bytes, "idx_out", ""}, {dist2_out, out_bytes, "dist2_out", ""}}, [&](const QueryCall& c) {
                         HIDEGS_LAUNCH("nearest_none", nearest_none_kernel, dim3(c.nb), dim3(kBlock), 0, c.s, Q, idx_out, dist2_out);
                     }))
        return c.rc;
    HIDEGS_LAUNCH("nearest_wave", nearest_wave_kernel, dim3(c.nb), dim3(kBlock), 0, c.s, c.ix, queries, Q, c.l.sort.keys_sorted,
                  c.l.sort.vals_sorted, idx_out, dist2_out, c.l.hard, c.l.counters);
    HIDEGS_LAUNCH("nearest_hard", nearest_hard_kernel, hard_grid(Q), dim3(kBlock), 0, c.s, c.ix, queries, Q, c.l.sort.keys_sorted,
                  c.l.sort.vals_sorted, idx_out, dist2_out, c.l.hard, c.l.counters);
    return check_launch("nearest_query", c.s, 0);
}

extern "C" size_t hidegs_nearest_query_k_scratch_bytes(long long P, long long Q, int k)
{
    return hidegs::query_k_scratch_bytes(P, Q, k);
}

extern "C" int hidegs_nearest_query_k(const void* index, size_t index_bytes, long long P, void* scratch, size_t scratch_bytes,
                                      const float* queries, long long Q, int k, const int32_t* exclude, int32_t* idx_out,
                                      float* dist2_out, void* stream)
{
    return hidegs::query_k(index, index_bytes, P, scratch, scratch_bytes, queries, Q, k, exclude, idx_out, dist2_out, stream);
}

extern "C" size_t hidegs_nearest_query_within_scratch_bytes(long long P, long long Q, int k)
{
    return hidegs::query_within_scratch_bytes(P, Q, k);
}

extern "C" int hidegs_nearest_query_within(const void* index, size_t index_bytes, long long P, void* scratch,
                                           size_t scratch_bytes, const float* queries, long long Q, const float* r2, int k,
                                           int max_count, const int32_t* exclude, int32_t* count_out, int32_t* idx_out,
                                           float* dist2_out, void* stream)
{
    return hidegs::query_within(index, index_bytes, P, scratch, scratch_bytes, queries, Q, r2, k, max_count, exclude, count_out,
                                idx_out, dist2_out, stream);
}

extern "C" int hidegs_nearest_index_order(const void* index, size_t index_bytes, long long P, int32_t* order_out, void* stream)
{
    return hidegs::index_order(index, index_bytes, P, order_out, stream);
}

extern "C" size_t hidegs_nearest_list_offsets_scratch_bytes(long long P, long long Q)
{
    return hidegs::list_offsets_scratch_bytes(P, Q);
}

extern "C" int hidegs_nearest_list_offsets(const void* index, size_t index_bytes, long long P, void* scratch,
                                           size_t scratch_bytes, const float* queries, long long Q, const float* r2,
                                           const int32_t* exclude, int32_t* starts_out, uint32_t* info_out, void* stream)
{
    return hidegs::list_offsets(index, index_bytes, P, scratch, scratch_bytes, queries, Q, r2, exclude, starts_out, info_out,
                                stream);
}

extern "C" size_t hidegs_nearest_list_fill_scratch_bytes(long long P, long long Q)
{
    return hidegs::list_fill_scratch_bytes(P, Q);
}

extern "C" int hidegs_nearest_list_fill(const void* index, size_t index_bytes, long long P, void* scratch, size_t scratch_bytes,
                                        const float* queries, long long Q, const float* r2, const int32_t* exclude,
                                        const int32_t* starts, long long capacity, int32_t* rows_out, float* dist2_out,
                                        void* stream)
{
    return hidegs::list_fill(index, index_bytes, P, scratch, scratch_bytes, queries, Q, r2, exclude, starts, capacity, rows_out,
                             dist2_out, stream);
}

extern "C" size_t hidegs_nearest_components_within_scratch_bytes(long long) { return 0; }

extern "C" int hidegs_nearest_components_within(const void* index, size_t index_bytes, long long P, void* scratch,
                                                size_t scratch_bytes, const float* r2, int r2_is_per_row, int32_t* parent,
                                                void* stream)
{
    return hidegs::components_within(index, index_bytes, P, scratch, scratch_bytes, r2, r2_is_per_row, parent, stream);
}
