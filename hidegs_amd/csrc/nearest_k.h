// nearest_k.h -- the k-nearest query of the nearest-point index (include/hidegs_nearest_k.h): a stage of
// nearest.hip, included inside its namespace.  The index, the query keys, the Morton sort of the queries, the
// lower bounds, the hard list and the lane walk are nearest.hip's; what is new is that every searcher keeps its
// k best instead of its best, and that every filter takes its bound from the k-th best.
//
// A candidate is one u64, bits(d) << 32 | row: the contract's order is the unsigned order of these values, and
// a slot that holds nothing is ~0.  The excluded row is given ~0 where its value is formed, so it can enter no
// list.  A non-candidate row has a NaN distance, above +inf: it may sit in a list that has room, behind every
// candidate, and is stored as -1 / +inf like an empty slot.
//
// Exactness, as for k = 1: a box or a point is skipped only when its lower bound is strictly above an upper
// bound of the k-th best distance of every query it is skipped for.  While a query holds fewer than k that
// bound is +inf.  Each point is evaluated at most once per query (the seed leaves are left out of the walk and
// a leaf is listed once), so a list never holds a row twice.
//
//   LaneK<K>, the searcher of nearest_k_wave_kernel<K> (nearest.hip's lane_walk): the lane's K best are a
//     sorted array in registers (static indices only).  A call with k <= K keeps K - k slots at 0 below the
//     list: nothing is below 0, so they stay, the list's last entry is the k-th best whatever k is, and the
//     k results are the last k slots.
//   nearest_route_kernel<Searcher>: for k above kLaneKMax, sends every query that can have an answer to the
//     hard list.
//   hard_list_walk<RADIUS, LIST>: one wave per query of the hard list; lane i holds the i-th best.  With
//     RADIUS it is the fixed-radius query's as well (nearest_within.h), which counts and keeps what is in range.

constexpr int kLaneKMax = 16;  // the largest K of a lane's list: instantiated for 4, 8 and 16
constexpr int kNearestKMax = 64;
static_assert(kNearestKMax <= kWave, "the hard path holds one of the k best per lane");

__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int src)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// Lane i receives lane i - 1's value (DPP wave_shr:1); lane 0 keeps its own.  Every lane must be active.
__device__ __forceinline__ uint64_t wave_shr1_u64(uint64_t v)
{
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    const uint32_t slo = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);
    const uint32_t shi = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
    return ((uint64_t)shi << 32) | slo;
}

// The value of point c for a query that excludes row `excl` (0xffffffff and every value >= P exclude nothing).
__device__ __forceinline__ uint64_t pack_unless(float4 q, float4 c, uint32_t excl)
{
    return __float_as_uint(c.w) == excl ? ~0ull : pack(sqdist(q, c), c.w);
}

__device__ __forceinline__ uint32_t excluded_row(const int32_t* __restrict__ exclude, long long j)
{
    return exclude ? (uint32_t)exclude[j] : 0xffffffffu;
}

// The radius rule (nearest_within.h): rb, the bits of a squared radius, and whether anything can be in range
// of it at all.  For r2 >= 0 clearing the sign bit is r2 + 0.0f: -0 is 0.
__device__ __forceinline__ bool radius_bits(float r2, uint32_t& rb)
{
    rb = __float_as_uint(r2) & 0x7fffffffu;
    return r2 >= 0.f;  // false for a NaN
}

__device__ __forceinline__ bool in_reach(uint64_t v, uint32_t rb) { return (uint32_t)(v >> 32) <= rb; }

// list is ascending and v < list[K - 1]: v takes its place, the last entry leaves.
template <int K>
__device__ __forceinline__ void insert_k(uint64_t (&list)[K], uint64_t v)
{
#pragma unroll
    for (int i = K - 1; i >= 1; i--) list[i] = v < list[i - 1] ? list[i - 1] : min(v, list[i]);
    list[0] = min(v, list[0]);
}

// The searcher of the k nearest (k <= K, wave-uniform).
template <int K>
struct LaneK {
    static constexpr bool kUnrollSeed = false, kCanFinish = false;
    int k;
    const int32_t* exclude;
    int32_t* idx_out;
    float* dist2_out;
    uint32_t excl = 0xffffffffu;
    uint64_t list[K];  // ascending; list[K - 1] is the k-th best

    __device__ __forceinline__ bool load(long long j)
    {
        excl = excluded_row(exclude, j);
        return true;
    }
    __device__ __forceinline__ void reset()
    {
#pragma unroll
        for (int i = 0; i < K; i++) list[i] = i < K - k ? 0ull : ~0ull;
    }
    __device__ __forceinline__ void eval(float4 q, float4 c)
    {
        const uint64_t v = pack_unless(q, c, excl);
        if (v < list[K - 1]) insert_k(list, v);
    }
    __device__ __forceinline__ uint32_t bound(bool active, bool& live) const
    {
        live = active;
        return bound_bits(list[K - 1]);
    }
    __device__ __forceinline__ void store(long long j) const
    {
#pragma unroll
        for (int i = 0; i < K; i++)
            if (i >= K - k) store_result(list[i], j * k + (i - (K - k)), idx_out, dist2_out);
    }
    __device__ __forceinline__ void store_none(long long j) const
    {
        for (int i = 0; i < k; i++) store_result(~0ull, j * k + i, idx_out, dist2_out);
    }
};

template <int K>
__global__ __launch_bounds__(kBlock) void nearest_k_wave_kernel(IndexView ix, const float* __restrict__ queries, long long Q,
                                                                const uint64_t* __restrict__ qkeys,
                                                                const uint32_t* __restrict__ qorder, int k,
                                                                const int32_t* __restrict__ exclude, int32_t* __restrict__ idx_out,
                                                                float* __restrict__ dist2_out, uint32_t* __restrict__ hard,
                                                                Counters* __restrict__ counters)
{
    LaneK<K> sr{k, exclude, idx_out, dist2_out};
    lane_walk(sr, ix, queries, Q, qkeys, qorder, hard, counters);
}

// k above kLaneKMax, a thread per query: one that can have no answer (it is not finite, or its searcher says so)
// is answered here, every other one goes to the hard list.
template <class Searcher>
__global__ __launch_bounds__(kBlock) void nearest_route_kernel(const float* __restrict__ queries, long long Q,
                                                               const uint32_t* __restrict__ qorder, Searcher sr,
                                                               uint32_t* __restrict__ hard, Counters* __restrict__ counters)
{
    const long long s = (long long)blockIdx.x * kBlock + threadIdx.x;
    long long j = 0;
    bool inq = s < Q;
    if (inq) {
        j = qorder[s];
        inq = j < Q;
    }
    bool active = false;
    if (inq) {
        active = sr.load(j) && finite3(queries[3 * j], queries[3 * j + 1], queries[3 * j + 2]);
        if (!active) sr.store_none(j);
    }
    push_hard(active, s, hard, counters);
}

// One wave per hard query, for both list queries.  Lane i holds the i-th best (~0: none yet); kth is lane
// k - 1's value, read again after every insertion; bnd is the bound of every filter, formed again after every
// leaf.  With RADIUS only what is in range is kept, count (wave-uniform) is how many were, and bnd follows
// nearest_within.h's rule; without, bnd is the k-th best's bits.  LIST is k > 0: without it there is no list, kth
// is 0 (nothing is below it) and a saturated query leaves every loop.
template <bool RADIUS, bool LIST>
__device__ __forceinline__ void hard_list_walk(const IndexView& ix, const float* __restrict__ queries, long long Q,
                                               const uint64_t* __restrict__ qkeys, const uint32_t* __restrict__ qorder,
                                               const float* __restrict__ r2, int k, uint32_t max_count,
                                               const int32_t* __restrict__ exclude, int32_t* __restrict__ count_out,
                                               int32_t* __restrict__ idx_out, float* __restrict__ dist2_out,
                                               const uint32_t* __restrict__ hard, const Counters* __restrict__ counters)
{
    static_assert(RADIUS || LIST, "without a radius there is a list");
    const int lane = lane_id();
    const long long P = ix.P, nleaves = ix.nleaves;
    const uint32_t nhard = min(counters->hard, (uint32_t)Q);
    const uint32_t nw = gridDim.x * kWaves;
    for (uint32_t h = blockIdx.x * kWaves + threadIdx.x / kWave; h < nhard; h += nw) {
        const long long s = hard[h];
        if (s >= Q) continue;  // written by the launch before: below Q by construction
        const long long j = qorder[s];
        if (j >= Q) continue;
        const float4 q = make_float4(queries[3 * j], queries[3 * j + 1], queries[3 * j + 2], 0.f);
        const uint32_t excl = excluded_row(exclude, j);
        uint32_t rb = kInfBits;
        if constexpr (RADIUS)
            if (!radius_bits(r2[j], rb)) continue;  // never listed: answered by the launch before
        const long long L = find_leaf(ix.leaf_keys, nleaves, qkeys[s], lane);
        uint64_t top = ~0ull, kth = LIST ? ~0ull : 0ull;
        uint32_t count = 0;
        uint32_t bnd = rb;
        const auto open = [&] { return LIST || count < max_count; };  // wave-uniform

        // The 64 points of leaf C, one per lane: those to keep (with RADIUS, those in range, which are counted)
        // that are below the k-th best are inserted one by one, lowest lane first.  A value's rank is the number
        // of entries below it; the entries from there on move up a lane.
        auto batch = [&](long long C) {
            const long long c = C * kLeaf + lane;
            uint64_t v = ~0ull;
            if (c < P) v = pack_unless(q, ix.sp[c], excl);
            bool keep = true;
            if constexpr (RADIUS) {
                keep = in_reach(v, rb);
                count += (uint32_t)__popcll(__ballot(keep));
            }
            uint64_t m = LIST ? __ballot(keep && v < kth) : 0ull;
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                const uint64_t cv = readlane_u64(v, b);
                if (!(cv < kth)) continue;  // wave-uniform: the bound has come down since the ballot
                const int rank = __popcll(__ballot(top < cv));  // the entries ascend: lanes 0 .. rank - 1; rank < k
                const uint64_t up = wave_shr1_u64(top);
                top = lane > rank ? up : (lane == rank ? cv : top);
                kth = readlane_u64(top, k - 1);
            }
            bnd = RADIUS && count < max_count ? rb : bound_bits(kth);
        };

        for (long long C = max(L - 1, 0ll); C <= min(L + 1, nleaves - 1); C++) batch(C);
        for (int s0 = 0; s0 < ix.nsuper && open(); s0 += kWave) {  // one super-box per lane
            const int sidx = s0 + lane;
            bool pass = false;
            if (sidx < ix.nsuper) pass = point_lb_bits(ix.supers[sidx], q) <= bnd;
            uint64_t smask = __ballot(pass);
            while (smask && open()) {
                const int S = s0 + __builtin_ctzll(smask);
                smask &= smask - 1;
                const long long l = (long long)S * kFan + lane;
                uint32_t llb = 0xffffffffu;  // above every bound: no leaf, or one of the seed
                if (l < nleaves && (l < L - 1 || l > L + 1)) llb = point_lb_bits(ix.leaves[l], q);
                uint64_t lmask = __ballot(llb <= bnd);
                while (lmask && open()) {
                    const int b = __builtin_ctzll(lmask);
                    lmask &= lmask - 1;
                    if ((uint32_t)__builtin_amdgcn_readlane((int)llb, b) > bnd) continue;  // it has come down since
                    batch((long long)S * kFan + b);
                }
            }
        }
        if constexpr (RADIUS)
            if (lane == 0) count_out[j] = (int32_t)min(count, max_count);
        if (LIST && lane < k) store_result(top, j * k + lane, idx_out, dist2_out);
    }
}

__global__ __launch_bounds__(kBlock) void nearest_k_hard_kernel(IndexView ix, const float* __restrict__ queries, long long Q,
                                                                const uint64_t* __restrict__ qkeys,
                                                                const uint32_t* __restrict__ qorder, int k,
                                                                const int32_t* __restrict__ exclude, int32_t* __restrict__ idx_out,
                                                                float* __restrict__ dist2_out, const uint32_t* __restrict__ hard,
                                                                const Counters* __restrict__ counters)
{
    hard_list_walk<false, true>(ix, queries, Q, qkeys, qorder, nullptr, k, 0u, exclude, nullptr, idx_out, dist2_out, hard, counters);
}

// The query scratch is nearest_query's: the counter word, the (key, row) sort, the hard list.
size_t query_k_scratch_bytes(long long P, long long Q, int k)
{
    return Q > 0 && in_range(Q) && in_range(P) && k >= 1 && k <= kNearestKMax ? query_layout(nullptr, Q).total : 0;
}

template <int K>
void launch_k_wave(const QueryCall& c, const float* queries, long long Q, int k, const int32_t* exclude, int32_t* idx_out,
                   float* dist2_out)
{
    HIDEGS_LAUNCH("nearest_k_wave", nearest_k_wave_kernel<K>, dim3(c.nb), dim3(kBlock), 0, c.s, c.ix, queries, Q,
                  c.l.sort.keys_sorted, c.l.sort.vals_sorted, k, exclude, idx_out, dist2_out, c.l.hard, c.l.counters);
}

int query_k(const void* index, size_t index_bytes, long long P, void* scratch, size_t scratch_bytes, const float* queries,
            long long Q, int k, const int32_t* exclude, int32_t* idx_out, float* dist2_out, void* stream)
{
    const size_t out_bytes = (size_t)Q * (size_t)k * 4;
    QueryCall c;
    if (!begin_query(c, "nearest_query_k", stream, index, index_bytes, P, scratch, scratch_bytes, queries, Q, k, 1, kNearestKMax,
                     nullptr, {{exclude, (size_t)Q * 4, "exclude"}},
                     {{idx_out, out_bytes, "idx_out", ""}, {dist2_out, out_bytes, "dist2_out", ""}}, [&](const QueryCall& c) {
                         const long long n = Q * k;
                         HIDEGS_LAUNCH("nearest_none", nearest_none_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0,
                                       c.s, n, idx_out, dist2_out);
                     }))
        return c.rc;
    if (k <= 4)
        launch_k_wave<4>(c, queries, Q, k, exclude, idx_out, dist2_out);
    else if (k <= 8)
        launch_k_wave<8>(c, queries, Q, k, exclude, idx_out, dist2_out);
    else if (k <= kLaneKMax)
        launch_k_wave<kLaneKMax>(c, queries, Q, k, exclude, idx_out, dist2_out);
    else
        HIDEGS_LAUNCH("nearest_k_route", nearest_route_kernel<LaneK<1>>, dim3(c.nb), dim3(kBlock), 0, c.s, queries, Q,
                      c.l.sort.vals_sorted, LaneK<1>{k, exclude, idx_out, dist2_out}, c.l.hard, c.l.counters);
    HIDEGS_LAUNCH("nearest_k_hard", nearest_k_hard_kernel, hard_grid(Q), dim3(kBlock), 0, c.s, c.ix, queries, Q,
                  c.l.sort.keys_sorted, c.l.sort.vals_sorted, k, exclude, idx_out, dist2_out, c.l.hard, c.l.counters);
    return check_launch("nearest_query_k", c.s, 0);
}
