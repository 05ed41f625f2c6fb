// nearest_within.h -- the fixed-radius query of the nearest-point index (include/hidegs_nearest_within.h): a
// stage of nearest.hip, included inside its namespace after nearest_k.h.  The index, the query keys, the Morton
// sort of the queries, the lower bounds, the hard list and the lane walk are nearest.hip's, the u64 candidates,
// the route kernel and the wave-per-query walk nearest_k.h's; what is new is that every searcher counts the
// candidates within its query's radius, keeps the k best of those only, and takes the bound of every filter from
// one rule.
//
// In range: bits(d) <= rb, the bits of the query's squared radius (the excluded row's ~0 and a non-candidate's
// NaN are above every rb).  A query whose radius is negative or a NaN is answered where a non-finite query is.
//
// One bound per query: while its count is below max_count the bound is rb -- every candidate in range is still
// to be counted.  Once the count has reached max_count the count is settled, and the bound is the k-th best's
// bits: the list is full by then (max_count >= k) of values in range, so that bound is at most rb.  With k = 0
// the query is finished at that point.  A value is counted iff it is in range, and inserted iff it is in range
// and below the k-th best.
//
// Exactness: below saturation every box whose lower bound is <= rb is searched (an equal bound is searched, not
// skipped), and each point is evaluated at most once per query (the seed leaves are left out of the walk and a
// leaf is listed once): the count is exact.  After saturation the count is max_count by definition and
// nearest_k.h's k-th-best argument covers the list.  Seeds, order and bail-outs change the speed only.
//
//   LaneWithin<K>, K = 0, 4, 8, 16, the searcher of nearest_within_wave_kernel<K> (nearest.hip's lane_walk):
//     LaneK's list with a count per lane.  K = 0 keeps no list.  A large radius makes most waves bail: they hand
//     their queries to the hard list, as intended.
//   nearest_within_wave_own_kernel<16>: K = 16 runs lane_walk's text written out, for its registers (see there).
//   nearest_within_hard_kernel<LIST>: nearest_k.h's hard_list_walk with the radius.

// The searcher of the count within a radius and of the k nearest of those (k <= K, wave-uniform).
template <int K>
struct LaneWithin {
    static constexpr bool kUnrollSeed = false, kCanFinish = true;
    LaneK<(K ? K : 1)> in;  // the k best in range; at K = 0 only its arguments
    const float* r2;
    uint32_t max_count;
    int32_t* count_out;
    uint32_t rb = 0, count = 0;

    __device__ __forceinline__ bool load(long long j)
    {
        in.load(j);
        return radius_bits(r2[j], rb);
    }
    __device__ __forceinline__ void reset()
    {
        count = 0;
        if constexpr (K > 0) in.reset();
    }
    __device__ __forceinline__ void eval(float4 q, float4 c)
    {
        uint64_t v = pack_unless(q, c, in.excl);
        const bool reach = in_reach(v, rb);
        count += reach;  // at most once per point: below 2^31
        if constexpr (K > 0) {
            v = reach ? v : ~0ull;  // out of range: below no entry
            if (v < in.list[K - 1]) insert_k(in.list, v);
        }
    }
    // The lane's bound by the rule above; it is live until nothing more can change its answer.
    __device__ __forceinline__ uint32_t bound(bool active, bool& live) const
    {
        const bool open = count < max_count;
        live = active && (K > 0 || open);
        if (open) return rb;
        if constexpr (K > 0) return bound_bits(in.list[K - 1]);
        return 0u;
    }
    __device__ __forceinline__ void store(long long j) const
    {
        count_out[j] = (int32_t)min(count, max_count);
        if constexpr (K > 0) in.store(j);
    }
    __device__ __forceinline__ void store_none(long long j) const
    {
        count_out[j] = 0;
        in.store_none(j);
    }
};

// P == 0: one thread per query.
__global__ __launch_bounds__(kBlock) void nearest_within_none_kernel(long long Q, int k, int32_t* __restrict__ count_out,
                                                                     int32_t* __restrict__ idx_out,
                                                                     float* __restrict__ dist2_out)
{
    const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (j < Q) LaneWithin<0>{{k, nullptr, idx_out, dist2_out}, nullptr, 0u, count_out}.store_none(j);
}

// amdgpu_waves_per_eu(8): at K = 16 the compiler otherwise settles one register above the 64 that 8 waves allow.
template <int K>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8))) void nearest_within_wave_kernel(
    IndexView ix, const float* __restrict__ queries, long long Q, const uint64_t* __restrict__ qkeys,
    const uint32_t* __restrict__ qorder, const float* __restrict__ r2, int k, uint32_t max_count,
    const int32_t* __restrict__ exclude, int32_t* __restrict__ count_out, int32_t* __restrict__ idx_out,
    float* __restrict__ dist2_out, uint32_t* __restrict__ hard, Counters* __restrict__ counters)
{
    LaneWithin<K> sr{{k, exclude, idx_out, dist2_out}, r2, max_count, count_out};
    lane_walk(sr, ix, queries, Q, qkeys, qorder, hard, counters);
}

// K = 16 alone keeps the walk in a body of its own, lane_walk's text with the searcher written out.  It sits at
// exactly the 64 registers of 8 waves per SIMD, and through lane_walk the same instructions come out with other
// register numbers and run 5-9% slower where the lane path dominates (profiles/nearest_walk_refactor.md).  A
// change to lane_walk is made here as well.  The two functions below are LaneWithin's eval and bound for it.

// The lane's count and list against the point held by lane c of `pt`, broadcast to every lane.
template <int K>
__device__ __forceinline__ void eval_lane_within(float4 pt, int c, float4 q, uint32_t excl, uint32_t rb, uint32_t& count,
                                                 uint64_t (&list)[K ? K : 1])
{
    const float4 p = make_float4(uniform_lane(pt.x, c), uniform_lane(pt.y, c), uniform_lane(pt.z, c), uniform_lane(pt.w, c));
    uint64_t v = pack_unless(q, p, excl);
    const bool in = in_reach(v, rb);
    count += in;  // at most once per point: below 2^31
    if constexpr (K > 0) {
        v = in ? v : ~0ull;  // out of range: below no entry
        if (v < list[K - 1]) insert_k(list, v);
    }
}

// The lane's bound by the rule above; `live` is false once nothing more can change its answer.
template <int K>
__device__ __forceinline__ uint32_t bound_within(bool active, uint32_t count, uint32_t max_count, uint32_t rb,
                                                 const uint64_t (&list)[K ? K : 1], bool& live)
{
    const bool open = count < max_count;
    live = active && (K > 0 || open);
    if (open) return rb;
    if constexpr (K > 0) return bound_bits(list[K - 1]);
    return 0u;
}

template <int K>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8))) void nearest_within_wave_own_kernel(
    IndexView ix, const float* __restrict__ queries, long long Q, const uint64_t* __restrict__ qkeys,
    const uint32_t* __restrict__ qorder, const float* __restrict__ r2, int k, uint32_t max_count,
    const int32_t* __restrict__ exclude, int32_t* __restrict__ count_out, int32_t* __restrict__ idx_out,
    float* __restrict__ dist2_out, uint32_t* __restrict__ hard, Counters* __restrict__ counters)
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
    uint32_t excl = 0xffffffffu, rb = 0;
    bool reach = false;
    if (inq) {
        q = make_float4(queries[3 * j], queries[3 * j + 1], queries[3 * j + 2], 0.f);
        excl = excluded_row(exclude, j);
        reach = radius_bits(r2[j], rb);
    }
    const bool active = inq && reach && finite3(q.x, q.y, q.z);
    if (inq && !active) LaneWithin<0>{{k, nullptr, idx_out, dist2_out}, nullptr, 0u, count_out}.store_none(j);
    if (!__ballot(active)) return;

    const long long P = ix.P, nleaves = ix.nleaves;
    {
        const long long lf = find_leaf(ix.leaf_keys, nleaves, qkeys[base], lane);
        const long long ll = find_leaf(ix.leaf_keys, nleaves, qkeys[min(base + kWave - 1, Q - 1)], lane);
        if (ll - lf > kSpanBail) {
            push_hard(active, s, hard, counters);
            return;
        }
    }
    uint32_t count = 0;
    uint64_t list[K ? K : 1];  // ascending; list[K - 1] is the k-th best
#pragma unroll
    for (int i = 0; i < (K ? K : 1); i++) list[i] = i < K - k ? 0ull : ~0ull;  // k is wave-uniform

    // seed: the leaf of the wave's median key and its two Morton neighbours, every point against every lane
    const long long Ls = find_leaf(ix.leaf_keys, nleaves, qkeys[min(base + kWave / 2, Q - 1)], lane);
    for (long long C = max(Ls - 1, 0ll); C <= min(Ls + 1, nleaves - 1); C++) {
        const float4 pt = ix.sp[min(C * kLeaf + lane, P - 1)];
        const int nc = (int)min((long long)kLeaf, P - C * kLeaf);
        for (int c = 0; c < nc; c++) eval_lane_within<K>(pt, c, q, excl, rb, count, list);  // wave-uniform
    }

    // the wave's query AABB and the largest bound of its live lanes: the coarse filter
    const float4 qlo = make_float4(wave_min(active ? q.x : FLT_MAX), wave_min(active ? q.y : FLT_MAX),
                                   wave_min(active ? q.z : FLT_MAX), 0.f);
    const float4 qhi = make_float4(wave_max(active ? q.x : -FLT_MAX), wave_max(active ? q.y : -FLT_MAX),
                                   wave_max(active ? q.z : -FLT_MAX), 0.f);
    bool live;
    uint32_t ub = bound_within<K>(active, count, max_count, rb, list, live);
    ub = wave_max_u32(live ? ub : 0u);

    uint32_t* cand = s_list[wave];
    int ncand = 0;
    bool bail = false;
    const int nsuper = __ballot(live) ? ix.nsuper : 0;  // every lane finished by its seed: no walk
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
            if (ncand + cnt > kBailout) {
                bail = true;
                break;
            }
            if (lpass) cand[ncand + __popcll(lm & lanes_below(lane))] = (uint32_t)l;
            ncand += cnt;
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (bail) {
        push_hard(active, s, hard, counters);  // the hard kernel starts each of them again from nothing
        return;
    }

    for (int i = 0; i < ncand; i++) {
        const long long C = (long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)cand[i]);
        const Box lb = ix.leaves[C];  // wave-uniform address
        // fine filter: some live lane's own bound reaches the leaf
        const uint32_t bound = bound_within<K>(active, count, max_count, rb, list, live);
        if (!__ballot(live && point_lb_bits(lb, q) <= bound)) continue;
        const float4 pt = ix.sp[min(C * kLeaf + lane, P - 1)];
        const int nc = (int)min((long long)kLeaf, P - C * kLeaf);
        // a point is evaluated if it is a candidate within the largest live bound of the query AABB
        uint64_t pm = __ballot(lane < nc && pt.x == pt.x && point_lb_bits(Box{qlo, qhi}, pt) <= ub);
        while (pm) {
            const int c = __builtin_ctzll(pm);
            pm &= pm - 1;
            eval_lane_within<K>(pt, c, q, excl, rb, count, list);
        }
        const uint32_t after = bound_within<K>(active, count, max_count, rb, list, live);
        ub = wave_max_u32(live ? after : 0u);
    }
    if (active) {
        count_out[j] = (int32_t)min(count, max_count);
        if constexpr (K > 0) {
#pragma unroll
            for (int i = 0; i < K; i++)
                if (i >= K - k) store_result(list[i], j * k + (i - (K - k)), idx_out, dist2_out);
        }
    }
}

// Two instantiations: with k as a run-time condition of the loops the kernel needs 104-106 SGPRs, 7 waves per SIMD.
template <bool LIST>
__global__ __launch_bounds__(kBlock) void nearest_within_hard_kernel(IndexView ix, const float* __restrict__ queries, long long Q,
                                                                     const uint64_t* __restrict__ qkeys,
                                                                     const uint32_t* __restrict__ qorder,
                                                                     const float* __restrict__ r2, int k, uint32_t max_count,
                                                                     const int32_t* __restrict__ exclude,
                                                                     int32_t* __restrict__ count_out, int32_t* __restrict__ idx_out,
                                                                     float* __restrict__ dist2_out, const uint32_t* __restrict__ hard,
                                                                     const Counters* __restrict__ counters)
{
    hard_list_walk<true, LIST>(ix, queries, Q, qkeys, qorder, r2, k, max_count, exclude, count_out, idx_out, dist2_out, hard,
                               counters);
}

// The query scratch is nearest_query's: the counter word, the (key, row) sort, the hard list.
size_t query_within_scratch_bytes(long long P, long long Q, int k)
{
    return Q > 0 && in_range(Q) && in_range(P) && k >= 0 && k <= kNearestKMax ? query_layout(nullptr, Q).total : 0;
}

template <int K>
constexpr auto within_wave_kernel()
{
    if constexpr (K == kLaneKMax)
        return &nearest_within_wave_own_kernel<K>;
    else
        return &nearest_within_wave_kernel<K>;
}

template <int K>
void launch_within_wave(const QueryCall& c, const float* queries, long long Q, const float* r2, int k, int max_count,
                        const int32_t* exclude, int32_t* count_out, int32_t* idx_out, float* dist2_out)
{
    HIDEGS_LAUNCH("nearest_within_wave", within_wave_kernel<K>(), dim3(c.nb), dim3(kBlock), 0, c.s, c.ix, queries, Q,
                  c.l.sort.keys_sorted, c.l.sort.vals_sorted, r2, k, (uint32_t)max_count, exclude, count_out, idx_out, dist2_out,
                  c.l.hard, c.l.counters);
}

int query_within(const void* index, size_t index_bytes, long long P, void* scratch, size_t scratch_bytes, const float* queries,
                 long long Q, const float* r2, int k, int max_count, const int32_t* exclude, int32_t* count_out,
                 int32_t* idx_out, float* dist2_out, void* stream)
{
    const size_t out_bytes = (size_t)Q * (size_t)k * 4;  // 0 at k == 0: those two overlap nothing
    const char* with_k = k > 0 ? " with k > 0" : nullptr;
    QueryCall c;
    if (!begin_query(c, "nearest_query_within", stream, index, index_bytes, P, scratch, scratch_bytes, queries, Q, k, 0,
                     kNearestKMax, max_count < std::max(k, 1) ? "max_count must be in [max(k, 1), 2^31)" : nullptr,
                     {{r2, (size_t)Q * 4, "r2", ""}, {exclude, (size_t)Q * 4, "exclude"}},
                     {{count_out, (size_t)Q * 4, "count_out", ""},
                      {idx_out, out_bytes, "idx_out", with_k},
                      {dist2_out, out_bytes, "dist2_out", with_k}},
                     [&](const QueryCall& c) {
                         HIDEGS_LAUNCH("nearest_within_none", nearest_within_none_kernel, dim3(c.nb), dim3(kBlock), 0, c.s, Q, k,
                                       count_out, idx_out, dist2_out);
                     }))
        return c.rc;
    if (k == 0)
        launch_within_wave<0>(c, queries, Q, r2, k, max_count, exclude, count_out, idx_out, dist2_out);
    else if (k <= 4)
        launch_within_wave<4>(c, queries, Q, r2, k, max_count, exclude, count_out, idx_out, dist2_out);
    else if (k <= 8)
        launch_within_wave<8>(c, queries, Q, r2, k, max_count, exclude, count_out, idx_out, dist2_out);
    else if (k <= kLaneKMax)
        launch_within_wave<kLaneKMax>(c, queries, Q, r2, k, max_count, exclude, count_out, idx_out, dist2_out);
    else
        HIDEGS_LAUNCH("nearest_within_route", nearest_route_kernel<LaneWithin<0>>, dim3(c.nb), dim3(kBlock), 0, c.s, queries, Q,
                      c.l.sort.vals_sorted, LaneWithin<0>{{k, exclude, idx_out, dist2_out}, r2, (uint32_t)max_count, count_out},
                      c.l.hard, c.l.counters);
    if (k == 0)
        HIDEGS_LAUNCH("nearest_within_hard", nearest_within_hard_kernel<false>, hard_grid(Q), dim3(kBlock), 0, c.s, c.ix, queries, Q,
                      c.l.sort.keys_sorted, c.l.sort.vals_sorted, r2, k, (uint32_t)max_count, exclude, count_out, idx_out,
                      dist2_out, c.l.hard, c.l.counters);
    else
        HIDEGS_LAUNCH("nearest_within_hard", nearest_within_hard_kernel<true>, hard_grid(Q), dim3(kBlock), 0, c.s, c.ix, queries, Q,
                      c.l.sort.keys_sorted, c.l.sort.vals_sorted, r2, k, (uint32_t)max_count, exclude, count_out, idx_out,
                      dist2_out, c.l.hard, c.l.counters);
    return check_launch("nearest_query_within", c.s, 0);
}
