// nearest_within.h -- the fixed-radius query of the nearest-point index (include/hidegs_nearest_within.h): a
// stage of nearest.hip, included inside its namespace after nearest_k.h.  The index, the query keys, the Morton
// sort of the queries, the lower bounds, the hard list and the u64 candidates are nearest.hip's and
// nearest_k.h's; what is new is that every searcher counts the candidates within its query's radius, keeps the
// k best of those only, and takes the bound of every filter from one rule.
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
//   nearest_within_wave_kernel<K>, K = 0, 4, 8, 16: nearest_k_wave_kernel's walk, one lane per sorted query,
//     with a count per lane.  K = 0 keeps no list.  A large radius makes most waves bail: they hand their
//     queries to the hard list, as intended.
//   nearest_within_route_kernel: for k above kLaneKMax, sends every query that can have an answer there.
//   nearest_within_hard_kernel: one wave per query of the hard list; lane i holds the i-th best, the count is
//     wave-uniform.

// rb and whether anything can be in range at all.  For r2 >= 0 clearing the sign bit is r2 + 0.0f: -0 is 0.
__device__ __forceinline__ bool radius_bits(float r2, uint32_t& rb)
{
    rb = __float_as_uint(r2) & 0x7fffffffu;
    return r2 >= 0.f;  // false for a NaN
}

__device__ __forceinline__ bool in_reach(uint64_t v, uint32_t rb) { return (uint32_t)(v >> 32) <= rb; }

__device__ __forceinline__ void store_none_within(long long j, int k, int32_t* __restrict__ count_out,
                                                  int32_t* __restrict__ idx_out, float* __restrict__ dist2_out)
{
    count_out[j] = 0;
    store_none_k(j, k, idx_out, dist2_out);
}

// P == 0: one thread per query.
__global__ __launch_bounds__(kBlock) void nearest_within_none_kernel(long long Q, int k, int32_t* __restrict__ count_out,
                                                                     int32_t* __restrict__ idx_out,
                                                                     float* __restrict__ dist2_out)
{
    const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (j < Q) store_none_within(j, k, count_out, idx_out, dist2_out);
}

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

// amdgpu_waves_per_eu(8): at K = 16 the compiler otherwise settles one register above the 64 that 8 waves allow.
template <int K>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8))) void nearest_within_wave_kernel(
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
    if (inq && !active) store_none_within(j, k, count_out, idx_out, dist2_out);
    if (!__ballot(active)) return;

    const long long P = ix.P, nleaves = ix.nleaves;
    {
        const long long lf = find_leaf(ix.leaf_keys, nleaves, qkeys[base], lane);
        const long long ll = find_leaf(ix.leaf_keys, nleaves, qkeys[min(base + kWave - 1, Q - 1)], lane);
        if (ll - lf > kSpanBail) {
            push_hard(active, s, lane, hard, counters);
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
        if (sidx < nsuper) pass = box_box_lb(ix.supers[sidx], qlo, qhi) <= ub;
        uint64_t smask = __ballot(pass);
        while (smask) {
            const int S = s0 + __builtin_ctzll(smask);
            smask &= smask - 1;
            const long long l = (long long)S * kFan + lane;
            bool lpass = false;
            if (l < nleaves && (l < Ls - 1 || l > Ls + 1))  // those three were the seed
                lpass = box_box_lb(ix.leaves[l], qlo, qhi) <= ub;
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
        push_hard(active, s, lane, hard, counters);  // the hard kernel starts each of them again from nothing
        return;
    }

    for (int i = 0; i < ncand; i++) {
        const long long C = (long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)cand[i]);
        const Box lb = ix.leaves[C];  // wave-uniform address
        // fine filter: some live lane's own bound reaches the leaf
        const uint32_t bound = bound_within<K>(active, count, max_count, rb, list, live);
        if (!__ballot(live && box_point_lb(lb, q) <= bound)) continue;
        const float4 pt = ix.sp[min(C * kLeaf + lane, P - 1)];
        const int nc = (int)min((long long)kLeaf, P - C * kLeaf);
        // a point is evaluated if it is a candidate within the largest live bound of the query AABB
        uint64_t pm = __ballot(lane < nc && pt.x == pt.x && box_point_lb(Box{qlo, qhi}, pt) <= ub);
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

// k above kLaneKMax: a query that is not finite or whose radius takes nothing is answered here, every other
// one goes to the hard list.
__global__ __launch_bounds__(kBlock) void nearest_within_route_kernel(const float* __restrict__ queries, long long Q,
                                                                      const uint32_t* __restrict__ qorder,
                                                                      const float* __restrict__ r2, int k,
                                                                      int32_t* __restrict__ count_out, int32_t* __restrict__ idx_out,
                                                                      float* __restrict__ dist2_out, uint32_t* __restrict__ hard,
                                                                      Counters* __restrict__ counters)
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
        uint32_t rb;
        active = radius_bits(r2[j], rb) && finite3(queries[3 * j], queries[3 * j + 1], queries[3 * j + 2]);
        if (!active) store_none_within(j, k, count_out, idx_out, dist2_out);
    }
    push_hard(active, s, lane_id(), hard, counters);
}

// One wave per hard query.  Lane i holds the i-th best in range (~0: none yet); kth is lane k - 1's value, read
// again after every insertion; count is wave-uniform.  LIST is k > 0: without it there is no list, kth is 0
// (nothing is below it) and a saturated query leaves every loop.
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
        uint32_t rb;
        if (!radius_bits(r2[j], rb)) continue;  // never listed: answered by the launch before
        const long long L = find_leaf(ix.leaf_keys, nleaves, qkeys[s], lane);
        uint64_t top = ~0ull, kth = LIST ? ~0ull : 0ull;
        uint32_t count = 0;
        uint32_t bnd = rb;  // the bound by the rule above, formed again after every leaf

        // The 64 points of leaf C, one per lane: those in range are counted, and those of them below the k-th
        // best are inserted one by one, lowest lane first, as in nearest_k_hard_kernel.
        auto batch = [&](long long C) {
            const long long c = C * kLeaf + lane;
            uint64_t v = ~0ull;
            if (c < P) v = pack_unless(q, ix.sp[c], excl);
            const bool in = in_reach(v, rb);
            count += (uint32_t)__popcll(__ballot(in));
            uint64_t m = LIST ? __ballot(in && v < kth) : 0ull;
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
            bnd = count < max_count ? rb : bound_bits(kth);
        };

        for (long long C = max(L - 1, 0ll); C <= min(L + 1, nleaves - 1); C++) batch(C);
        // with k == 0 a saturated query is finished: a wave-uniform way out of every loop
        for (int s0 = 0; s0 < ix.nsuper && (LIST || count < max_count); s0 += kWave) {  // one super-box per lane
            const int sidx = s0 + lane;
            bool pass = false;
            if (sidx < ix.nsuper) pass = box_point_lb(ix.supers[sidx], q) <= bnd;
            uint64_t smask = __ballot(pass);
            while (smask && (LIST || count < max_count)) {
                const int S = s0 + __builtin_ctzll(smask);
                smask &= smask - 1;
                const long long l = (long long)S * kFan + lane;
                uint32_t llb = 0xffffffffu;  // above every bound: no leaf, or one of the seed
                if (l < nleaves && (l < L - 1 || l > L + 1)) llb = box_point_lb(ix.leaves[l], q);
                uint64_t lmask = __ballot(llb <= bnd);
                while (lmask && (LIST || count < max_count)) {
                    const int b = __builtin_ctzll(lmask);
                    lmask &= lmask - 1;
                    if ((uint32_t)__builtin_amdgcn_readlane((int)llb, b) > bnd) continue;
                    batch((long long)S * kFan + b);
                }
            }
        }
        if (lane == 0) count_out[j] = (int32_t)min(count, max_count);
        if (LIST && lane < k) store_result(top, j * k + lane, idx_out, dist2_out);
    }
}

// The query scratch is nearest_query's: the counter word, the (key, row) sort, the hard list.
size_t query_within_scratch_bytes(long long P, long long Q, int k)
{
    return Q > 0 && in_range(Q) && in_range(P) && k >= 0 && k <= kNearestKMax ? query_layout(nullptr, Q).total : 0;
}

template <int K>
void launch_within_wave(hipStream_t s, unsigned nwg, const IndexView& ix, const float* queries, long long Q, const QueryLayout& l,
                        const float* r2, int k, int max_count, const int32_t* exclude, int32_t* count_out, int32_t* idx_out,
                        float* dist2_out)
{
    HIDEGS_LAUNCH("nearest_within_wave", nearest_within_wave_kernel<K>, dim3(nwg), dim3(kBlock), 0, s, ix, queries, Q,
                  l.sort.keys_sorted, l.sort.vals_sorted, r2, k, (uint32_t)max_count, exclude, count_out, idx_out, dist2_out,
                  l.hard, l.counters);
}

int query_within(const void* index, size_t index_bytes, long long P, void* scratch, size_t scratch_bytes, const float* queries,
                 long long Q, const float* r2, int k, int max_count, const int32_t* exclude, int32_t* count_out,
                 int32_t* idx_out, float* dist2_out, void* stream)
{
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_nearest_query_within", s)) return rc;
    if (k < 0 || k > kNearestKMax) return fail(HIDEGS_E_ARG, "nearest_query_within: k must be in [0, 64]");
    if (max_count < std::max(k, 1))
        return fail(HIDEGS_E_ARG, "nearest_query_within: max_count must be in [max(k, 1), 2^31)");
    if (!in_range(P)) return fail(HIDEGS_E_ARG, "nearest_query_within: P must be in [0, 2^31)");
    if (!in_range(Q)) return fail(HIDEGS_E_ARG, "nearest_query_within: Q must be in [0, 2^31)");
    if (Q == 0) return 0;
    if (!queries) return fail(HIDEGS_E_ARG, "nearest_query_within: NULL queries");
    if (!r2) return fail(HIDEGS_E_ARG, "nearest_query_within: NULL r2");
    if (!count_out) return fail(HIDEGS_E_ARG, "nearest_query_within: NULL count_out");
    if (k > 0 && !idx_out) return fail(HIDEGS_E_ARG, "nearest_query_within: NULL idx_out with k > 0");
    if (k > 0 && !dist2_out) return fail(HIDEGS_E_ARG, "nearest_query_within: NULL dist2_out with k > 0");
    if (P > 0) {
        if (!index || !aligned16(index) || index_bytes < index_layout(nullptr, P).total)
            return fail(HIDEGS_E_ARG, "nearest_query_within: index buffer NULL, not 16-byte aligned or too small for P");
        if (!scratch || !aligned16(scratch) || scratch_bytes < query_layout(nullptr, Q).total)
            return fail(HIDEGS_E_ARG, "nearest_query_within: scratch buffer NULL, not 16-byte aligned or too small");
    } else {
        index = nullptr, index_bytes = 0, scratch = nullptr, scratch_bytes = 0;  // not used
    }
    struct Span {
        const void* p;
        size_t n;
        const char* name;
    };
    const size_t out_bytes = (size_t)Q * (size_t)k * 4;  // 0 at k == 0: those two overlap nothing
    const Span outputs[] = {{count_out, (size_t)Q * 4, "count_out"}, {idx_out, out_bytes, "idx_out"}, {dist2_out, out_bytes, "dist2_out"}};
    const Span inputs[] = {{queries, (size_t)Q * 12, "queries"},
                           {r2, (size_t)Q * 4, "r2"},
                           {exclude, (size_t)Q * 4, "exclude"},
                           {index, index_bytes, "the index"},
                           {scratch, scratch_bytes, "scratch"}};
    for (const auto& in : inputs)
        for (const auto& out : outputs)
            if (overlap(out.p, out.n, in.p, in.n))
                return fail(HIDEGS_E_ARG, std::string("nearest_query_within: ") + out.name + " overlaps " + in.name);
    for (int a = 0; a < 3; a++)
        for (int b = a + 1; b < 3; b++)
            if (overlap(outputs[a].p, outputs[a].n, outputs[b].p, outputs[b].n))
                return fail(HIDEGS_E_ARG, std::string("nearest_query_within: ") + outputs[b].name + " overlaps " + outputs[a].name);
    const unsigned nb = (unsigned)ceil_div(Q, kBlock);  // a thread per query; in the wave kernel, a wave per 64 sorted queries
    if (P == 0) {
        HIDEGS_LAUNCH("nearest_within_none", nearest_within_none_kernel, dim3(nb), dim3(kBlock), 0, s, Q, k, count_out, idx_out,
                      dist2_out);
        return check_launch("nearest_query_within", s, 0);
    }
    const IndexLayout il = index_layout(const_cast<void*>(index), P);
    const IndexView ix{il.frame, il.sp, il.leaves, il.supers, il.leaf_keys, P, il.nleaves, il.nsuper};
    const QueryLayout l = query_layout(scratch, Q);
    if (hipMemsetAsync(l.counters, 0, sizeof(Counters), s) != hipSuccess)
        return fail(HIDEGS_E_HIP, "nearest_query_within: clearing the counter failed");
    HIDEGS_LAUNCH("nearest_query_keys", nearest_query_keys_kernel, dim3(nb), dim3(kBlock), 0, s, queries, Q, ix.frame,
                  l.sort.keys, l.sort.vals);
    if (int rc = sort_pairs_u64(l.sort.sort_tmp, l.sort.sort_bytes, l.sort.keys, l.sort.keys_sorted, l.sort.vals,
                                l.sort.vals_sorted, Q, 0, 3 * kMortonBits, s))
        return rc;
    if (k == 0)
        launch_within_wave<0>(s, nb, ix, queries, Q, l, r2, k, max_count, exclude, count_out, idx_out, dist2_out);
    else if (k <= 4)
        launch_within_wave<4>(s, nb, ix, queries, Q, l, r2, k, max_count, exclude, count_out, idx_out, dist2_out);
    else if (k <= 8)
        launch_within_wave<8>(s, nb, ix, queries, Q, l, r2, k, max_count, exclude, count_out, idx_out, dist2_out);
    else if (k <= kLaneKMax)
        launch_within_wave<kLaneKMax>(s, nb, ix, queries, Q, l, r2, k, max_count, exclude, count_out, idx_out, dist2_out);
    else
        HIDEGS_LAUNCH("nearest_within_route", nearest_within_route_kernel, dim3(nb), dim3(kBlock), 0, s, queries, Q,
                      l.sort.vals_sorted, r2, k, count_out, idx_out, dist2_out, l.hard, l.counters);
    const dim3 hgrid(std::min<unsigned>(kHardGrid, (unsigned)ceil_div(Q, kWaves)));
    if (k == 0)
        HIDEGS_LAUNCH("nearest_within_hard", nearest_within_hard_kernel<false>, hgrid, dim3(kBlock), 0, s, ix, queries, Q,
                      l.sort.keys_sorted, l.sort.vals_sorted, r2, k, (uint32_t)max_count, exclude, count_out, idx_out,
                      dist2_out, l.hard, l.counters);
    else
        HIDEGS_LAUNCH("nearest_within_hard", nearest_within_hard_kernel<true>, hgrid, dim3(kBlock), 0, s, ix, queries, Q,
                      l.sort.keys_sorted, l.sort.vals_sorted, r2, k, (uint32_t)max_count, exclude, count_out, idx_out,
                      dist2_out, l.hard, l.counters);
    return check_launch("nearest_query_within", s, 0);
}
