// nearest_k.h -- the k-nearest query of the nearest-point index (include/hidegs_nearest_k.h): a stage of
// nearest.hip, included inside its namespace.  The index, the query keys, the Morton sort of the queries, the
// lower bounds and the hard list are nearest.hip's; what is new is that every searcher keeps its k best
// instead of its best, and that every filter takes its bound from the k-th best.
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
//   nearest_k_wave_kernel<K>: nearest_wave_kernel's walk, one lane per sorted query; the lane's K best are a
//     sorted array in registers (static indices only).  A call with k <= K keeps K - k slots at 0 below the
//     list: nothing is below 0, so they stay, the list's last entry is the k-th best whatever k is, and the
//     k results are the last k slots.
//   nearest_k_route_kernel: for k above kLaneKMax, sends every finite query to the hard list.
//   nearest_k_hard_kernel: one wave per query of the hard list; lane i holds the i-th best.

constexpr int kLaneKMax = 16;  // the largest K of nearest_k_wave_kernel: instantiated for 4, 8 and 16
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

// list is ascending and v < list[K - 1]: v takes its place, the last entry leaves.
template <int K>
__device__ __forceinline__ void insert_k(uint64_t (&list)[K], uint64_t v)
{
#pragma unroll
    for (int i = K - 1; i >= 1; i--) list[i] = v < list[i - 1] ? list[i - 1] : min(v, list[i]);
    list[0] = min(v, list[0]);
}

// The list against the point held by lane c of `pt`, broadcast to every lane.
template <int K>
__device__ __forceinline__ void eval_lane_k(float4 pt, int c, float4 q, uint32_t excl, uint64_t (&list)[K])
{
    const float4 p = make_float4(uniform_lane(pt.x, c), uniform_lane(pt.y, c), uniform_lane(pt.z, c), uniform_lane(pt.w, c));
    const uint64_t v = pack_unless(q, p, excl);
    if (v < list[K - 1]) insert_k(list, v);
}

__device__ __forceinline__ void store_none_k(long long j, int k, int32_t* __restrict__ idx_out, float* __restrict__ dist2_out)
{
    for (int i = 0; i < k; i++) store_result(~0ull, j * k + i, idx_out, dist2_out);
}

template <int K>
__global__ __launch_bounds__(kBlock) void nearest_k_wave_kernel(IndexView ix, const float* __restrict__ queries, long long Q,
                                                                const uint64_t* __restrict__ qkeys,
                                                                const uint32_t* __restrict__ qorder, int k,
                                                                const int32_t* __restrict__ exclude, int32_t* __restrict__ idx_out,
                                                                float* __restrict__ dist2_out, uint32_t* __restrict__ hard,
                                                                Counters* __restrict__ counters)
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
    uint32_t excl = 0xffffffffu;
    if (inq) {
        q = make_float4(queries[3 * j], queries[3 * j + 1], queries[3 * j + 2], 0.f);
        excl = excluded_row(exclude, j);
    }
    const bool active = inq && finite3(q.x, q.y, q.z);
    if (inq && !active) store_none_k(j, k, idx_out, dist2_out);
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
    uint64_t list[K];  // ascending; list[K - 1] is the k-th best
#pragma unroll
    for (int i = 0; i < K; i++) list[i] = i < K - k ? 0ull : ~0ull;  // k is wave-uniform

    // seed: the leaf of the wave's median key and its two Morton neighbours, every point against every lane
    const long long Ls = find_leaf(ix.leaf_keys, nleaves, qkeys[min(base + kWave / 2, Q - 1)], lane);
    for (long long C = max(Ls - 1, 0ll); C <= min(Ls + 1, nleaves - 1); C++) {
        const float4 pt = ix.sp[min(C * kLeaf + lane, P - 1)];
        const int nc = (int)min((long long)kLeaf, P - C * kLeaf);
        for (int c = 0; c < nc; c++) eval_lane_k(pt, c, q, excl, list);  // wave-uniform
    }

    // the wave's query AABB and the largest k-th bound of its lanes: the coarse filter
    const float4 qlo = make_float4(wave_min(active ? q.x : FLT_MAX), wave_min(active ? q.y : FLT_MAX),
                                   wave_min(active ? q.z : FLT_MAX), 0.f);
    const float4 qhi = make_float4(wave_max(active ? q.x : -FLT_MAX), wave_max(active ? q.y : -FLT_MAX),
                                   wave_max(active ? q.z : -FLT_MAX), 0.f);
    uint32_t ub = wave_max_u32(active ? bound_bits(list[K - 1]) : 0u);

    uint32_t* cand = s_list[wave];
    int ncand = 0;
    bool bail = false;
    for (int s0 = 0; s0 < ix.nsuper && !bail; s0 += kWave) {  // one super-box per lane
        const int sidx = s0 + lane;
        bool pass = false;
        if (sidx < ix.nsuper) pass = box_box_lb(ix.supers[sidx], qlo, qhi) <= ub;
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
        push_hard(active, s, lane, hard, counters);
        return;
    }

    for (int i = 0; i < ncand; i++) {
        const long long C = (long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)cand[i]);
        const Box lb = ix.leaves[C];  // wave-uniform address
        // fine filter: some lane's own k-th bound reaches the leaf
        if (!__ballot(active && box_point_lb(lb, q) <= bound_bits(list[K - 1]))) continue;
        const float4 pt = ix.sp[min(C * kLeaf + lane, P - 1)];
        const int nc = (int)min((long long)kLeaf, P - C * kLeaf);
        // a point is evaluated if it is a candidate within the largest k-th bound of the query AABB
        uint64_t pm = __ballot(lane < nc && pt.x == pt.x && box_point_lb(Box{qlo, qhi}, pt) <= ub);
        while (pm) {
            const int c = __builtin_ctzll(pm);
            pm &= pm - 1;
            eval_lane_k(pt, c, q, excl, list);
        }
        ub = wave_max_u32(active ? bound_bits(list[K - 1]) : 0u);
    }
    if (active) {
#pragma unroll
        for (int i = 0; i < K; i++)
            if (i >= K - k) store_result(list[i], j * k + (i - (K - k)), idx_out, dist2_out);
    }
}

// k above kLaneKMax: a non-finite query is answered here, every other one goes to the hard list.
__global__ __launch_bounds__(kBlock) void nearest_k_route_kernel(const float* __restrict__ queries, long long Q,
                                                                 const uint32_t* __restrict__ qorder, int k,
                                                                 int32_t* __restrict__ idx_out, float* __restrict__ dist2_out,
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
        active = finite3(queries[3 * j], queries[3 * j + 1], queries[3 * j + 2]);
        if (!active) store_none_k(j, k, idx_out, dist2_out);
    }
    push_hard(active, s, lane_id(), hard, counters);
}

// One wave per hard query.  Lane i holds the i-th best (~0: none yet); kth is lane k - 1's value, the bound
// of every filter, read again after every insertion.
__global__ __launch_bounds__(kBlock) void nearest_k_hard_kernel(IndexView ix, const float* __restrict__ queries, long long Q,
                                                                const uint64_t* __restrict__ qkeys,
                                                                const uint32_t* __restrict__ qorder, int k,
                                                                const int32_t* __restrict__ exclude, int32_t* __restrict__ idx_out,
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
        const long long L = find_leaf(ix.leaf_keys, nleaves, qkeys[s], lane);
        uint64_t top = ~0ull, kth = ~0ull;

        // The 64 points of leaf C, one per lane: those below the k-th best are inserted one by one, lowest lane
        // first.  Its rank is the number of entries below it; the entries from there on move up a lane.
        auto batch = [&](long long C) {
            const long long c = C * kLeaf + lane;
            uint64_t v = ~0ull;
            if (c < P) v = pack_unless(q, ix.sp[c], excl);
            uint64_t m = __ballot(v < kth);
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
        };

        for (long long C = max(L - 1, 0ll); C <= min(L + 1, nleaves - 1); C++) batch(C);
        for (int s0 = 0; s0 < ix.nsuper; s0 += kWave) {  // one super-box per lane
            const int sidx = s0 + lane;
            bool pass = false;
            if (sidx < ix.nsuper) pass = box_point_lb(ix.supers[sidx], q) <= bound_bits(kth);
            uint64_t smask = __ballot(pass);
            while (smask) {
                const int S = s0 + __builtin_ctzll(smask);
                smask &= smask - 1;
                const long long l = (long long)S * kFan + lane;
                uint32_t llb = 0xffffffffu;  // above every bound: no leaf, or one of the seed
                if (l < nleaves && (l < L - 1 || l > L + 1)) llb = box_point_lb(ix.leaves[l], q);
                uint64_t lmask = __ballot(llb <= bound_bits(kth));
                while (lmask) {
                    const int b = __builtin_ctzll(lmask);
                    lmask &= lmask - 1;
                    if ((uint32_t)__builtin_amdgcn_readlane((int)llb, b) > bound_bits(kth)) continue;
                    batch((long long)S * kFan + b);
                }
            }
        }
        if (lane < k) store_result(top, j * k + lane, idx_out, dist2_out);
    }
}

// The query scratch is nearest_query's: the counter word, the (key, row) sort, the hard list.
size_t query_k_scratch_bytes(long long P, long long Q, int k)
{
    return Q > 0 && in_range(Q) && in_range(P) && k >= 1 && k <= kNearestKMax ? query_layout(nullptr, Q).total : 0;
}

template <int K>
void launch_k_wave(hipStream_t s, unsigned nwg, const IndexView& ix, const float* queries, long long Q, const QueryLayout& l,
                   int k, const int32_t* exclude, int32_t* idx_out, float* dist2_out)
{
    HIDEGS_LAUNCH("nearest_k_wave", nearest_k_wave_kernel<K>, dim3(nwg), dim3(kBlock), 0, s, ix, queries, Q,
                  l.sort.keys_sorted, l.sort.vals_sorted, k, exclude, idx_out, dist2_out, l.hard, l.counters);
}

int query_k(const void* index, size_t index_bytes, long long P, void* scratch, size_t scratch_bytes, const float* queries,
            long long Q, int k, const int32_t* exclude, int32_t* idx_out, float* dist2_out, void* stream)
{
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_nearest_query_k", s)) return rc;
    if (k < 1 || k > kNearestKMax) return fail(HIDEGS_E_ARG, "nearest_query_k: k must be in [1, 64]");
    if (!in_range(P)) return fail(HIDEGS_E_ARG, "nearest_query_k: P must be in [0, 2^31)");
    if (!in_range(Q)) return fail(HIDEGS_E_ARG, "nearest_query_k: Q must be in [0, 2^31)");
    if (Q == 0) return 0;
    if (!queries) return fail(HIDEGS_E_ARG, "nearest_query_k: NULL queries");
    if (!idx_out) return fail(HIDEGS_E_ARG, "nearest_query_k: NULL idx_out");
    if (!dist2_out) return fail(HIDEGS_E_ARG, "nearest_query_k: NULL dist2_out");
    if (P > 0) {
        if (!index || !aligned16(index) || index_bytes < index_layout(nullptr, P).total)
            return fail(HIDEGS_E_ARG, "nearest_query_k: index buffer NULL, not 16-byte aligned or too small for P");
        if (!scratch || !aligned16(scratch) || scratch_bytes < query_layout(nullptr, Q).total)
            return fail(HIDEGS_E_ARG, "nearest_query_k: scratch buffer NULL, not 16-byte aligned or too small");
    } else {
        index = nullptr, index_bytes = 0, scratch = nullptr, scratch_bytes = 0;  // not used
    }
    const size_t out_bytes = (size_t)Q * (size_t)k * 4;
    struct {
        const void* p;
        size_t n;
        const char* name;
    } const inputs[] = {{queries, (size_t)Q * 12, "queries"},
                        {exclude, (size_t)Q * 4, "exclude"},
                        {index, index_bytes, "the index"},
                        {scratch, scratch_bytes, "scratch"}};
    for (const auto& in : inputs) {
        if (overlap(idx_out, out_bytes, in.p, in.n))
            return fail(HIDEGS_E_ARG, std::string("nearest_query_k: idx_out overlaps ") + in.name);
        if (overlap(dist2_out, out_bytes, in.p, in.n))
            return fail(HIDEGS_E_ARG, std::string("nearest_query_k: dist2_out overlaps ") + in.name);
    }
    if (overlap(idx_out, out_bytes, dist2_out, out_bytes))
        return fail(HIDEGS_E_ARG, "nearest_query_k: dist2_out overlaps idx_out");
    if (P == 0) {
        const long long n = Q * k;
        HIDEGS_LAUNCH("nearest_none", nearest_none_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, s, n, idx_out,
                      dist2_out);
        return check_launch("nearest_query_k", s, 0);
    }
    const IndexLayout il = index_layout(const_cast<void*>(index), P);
    const IndexView ix{il.frame, il.sp, il.leaves, il.supers, il.leaf_keys, P, il.nleaves, il.nsuper};
    const QueryLayout l = query_layout(scratch, Q);
    if (hipMemsetAsync(l.counters, 0, sizeof(Counters), s) != hipSuccess)
        return fail(HIDEGS_E_HIP, "nearest_query_k: clearing the counter failed");
    const unsigned nb = (unsigned)ceil_div(Q, kBlock);  // a thread per query; in the wave kernel, a wave per 64 sorted queries
    HIDEGS_LAUNCH("nearest_query_keys", nearest_query_keys_kernel, dim3(nb), dim3(kBlock), 0, s, queries, Q, ix.frame,
                  l.sort.keys, l.sort.vals);
    if (int rc = sort_pairs_u64(l.sort.sort_tmp, l.sort.sort_bytes, l.sort.keys, l.sort.keys_sorted, l.sort.vals,
                                l.sort.vals_sorted, Q, 0, 3 * kMortonBits, s))
        return rc;
    if (k <= 4)
        launch_k_wave<4>(s, nb, ix, queries, Q, l, k, exclude, idx_out, dist2_out);
    else if (k <= 8)
        launch_k_wave<8>(s, nb, ix, queries, Q, l, k, exclude, idx_out, dist2_out);
    else if (k <= kLaneKMax)
        launch_k_wave<kLaneKMax>(s, nb, ix, queries, Q, l, k, exclude, idx_out, dist2_out);
    else
        HIDEGS_LAUNCH("nearest_k_route", nearest_k_route_kernel, dim3(nb), dim3(kBlock), 0, s, queries, Q, l.sort.vals_sorted, k,
                      idx_out, dist2_out, l.hard, l.counters);
    HIDEGS_LAUNCH("nearest_k_hard", nearest_k_hard_kernel, dim3(std::min<unsigned>(kHardGrid, (unsigned)ceil_div(Q, kWaves))),
                  dim3(kBlock), 0, s, ix, queries, Q, l.sort.keys_sorted, l.sort.vals_sorted, k, exclude, idx_out, dist2_out,
                  l.hard, l.counters);
    return check_launch("nearest_query_k", s, 0);
}
