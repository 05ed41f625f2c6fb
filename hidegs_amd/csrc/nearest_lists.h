// nearest_lists.h -- the neighbour lists of the nearest-point index (include/hidegs_nearest_lists.h): a stage of
// nearest.hip, included inside its namespace after nearest_within.h.  The index, begin_query, the lower bounds and
// hard_grid are nearest.hip's, pack_unless, in_reach and radius_bits nearest_k.h's, and the count of every list is
// nearest_within.h's query_within with k = 0 and no cap, called as it stands.  What is new is the kernel that
// writes the lists.
//
// Rule: the list of a query is the candidates in range in ascending position of the index.  One bound per query,
// rb, the bits of its squared radius, fixed for the whole walk; no seeds.  Every super-box whose lower bound is
// <= rb is opened in ascending order, in it every leaf whose lower bound is <= rb in ascending order, and in it
// the 64 points, one per lane: those in range are written behind what the query has written so far, lowest lane
// first.  A position in the index is (super-box, leaf, lane), so the order of writing is the order of position.
//
// Exactness: a box is skipped only when its lower bound is strictly above rb, and every distance in it is at
// least that bound (nearest.hip: the distance's own monotone expression on componentwise smaller gaps), so every
// point in range is met; a leaf belongs to one super-box and is met once, so it is met exactly once.  The
// in-range test is the count kernels' own expression on the same value (pack_unless, in_reach), so a list has as
// many entries as query_within counted, and starts[j] + i stays below starts[j + 1].
//
//   nearest_index_order_kernel: the fourth component of every stored point is its row (nearest_gather_kernel
//     writes it for candidates and non-candidates alike).
//   nearest_list_info_kernel: M in 64 bits, the longest list and the number of non-empty ones, by one integer
//     atomic each per wave on words that the call cleared; also starts_out[0].
//   nearest_list_fill_kernel<DIST>: one wave per query in sorted-query order, capped like every wave-per-query
//     launch.  Every loop is bounded by nsuper, a ballot's bits or Q; no workgroup waits on another.

constexpr int kInfoGrid = 1024;  // workgroups of nearest_list_info_kernel at most

__global__ __launch_bounds__(kBlock) void nearest_index_order_kernel(const float4* __restrict__ sp, long long P,
                                                                     int32_t* __restrict__ order_out)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < P) order_out[i] = (int32_t)__float_as_uint(sp[i].w);
}

// starts_out[1 + j] holds query j's count (the scan comes after this kernel).  info was cleared by the call.
__global__ __launch_bounds__(kBlock) void nearest_list_info_kernel(int32_t* __restrict__ starts_out, long long Q,
                                                                   uint32_t* __restrict__ info)
{
    unsigned long long sum = 0;
    uint32_t longest = 0, filled = 0;
    for (long long j = (long long)blockIdx.x * kBlock + threadIdx.x; j < Q; j += (long long)gridDim.x * kBlock) {
        const uint32_t c = (uint32_t)starts_out[1 + j];
        sum += c;
        longest = max(longest, c);
        filled += c != 0;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, kWave);
    longest = wave_max_u32(longest);
    filled = wave_sum_u32(filled);
    if (lane_id() == 0 && filled) {  // the three are 0 together
        atomicAdd(reinterpret_cast<unsigned long long*>(info), sum);  // info is 8-byte aligned
        atomicMax(info + 2, longest);
        atomicAdd(info + 3, filled);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) starts_out[0] = 0;
}

// One wave per query.  base, end and every mask are wave-uniform; the lanes differ in the box, leaf or point they
// hold.  A position is written iff it is in [beg, end), and end <= capacity: no store leaves the caller's buffers
// whatever `starts` holds.
template <bool DIST>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8))) void nearest_list_fill_kernel(
    IndexView ix, const float* __restrict__ queries, long long Q, const uint32_t* __restrict__ qorder,
    const float* __restrict__ r2, const int32_t* __restrict__ exclude, const int32_t* __restrict__ starts, uint32_t capacity,
    int32_t* __restrict__ rows_out, float* __restrict__ dist2_out)
{
    const int lane = lane_id();
    const long long P = ix.P, nleaves = ix.nleaves;
    const int nsuper = ix.nsuper;
    const long long nw = (long long)gridDim.x * kWaves;
    for (long long s = (long long)blockIdx.x * kWaves + threadIdx.x / kWave; s < Q; s += nw) {
        const long long j = qorder[s];
        if (j >= Q) continue;  // a permutation of [0, Q) by construction
        const int32_t beg = starts[j], stop = starts[j + 1];
        if (beg < 0 || stop <= beg) continue;  // an empty list, or no span at all
        const uint32_t end = min((uint32_t)stop, capacity);
        uint32_t base = (uint32_t)beg;
        if (base >= end) continue;  // wholly behind the cut
        const float4 q = make_float4(queries[3 * j], queries[3 * j + 1], queries[3 * j + 2], 0.f);
        uint32_t rb;
        if (!radius_bits(r2[j], rb) || !finite3(q.x, q.y, q.z)) continue;  // nothing is in range
        const uint32_t excl = excluded_row(exclude, j);

        for (int s0 = 0; s0 < nsuper && base < end; s0 += kWave) {  // one super-box per lane
            const int sidx = s0 + lane;
            bool pass = false;
            if (sidx < nsuper) pass = point_lb_bits(ix.supers[sidx], q) <= rb;
            uint64_t smask = __ballot(pass);
            while (smask && base < end) {
                const int S = s0 + __builtin_ctzll(smask);
                smask &= smask - 1;
                const long long l = (long long)S * kFan + lane;  // one leaf per lane
                bool lpass = false;
                if (l < nleaves) lpass = point_lb_bits(ix.leaves[l], q) <= rb;
                uint64_t lmask = __ballot(lpass);
                while (lmask && base < end) {
                    const long long c = ((long long)S * kFan + __builtin_ctzll(lmask)) * kLeaf + lane;  // one point per lane
                    lmask &= lmask - 1;
                    uint64_t v = ~0ull;
                    if (c < P) v = pack_unless(q, ix.sp[c], excl);
                    const bool in = in_reach(v, rb);
                    const uint64_t m = __ballot(in);
                    const uint32_t pos = base + (uint32_t)__popcll(m & lanes_below(lane));
                    if (in && pos < end) {
                        rows_out[pos] = (int32_t)(uint32_t)v;
                        if constexpr (DIST) dist2_out[pos] = __uint_as_float((uint32_t)(v >> 32));
                    }
                    base += (uint32_t)__popcll(m);  // below end + 64: no wrap
                }
            }
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------
// What hidegs_nearest_list_offsets carves from its scratch: the count query's own scratch, then the scan's.
struct OffsetsLayout {
    void* query;
    size_t query_bytes;
    void* scan_tmp;
    size_t scan_bytes;
    size_t total;
};

OffsetsLayout offsets_layout(void* base, long long Q)
{
    OffsetsLayout l;
    Carver c(base);
    l.query_bytes = query_layout(nullptr, Q).total;
    l.query = c.take<char>(l.query_bytes);
    l.scan_bytes = hidegs_scan_scratch_bytes(Q);
    l.scan_tmp = c.take<char>(l.scan_bytes);
    l.total = c.used;
    return l;
}

size_t list_offsets_scratch_bytes(long long P, long long Q)
{
    return Q > 0 && in_range(Q) && in_range(P) ? offsets_layout(nullptr, Q).total : 0;
}

size_t list_fill_scratch_bytes(long long P, long long Q)
{
    return Q > 0 && in_range(Q) && in_range(P) ? query_layout(nullptr, Q).total : 0;
}

int index_order(const void* index, size_t index_bytes, long long P, int32_t* order_out, void* stream)
{
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_nearest_index_order", s)) return rc;
    if (!in_range(P)) return fail(HIDEGS_E_ARG, "nearest_index_order: P must be in [0, 2^31)");
    if (P == 0) return 0;
    if (!order_out) return fail(HIDEGS_E_ARG, "nearest_index_order: NULL order_out");
    if (!index || !aligned16(index) || index_bytes < index_layout(nullptr, P).total)
        return fail(HIDEGS_E_ARG, "nearest_index_order: index buffer NULL, not 16-byte aligned or too small for P");
    if (overlap(order_out, (size_t)P * 4, index, index_bytes))
        return fail(HIDEGS_E_ARG, "nearest_index_order: order_out overlaps the index");
    const IndexLayout il = index_layout(const_cast<void*>(index), P);
    HIDEGS_LAUNCH("nearest_index_order", nearest_index_order_kernel, dim3((unsigned)ceil_div(P, kBlock)), dim3(kBlock), 0, s,
                  il.sp, P, order_out);
    return check_launch("nearest_index_order", s, 0);
}

int list_offsets(const void* index, size_t index_bytes, long long P, void* scratch, size_t scratch_bytes, const float* queries,
                 long long Q, const float* r2, const int32_t* exclude, int32_t* starts_out, uint32_t* info_out, void* stream)
{
    const std::string who = "nearest_list_offsets: ";
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_nearest_list_offsets", s)) return rc;
    if (!in_range(P)) return fail(HIDEGS_E_ARG, who + "P must be in [0, 2^31)");
    if (!in_range(Q)) return fail(HIDEGS_E_ARG, who + "Q must be in [0, 2^31)");
    if (!starts_out) return fail(HIDEGS_E_ARG, who + "NULL starts_out");
    if (!info_out || (reinterpret_cast<uintptr_t>(info_out) & 7))
        return fail(HIDEGS_E_ARG, who + "info_out NULL or not 8-byte aligned");
    const Span outputs[2] = {{starts_out, (size_t)(Q + 1) * 4, "starts_out"}, {info_out, 16, "info_out"}};
    const bool search = P > 0 && Q > 0;
    if (Q > 0) {
        if (!queries) return fail(HIDEGS_E_ARG, who + "NULL queries");
        if (!r2) return fail(HIDEGS_E_ARG, who + "NULL r2");
    }
    if (search) {
        if (!index || !aligned16(index) || index_bytes < index_layout(nullptr, P).total)
            return fail(HIDEGS_E_ARG, who + "index buffer NULL, not 16-byte aligned or too small for P");
        if (!scratch || !aligned16(scratch) || scratch_bytes < offsets_layout(nullptr, Q).total)
            return fail(HIDEGS_E_ARG, who + "scratch buffer NULL, not 16-byte aligned or too small");
    } else {
        index = nullptr, index_bytes = 0, scratch = nullptr, scratch_bytes = 0;  // not used
    }
    const Span inputs[5] = {{queries, (size_t)Q * 12, "queries"}, {r2, (size_t)Q * 4, "r2"}, {exclude, (size_t)Q * 4, "exclude"},
                            {index, index_bytes, "the index"}, {scratch, scratch_bytes, "scratch"}};
    for (const Span& in : inputs)
        for (const Span& out : outputs)
            if (overlap(out.p, out.n, in.p, in.n)) return fail(HIDEGS_E_ARG, who + out.name + " overlaps " + in.name);
    if (overlap(outputs[0].p, outputs[0].n, outputs[1].p, outputs[1].n))
        return fail(HIDEGS_E_ARG, who + "info_out overlaps starts_out");

    if (hipMemsetAsync(info_out, 0, 16, s) != hipSuccess) return fail(HIDEGS_E_HIP, who + "clearing info_out failed");
    if (!search) {  // every list is empty
        if (hipMemsetAsync(starts_out, 0, (size_t)(Q + 1) * 4, s) != hipSuccess)
            return fail(HIDEGS_E_HIP, who + "clearing starts_out failed");
        return check_launch("nearest_list_offsets", s, 0);
    }
    const OffsetsLayout l = offsets_layout(scratch, Q);
    // the exact counts, by the count query as it stands, into starts_out[1 .. Q]
    if (int rc = query_within(index, index_bytes, P, l.query, l.query_bytes, queries, Q, r2, 0, (int)kNearestMax, exclude,
                              starts_out + 1, nullptr, nullptr, stream))
        return rc;
    const unsigned nb = (unsigned)std::min<long long>(kInfoGrid, ceil_div(Q, kBlock));
    HIDEGS_LAUNCH("nearest_list_info", nearest_list_info_kernel, dim3(nb), dim3(kBlock), 0, s, starts_out, Q, info_out);
    uint32_t* counts = reinterpret_cast<uint32_t*>(starts_out + 1);
    if (int rc = hidegs_inclusive_scan_u32(l.scan_tmp, l.scan_bytes, counts, counts, Q, stream)) return rc;
    return check_launch("nearest_list_offsets", s, 0);
}

int list_fill(const void* index, size_t index_bytes, long long P, void* scratch, size_t scratch_bytes, const float* queries,
              long long Q, const float* r2, const int32_t* exclude, const int32_t* starts, long long capacity, int32_t* rows_out,
              float* dist2_out, void* stream)
{
    const long long cap = std::min(std::max(capacity, 0ll), kNearestMax);  // positions are below 2^31
    const size_t out_bytes = (size_t)cap * 4;  // 0 at capacity == 0: those two overlap nothing
    QueryCall c;
    if (!begin_query(c, "nearest_list_fill", stream, index, index_bytes, P, scratch, scratch_bytes, queries, Q, 0, 0, 0,
                     capacity < 0 ? "capacity must not be negative" : nullptr,
                     {{r2, (size_t)Q * 4, "r2", ""}, {exclude, (size_t)Q * 4, "exclude"}, {starts, (size_t)(Q + 1) * 4, "starts", ""}},
                     {{rows_out, out_bytes, "rows_out", cap > 0 ? " with capacity > 0" : nullptr},
                      {dist2_out, out_bytes, "dist2_out"}},
                     [](const QueryCall&) {}))  // P == 0: every list is empty, nothing to write
        return c.rc;
    if (cap == 0) return check_launch("nearest_list_fill", c.s, 0);
    if (dist2_out)
        HIDEGS_LAUNCH("nearest_list_fill", nearest_list_fill_kernel<true>, hard_grid(Q), dim3(kBlock), 0, c.s, c.ix, queries, Q,
                      c.l.sort.vals_sorted, r2, exclude, starts, (uint32_t)cap, rows_out, dist2_out);
    else
        HIDEGS_LAUNCH("nearest_list_fill", nearest_list_fill_kernel<false>, hard_grid(Q), dim3(kBlock), 0, c.s, c.ix, queries, Q,
                      c.l.sort.vals_sorted, r2, exclude, starts, (uint32_t)cap, rows_out, dist2_out);
    return check_launch("nearest_list_fill", c.s, 0);
}
