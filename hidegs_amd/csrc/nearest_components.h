// nearest_components.h -- connected components within a radius, fused with the search
// (hidegs_nearest_components_within, include/hidegs_components.h): a stage of nearest.hip, included inside its
// namespace after nearest_lists.h.  The walk is nearest_list_fill_kernel's, the in-range test the count kernels' own
// expression (pack_unless, in_reach, radius_bits of nearest_k.h), find and unite union_find.h's.
//
// The queries are the index's own points in the index's own order: the wave that serves position s reads its
// query from ix.sp[s], whose fourth component is the row, so there are no query keys, no query sort and no scratch.
// Where the fill kernel stores a candidate in range, the lane that holds it links the candidate's root to the
// query's, found once per wave and refreshed by the lane, unless the two are one already.  No list is written,
// there is no offsets pass and nothing is searched twice.
//
// With one radius for all rows the distance is symmetric in every bit ((p - q) is -(q - p) exactly), so the edge
// {a, b} is met from both ends; the walk then looks only at positions below its own, which halves the boxes it
// opens and the unites it makes.  With a radius per row it looks at every position but its own: the edge exists if
// either end reaches the other.
//
//   nearest_components_kernel<PER_ROW>: one wave per position, capped like every wave-per-query launch.  Every
//     loop is bounded by nsuper, a ballot's bits or P; no workgroup waits on another.

template <bool PER_ROW>
__global__ __launch_bounds__(kBlock) void nearest_components_kernel(IndexView ix, const float* __restrict__ r2,
                                                                    int32_t* __restrict__ parent)
{
    const int lane = lane_id();
    const long long P = ix.P, nleaves = ix.nleaves;
    const long long nw = (long long)gridDim.x * kWaves;
    for (long long s = (long long)blockIdx.x * kWaves + threadIdx.x / kWave; s < P; s += nw) {
        const float4 q = ix.sp[s];  // wave-uniform address
        if (!(q.x == q.x)) continue;  // no candidate: stored as NaNs
        const uint32_t j = __float_as_uint(q.w);
        if (j >= (uint32_t)P) continue;  // a permutation of [0, P) by construction
        const int32_t pj = uf_load(parent + j);
        if (pj < 0) continue;  // no node
        uint32_t rb;
        if (!radius_bits(PER_ROW ? r2[j] : r2[0], rb)) continue;  // nothing is in range
        const long long cend = PER_ROW ? P : s;  // positions [0, cend) but s itself
        // The query's root, found once for the wave from the word just read.  It may go stale while the wave walks
        // (another root goes below it); it stays a row of j's component, so a candidate whose root it is needs nothing,
        // and any other is linked to the root found from it afresh: loads only, where a swap on a stale root would
        // be an atomic that fails for every candidate of the wave.
        int32_t sj;
        const int32_t rj = uf_find_from<true>(parent, (int32_t)j, pj, sj);
        const long long nl = (cend + kLeaf - 1) / kLeaf;    // the leaves and super-boxes that hold them
        const int nsuper = (int)((nl + kFan - 1) / kFan);

        for (int s0 = 0; s0 < nsuper; s0 += kWave) {  // one super-box per lane
            const int sidx = s0 + lane;
            bool pass = false;
            if (sidx < nsuper) pass = point_lb_bits(ix.supers[sidx], q) <= rb;
            uint64_t smask = __ballot(pass);
            while (smask) {
                const int S = s0 + __builtin_ctzll(smask);
                smask &= smask - 1;
                const long long l = (long long)S * kFan + lane;  // one leaf per lane
                bool lpass = false;
                if (l < nl && l < nleaves) lpass = point_lb_bits(ix.leaves[l], q) <= rb;
                uint64_t lmask = __ballot(lpass);
                while (lmask) {
                    const long long c = ((long long)S * kFan + __builtin_ctzll(lmask)) * kLeaf + lane;  // one point per lane
                    lmask &= lmask - 1;
                    uint64_t v = ~0ull;
                    if (c < cend && c != s) v = pack_unless(q, ix.sp[c], 0xffffffffu);
                    const uint32_t r = (uint32_t)v;
                    if (in_reach(v, rb) && r < (uint32_t)P) {
                        int32_t sr;
                        const int32_t rr = uf_find<true>(parent, (int32_t)r, sr);
                        if (rr != rj) {  // else joined already: nothing to read or write
                            int32_t sq;
                            const int32_t rq = uf_find<true>(parent, rj, sq);  // one load while rj is still a root
                            uf_link(parent, rq, sq, rr, sr);
                        }
                    }
                }
            }
        }
    }
}

int components_within(const void* index, size_t index_bytes, long long P, void* scratch, size_t scratch_bytes, const float* r2,
                      int r2_is_per_row, int32_t* parent, void* stream)
{
    const std::string who = "nearest_components_within: ";
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_nearest_components_within", s)) return rc;
    if (!in_range(P)) return fail(HIDEGS_E_ARG, who + "P must be in [0, 2^31)");
    if (P == 0) return 0;
    if (!r2) return fail(HIDEGS_E_ARG, who + "NULL r2");
    if (!parent) return fail(HIDEGS_E_ARG, who + "NULL parent");
    if (!index || !aligned16(index) || index_bytes < index_layout(nullptr, P).total)
        return fail(HIDEGS_E_ARG, who + "index buffer NULL, not 16-byte aligned or too small for P");
    const Span inputs[3] = {{index, index_bytes, "the index"},
                            {r2, r2_is_per_row ? (size_t)P * 4 : 4, "r2"},
                            {scratch, scratch_bytes, "scratch"}};
    for (const Span& in : inputs)
        if (overlap(parent, (size_t)P * 4, in.p, in.n)) return fail(HIDEGS_E_ARG, who + "parent overlaps " + in.name);
    const IndexLayout il = index_layout(const_cast<void*>(index), P);
    const IndexView ix{il.frame, il.sp, il.leaves, il.supers, il.leaf_keys, P, il.nleaves, il.nsuper};
    if (r2_is_per_row)
        HIDEGS_LAUNCH("nearest_components", nearest_components_kernel<true>, hard_grid(P), dim3(kBlock), 0, s, ix, r2, parent);
    else
        HIDEGS_LAUNCH("nearest_components", nearest_components_kernel<false>, hard_grid(P), dim3(kBlock), 0, s, ix, r2, parent);
    return check_launch("nearest_components_within", s, 0);
}
