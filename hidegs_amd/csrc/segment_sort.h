// segment_sort.h -- the segmented stage's kernels: SegLds, sort_segment, open_local, segment_sort_kernel,
// and the queue's big_segment_kernel and piece_sort_kernel.
// Included by primitives.hip inside namespace hidegs::{anonymous}, after hot_queue.h.
#pragma once

union SegLds {
    SegShared lsd;
    BucketShared bucket;
    BigShared big;
    struct {
        BigShared big;
        EmitShared emit;
        uint32_t list[kBlock];  // segment_sort_kernel's scouts: the hot tiles of one sweep
        uint32_t nlist;
    } queue;
};

// big_segment_kernel's LDS: the queue forms, or one WIDE job's buffers (152 KB: one worker per CU)
union QueueLds {
    SegLds seg;
    WideShared wide;
};

// The steps of the bucket form (segment_forms.h) that sort_segment and segment_sort_kernel share.  Thread
// t's item q is pair t + q * kBlock of the segment; the register arrays are passed by reference.  Steps 3
// and 4 (fill and rank) are written out in both: as a shared helper they cost piece_sort_kernel a
// spilled VGPR (8 B/lane of scratch).

// The segment's pairs into registers, with the MIN / MAX of their low halves and hd, the OR of
// (high half ^ ref_hi): nonzero when any pair's high half differs from the first pair's.
// Packed: src_k holds {low key half, value} records (radix_scatter_kernel's Packed output) and every
// high half is ref_hi, the segment id; src_v is not read and hd is left alone.
template <bool Packed = false>
__device__ __forceinline__ void seg_load(const uint64_t* __restrict__ src_k, const uint32_t* __restrict__ src_v,
                                         const uint32_t begin, const uint32_t m, const uint32_t ref_hi,
                                         uint64_t (&k)[kSegItems], uint32_t (&v)[kSegItems], uint32_t& lo, uint32_t& hi,
                                         uint32_t& hd)
{
    const int t = threadIdx.x;
    uint2 rec[kSegItems];  // Packed: the records as loaded (not Packed: unused, k and v are loaded as they are)
    // First pass: the loads alone, all of a thread's items in flight together.
#pragma unroll
    for (int q = 0; q < kSegItems; q++) {
        const uint32_t i = t + q * kBlock;
        if (i < m) {
            if (Packed) {
                rec[q] = reinterpret_cast<const uint2*>(src_k)[begin + i];
            } else {
                k[q] = src_k[begin + i];
                v[q] = src_v[begin + i];
            }
        }
    }
    // Second pass: every use of a loaded value -- the Packed key and value formed from the record, MIN / MAX, hd.
    // In the load's own branch a use, even the move that forms a Packed key, puts a wait for item q's load in
    // front of item q + 1's: eight global round trips in a row where one is enough.  A thread without item q has
    // no later item either: the pass ends there, so rec[q] of an absent item, which was never written, is never
    // read, and a short segment's waves do not test eight masks a second time.
#pragma unroll
    for (int q = 0; q < kSegItems; q++) {
        if (t + q * kBlock >= m) break;
        if (Packed) {
            k[q] = ((uint64_t)ref_hi << 32) | rec[q].x;
            v[q] = rec[q].y;
        }
        const uint32_t x = (uint32_t)k[q];
        lo = min(lo, x);
        hi = max(hi, x);
        if (!Packed) hd |= (uint32_t)(k[q] >> 32) ^ ref_hi;
    }
}

// The pairs seg_load<true> expanded, written back where they were read (each thread its own elements).
template <StorePolicy P = kPlain>
__device__ __forceinline__ void store_loaded(const uint64_t (&k)[kSegItems], const uint32_t (&v)[kSegItems],
                                             const uint32_t begin, const uint32_t m, uint64_t* dk, uint32_t* dv)
{
#pragma unroll
    for (int q = 0; q < kSegItems; q++) {
        const uint32_t i = threadIdx.x + q * kBlock;
        if (i < m) {
            stream_store<P>(&dk[begin + i], k[q]);
            stream_store<P>(&dv[begin + i], v[q]);
        }
    }
}

// Steps 1 and 2: the bucket histogram (bucket = (x - base_lo) >> shift, over the segment's key range; sh.fill
// zeroed by the caller), the bucket starts into sh.start and sh.fill.  Returns the fullest bucket's
// count; mixed_hi: whether any thread's hd is nonzero (OneHi: no pair's is, by construction -- hd is
// not looked at).
template <bool OneHi = false>
__device__ __forceinline__ uint32_t bucket_starts(const uint64_t (&k)[kSegItems], const uint32_t m,
                                                  const uint32_t base_lo, const int shift, const uint32_t hd,
                                                  BucketShared& sh, uint32_t* s_and, uint32_t* s_max,
                                                  uint32_t& mixed_hi)
{
    const int t = threadIdx.x, lane = lane_id(), wave = t / kWave;
#pragma unroll
    for (int q = 0; q < kSegItems; q++)
        if (t + q * kBlock < m) atomicAdd(&sh.fill[((uint32_t)k[q] - base_lo) >> shift], 1u);
    __syncthreads();
    // exclusive scan, 4 buckets per thread
    uint32_t c[kBuckets / kBlock], sum = 0, mx = 0;
#pragma unroll
    for (int j = 0; j < kBuckets / kBlock; j++) {
        c[j] = sh.fill[t * (kBuckets / kBlock) + j];
        sum += c[j];
        mx = c[j] > mx ? c[j] : mx;
    }
    uint32_t dummy;
    uint32_t pre = block_exclusive_scan(sum, s_max, &dummy);  // its barriers order the reads above
    mx = wave_max_u32(mx);
    if (OneHi) {
        if (lane == 0) s_and[wave] = mx;
    } else {
        const bool wave_hd = __ballot(hd != 0u) != 0ull;
        if (lane == 0) s_and[wave] = mx | (wave_hd ? 0x80000000u : 0u);  // mx <= kSegCap: bit 31 is free
    }
#pragma unroll
    for (int j = 0; j < kBuckets / kBlock; j++) {
        sh.start[t * (kBuckets / kBlock) + j] = pre;
        sh.fill[t * (kBuckets / kBlock) + j] = pre;
        pre += c[j];
    }
    __syncthreads();
    uint32_t fullest = 0;
    mixed_hi = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; w++) {
        const uint32_t f = OneHi ? s_and[w] : s_and[w] & 0x7fffffffu;
        fullest = f > fullest ? f : fullest;
        if (!OneHi) mixed_hi |= s_and[w] >> 31;
    }
    return fullest;
}

// Step 5 stages (key, value) by final position in LDS, then stores the segment contiguously (stores
// straight from registers scatter 8- and 4-byte writes over the segment: 78 -> 50 us at 8M pairs).
// Both forms follow a barrier after the ranking: the staging reuses sh.
// Compact form, one high half (ref_hi) for the whole segment: {low half, value} records, 8 B per pair in
// one LDS write at its final position and one read, so a segment of up to kSegCap pairs goes through LDS
// in one pass; the keys are rebuilt on store.
template <StorePolicy P = kPlain>
__device__ __forceinline__ void stage_compact(const uint64_t (&k)[kSegItems], const uint32_t (&v)[kSegItems],
                                              const uint32_t (&pos)[kSegItems], const uint32_t begin,
                                              const uint32_t m, const uint32_t ref_hi, BucketShared& sh, uint64_t* dk,
                                              uint32_t* dv)
{
    const int t = threadIdx.x;
    uint2* stage = reinterpret_cast<uint2*>(&sh);
#pragma unroll
    for (int q = 0; q < kSegItems; q++)
        if (t + q * kBlock < m) stage[pos[q]] = make_uint2((uint32_t)k[q], v[q]);
    __syncthreads();
    const uint64_t khi = (uint64_t)ref_hi << 32;
#pragma unroll
    for (int q = 0; q < kSegItems; q++) {
        const uint32_t i = t + q * kBlock;
        if (i < m) {
            const uint2 rec = stage[i];
            stream_store<P>(&dk[begin + i], khi | rec.x);
            stream_store<P>(&dv[begin + i], rec.y);
        }
    }
}

// Whole keys: keys and values together for up to kSegRun pairs, else the keys, then the values.
template <StorePolicy P = kPlain>
__device__ __forceinline__ void stage_pairs(const uint64_t (&k)[kSegItems], const uint32_t (&v)[kSegItems],
                                            const uint32_t (&pos)[kSegItems], const uint32_t begin, const uint32_t m,
                                            BucketShared& sh, uint64_t* dk, uint32_t* dv)
{
    const int t = threadIdx.x;
    uint64_t* stage_k = reinterpret_cast<uint64_t*>(&sh);
    uint32_t* stage_v = reinterpret_cast<uint32_t*>(stage_k + kSegRun);
    const bool together = m <= (uint32_t)kSegRun;  // block-uniform
#pragma unroll
    for (int q = 0; q < kSegItems; q++) {
        if (t + q * kBlock < m) {
            stage_k[pos[q]] = k[q];
            if (together) stage_v[pos[q]] = v[q];
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kSegItems; q++) {
        const uint32_t i = t + q * kBlock;
        if (i < m) {
            stream_store<P>(&dk[begin + i], stage_k[i]);
            if (together) stream_store<P>(&dv[begin + i], stage_v[i]);
        }
    }
    if (together) return;
    __syncthreads();
    stage_v = reinterpret_cast<uint32_t*>(&sh);
#pragma unroll
    for (int q = 0; q < kSegItems; q++)
        if (t + q * kBlock < m) stage_v[pos[q]] = v[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kSegItems; q++) {
        const uint32_t i = t + q * kBlock;
        if (i < m) stream_store<P>(&dv[begin + i], stage_v[i]);
    }
}

// One segment of m <= kSegCap pairs sorted by the low 32 key bits: the bucket form, or its LSD
// fallback for crowded buckets (segment_sort_kernel runs the same steps).  InPlace: (src_k, src_v) ==
// (dst_k, dst_v); otherwise the pairs are read from alt and written to keys (a piece of a partitioned
// hot tile).
template <bool InPlace>
__device__ __forceinline__ void sort_segment(const uint64_t* __restrict__ src_k, const uint32_t* __restrict__ src_v,
                                             uint64_t* __restrict__ dst_k, uint32_t* __restrict__ dst_v,
                                             const uint32_t begin, const uint32_t m, SegLds& lds, uint32_t* s_and,
                                             uint32_t* s_or, uint32_t* s_max)
{
    uint64_t* dk = InPlace ? const_cast<uint64_t*>(src_k) : dst_k;
    uint32_t* dv = InPlace ? const_cast<uint32_t*>(src_v) : dst_v;
    const int t = threadIdx.x;
    uint64_t k[kSegItems];
    uint32_t v[kSegItems];
    uint32_t lo = 0xffffffffu, hi = 0;
    const uint32_t ref_hi = m ? (uint32_t)(src_k[begin] >> 32) : 0u;  // see segment_sort_kernel (m == 0: no read)
    uint32_t hd = 0;
    seg_load(src_k, src_v, begin, m, ref_hi, k, v, lo, hi, hd);
    BucketShared& sh = lds.bucket;
    for (int i = t; i < kBuckets; i += kBlock) sh.fill[i] = 0u;
    const SegRange st = segment_range(lo, hi, s_and, s_or);
    if (st.lo == st.hi) {  // equal low keys: the input order is the stable order
        if (!InPlace) {
#pragma unroll
            for (int q = 0; q < kSegItems; q++) {
                const uint32_t i = t + q * kBlock;
                if (i < m) {
                    dk[begin + i] = k[q];
                    dv[begin + i] = v[q];
                }
            }
        }
        return;
    }
    const int shift = st.shift;
    uint32_t mixed_hi;
    const uint32_t fullest = bucket_starts(k, m, st.lo, shift, hd, sh, s_and, s_max, mixed_hi);
    if (fullest > (uint32_t)kMaxBucket || shift + kIndexBits > 32) {  // crowded depths, or fields too
        // wide for 32 bits: the LSD form (block-uniform branch)
        const uint32_t diff = segment_diff(k, m, s_max, s_or);  // (s_and is still being read; these two are free)
        segment_sort_lsd<InPlace>(src_k, src_v, dst_k, dst_v, begin, m, diff, lds.lsd);
        return;
    }
    const uint32_t base_lo = st.lo;
    const uint32_t lowmask = (uint32_t)((1ull << shift) - 1ull);
    // 3. fill the buckets in any order
    uint32_t me[kSegItems];
    uint32_t bucket[kSegItems];
#pragma unroll
    for (int q = 0; q < kSegItems; q++) {
        const uint32_t i = t + q * kBlock;
        if (i < m) {
            const uint32_t x = (uint32_t)k[q] - base_lo;
            bucket[q] = x >> shift;
            me[q] = ((x & lowmask) << kIndexBits) | i;
            sh.comb[atomicAdd(&sh.fill[bucket[q]], 1u)] = me[q];
        }
    }
    __syncthreads();
    // 4. exact rank inside the bucket
    uint32_t pos[kSegItems];
#pragma unroll
    for (int q = 0; q < kSegItems; q++) {
        if (t + q * kBlock < m) {
            const uint32_t s0 = sh.start[bucket[q]], e0 = sh.fill[bucket[q]];
            uint32_t rank = 0;
            for (uint32_t j = s0; j < e0; j++) rank += sh.comb[j] < me[q] ? 1u : 0u;
            pos[q] = s0 + rank;
        }
    }
    __syncthreads();
    if (!mixed_hi) {
        stage_compact(k, v, pos, begin, m, ref_hi, sh, dk, dv);
        return;
    }
    stage_pairs(k, v, pos, begin, m, sh, dk, dv);
}

// A record's first two phases (REDUCE, HIST) run by the workgroup that opens it, inside
// segment_sort_kernel where the other segments' sorts hide them, for a tile of up to kOpenLocal
// pairs: the queue then starts at the SCATTER jobs.
// (The SCATTER phase too in the opener measured slower: DESIGN.md, range digits.)
constexpr int kOpenLocal = 24576;
static_assert(kOpenLocal <= (int)kGroupChunks * kChunk, "open_local plans an ungrouped record (pending == chunks)");
constexpr int kScouts = HIDEGS_SCOUTS;  // the knob is primitives.hip's
constexpr int kScoutItems = 32;  // segments per scout thread per sweep (a sweep: 8192 segments)
// a scout's share of one sweep's hot tiles fits its kBlock-entry list
static_assert(kScouts == 0 || kBlock * kScoutItems <= kScouts * kBlock, "HIDEGS_SCOUTS: at least 32 scouts (or 0)");
__device__ __forceinline__ void open_local(const uint64_t* keys, const BigQueue& q, const uint32_t begin,
                                           const uint32_t m, BigShared& sh, EmitShared& e, uint32_t* s_and,
                                           uint32_t* s_or)
{
    const int t = threadIdx.x, lane = lane_id(), wave = t / kWave;
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (uint32_t i0 = 0; i0 < m; i0 += kChunk) {
        uint32_t x[kChunk / kBlock];
#pragma unroll
        for (int u = 0; u < kChunk / kBlock; u++) {
            const uint32_t i = i0 + u * kBlock + t;
            x[u] = key_low(keys, begin + (i < m ? i : 0u));  // a repeat changes no MIN / MAX
        }
#pragma unroll
        for (int u = 0; u < kChunk / kBlock; u++) {
            lo = min(lo, x[u]);
            hi = max(hi, x[u]);
        }
    }
    wave_min_max(lo, hi);
    if (lane == 0) {
        s_and[wave] = lo;
        s_or[wave] = hi;
    }
    __syncthreads();
    for (int w = 0; w < kWavesPerBlock; w++) {
        lo = min(lo, s_and[w]);
        hi = max(hi, s_or[w]);
    }
    if (lo == hi) return;  // equal low keys: in stable order already (block-uniform)
    if (t == 0) {
        runs_begin(e);
        const uint4 r = record_run<false>(q, begin, m, 0u, true, lo, hi);
        e.run[0] = r;
        e.base = (r.x & 0xffu) == J_HIST ? q.rec[r.y].pool : ~0u;
        if (e.base == ~0u) add_run(e, r);  // the table or pool is full: a GLOBAL job
    }
    __syncthreads();
    const uint32_t pool = e.base, rec = e.run[0].y, chunks = (m + kChunk - 1) / kChunk;
    if (pool != ~0u) {
        int shift, bits;
        range_digit(lo, hi, shift, bits);  // the record's digit (set_digit)
        const uint32_t mask = (1u << bits) - 1u;
        uint32_t* col = q.pool + pool + t;
        for (uint32_t c = 0; c < chunks; c++) {
            const uint32_t c0 = c * kChunk;
            col[c * kRadix] = chunk_hist(keys, begin + c0, m - c0 < (uint32_t)kChunk ? m - c0 : (uint32_t)kChunk,
                                         lo, shift, mask, sh);
        }
        __syncthreads();
        plan_scatter<false>(col, chunks, begin, sh);
        if (t == 0) {
            runs_begin(e);
            add_run(e, J_SCATTER, 0u, rec, 0u, chunks);  // pending == chunks already
        }
    }
    emit_jobs(q, e);
}

// A segment of packed records (radix_scatter_kernel's Packed output) rewritten in place as whole pairs:
// keys[i] = seg << 32 | low half, vals[i] = value.  Each thread rewrites the elements it read itself,
// kExpandItems loads in flight.  The low halves keep their values and places, so whoever reads only
// those meanwhile (a scout's open_local) sees no change.
constexpr int kExpandItems = 8;
template <StorePolicy P = kPlain>
__device__ __forceinline__ void expand_records(uint64_t* keys, uint32_t* vals, const uint32_t begin, const uint32_t m,
                                               const uint32_t seg)
{
    const uint2* recs = reinterpret_cast<const uint2*>(keys);
    const uint64_t khi = (uint64_t)seg << 32;
    for (uint32_t i0 = 0; i0 < m; i0 += kExpandItems * kBlock) {
        uint2 rec[kExpandItems];
#pragma unroll
        for (int u = 0; u < kExpandItems; u++) {
            const uint32_t i = i0 + u * kBlock + threadIdx.x;
            rec[u] = i < m ? recs[begin + i] : make_uint2(0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < kExpandItems; u++) {
            const uint32_t i = i0 + u * kBlock + threadIdx.x;
            if (i < m) {
                stream_store<P>(&keys[begin + i], khi | rec[u].x);
                stream_store<P>(&vals[begin + i], rec[u].y);
            }
        }
    }
}

// Workgroup b sorts segment b in place by the low 32 key bits (sort_segment); a segment of more
// than kSegCap pairs becomes a record of the partition queue (big_segment_kernel runs it).
// Packed: `keys` arrives as packed records and segment b's high key half is b.  Every way out leaves
// whole keys and values behind; a segment that this kernel does not sort itself is expanded in place
// by its own workgroup first, so the queue's kernels and the one-workgroup forms see ordinary pairs.
// Out: the policy of the stores that leave a sorted (or expanded) segment behind for the caller -- stage_compact,
// stage_pairs, expand_records, store_loaded.  They are contiguous runs that this kernel does not read again (but for
// store_loaded's, which the same workgroup's LSD form reads behind a barrier); written
// through (kThrough), a workgroup's lines leave the L2 while the others still sort instead of all at the kernel's end:
// segment_sort 40.4 -> 38.6 us at the 1080p view, the step -1.9 us.  Only up to kThroughMaxN pairs: the 4K frame's
// 42.9M pairs, whose output no longer fits the 256 MB MALL, went 0.699 -> 0.719 ms per step (kStream: +0.5 us at
// 1080p; profiles/r13_store_policy.md).  ranges_out, the queue's hand-offs (a hot tile's expansion, emit_jobs,
// record_run, the pool) and sort_segment, which piece_sort_kernel shares, keep plain stores.
constexpr long long kThroughMaxN = kNarrowMaxN;
template <bool Packed, StorePolicy Out = kPlain>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(Packed ? kSegWavesPacked : kSegWaves)))
void segment_sort_kernel(uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, const uint32_t* __restrict__ starts,
                         uint2* __restrict__ ranges_out, const int nseg, const BigQueue q)
{
    __shared__ __attribute__((aligned(16))) SegLds lds;
    __shared__ uint32_t s_and[kWavesPerBlock], s_or[kWavesPerBlock], s_max[kWavesPerBlock];
    if (kScouts > 0 && blockIdx.x < (unsigned)kScouts) {
        // a scout: the first workgroups dispatched find the hot tiles (over kQueueMin pairs) and start
        // them -- the local phases of open_local, or a queue record -- while the other workgroups sort
        // the ordinary tiles, instead of wherever in the grid the hot tile's own workgroup would run.
        // Every scout sweeps all segments and numbers the hot ones the same way (thread-major within a
        // sweep); scout b takes the hot tiles numbered b mod kScouts, so the hot tiles of one image
        // region -- neighbouring segment ids -- are opened side by side, not by one scout in turn
        // (71 hot tiles of a skewed view: 1.13 ms of segment_sort with 16 scouts of 256-segment stripes)
        uint32_t* list = lds.queue.list;
        uint32_t carry = 0u;  // hot tiles numbered in earlier sweeps
        for (uint32_t s0 = 0; s0 < (uint32_t)nseg; s0 += kBlock * kScoutItems) {
            if (threadIdx.x == 0) lds.queue.nlist = 0u;
            uint32_t hot = 0u;  // bit u: segment s0 + u * kBlock + threadIdx.x is hot
#pragma unroll 8
            for (int u = 0; u < kScoutItems; u++) {
                const uint32_t sg = s0 + (uint32_t)u * kBlock + threadIdx.x;
                if (sg < (uint32_t)nseg && starts[sg + 1] - starts[sg] > (uint32_t)kQueueMin) hot |= 1u << u;
            }
            uint32_t nhot;
            const uint32_t base = carry + block_exclusive_scan((uint32_t)__builtin_popcount(hot), s_max, &nhot);
            carry += nhot;  // block-uniform
            if (nhot == 0u) continue;
            uint32_t ord = base;
            for (uint32_t h = hot; h; h &= h - 1u, ord++)
                if (ord % (uint32_t)kScouts == blockIdx.x)
                    list[atomicAdd(&lds.queue.nlist, 1u)] = s0 + (uint32_t)__builtin_ctz(h) * kBlock + threadIdx.x;
            __syncthreads();
            const uint32_t nl = lds.queue.nlist;  // workgroup-uniform
            for (uint32_t j = 0; j < nl; j++) {
                const uint32_t sg2 = list[j], b = starts[sg2], mm = starts[sg2 + 1] - b;
                if (HIDEGS_WIDE_SCOUTS && mm <= (uint32_t)kWideCap) {  // one WIDE job (a queue worker sorts it in LDS)
                    if (threadIdx.x == 0) {
                        runs_begin(lds.queue.emit);
                        add_run(lds.queue.emit, J_WIDE, 0u, b, mm, 1u);
                    }
                    emit_jobs(q, lds.queue.emit);
                } else if (mm <= (uint32_t)kOpenLocal) {
                    open_local(keys, q, b, mm, lds.queue.big, lds.queue.emit, s_and, s_or);
                } else {
                    if (threadIdx.x == 0) {
                        runs_begin(lds.queue.emit);
                        add_run(lds.queue.emit, record_run(q, b, mm, 0u, false, 0u, 0u));
                    }
                    emit_jobs(q, lds.queue.emit);
                }
                __syncthreads();  // the LDS is reused by the next one
            }
        }
        return;
    }
    const uint32_t seg = blockIdx.x - kScouts;
    // segment seg is [starts[seg], starts[seg + 1]); with ranges_out it is also tile seg's range,
    // (0, 0) when empty -- identifyTileRanges' result
    const uint2 r = make_uint2(starts[seg], starts[seg + 1]);
    if (ranges_out && threadIdx.x == 0) ranges_out[seg] = r.y > r.x ? r : make_uint2(0u, 0u);
    const uint32_t begin = r.x, m = r.y - r.x;
    if (r.y <= r.x + 1) {  // absent or single pair: already in place
        if (Packed && r.y == r.x + 1) expand_records<Out>(keys, vals, begin, 1u, seg);
        return;
    }
    if (m > (uint32_t)kSegCap) {
        if (Packed) {
            // (a scout may be reading the segment's low key halves meanwhile: they do not change)
            expand_records(keys, vals, begin, m, seg);
            if (m <= (uint32_t)kQueueMin || kScouts == 0) __syncthreads();  // this workgroup reads the pairs next
        }
        if (m <= (uint32_t)kQueueMin) {  // mildly hot: this workgroup, overlapped with the others
            segment_sort_global(keys, vals, q.alt_k, q.alt_v, begin, m, lds.big);
            return;
        }
        if (kScouts > 0) return;  // hot: a scout has it
        if (m <= (uint32_t)kOpenLocal) {
            open_local(keys, q, begin, m, lds.queue.big, lds.queue.emit, s_and, s_or);
            return;
        }
        if (threadIdx.x == 0) {
            runs_begin(lds.queue.emit);
            add_run(lds.queue.emit, record_run(q, begin, m, 0u, false, 0u, 0u));
        }
        emit_jobs(q, lds.queue.emit);
        return;
    }
    // sort_segment<true>'s body, written out.  Shared with it (the helpers above): the load, the bucket
    // histogram / start scan / fullest reduction, and both stage stores.  Not shared: this frame and the
    // fill and rank (steps 3, 4).  As one inlined sort_segment<true> call the kernel needs 228 B/lane of
    // scratch at the 72-VGPR budget of kSegWaves (the register allocator sees it differently).
    const int t = threadIdx.x;
    uint64_t k[kSegItems];
    uint32_t v[kSegItems];
    uint32_t lo = 0xffffffffu, hi = 0;
    // the segment's first high key half: the segment id (tile), and with no bits above end_bit -- as
    // hidegs_sort_tile_pairs' callers guarantee -- every pair's high half; `hd` records any that differs
    // (Packed: the segment id itself, with no load to wait for, and nothing to record)
    const uint32_t ref_hi = Packed ? seg : (uint32_t)(keys[begin] >> 32);
    uint32_t hd = 0;
    seg_load<Packed>(keys, vals, begin, m, ref_hi, k, v, lo, hi, hd);
    BucketShared& sh = lds.bucket;
    for (int i = t; i < kBuckets; i += kBlock) sh.fill[i] = 0u;
    const SegRange st = segment_range(lo, hi, s_and, s_or);
    if (st.lo == st.hi) {  // equal low keys: the input order is the stable order
        // (read again, not stored from k and v: keeping those live to here costs scratch)
        if (Packed) expand_records<Out>(keys, vals, begin, m, seg);
        return;
    }
    const int shift = st.shift;
    uint32_t mixed_hi;
    const uint32_t fullest = bucket_starts<Packed>(k, m, st.lo, shift, hd, sh, s_and, s_max, mixed_hi);
    if (fullest > (uint32_t)kMaxBucket || shift + kIndexBits > 32) {  // crowded depths, or fields too
        // wide for 32 bits: the LSD form (block-uniform branch), which reads whole pairs
        if (Packed) store_loaded<Out>(k, v, begin, m, keys, vals);
        // the bits that vary, from the registers; its barrier also publishes the pairs just stored
        // (s_and is still being read; s_max and s_or are free)
        const uint32_t diff = segment_diff(k, m, s_max, s_or);
        segment_sort_lsd<true>(keys, vals, nullptr, nullptr, begin, m, diff, lds.lsd);
        return;
    }
    const uint32_t base_lo = st.lo;
    const uint32_t lowmask = (uint32_t)((1ull << shift) - 1ull);
    // 3. fill the buckets in any order
#pragma unroll
    for (int q = 0; q < kSegItems; q++) {
        const uint32_t i = t + q * kBlock;
        if (i < m) {
            const uint32_t x = (uint32_t)k[q] - base_lo;
            sh.comb[atomicAdd(&sh.fill[x >> shift], 1u)] = ((x & lowmask) << kIndexBits) | i;
        }
    }
    __syncthreads();
    // 4. exact rank inside the bucket.  The bucket and the (low bits, index) word are worked out again
    // from the low key half (three VALU instructions) and not held over the barrier: 16 VGPRs, which
    // the 8-waves-per-SIMD budget of the Packed instance does not have.  The empty asm keeps the
    // compiler from reusing the fill step's values.
    uint32_t pos[kSegItems];
#pragma unroll
    for (int q = 0; q < kSegItems; q++) {
        const uint32_t i = t + q * kBlock;
        if (i < m) {
            uint32_t x = (uint32_t)k[q];
            asm volatile("" : "+v"(x));
            x -= base_lo;
            const uint32_t b = x >> shift, me = ((x & lowmask) << kIndexBits) | i;
            const uint32_t s0 = sh.start[b], e0 = sh.fill[b];
            uint32_t rank = 0;
            for (uint32_t j = s0; j < e0; j++) rank += sh.comb[j] < me ? 1u : 0u;
            pos[q] = s0 + rank;
        }
    }
    __syncthreads();
    if (Packed || !mixed_hi) {  // (Packed: one high half by construction)
        stage_compact<Out>(k, v, pos, begin, m, ref_hi, sh, keys, vals);
        return;
    }
    stage_pairs<Out>(k, v, pos, begin, m, sh, keys, vals);
}

// The last workgroup to count `pending` down (a record's phase, or a chunk group of its HIST phase)
// goes on (returns true); the others return false.  The caller's global writes are published before
// the count-down.
__device__ __forceinline__ bool finish_phase(uint32_t& pending, uint32_t* s_flag)
{
    wave_stores_done();
    __syncthreads();
    if (threadIdx.x == 0) {
        release_lane();
        const bool last = __hip_atomic_fetch_add(&pending, 0xffffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1u;
        if (last) acquire_lane();
        *s_flag = last;
    }
    __syncthreads();
    return *s_flag != 0;
}

// The partition queue's workers: kQueueBlocks workgroups take jobs until none is left or in
// flight.  With no hot tile (the common case) every workgroup reads one counter and exits.
__global__ __launch_bounds__(kBlock) void big_segment_kernel(uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                             uint64_t* __restrict__ alt_k,
                                                             uint32_t* __restrict__ alt_v, const BigQueue q)
{
    __shared__ __attribute__((aligned(16))) QueueLds qlds;
    __shared__ uint32_t s_and[kWavesPerBlock], s_or[kWavesPerBlock], s_max[kWavesPerBlock];
    __shared__ uint4 s_job;
    __shared__ uint32_t s_flag;
    SegLds& lds = qlds.seg;
    const int t = threadIdx.x, lane = lane_id(), wave = t / kWave;
    BigShared& sh = lds.queue.big;
    EmitShared& e = lds.queue.emit;
    if (t == 0) s_flag = q_peek(&q.ctl[kCtlStride * Q_RESERVE]);
    __syncthreads();
    if (s_flag == 0) return;  // nothing was queued (the queue was filled by the previous launch)
#ifdef HIDEGS_QUEUE_TRACE
    unsigned long long t_claim = 0, t_got = 0;
    uint32_t t_index = 0;
#endif
    for (;;) {
        __syncthreads();  // the previous job's LDS use is over
        if (t == 0) {
            // the claim only hands out a slot index: relaxed (an acq_rel RMW here is an L2 writeback
            // and invalidate per job; the job's data is acquired after its tag is seen)
            const uint32_t i = __hip_atomic_fetch_add(&q.ctl[kCtlStride * Q_HEAD], 1u, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
#ifdef HIDEGS_QUEUE_TRACE
            t_claim = wall_clock64();
            t_index = i;
#endif
            uint4 job = make_uint4(J_EXIT, 0u, 0u, 0u);
            uint32_t polls = 0, backoff = 1;
            bool reserved = false;  // slot i is reserved: a job will be published there (reserve only grows)
            for (; polls < kMaxPolls; polls++) {
                if (i < q.job_cap && q_peek(&q.job[i].w) != 0u) {
                    acquire_lane();  // for the whole workgroup (see wave_stores_done)
                    job = q.job[i];
                    break;
                }
                // the shared counters are polled only while slot i is not reserved (reading `done` on
                // one poll in 4 only, or backing off to 64 sleeps, measured slower: DESIGN.md)
                if (!reserved) {
                    const uint32_t r0 = q_peek(&q.ctl[kCtlStride * Q_RESERVE]);
                    reserved = i < r0 && i < q.job_cap;
                    if (!reserved && q_peek(&q.ctl[kCtlStride * Q_DONE]) == r0) {
                        // confirm in order: `done` (acquire) before `reserve`
                        const uint32_t d = q_load(&q.ctl[kCtlStride * Q_DONE]);
                        const uint32_t r = q_load(&q.ctl[kCtlStride * Q_RESERVE]);
                        if (d == r && i >= r) break;  // nothing queued, nothing in flight: the end
                    }
                }
                for (uint32_t k = 0; k < backoff; k++) __builtin_amdgcn_s_sleep(8);  // ~0.2 us each
                backoff = backoff < kBackoffMax ? 2u * backoff : kBackoffMax;
            }
            if (polls == kMaxPolls) q_flag(q, 4u);
            s_job = job;
#ifdef HIDEGS_QUEUE_TRACE
            t_got = wall_clock64();
#endif
        }
        __syncthreads();
        const uint4 job = s_job;
        const uint32_t type = job.x & 0xffu, src = job.x >> 8;
        if (type == J_EXIT) return;

        if (type == J_WIDE) {
            wide_sort(keys, vals, alt_k, alt_v, job.y, job.z, src, qlds.wide);
        } else if (type == J_SMALL) {
            if (src)
                sort_segment<false>(alt_k, alt_v, keys, vals, job.y, job.z, lds, s_and, s_or, s_max);
            else
                sort_segment<true>(keys, vals, nullptr, nullptr, job.y, job.z, lds, s_and, s_or, s_max);
        } else if (type == J_COPY) {
            for (uint32_t i = t; i < job.z; i += kBlock) {
                keys[job.y + i] = alt_k[job.y + i];
                vals[job.y + i] = alt_v[job.y + i];
            }
        } else if (type == J_GLOBAL) {
            if (src) {
                for (uint32_t i = t; i < job.z; i += kBlock) {
                    keys[job.y + i] = alt_k[job.y + i];
                    vals[job.y + i] = alt_v[job.y + i];
                }
                __syncthreads();
            }
            segment_sort_global(keys, vals, alt_k, alt_v, job.y, job.z, sh);
        } else {  // a chunk job of record job.y
            BigSeg& s = q.rec[job.y];
            const uint32_t c = job.z, begin = s.begin, m = s.m, chunks = s.chunks, csize = s.csize;
            const uint32_t c0 = c * csize, cnt = m - c0 < csize ? m - c0 : csize;
            const uint64_t* sk = s.src ? alt_k : keys;
            uint32_t* col = q.pool + s.pool + t;  // this thread's digit column
            if (type == J_REDUCE) {
                uint32_t lo = 0xffffffffu, hi = 0u;
                for (uint32_t i0 = 0; i0 < cnt; i0 += kQueueIlp * kChunk) {
                    uint32_t x[kQueueIlp * kChunk / kBlock];
#pragma unroll
                    for (int u = 0; u < kQueueIlp * kChunk / kBlock; u++) {
                        const uint32_t i = i0 + t + u * kBlock;
                        x[u] = i < cnt ? (uint32_t)sk[begin + c0 + i] : 0xffffffffu;
                    }
#pragma unroll
                    for (int u = 0; u < kQueueIlp * kChunk / kBlock; u++) {
                        const uint32_t i = i0 + t + u * kBlock;
                        lo = min(lo, x[u]);
                        hi = i < cnt ? max(hi, x[u]) : hi;
                    }
                }
                wave_min_max(lo, hi);
                if (lane == 0) {
                    s_and[wave] = lo;
                    s_or[wave] = hi;
                }
                __syncthreads();
                if (t == 0) {
                    for (int w = 0; w < kWavesPerBlock; w++) {
                        lo = min(lo, s_and[w]);
                        hi = max(hi, s_or[w]);
                    }
                    __hip_atomic_fetch_min(&s.lo_bits, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_max(&s.hi_bits, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (finish_phase(s.pending, &s_flag)) {
                    if (t == 0) {
                        runs_begin(e);
                        const uint32_t rlo = q_load(&s.lo_bits), rhi = q_load(&s.hi_bits);
                        if (rlo == rhi) {  // equal low keys: already in stable order
                            if (s.src) add_run(e, J_COPY, 1u, begin, m, (m + kChunk - 1) / kChunk);
                        } else {
                            set_digit(s, rlo, rhi);
                            s.pending = hist_countdown(q, s);
                            add_run(e, J_HIST, 0u, job.y, 0u, chunks);
                        }
                    }
                    emit_jobs(q, e);
                }
            } else if (type == J_HIST) {
                const int shift = (int)s.shift;
                const uint32_t mask = (1u << s.bits) - 1u;
                col[c * kRadix] = chunk_hist<kQueueIlp>(sk, begin + c0, cnt, s.lo, shift, mask, sh);
                const uint32_t ng = num_groups(chunks);
                bool last;
                if (ng) {  // the group's countdown first; its last chunk scans the group's rows
                    const uint32_t G = group_chunks(chunks), g = c / G, g0 = g * G;
                    last = finish_phase(q.pool[s.pool + (chunks + 4 + ng) * kRadix + g], &s_flag);
                    if (last) {
                        col[(chunks + 4 + g) * kRadix] = scan_column(col, g0, chunks - g0 < G ? chunks - g0 : G, 0u);
                        last = finish_phase(s.pending, &s_flag);
                    }
                } else {
                    last = finish_phase(s.pending, &s_flag);
                }
                if (last) {
                    plan_scatter(col, chunks, begin, sh);
                    if (t == 0) {
                        s.pending = chunks;
                        runs_begin(e);
                        add_run(e, J_SCATTER, 0u, job.y, 0u, chunks);
                    }
                    emit_jobs(q, e);
                }
            } else {  // J_SCATTER
                const int shift = (int)s.shift;
                const uint32_t mask = (1u << s.bits) - 1u;
                const uint32_t dst = s.src ^ 1u;
                const uint32_t* sv = s.src ? alt_v : vals;
                uint64_t* dk = dst ? alt_k : keys;
                uint32_t* dv = dst ? alt_v : vals;
                const uint32_t ng = num_groups(chunks);  // grouped: + the group's base
                sh.run[t] = col[c * kRadix] + (ng ? col[(chunks + 4 + c / group_chunks(chunks)) * kRadix] : 0u);
                sh.aux[0][t] = 0xffffffffu;
                sh.aux[1][t] = 0u;
                scatter_steps<true>(sk, sv, dk, dv, begin + c0, cnt, s.lo, shift, mask, begin, begin + m, sh);
                // this chunk's per-digit MIN / MAX into the record's (digits it holds only)
                if (sh.aux[0][t] != 0xffffffffu || sh.aux[1][t] != 0u) {
                    __hip_atomic_fetch_min(&col[(chunks + 2) * kRadix], sh.aux[0][t], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_max(&col[(chunks + 3) * kRadix], sh.aux[1][t], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                }
                if (finish_phase(s.pending, &s_flag)) {
                    cut_pieces(q, e, sh, col, chunks, begin, m, shift, dst);
                    emit_jobs(q, e);
                }
            }
        }
        // `done` only ends the queue (no data hangs on it): the jobs this one queued are
        // published already, and the pairs it wrote are for kernel completion or a publish
        __syncthreads();
        if (t == 0) __hip_atomic_fetch_add(&q.ctl[kCtlStride * Q_DONE], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifdef HIDEGS_QUEUE_TRACE
        if (t == 0) {
            const unsigned int slot = atomicAdd(&g_qtrace_n, 1u);
            if (slot < kQTraceCap) {
                const uint32_t last = (type == J_REDUCE || type == J_HIST || type == J_SCATTER) && s_flag ? 0x80u : 0u;
                g_qtrace[slot][0] = (unsigned long long)(type | last | (blockIdx.x << 8)) | ((unsigned long long)t_index << 32);
                g_qtrace[slot][1] = t_claim;
                g_qtrace[slot][2] = t_got;
                g_qtrace[slot][3] = wall_clock64();
            }
        }
#endif
    }
}

// The queue's pieces (<= kSegCap pairs each, cut from partitioned hot tiles), sorted after the queue
// has drained, at segment_sort_kernel's occupancy instead of one queue worker per CU: 7888 pieces of
// a one-tile view took the queue ~250 us as SMALL jobs.  With no hot tile the list is empty and
// every workgroup reads one counter and exits.
constexpr int kPieceBlocks = 256 * kPieceWaves;  // one workgroup per resident slot
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kPieceWaves))) void piece_sort_kernel(
    uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, const uint64_t* __restrict__ alt_k,
    const uint32_t* __restrict__ alt_v, const BigQueue q, uint32_t* async_err)
{
    __shared__ __attribute__((aligned(16))) SegLds lds;
    __shared__ uint32_t s_and[kWavesPerBlock], s_or[kWavesPerBlock], s_max[kWavesPerBlock];
    // the queue has drained (stream order): its error word is final.  A set word is ORed into the
    // stream's mapped host word (vector load and store at system scope), which an entry-point call on
    // this stream takes as HIDEGS_E_ASYNC.  Not an atomic OR (system-scope atomics on host memory are
    // not relied on): earlier sorts on the stream have finished, so only the host's take can fall
    // between the load and the store, and then those bits are reported twice -- never lost.
    if (async_err && blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t err = q_peek(&q.ctl[kCtlStride * Q_ERROR]);
        if (err) {
            const uint32_t old = __hip_atomic_load(async_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(async_err, old | err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    const uint32_t np = min(q.ctl[kCtlStride * Q_NPIECE], q.piece_cap);
    for (uint32_t p = blockIdx.x; p < np; p += gridDim.x) {
        const uint2 e = q.piece[p];
        const uint32_t m = e.y & 0x7fffffffu;
        if (e.y >> 31)
            sort_segment<false>(alt_k, alt_v, keys, vals, e.x, m, lds, s_and, s_or, s_max);
        else
            sort_segment<true>(keys, vals, nullptr, nullptr, e.x, m, lds, s_and, s_or, s_max);
        __syncthreads();  // the LDS is reused by the next piece
    }
}
