// segment_forms.h -- the sorts of one segment by its low 32 key bits: SegShared and lds_radix_sort, the
// BigShared step helpers, segment_sort_global, segment_sort_lsd, SegStats and BucketShared.
// Included by primitives.hip inside namespace hidegs::{anonymous}, after radix.h.
#pragma once

// ============================== segmented sort =================================
//
// Keys whose bits [32, end_bit) are a small segment id -- the (tile | depth) keys of the
// binning stage -- are sorted in two stages with the same result as the LSD sort over
// [0, end_bit): (1) the LSD passes above over [32, end_bit) only, which partition the pairs
// stably by segment; (2) one workgroup per segment sorts it stably by the low 32 bits.
// Global traffic drops from 6 LSD passes to 2 plus one read/write of every pair.
//
// Stage (2) has three forms, chosen per segment (block-uniform):
//   bucket form  (<= kSegCap pairs, the common case): bucket by the top 10 varying low-key bits,
//                exact rank inside each bucket, LDS-staged in-place stores -- see segment_sort_kernel;
//   LSD form     (a bucket over kMaxBucket pairs: crowded depths): 8-bit LDS LSD passes over the
//                varying bits, two runs of <= kSegRun merged by rank;
//   global form  (> kSegCap pairs: a hot tile): 4 LSD passes through global memory.
constexpr int kSegRun = 1024;            // pairs per LDS-sorted run
constexpr int kSegCap = 2 * kSegRun;     // largest segment sorted by segment_sort_kernel
constexpr int kRunItems = kSegRun / kBlock;  // run items per thread (rounds of 64 per wave)
constexpr int kSegItems = kSegCap / kBlock;  // segment items per thread

// LDS of one workgroup: two (low key, index-in-segment) buffers of one run plus ranking state.
struct SegShared {
    uint32_t k[2][kSegRun];
    uint16_t i[2][kSegRun];  // index in segment (< kSegCap)
    uint32_t cnt[kWavesPerBlock][kRadix];
    uint32_t start[kRadix];
    uint32_t wave[kWavesPerBlock];
};

// Stable LSD sort of the n <= kSegRun (k, i) pairs in buffer 0 by the key bits set in `diff`
// (8-bit digits; a digit that is constant over the segment is skipped).  Returns the buffer
// holding the result.  Wave w ranks items [w*C, w*C + C) in (round, lane) order.
__device__ __forceinline__ int lds_radix_sort(SegShared& sh, const uint32_t n, const uint32_t diff)
{
    const int t = threadIdx.x, lane = lane_id(), wave = t / kWave;
    const uint32_t C = ((n + kBlock - 1) / kBlock) * kWave;
    const int rounds = (int)(C / kWave);
    const uint32_t w0 = wave * C;
    int cur = 0;
    for (int shift = 0; shift < 32; shift += kRadixBits) {
        const uint32_t vary = (diff >> shift) & (kRadix - 1);
        if (vary == 0) continue;  // digit constant over the segment (block-uniform)
        for (int i = t; i < kWavesPerBlock * kRadix; i += kBlock) (&sh.cnt[0][0])[i] = 0;
        __syncthreads();
        uint32_t k[kRunItems], id[kRunItems], rank[kRunItems];
        bool ok[kRunItems];
#pragma unroll
        for (int q = 0; q < kRunItems; q++) {
            const uint32_t i = w0 + q * kWave + lane;
            ok[q] = q < rounds && i < n;
            k[q] = ok[q] ? sh.k[cur][i] : 0u;
            id[q] = ok[q] ? sh.i[cur][i] : 0u;
        }
        if (rounds == kRunItems) {
            wave_rank<uint32_t, kRunItems>(k, ok, shift, kRadix - 1, sh.cnt[wave], rank, vary);
        } else {  // rounds past `rounds` hold no item: skip their ranking (block-uniform)
#pragma unroll
            for (int q = 0; q < kRunItems; q++) {
                if (q < rounds) {
                    uint32_t kk[1] = {k[q]}, rr[1];
                    bool oo[1] = {ok[q]};
                    wave_rank<uint32_t, 1>(kk, oo, shift, kRadix - 1, sh.cnt[wave], rr, vary);
                    rank[q] = rr[0];
                }
            }
        }
        __syncthreads();
        const uint32_t tot = digit_wave_prefix(sh.cnt);
        uint32_t dummy;
        sh.start[t] = block_exclusive_scan(tot, sh.wave, &dummy);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kRunItems; q++) {
            if (ok[q]) {
                const uint32_t dd = digit_of(k[q], shift, kRadix - 1);
                const uint32_t pos = sh.start[dd] + sh.cnt[wave][dd] + rank[q];
                sh.k[cur ^ 1][pos] = k[q];
                sh.i[cur ^ 1][pos] = id[q];
            }
        }
        __syncthreads();
        cur ^= 1;
    }
    return cur;
}

// Number of the n sorted keys in a[] that are < key (or <= key when `inclusive`).
__device__ __forceinline__ uint32_t lds_rank(const uint32_t* a, uint32_t n, uint32_t key, bool inclusive)
{
    uint32_t lo = 0, len = n;
    while (len > 0) {
        const uint32_t half = len >> 1;
        const uint32_t v = a[lo + half];
        const bool go_right = inclusive ? (v <= key) : (v < key);
        lo = go_right ? lo + half + 1 : lo;
        len = go_right ? len - half - 1 : half;
    }
    return lo;
}

// Every lane gets the wave's result (wave_reduce_u32: DPP moves, all lanes active).
__device__ __forceinline__ void wave_and_or(uint32_t& a, uint32_t& o)
{
    a = wave_and_u32(a);
    o = wave_or_u32(o);
}

__device__ __forceinline__ void wave_min_max(uint32_t& lo, uint32_t& hi)
{
    lo = wave_min_u32(lo);
    hi = wave_max_u32(hi);
}

// LDS of the oversized-segment forms (the one-workgroup global form, the partition jobs).
struct BigShared {
    uint32_t cnt[kWavesPerBlock][kRadix];
    uint32_t hist[kRadix];
    uint32_t run[kRadix];  // running destination of each digit
    uint32_t aux[2][kRadix];  // partition jobs: MIN / MAX of each digit's low key halves
    uint32_t wave[kWavesPerBlock];
};

// One stable step of a digit pass through global memory: the cnt <= kBigItems * kBlock items
// [base, base + cnt) of (sk, sv) are ranked by digit ((low key half - dbase) >> shift) & mask inside the step (wave w
// owns items [w * 512, w * 512 + 512) in (round, lane) order) and item i goes to
// sh.run[digit] + its rank, then sh.run advances by the step's digit counts.  sh.run must be set
// before the call (its first barrier publishes it).  Destinations outside [lo, hi) are dropped:
// never, for consistent offsets -- a guard, not a case.
constexpr int kBigItems = 8;
constexpr int kBigStep = kBigItems * kBlock;  // 2048
// A step's pairs in registers: wave w's items [w * 512, w * 512 + 512) of [base, base + cnt), in
// (round, lane) order; absent items read as 0.
__device__ __forceinline__ void step_load(const uint64_t* sk, const uint32_t* sv, const uint32_t base,
                                          const uint32_t cnt, uint64_t (&k)[kBigItems], uint32_t (&v)[kBigItems])
{
    const uint32_t w0 = (threadIdx.x / kWave) * (kBigItems * kWave);
#pragma unroll
    for (int q = 0; q < kBigItems; q++) {
        const uint32_t i = w0 + q * kWave + lane_id();
        k[q] = i < cnt ? sk[base + i] : 0ull;
        v[q] = i < cnt ? sv[base + i] : 0u;
    }
}

// Track: also fold each item's low key half into sh.aux[0][digit] (MIN) and sh.aux[1][digit] (MAX).
// (Write-through `sc1` stores here, so that the SCATTER job's release had fewer dirty lines to write
// back, measured slower: one tile 1044 -> 1188 us, D2 0.5:0.02 516 -> 547 us.)
template <bool Track = false>
__device__ __forceinline__ void step_scatter(const uint64_t (&k)[kBigItems], const uint32_t (&v)[kBigItems],
                                             const uint32_t cnt, uint64_t* dk, uint32_t* dv, const uint32_t dbase,
                                             const int shift, const uint32_t mask, const uint32_t lo,
                                             const uint32_t hi, BigShared& sh)
{
    const int t = threadIdx.x;
    const int lane = lane_id();
    const int wave = t / kWave;
    for (int i = t; i < kWavesPerBlock * kRadix; i += kBlock) (&sh.cnt[0][0])[i] = 0;
    __syncthreads();
    bool ok[kBigItems];
    uint32_t rank[kBigItems];
    const uint32_t w0 = wave * (kBigItems * kWave);
#pragma unroll
    for (int q = 0; q < kBigItems; q++) ok[q] = w0 + q * kWave + lane < cnt;
    wave_rank<uint64_t, kBigItems, true>(k, ok, shift, mask, sh.cnt[wave], rank, mask, dbase);
    __syncthreads();
    const uint32_t tot = digit_wave_prefix(sh.cnt);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kBigItems; q++) {
        if (ok[q]) {
            const uint32_t dd = (((uint32_t)k[q] - dbase) >> shift) & mask;
            const uint32_t dst = sh.run[dd] + sh.cnt[wave][dd] + rank[q];
            if (dst >= lo && dst < hi) {
                dk[dst] = k[q];
                dv[dst] = v[q];
            }
            if (Track) {
                atomicMin(&sh.aux[0][dd], (uint32_t)k[q]);
                atomicMax(&sh.aux[1][dd], (uint32_t)k[q]);
            }
        }
    }
    __syncthreads();
    sh.run[threadIdx.x] += tot;
    __syncthreads();
}

__device__ __forceinline__ void scatter_step(const uint64_t* sk, const uint32_t* sv, uint64_t* dk, uint32_t* dv,
                                             const uint32_t base, const uint32_t cnt, const uint32_t dbase,
                                             const int shift, const uint32_t mask, const uint32_t lo,
                                             const uint32_t hi, BigShared& sh)
{
    uint64_t k[kBigItems];
    uint32_t v[kBigItems];
    step_load(sk, sv, base, cnt, k, v);
    step_scatter(k, v, cnt, dk, dv, dbase, shift, mask, lo, hi, sh);
}

// scatter_step over [base, base + cnt) in kBigStep steps, the next step's pairs loaded while the
// current one is ranked and stored (the queue's workers run one wave per SIMD: latency is hidden
// by the wave's own loads in flight or not at all; barriers do not wait for global loads).
template <bool Track = false>
__device__ __forceinline__ void scatter_steps(const uint64_t* sk, const uint32_t* sv, uint64_t* dk, uint32_t* dv,
                                              const uint32_t base, const uint32_t cnt, const uint32_t dbase,
                                              const int shift, const uint32_t mask, const uint32_t lo,
                                              const uint32_t hi, BigShared& sh)
{
    uint64_t k[kBigItems], kn[kBigItems];
    uint32_t v[kBigItems], vn[kBigItems];
    step_load(sk, sv, base, cnt < (uint32_t)kBigStep ? cnt : (uint32_t)kBigStep, k, v);
    for (uint32_t b0 = 0; b0 < cnt; b0 += kBigStep) {
        const uint32_t c = cnt - b0 < (uint32_t)kBigStep ? cnt - b0 : (uint32_t)kBigStep;
        const uint32_t b1 = b0 + kBigStep;
        if (b1 < cnt) step_load(sk, sv, base + b1, cnt - b1 < (uint32_t)kBigStep ? cnt - b1 : (uint32_t)kBigStep, kn, vn);
        step_scatter<Track>(k, v, c, dk, dv, dbase, shift, mask, lo, hi, sh);
#pragma unroll
        for (int q = 0; q < kBigItems; q++) {
            k[q] = kn[q];
            v[q] = vn[q];
        }
    }
}

// A segment of more than kSegCap pairs sorted by ONE workgroup: 4 stable LSD passes over the low
// 32 bits through global memory (keys/vals <-> alt within the segment's range).  The last resort
// of the partition queue below (its capacity exhausted); hot tiles normally go through the queue.
__device__ __forceinline__ void segment_sort_global(uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                    uint64_t* __restrict__ alt_k, uint32_t* __restrict__ alt_v,
                                                    const uint32_t begin, const uint32_t m, BigShared& sh)
{
    const int t = threadIdx.x;
    for (int pass = 0; pass < 4; pass++) {
        const int shift = pass * kRadixBits;
        const uint64_t* sk = (pass & 1) ? alt_k : keys;
        const uint32_t* sv = (pass & 1) ? alt_v : vals;
        uint64_t* dk = (pass & 1) ? keys : alt_k;
        uint32_t* dv = (pass & 1) ? vals : alt_v;
        sh.hist[t] = 0;
        __syncthreads();
        for (uint32_t i = t; i < m; i += kBlock) atomicAdd(&sh.hist[digit_of(sk[begin + i], shift, kRadix - 1)], 1u);
        __syncthreads();
        uint32_t dummy;
        sh.run[t] = begin + block_exclusive_scan(sh.hist[t], sh.wave, &dummy);
        for (uint32_t c0 = 0; c0 < m; c0 += kBigStep)
            scatter_step(sk, sv, dk, dv, begin + c0, m - c0 < (uint32_t)kBigStep ? m - c0 : (uint32_t)kBigStep, 0u,
                         shift, kRadix - 1, begin, begin + m, sh);
    }
}

// LSD form of the per-segment sort (the fallback of segment_sort_kernel for segments whose
// depth bits crowd into a few buckets): run A (<= kSegRun) sorted in LDS, run B parked in registers
// and sorted after it, the two merged by rank; every item's high key half and value gathered by
// its index in the segment and written in place.  `diff` = the low key bits that vary.
// The segment is read from (src_k, src_v) and written to (dst_k, dst_v): the same buffers (in
// place: every read precedes the first write) or alt -> keys (a piece of a partitioned hot tile).
// InPlace: dst is ignored and written through pointers based on src (keeps __restrict__ valid).
template <bool InPlace>
__device__ __forceinline__ void segment_sort_lsd(const uint64_t* __restrict__ src_k, const uint32_t* __restrict__ src_v,
                                                 uint64_t* __restrict__ dst_k, uint32_t* __restrict__ dst_v,
                                                 const uint32_t begin, const uint32_t m, const uint32_t diff,
                                                 SegShared& sh)
{
    uint64_t* dk = InPlace ? const_cast<uint64_t*>(src_k) : dst_k;
    uint32_t* dv = InPlace ? const_cast<uint32_t*>(src_v) : dst_v;
    const int t = threadIdx.x;
    const uint32_t na = m < (uint32_t)kSegRun ? m : (uint32_t)kSegRun, nb = m - na;
    uint32_t bk[kRunItems];
#pragma unroll
    for (int q = 0; q < kRunItems; q++) {
        const uint32_t i = t + q * kBlock;
        if (i < na) {
            sh.k[0][i] = (uint32_t)src_k[begin + i];
            sh.i[0][i] = i;
        }
        bk[q] = i < nb ? (uint32_t)src_k[begin + kSegRun + i] : 0u;
    }
    __syncthreads();
    const int ca = lds_radix_sort(sh, na, diff);

    // final (position, low key, index) of this thread's items: position t + 256 q
    uint32_t fk[kSegItems], fi[kSegItems], fp[kSegItems];
    bool fok[kSegItems];
    if (nb == 0) {
#pragma unroll
        for (int q = 0; q < kSegItems; q++) {
            const uint32_t i = t + q * kBlock;
            fok[q] = q < kRunItems && i < na;
            fp[q] = i;
            fk[q] = fok[q] ? sh.k[ca][i] : 0u;
            fi[q] = fok[q] ? sh.i[ca][i] : 0u;
        }
    } else {
        // park sorted run A in registers, sort run B, then merge by rank
        uint32_t ak[kRunItems], ai[kRunItems];
#pragma unroll
        for (int q = 0; q < kRunItems; q++) {
            ak[q] = sh.k[ca][t + q * kBlock];
            ai[q] = sh.i[ca][t + q * kBlock];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kRunItems; q++) {
            const uint32_t i = t + q * kBlock;
            if (i < nb) {
                sh.k[0][i] = bk[q];
                sh.i[0][i] = kSegRun + i;
            }
        }
        __syncthreads();
        const int cb = lds_radix_sort(sh, nb, diff);
#pragma unroll
        for (int q = 0; q < kRunItems; q++) {
            sh.k[cb ^ 1][t + q * kBlock] = ak[q];
            sh.i[cb ^ 1][t + q * kBlock] = ai[q];
        }
        __syncthreads();
        // stable merge: an A item precedes every B item with an equal key (A indices are smaller)
#pragma unroll
        for (int q = 0; q < kRunItems; q++) {
            const uint32_t i = t + q * kBlock;
            fok[q] = true;
            fk[q] = ak[q];
            fi[q] = ai[q];
            fp[q] = i + lds_rank(sh.k[cb], nb, ak[q], false);
            const uint32_t j = i;
            fok[kRunItems + q] = j < nb;
            fk[kRunItems + q] = fok[kRunItems + q] ? sh.k[cb][j] : 0u;
            fi[kRunItems + q] = fok[kRunItems + q] ? sh.i[cb][j] : 0u;
            fp[kRunItems + q] = fok[kRunItems + q] ? j + lds_rank(sh.k[cb ^ 1], kSegRun, fk[kRunItems + q], true) : 0u;
        }
    }
    // gather each item's high key half and value by its index in the segment (the segment is
    // unmodified until every workgroup thread has gathered), then write
    uint32_t hi[kSegItems], v[kSegItems];
#pragma unroll
    for (int q = 0; q < kSegItems; q++) {
        if (fok[q]) {
            hi[q] = (uint32_t)(src_k[begin + fi[q]] >> 32);
            v[q] = src_v[begin + fi[q]];
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kSegItems; q++) {
        if (fok[q]) {
            dk[begin + fp[q]] = ((uint64_t)hi[q] << 32) | fk[q];
            dv[begin + fp[q]] = v[q];
        }
    }
}

// Bucket form (the common case).  The segment's top kBucketBits varying low-key bits pick a
// bucket; a counting pass (LDS atomics, any order) gives every bucket its place, and each item's
// place inside its bucket is its exact rank there by (key bits below the bucket digit, index in
// segment) -- one 32-bit compare per bucket member (the two fields fit 32 bits when the top
// varying bit is <= 30, as for the float bits of positive depths; otherwise the LSD form runs).  Equal keys are therefore ordered by their input
// index, which is the stable order; no ballots and three workgroup barriers in place of the LSD
// form's four per 8-bit pass.  Each item's key and value stay in registers from the load to the
// in-place store (every load of the segment precedes the first barrier).
constexpr int kBucketBits = 10;
constexpr int kBuckets = 1 << kBucketBits;
constexpr int kMaxBucket = 128;  // a fuller bucket sends the segment to the LSD form
constexpr int kIndexBits = 11;   // index in segment < kSegCap
constexpr int kSegWaves = 7;  // waves per SIMD segment_sort_kernel's register budget is set for (17 KB of LDS allows 9)
constexpr int kSegWavesPacked = 8;  // ... and of its Packed instance (the tile sort's), which holds no high key halves

static_assert(kSegCap <= (1 << kIndexBits), "segment index must fit its field");

// The segment's low-key statistics for the bucket form: diff (the bits that vary: AND ^ OR) and the
// smallest low key lo, with the bucket digit over the keys' RANGE [lo, hi]: bucket = (x - lo) >> shift
// with shift = bits(hi - lo) - kBucketBits.  Float depth bits spread over many exponents (0.2 .. 100:
// bits 23..30 all vary, the top ten varying bits leave ~40 of 1024 buckets in use) fill the buckets
// evenly this way; the order is the same, x - lo being monotone over the segment.  Every thread
// passes its own partial a / o / lo / hi; s0, s1 hold kWavesPerBlock words each.
struct SegStats {
    uint32_t diff, lo;
    int shift, dbits;
};
__device__ __forceinline__ SegStats segment_stats(uint32_t a, uint32_t o, uint32_t lo, uint32_t hi, uint32_t* s0,
                                                  uint32_t* s1)
{
    const int lane = lane_id(), wave = threadIdx.x / kWave;
    wave_and_or(a, o);
    wave_min_max(lo, hi);
    if (lane == 0) {
        s0[wave] = a;
        s1[wave] = o;
    }
    __syncthreads();
    uint32_t aa = 0xffffffffu, oo = 0u;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; w++) {
        aa &= s0[w];
        oo |= s1[w];
    }
    __syncthreads();
    if (lane == 0) {
        s0[wave] = lo;
        s1[wave] = hi;
    }
    __syncthreads();
    uint32_t ll = 0xffffffffu, hh = 0u;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; w++) {
        ll = min(ll, s0[w]);
        hh = max(hh, s1[w]);
    }
    SegStats st;
    st.diff = aa ^ oo;
    st.lo = ll;
    const int nbits = hh > ll ? 32 - __builtin_clz(hh - ll) : 0;
    st.dbits = nbits < kBucketBits ? nbits : kBucketBits;
    st.shift = nbits - st.dbits;
    return st;
}

// What the bucket form itself needs of those, in one round: each wave's MIN / MAX into LDS behind one
// barrier (which also orders the caller's zeroing of the bucket counters).  lo == hi: equal low keys.
// s0, s1 (kWavesPerBlock words each) must be free on entry and hold the waves' values afterwards.
struct SegRange {
    uint32_t lo, hi;
    int shift;
};
__device__ __forceinline__ SegRange segment_range(uint32_t lo, uint32_t hi, uint32_t* s0, uint32_t* s1)
{
    const int lane = lane_id(), wave = threadIdx.x / kWave;
    wave_min_max(lo, hi);
    if (lane == 0) {
        s0[wave] = lo;
        s1[wave] = hi;
    }
    __syncthreads();
    SegRange r;
    r.lo = 0xffffffffu;
    r.hi = 0u;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; w++) {
        r.lo = min(r.lo, s0[w]);
        r.hi = max(r.hi, s1[w]);
    }
    const int nbits = r.hi > r.lo ? 32 - __builtin_clz(r.hi - r.lo) : 0;
    r.shift = nbits - (nbits < kBucketBits ? nbits : kBucketBits);
    return r;
}

// The low key bits that vary over the segment (AND ^ OR), for the LSD form: computed on the way into it
// from the pairs still in registers, the bucket form having no use for them.  s0, s1 must be free on
// entry; the barrier inside is the one the LSD form needs before it reuses the bucket form's LDS.
__device__ __forceinline__ uint32_t segment_diff(const uint64_t (&k)[kSegItems], const uint32_t m, uint32_t* s0,
                                                 uint32_t* s1)
{
    const int lane = lane_id(), wave = threadIdx.x / kWave;
    uint32_t a = 0xffffffffu, o = 0u;
#pragma unroll
    for (int q = 0; q < kSegItems; q++) {
        if (threadIdx.x + q * kBlock < m) {
            a &= (uint32_t)k[q];
            o |= (uint32_t)k[q];
        }
    }
    wave_and_or(a, o);
    if (lane == 0) {
        s0[wave] = a;
        s1[wave] = o;
    }
    __syncthreads();
    uint32_t aa = 0xffffffffu, oo = 0u;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; w++) {
        aa &= s0[w];
        oo |= s1[w];
    }
    return aa ^ oo;
}


struct BucketShared {
    uint32_t comb[kSegCap];   // (key bits below the digit << kIndexBits) | index, grouped by bucket
    uint32_t start[kBuckets];
    uint32_t fill[kBuckets];  // histogram, then the running fill pointer (= bucket end after filling)
};
// after ranking, the whole struct stages the sorted segment: keys (u64) then values (u32) when
// they fit together (<= kSegRun pairs), else keys and values one after the other
static_assert(sizeof(BucketShared) >= kSegCap * sizeof(uint64_t), "staging of the keys");
static_assert(sizeof(BucketShared) >= kSegRun * (sizeof(uint64_t) + sizeof(uint32_t)), "staging of a run");
// (compact: low halves + values staged in one pass when the segment's high key halves are all equal)
static_assert(sizeof(BucketShared) >= kSegCap * 2 * sizeof(uint32_t), "compact staging of a segment");
