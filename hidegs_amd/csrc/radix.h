// radix.h -- one LSD radix pass: digit_of, wave_rank, the tile histogram, the per-digit scan over tiles,
// segment_starts and radix_scatter_kernel.  Included by primitives.hip inside namespace hidegs::{anonymous},
// after the shared constants (kTile, kItems, kRadix) and scan.h.
#pragma once

// ============================== radix sort =====================================

template <typename K>
__device__ __forceinline__ uint32_t digit_of(K key, int shift, uint32_t mask)
{
    return (uint32_t)(key >> shift) & mask;
}

// Stable wave64 ranking of R rounds of items (round r, lane l = the wave's item r*64 + l,
// in input order).  cnt = this wave's 256 digit counters, zero on entry; on exit cnt[d] is
// the number of valid items with digit d and rank[r] the item's position among them.
// The lanes sharing a digit are found with one ballot per digit bit; bits outside `vary`
// are equal in every item (a caller's guarantee) and need none.  The lowest lane of each
// digit group bumps the counter (LDS ops of one wave retire in order, so the read precedes
// the write).
// With Based, the digit is taken of (low key half - dbase) instead (the partition queue's digits).
// With LaneMask, the lanes sharing a digit are found through LDS instead of by ballots: lane_mask =
// one 64-bit word per digit for this wave, zero on entry and again on exit.  Every valid lane ORs its
// lane bit into its digit's word and reads the word back: an OR has no order, so the word does not
// depend on the order in which the LDS serves the lanes of one atomic instruction, and the rank among
// the lanes below is the same mbcnt as in the ballot form.  The lowest lane of the group clears the
// word behind the read.  One atomic and one 8-byte read per round in place of ~7 VALU instructions
// per varying digit bit; `vary` is unused.
template <typename K, int R, bool Based = false, bool LaneMask = false>
__device__ __forceinline__ void wave_rank(const K (&k)[R], const bool (&ok)[R], int shift, uint32_t mask,
                                          uint32_t* cnt, uint32_t (&rank)[R], uint32_t vary, uint32_t dbase = 0u,
                                          uint64_t* lane_mask = nullptr)
{
    if (LaneMask) {
        const uint64_t bit = 1ull << lane_id();
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t d = Based ? ((((uint32_t)k[r]) - dbase) >> shift) & mask : digit_of(k[r], shift, mask);
            if (ok[r]) __hip_atomic_fetch_or(&lane_mask[d], bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __builtin_amdgcn_wave_barrier();
            uint64_t same = 0ull;  // lanes with the same digit
            uint32_t old = 0;
            if (ok[r]) {
                old = cnt[d];
                same = lane_mask[d];
            }
            __builtin_amdgcn_wave_barrier();
            const uint32_t below =
                __builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u));
            if (ok[r] && below == 0) {
                cnt[d] = old + (uint32_t)__popcll(same);
                lane_mask[d] = 0ull;
            }
            __builtin_amdgcn_wave_barrier();
            rank[r] = old + below;
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        const uint32_t d = Based ? ((((uint32_t)k[r]) - dbase) >> shift) & mask : digit_of(k[r], shift, mask);
        const uint64_t okb = __ballot(ok[r]);
        uint32_t mlo = (uint32_t)okb, mhi = (uint32_t)(okb >> 32);  // lanes with the same digit
#pragma unroll
        for (int b = 0; b < kRadixBits; b++) {
            if (!((vary >> b) & 1u)) continue;  // wave-uniform
            const uint32_t nb = ((d >> b) & 1u) - 1u;  // 0 when the bit is set, ~0 when clear
            const uint64_t bb = __ballot(nb == 0u);
            mlo &= nb ^ (uint32_t)bb;
            mhi &= nb ^ (uint32_t)(bb >> 32);
        }
        const uint32_t below = __builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u));
        uint32_t old = 0;
        if (ok[r]) old = cnt[d];
        __builtin_amdgcn_wave_barrier();
        if (ok[r] && below == 0) cnt[d] = old + (uint32_t)(__popc(mlo) + __popc(mhi));
        __builtin_amdgcn_wave_barrier();
        rank[r] = old + below;
    }
}

// After every wave ranked (and a __syncthreads): thread d turns s_cnt[w][d] into the count of
// digit d in waves < w and returns the block's total for digit d.
__device__ __forceinline__ uint32_t digit_wave_prefix(uint32_t (*s_cnt)[kRadix])
{
    const int d = threadIdx.x;  // kBlock == kRadix
    uint32_t run = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; w++) {
        const uint32_t c = s_cnt[w][d];
        s_cnt[w][d] = run;
        run += c;
    }
    return run;
}

// counts[d * ntiles + tile] = number of keys of tile `tile` whose digit is d.
// zero_jobs: zero_count 16-byte slots cleared on the side (the hot-tile queue's job slots).
// Bytes: `keys` holds one digit byte per key instead (radix_scatter_kernel's kOutRecordsDigit output,
// a tile's 4096 bytes as one 16-byte load per thread); shift is ignored.
template <typename K, bool Bytes = false>
__global__ __launch_bounds__(kBlock) void radix_hist_kernel(const K* __restrict__ keys, long long n, int shift,
                                                            uint32_t mask, int ntiles, uint32_t* __restrict__ counts,
                                                            uint4* __restrict__ zero_jobs, uint32_t zero_count)
{
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < zero_count; j += gridDim.x * kBlock)
        zero_jobs[j] = make_uint4(0u, 0u, 0u, 0u);  // (as a kStream stream_store: level, profiles/r13_store_policy.md)
    __shared__ uint32_t s_hist[kWavesPerBlock][kRadix];
    const int t = threadIdx.x;
    const int wave = t / kWave;
    for (int i = t; i < kWavesPerBlock * kRadix; i += kBlock) (&s_hist[0][0])[i] = 0;
    __syncthreads();
    // neighbouring tiles on one XCD: the counts of 32 neighbouring tiles share a 128-byte line of
    // each digit row, which then fills in one L2 instead of being written back piecewise
    // (16.4 -> 13.5 us per pass at 8M keys)
    const int tile = xcd_swizzle(blockIdx.x, gridDim.x);
    const long long base = (long long)tile * kTile;
    K k[kItems];
    if (Bytes) {
        const uint8_t* dg = reinterpret_cast<const uint8_t*>(keys);
        static_assert(kItems == 16, "a thread's 16 digit bytes are one uint4");
        if (base + kTile <= n && (reinterpret_cast<uintptr_t>(dg) & 15) == 0) {
            const uint4 p = reinterpret_cast<const uint4*>(dg + base)[t];
            const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
            for (int j = 0; j < kItems; j++) atomicAdd(&s_hist[wave][(w[j / 4] >> (8 * (j % 4))) & mask], 1u);
        } else {
#pragma unroll
            for (int j = 0; j < kItems; j++) {
                const long long i = base + j * kBlock + t;
                if (i < n) atomicAdd(&s_hist[wave][dg[i] & mask], 1u);
            }
        }
    } else if (sizeof(K) == 8 && base + kTile <= n && (reinterpret_cast<uintptr_t>(keys) & 15) == 0) {
        // full tile: 16-byte loads, two keys each (the histogram does not care about item order)
        const ulonglong2* k2 = reinterpret_cast<const ulonglong2*>(keys + base);
#pragma unroll
        for (int j = 0; j < kItems / 2; j++) {
            const ulonglong2 p = k2[j * kBlock + t];
            k[2 * j] = (K)p.x;
            k[2 * j + 1] = (K)p.y;
        }
#pragma unroll
        for (int j = 0; j < kItems; j++) atomicAdd(&s_hist[wave][digit_of(k[j], shift, mask)], 1u);
    } else {
#pragma unroll
        for (int j = 0; j < kItems; j++) {
            long long i = base + j * kBlock + t;
            k[j] = (i < n) ? keys[i] : K(0);
        }
#pragma unroll
        for (int j = 0; j < kItems; j++) {
            long long i = base + j * kBlock + t;
            if (i < n) atomicAdd(&s_hist[wave][digit_of(k[j], shift, mask)], 1u);
        }
    }
    __syncthreads();
    // only the digit rows the pass has: radix_digit_scan_kernel's grid is mask + 1 rows, and radix_scatter_kernel
    // loads the rows above `mask` only into digits that no item has (a 6-bit pass wrote 192 rows of scattered
    // 4-byte stores that nothing read: 12.3 -> 11.1 us per launch at the 1080p view)
    for (int d = t; d <= (int)mask; d += kBlock) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; w++) c += s_hist[w][d];
        counts[(long long)d * ntiles + tile] = c;
    }
}

constexpr int kDigitItems = 8;
// One workgroup per digit: exclusive scan of counts[d][0..ntiles) in place; totals[d] = sum.
// low_totals (nlow <= 256 digit totals of the previous pass, or NULL): workgroup 0 also writes
// their exclusive scan to low_base (the segment starts of radix_scatter_kernel<K, true>).
__global__ __launch_bounds__(kBlock) void radix_digit_scan_kernel(uint32_t* __restrict__ counts, int ntiles,
                                                                  uint32_t* __restrict__ totals,
                                                                  const uint32_t* __restrict__ low_totals, int nlow,
                                                                  uint32_t* __restrict__ low_base)
{
    if (low_totals && blockIdx.x == 0) {
        __shared__ uint32_t s_low[kWavesPerBlock];
        uint32_t dummy;
        const uint32_t b = block_exclusive_scan((int)threadIdx.x < nlow ? low_totals[threadIdx.x] : 0u, s_low, &dummy);
        if ((int)threadIdx.x < nlow) low_base[threadIdx.x] = b;
    }
    __shared__ uint32_t s_wave[kWavesPerBlock];
    uint32_t* row = counts + (long long)blockIdx.x * ntiles;
    // kDigitItems per thread: one round (one memory latency) for up to 256 x that many tiles
    uint32_t carry = 0;
    for (int base = 0; base < ntiles; base += kBlock * kDigitItems) {
        uint32_t v[kDigitItems];
        uint32_t sum = 0;
#pragma unroll
        for (int j = 0; j < kDigitItems; j++) {
            int i = base + threadIdx.x * kDigitItems + j;
            v[j] = (i < ntiles) ? row[i] : 0u;
            sum += v[j];
        }
        uint32_t total;
        uint32_t pre = block_exclusive_scan(sum, s_wave, &total) + carry;
#pragma unroll
        for (int j = 0; j < kDigitItems; j++) {
            int i = base + threadIdx.x * kDigitItems + j;
            if (i < ntiles) row[i] = pre;
            pre += v[j];
        }
        carry += total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// Stable scatter of one tile.  LDS: one staging buffer of the tile's keys (values reuse it
// afterwards), per-wave digit counters -- 43 KB at 8 waves, 3 workgroups per CU (38 KB and 4 for the
// 128-digit instances, below).
// Global offsets: tile_prefix[d][tile] (per-digit exclusive scan over tiles) + exclusive scan
// of the digit totals.  (A single-pass decoupled look-back variant measured slower on MI355X:
// the chained tile-to-tile hand-off crosses the non-coherent per-XCD L2s at every hop.)
constexpr int kSWaves = 8;  // wave64s per scatter workgroup (the tile stays kTile pairs); 8 waves
                            // of 8 pairs each (66 VGPRs, 6 waves/SIMD) measured 2-3% faster than 4 of 16
constexpr int kSBlock = kSWaves * kWave;
constexpr int kSItems = kTile / kSBlock;  // pairs per thread
static_assert(kSBlock >= kRadix, "one thread per digit in the digit scans");

// radix_scatter_kernel<K, true>'s segment starts (see there); every thread of the workgroup calls it.
template <typename K, int R, int D = kRadix>  // D: digit capacity (> mask, and 1 << b0 <= D)
__device__ __forceinline__ void segment_starts(const K (&k)[R], const bool (&ok)[R], const int shift, const uint32_t mask,
                                            const long long n, const int tile, const int ntiles,
                                            const long long base, const uint32_t digit_base,
                                            const uint32_t p0, const int b0, uint32_t* starts)
{
    __shared__ uint32_t s_bhist[D];
    __shared__ uint32_t s_blist[D];
    __shared__ uint32_t s_nb;
    const int t = threadIdx.x, lane = lane_id(), wave = t / kWave;
    if (t == 0) {
        s_nb = 0u;
        if (tile == 0) starts[(mask + 1u) << b0] = (uint32_t)n;
    }
    if (b0 == 0) {  // one pass: the digit bases of tile 0 are the segment starts
        if (tile == 0 && t <= (int)mask) starts[t] = digit_base;
        return;
    }
    __syncthreads();  // s_nb
    // low values whose first position p0 = base0[t] lies in this tile (position n: the last tile)
    if (t < (1 << b0) && (((long long)p0 >= base && (long long)p0 < base + kTile) ||
                          ((long long)p0 >= n && tile == ntiles - 1)))
        s_blist[atomicAdd(&s_nb, 1u)] = (uint32_t)t | (((uint32_t)((long long)p0 - base)) << 8);
    __syncthreads();
    const uint32_t nb = s_nb;  // workgroup-uniform; 0 for most tiles
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t e = s_blist[b], L = e & 0xffu, r = e >> 8;  // the tile's pairs [0, r) precede L
        if (t < D) s_bhist[t] = 0u;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < R; q++) {
            const uint32_t li = (uint32_t)(wave * (R * kWave) + q * kWave + lane);
            if (ok[q] && li < r) atomicAdd(&s_bhist[digit_of(k[q], shift, mask)], 1u);
        }
        __syncthreads();
        if (t <= (int)mask) starts[((uint32_t)t << b0) | L] = digit_base + s_bhist[t];
        __syncthreads();
    }
}

// Starts (the segmented sort's last segment-bit pass): also the output position of each segment's
// first pair, starts[(H << b0) | L] for segment (H = this pass's digit, L = the b0 segment bits of
// the pass before), so that no kernel has to find the ranges in the sorted keys.  Pass 1 is stable
// and its input is ordered by L: segment (H, L) starts at this tile's global base of digit H plus
// the digit-H pairs of this tile that precede base0[L] (the first input position of L: the
// exclusive scan of pass 0's digit totals, totals0), for the tile that holds base0[L].  b0 == 0
// (one pass, the digit is the whole segment id): tile 0 writes starts[d] = base of digit d.
// starts[(mask + 1) << b0] = n closes the last segment.
// D = digit capacity: kRadix, or kNarrowRadix for passes of <= 7 bits, whose smaller LDS arrays
// (39 KB instead of 45 KB) let a fourth workgroup onto each CU: the 1080p binning sort (8.6M pairs,
// 6 + 7 bits) 189 -> 183 us.  Only up to kNarrowMaxN pairs: the 4K frame's 42.9M pairs (7 + 8 bits)
// went 880 -> 894 us with its 7-bit pass narrow -- a fourth workgroup's open digit runs cost more
// once a pass's output no longer stays in the 256 MB MALL (profiles/r04_narrow_scatter.md).
// Records (hidegs_sort_tile_pairs only, whose tile id is the whole high key half): between its kernels
// the sort carries one 8-byte record {low key half, value} per pair instead of a 12-byte pair.
//   Out == kOutRecords (with Starts, the last pass): the records go to keys_out at the pairs' final
//     indices and vals_out is not written; segment_sort_kernel<true> knows the high half, the segment
//     id, from starts[] and puts whole pairs back.
//   Out == kOutRecordsDigit (the first of two passes): also each pair's digit of the NEXT pass
//     (next_shift, next_mask), one byte per pair at vals_out, which is all the next histogram reads.
//   RecIn (the second pass): keys_in holds records and vals_in the digit bytes; the key is formed in
//     registers as digit << shift | low half, so the ranking and the starts run unchanged.
// A record tile is staged once; the digit of a staged position comes from a byte per position kept in
// the per-wave counters' LDS, dead by then (the next pass's digit bytes take a second, 4 KB round).
// (The 128-digit kOutRecordsDigit instance spills 16 B/lane at its 64-VGPR budget; the 256-digit one in its
// place measured the same: profiles/r09_tile_sort_records.md.)
constexpr int kNarrowRadix = 128;
constexpr long long kNarrowMaxN = 12ll << 20;
constexpr int kOutPairs = 0, kOutRecords = 1, kOutRecordsDigit = 2;
template <typename K, bool Starts = false, int D = kRadix, int Out = kOutPairs, bool RecIn = false>
__global__ __launch_bounds__(kSBlock) __attribute__((amdgpu_waves_per_eu(D == kRadix ? 1 : 8))) void radix_scatter_kernel(const K* __restrict__ keys_in,
                                                                const uint32_t* __restrict__ vals_in,
                                                                K* __restrict__ keys_out, uint32_t* __restrict__ vals_out,
                                                                long long n, int shift, uint32_t mask, int ntiles,
                                                                const uint32_t* __restrict__ tile_prefix,
                                                                const uint32_t* __restrict__ totals,
                                                                const uint32_t* __restrict__ totals0, int b0,
                                                                uint32_t* __restrict__ starts, int next_shift,
                                                                uint32_t next_mask)
{
    __shared__ __attribute__((aligned(16))) K s_stage[kTile];  // keys by tile-local rank, then values
    __shared__ uint32_t s_cnt[kSWaves][D];              // per-wave running counters
    __shared__ uint32_t s_start[D];                     // tile-local start of each digit run
    __shared__ uint32_t s_off[D];                       // global position of tile-local position 0 of digit d
    __shared__ uint32_t s_wave[kSWaves];
    uint32_t* s_vals = reinterpret_cast<uint32_t*>(s_stage);

    const int t = threadIdx.x;
    const int lane = lane_id();
    // wave-uniform, and told so: the wave's LDS bases (counters, lane masks) and its items' offset stay in
    // scalar registers, which the 64-VGPR instances have none to spare for
    const int wave = __builtin_amdgcn_readfirstlane(t / kWave);
    const bool digit_thread = t < D;  // thread d owns digit d in the digit scans
    for (int i = t; i < kSWaves * D; i += kSBlock) (&s_cnt[0][0])[i] = 0;
    // neighbouring tiles on one XCD: 46.3 -> 42.9 us per pass at 8M pairs (their shared output lines at
    // digit-run ends merge in one L2); the same mapping for segment_sort measured 48.1 -> 49.7 us and is
    // not used there
    const int tile = xcd_swizzle(blockIdx.x, gridDim.x);
    const long long base = (long long)tile * kTile;
    const long long seg = base + (long long)wave * (kSItems * kWave);  // this wave's items
    // this tile's global digit offsets, loaded now so their latency hides behind the ranking (digits
    // above `mask` read stale counts that no item uses)
    const uint32_t digit_total = digit_thread ? totals[t] : 0u;
    const uint32_t digit_prefix = digit_thread ? tile_prefix[(long long)t * ntiles + tile] : 0u;
    const uint32_t low_base = Starts && b0 > 0 && t < (1 << b0) ? totals0[t] : 0u;  // base0[t]; b0 <= 8

    K k[kSItems];
    uint32_t v[kSItems];
    bool ok[kSItems];
    // the pass's input, dead after the pass, read with non-temporal loads so it does not displace the
    // output the next pass reads: scatter 42.8 -> 40.6 us (1080p D2 view), 4K sort 872 -> 834 us
    // (profiles/r04_scatter_nt.md)
    // RecIn: the wave's kSItems * 64 digit bytes are contiguous: one 8-byte load per lane, handed round
    // through the wave's part of the staging buffer (free until the ranks are known; LDS operations of
    // one wave retire in order).  Byte loads, 64 B per instruction, share their lines between two rounds
    // and measured 4.5 us slower per pass than the pairs they replace.
    static_assert(!RecIn || kSItems == 8, "a lane's share of the wave's digit bytes is one 8-byte load");
    uint8_t* s_part = reinterpret_cast<uint8_t*>(s_stage) + wave * (sizeof(K) * kTile / kSWaves);  // the wave's own part
    uint8_t* s_in = s_part;
    if (RecIn) {
        const uint8_t* dg = reinterpret_cast<const uint8_t*>(vals_in);
        const long long i8 = seg + lane * 8;
        uint64_t d8 = 0ull;
        if (i8 + 8 <= n && (reinterpret_cast<uintptr_t>(dg) & 7) == 0) {
            d8 = __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(dg + i8));
        } else {
            for (int b = 0; b < 8; b++)
                if (i8 + b < n) d8 |= (uint64_t)dg[i8 + b] << (8 * b);
        }
        *reinterpret_cast<uint64_t*>(s_in + lane * 8) = d8;
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int r = 0; r < kSItems; r++) {
        const long long i = seg + r * kWave + lane;
        ok[r] = i < n;
        if (RecIn) {
            const uint64_t rec = ok[r] ? __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(keys_in) + i) : 0ull;
            const uint32_t dg = s_in[r * kWave + lane];
            k[r] = (K)(((uint64_t)dg << shift) | (uint32_t)rec);
            v[r] = (uint32_t)(rec >> 32);
        } else {
            k[r] = ok[r] ? __builtin_nontemporal_load(keys_in + i) : K(0);
            v[r] = ok[r] ? __builtin_nontemporal_load(vals_in + i) : 0u;
        }
    }
    // the digits' global bases, scanned while the tile's loads are in flight (workgroup barriers
    // do not wait for global loads)
    uint32_t dummy;
    const uint32_t digit_base = block_exclusive_scan<kSWaves>(digit_total, s_wave, &dummy) + digit_prefix;
    // (at the end of the kernel instead, with the keys kept live: 73 VGPRs against 61, same time)
    if (Starts) segment_starts<K, kSItems, D>(k, ok, shift, mask, n, tile, ntiles, base, digit_base, low_base, b0, starts);
    // the ranking's lane masks (wave_rank's LaneMask form), D words of 8 bytes, live in the wave's own
    // part of the staging buffer as well: s_in's bytes are in k[] by now (LDS operations of one wave
    // retire in order), and the barrier after the ranking separates the masks from the staged keys
    static_assert(D * sizeof(uint64_t) <= sizeof(K) * kTile / kSWaves && D % kWave == 0, "the masks fit the wave's part");
    uint64_t* s_mask = reinterpret_cast<uint64_t*>(s_part);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < D / kWave; j++) s_mask[j * kWave + lane] = 0ull;
    __builtin_amdgcn_wave_barrier();
    uint32_t rank[kSItems];
    wave_rank<K, kSItems, false, true>(k, ok, shift, mask, s_cnt[wave], rank, mask, 0u, s_mask);
    __syncthreads();

    uint32_t tile_count_d = 0;  // thread d: count of digit d in waves before each wave, in place
    if (digit_thread) {
#pragma unroll
        for (int w = 0; w < kSWaves; w++) {
            const uint32_t c = s_cnt[w][t];
            s_cnt[w][t] = tile_count_d;
            tile_count_d += c;
        }
    }
    const uint32_t start_d = block_exclusive_scan<kSWaves>(tile_count_d, s_wave, &dummy);
    if (digit_thread) {
        s_start[t] = start_d;
        s_off[t] = digit_base - start_d;
    }
    __syncthreads();
    uint32_t pos[kSItems];
#pragma unroll
    for (int r = 0; r < kSItems; r++) {
        if (ok[r]) {
            const uint32_t dd = digit_of(k[r], shift, mask);
            pos[r] = s_start[dd] + s_cnt[wave][dd] + rank[r];
            if (Out == kOutPairs) s_stage[pos[r]] = k[r];
        }
    }
    __syncthreads();
    const int count = (int)((n - base) < kTile ? (n - base) : kTile);
    if (Out != kOutPairs) {  // after the barrier: every counter is read, their LDS takes the positions' digits
        static_assert(Out == kOutPairs || Starts == (Out == kOutRecords), "the last pass writes the final records");
        static_assert(sizeof(s_cnt) >= kTile && D <= 256, "a digit byte per staged position");
        uint8_t* s_digit = reinterpret_cast<uint8_t*>(&s_cnt[0][0]);
#pragma unroll
        for (int r = 0; r < kSItems; r++) {
            if (ok[r]) {
                s_stage[pos[r]] = (K)(((uint64_t)v[r] << 32) | (uint32_t)k[r]);
                s_digit[pos[r]] = (uint8_t)digit_of(k[r], shift, mask);
                // the next pass's digit rides above the position (< 4096): the keys die here
                if (Out == kOutRecordsDigit) pos[r] |= digit_of(k[r], next_shift, next_mask) << 16;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kSItems; j++) {  // run-contiguous: position i = t + kSBlock j
            const int i = t + j * kSBlock;
            if (i < count) {
                const uint32_t d = s_off[s_digit[i]] + i;
                // (A plain store: stream_store's kThrough here measured +3.7 us per step and kStream +15 us, and
                // +5 / +13 us when only the 128-byte lines wholly inside a digit run took the policy; the digit
                // bytes below as kStream +4 us: profiles/r13_store_policy.md.)
                if (d < n) keys_out[d] = s_stage[i];  // always true for consistent counts
            }
        }
        if (Out == kOutRecordsDigit) {
            __syncthreads();  // every record read: the staging buffer takes the next pass's digits
            uint8_t* s_next = reinterpret_cast<uint8_t*>(s_stage);
            uint8_t* digits_out = reinterpret_cast<uint8_t*>(vals_out);
#pragma unroll
            for (int r = 0; r < kSItems; r++)
                if (ok[r]) s_next[pos[r] & 0xffffu] = (uint8_t)(pos[r] >> 16);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kSItems; j++) {
                const int i = t + j * kSBlock;
                if (i < count) {  // (the destination again, not eight registers kept across the barriers)
                    const uint32_t d = s_off[s_digit[i]] + i;
                    if (d < n) digits_out[d] = s_next[i];
                }
            }
        }
        return;
    }
    uint32_t dst[kSItems];
#pragma unroll
    for (int j = 0; j < kSItems; j++) {  // keys, run-contiguous: position i = t + kSBlock j
        const int i = t + j * kSBlock;
        dst[j] = 0xffffffffu;
        if (i < count) {
            const K key = s_stage[i];
            dst[j] = s_off[digit_of(key, shift, mask)] + i;
            if (dst[j] < n) keys_out[dst[j]] = key;  // always true for consistent counts
        }
    }
    __syncthreads();  // every key read: the staging buffer takes the values
#pragma unroll
    for (int r = 0; r < kSItems; r++)
        if (ok[r]) s_vals[pos[r]] = v[r];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSItems; j++) {
        const int i = t + j * kSBlock;
        if (i < count && dst[j] < n) vals_out[dst[j]] = s_vals[i];
    }
}
