// primitives.hip -- the binning primitives of Rasterizer::forward as gfx950 kernels:
//
//   hidegs_inclusive_scan_u32   <- cub::DeviceScan::InclusiveSum of tiles_touched
//                                  (rasterizer_impl.cu:171,321)
//   hidegs_sort_pairs_u64/_u32  <- cub::DeviceRadixSort::SortPairs over bits [begin, end)
//                                  (rasterizer_impl.cu:193-196,354-362; simple_knn.cu:211-214)
//   hidegs_identify_tile_ranges <- cudaMemsetAsync(ranges) + identifyTileRanges
//                                  (rasterizer_impl.cu:364-371,120-142)
//   hidegs_sort_tile_pairs      <- SortPairs + memset + identifyTileRanges as one call
//                                  (rasterizer_impl.cu:354-371)
//   hidegs_higher_msb           <- getHigherMsb (rasterizer_impl.cu:35-50)
//
// Design (MI355X-first, not a CUB restatement):
//  * Tiles of 4096 items per 256-thread workgroup (4 x wave64, 16 items per lane),
//    global traffic in 16-byte-per-lane vector loads where the layout allows.
//  * Scan: tile sums, then a rescan in which each workgroup adds up the sums before it
//    (two stream-ordered launches, no inter-workgroup hand-off inside a launch).
//  * Radix sort: LSD, 8-bit digits, per pass three launches:
//      1. tile histogram  (per-wave LDS histograms, digit-major counts[d][tile])
//      2. per-digit exclusive scan over tiles (one workgroup per digit)
//      3. scatter: stable ranks from wave64 ballot matching (8 ballots give the
//         set of lanes sharing a digit), per-wave running counters in LDS,
//         a local sort of the tile in LDS, then run-contiguous global stores.
//    Stability is by construction: item order inside a wave is (round, lane),
//    waves own consecutive 1024-item segments, tiles are ordered by the scan.
// No kernel depends on dispatch order or XCD placement.
#include "block_scan.h"
#include "common.h"

#include <mutex>

namespace hidegs {
int identify_tile_ranges(const uint64_t* keys, long long n, uint32_t* ranges, int num_tiles, hipStream_t stream);

namespace {

constexpr int kBlock = 256;
constexpr int kItems = 16;  // items per thread of a radix tile
constexpr int kTile = kBlock * kItems;       // 4096
constexpr int kWavesPerBlock = kBlock / kWave;  // 4
constexpr int kRadixBits = 8;
constexpr int kRadix = 1 << kRadixBits;     // 256

#ifndef HIDEGS_SCOUTS
#define HIDEGS_SCOUTS 128  // segment_sort_kernel's first workgroups, which start the hot tiles (0: own workgroup)
#endif

inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// The kernels by stage, one translation unit: each header builds on the ones before it.
#include "scan.h"
#include "radix.h"
#include "segment_forms.h"
#include "queue_trace.h"
#include "hot_queue.h"
#include "segment_sort.h"

// ============================== tile ranges ====================================

// Tile ids >= num_tiles violate the caller contract; their entries are skipped rather
// than written out of bounds.
// tile = (key >> 32) & tile_mask (the public entry point passes all ones; the segmented sort
// masks to its segment bits).
// ranges[tile] = [first, last + 1) of the tile's keys (tile = (key >> 32) & tile_mask); tiles
// >= num_tiles are skipped.  Each thread checks 4 consecutive keys (two 16-byte loads) and the
// key before them; only the rare boundaries write.
constexpr int kRangeKeys = 4;
// zero (or NULL): the partition queue, reset for the segment_sort_kernel that follows -- its
// Q_WORDS counters and its job_cap slots (slot tags read 0 until published).
__global__ __launch_bounds__(kBlock) void identify_ranges_kernel(const uint64_t* __restrict__ keys, long long n,
                                                                 uint2* __restrict__ ranges, uint32_t num_tiles,
                                                                 uint32_t tile_mask)
{
    const long long i0 = ((long long)blockIdx.x * kBlock + threadIdx.x) * kRangeKeys;
    if (i0 >= n) return;
    uint32_t tile[kRangeKeys];
    if (i0 + kRangeKeys <= n && (reinterpret_cast<uintptr_t>(keys) & 15) == 0) {
        const ulonglong2* k2 = reinterpret_cast<const ulonglong2*>(keys + i0);
        const ulonglong2 a = k2[0], b = k2[1];
        tile[0] = (uint32_t)(a.x >> 32) & tile_mask;
        tile[1] = (uint32_t)(a.y >> 32) & tile_mask;
        tile[2] = (uint32_t)(b.x >> 32) & tile_mask;
        tile[3] = (uint32_t)(b.y >> 32) & tile_mask;
    } else {
#pragma unroll
        for (int j = 0; j < kRangeKeys; j++) tile[j] = i0 + j < n ? (uint32_t)(keys[i0 + j] >> 32) & tile_mask : 0u;
    }
    uint32_t prev = i0 == 0 ? 0u : (uint32_t)(keys[i0 - 1] >> 32) & tile_mask;
#pragma unroll
    for (int j = 0; j < kRangeKeys; j++) {
        const long long i = i0 + j;
        if (i >= n) break;
        const uint32_t cur = tile[j];
        if (i == 0) {  // the reference leaves .y of a single key's tile unset (n == 1)
            if (cur < num_tiles) ranges[cur].x = 0;
        } else {
            if (cur != prev) {
                if (prev < num_tiles) ranges[prev].y = (uint32_t)i;
                if (cur < num_tiles) ranges[cur].x = (uint32_t)i;
            }
            if (i == n - 1 && cur < num_tiles) ranges[cur].y = (uint32_t)n;
        }
        prev = cur;
    }
}

// ============================== host side ======================================


size_t scan_scratch(long long n)
{
    const int nt = ceil_div(n, kDevScanTile);
    return align_up((size_t)nt * sizeof(uint32_t)) + align_up(sizeof(uint32_t));
}

constexpr int kMaxSegmentBits = 16;        // segmented path: at most 65536 segments
constexpr long long kSegmentedMinN = 65536;  // below this the plain LSD passes are cheaper
constexpr long long kSegmentedMinAvg = 64;   // pairs per segment on average, else the plain passes: one
                                             // workgroup per ~30-pair segment (distCUDA2's 48-bit Morton
                                             // keys of 2M points) costs more than the 4 low-digit passes;
                                             // with its 16 segment bits distCUDA2 turns segmented at
                                             // 64 << 16 = 4,194,304 points
constexpr long long kTileSegmentedMinAvg = 8;  // the same for hidegs_sort_tile_pairs, per tile of the caller's grid: small
                                               // views (config 2, 100k Gaussians) took 6 plain passes, 105-115 us, against
                                               // 68-70 us segmented (64 / 32 / 16 / 8 / 1 A/B in DESIGN.md, "Small views")

// Capacities of the partition queue for n pairs.  Every record holds > kSegCap pairs and the
// records of one level are disjoint: <= n / 2049 per level, 5 levels (4 digits + the copy).  A
// record queues <= 3 jobs per chunk of >= 4096 pairs and <= 2 pieces per kSegRun pairs (a piece lies in
// one kSegRun window or is a digit of its own) -- under n / 39 jobs in all, so job_cap (n / 24,
// zeroed every call: n / 1.5 bytes) cannot overflow.  The pool (pool_rows(chunks) x 256 u32 per record)
// is sized for a few hot tiles' worth; a record that finds it (or the record table) full is sorted
// by one workgroup instead (a GLOBAL job) -- slower, same result.
BigQueue queue_caps(long long n)
{
    BigQueue q{};
    q.rec_cap = (uint32_t)(5 * (n / (kSegCap + 1)) + 8);
#ifdef HIDEGS_JOB_CAP  // tests only: a tiny job capacity forces the overflow path (tests/test_binning_gpu.py)
    q.job_cap = (uint32_t)HIDEGS_JOB_CAP;
#else
    q.job_cap = (uint32_t)(n / 24 + 1024);
#endif
    q.pool_cap = (uint32_t)(n / 2 + 16 * kRadix);
#ifdef HIDEGS_PIECE_CAP  // tests only: a tiny piece list sends the pieces beyond it to SMALL jobs
    q.piece_cap = (uint32_t)HIDEGS_PIECE_CAP;
#else
    q.piece_cap = (uint32_t)(n / 512 + 1024);  // <= 2 pieces per kSegRun pairs; beyond: SMALL jobs
#endif
    return q;
}

template <typename K>
size_t sort_scratch(long long n)
{
    const int nt = ceil_div(n, kTile);
    size_t b = align_up((size_t)n * sizeof(K)) + align_up((size_t)n * sizeof(uint32_t)) +
               align_up((size_t)kRadix * nt * sizeof(uint32_t)) + 2 * align_up(kRadix * sizeof(uint32_t));
    if (sizeof(K) == 8) {  // segmented path: the segment ranges and the partition queue
        const BigQueue q = queue_caps(n);
        b += align_up(sizeof(uint32_t) * (((size_t)1 << kMaxSegmentBits) + 1)) + align_up(kRadix * sizeof(uint32_t)) +
             align_up(Q_WORDS * sizeof(uint32_t)) +
             align_up((size_t)q.rec_cap * sizeof(BigSeg)) + align_up((size_t)q.job_cap * sizeof(uint4)) +
             align_up((size_t)q.pool_cap * sizeof(uint32_t)) + align_up((size_t)q.piece_cap * sizeof(uint2));
    }
    return b;
}

__global__ void identify_ranges_kernel(const uint64_t* __restrict__ keys, long long n, uint2* __restrict__ ranges,
                                       uint32_t num_tiles, uint32_t tile_mask);

// ranges_out (num_tiles entries) set: the tile ranges of the sorted keys are written too, with
// identify_tile_ranges' semantics; the caller guarantees key >> 32 < num_tiles.
template <typename K>
int sort_pairs(void* scratch, size_t scratch_bytes, const K* keys_in, K* keys_out, const uint32_t* vals_in,
               uint32_t* vals_out, long long n, int begin_bit, int end_bit, hipStream_t stream, const char* what,
               uint2* ranges_out = nullptr, int num_tiles = 0)
{
    const int kbits = (int)(8 * sizeof(K));
    if (n < 0 || begin_bit < 0 || end_bit > kbits || begin_bit > end_bit)
        return fail(HIDEGS_E_ARG, std::string(what) + ": bad size or bit range");
    if (n > 0x7fffffffLL) return fail(HIDEGS_E_ARG, std::string(what) + ": more than 2^31-1 items");
    if (n == 0)
        return ranges_out ? identify_tile_ranges(nullptr, 0, reinterpret_cast<uint32_t*>(ranges_out), num_tiles, stream)
                          : 0;
    if (!keys_in || !keys_out || !vals_in || !vals_out)
        return fail(HIDEGS_E_ARG, std::string(what) + ": NULL key/value pointer");
    if (keys_out == keys_in || vals_out == vals_in)
        return fail(HIDEGS_E_ARG, std::string(what) + ": in-place sorting is not supported");
    if (!scratch || scratch_bytes < sort_scratch<K>(n))
        return fail(HIDEGS_E_ARG, std::string(what) + ": scratch buffer too small");

    const int passes = (end_bit - begin_bit + kRadixBits - 1) / kRadixBits;
    if (passes == 0) {
        if (hipMemcpyAsync(keys_out, keys_in, n * sizeof(K), hipMemcpyDeviceToDevice, stream) != hipSuccess ||
            hipMemcpyAsync(vals_out, vals_in, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream) != hipSuccess)
            return fail(HIDEGS_E_HIP, std::string(what) + ": copy failed");
        return ranges_out ? identify_tile_ranges(reinterpret_cast<const uint64_t*>(keys_out), n,
                                                 reinterpret_cast<uint32_t*>(ranges_out), num_tiles, stream)
                          : 0;
    }
    const int nt = ceil_div(n, kTile);
    Carver c(scratch);
    K* alt_k = c.take<K>(n);
    uint32_t* alt_v = c.take<uint32_t>(n);
    uint32_t* counts = c.take<uint32_t>((size_t)kRadix * nt);
    uint32_t* totals_pass[2] = {c.take<uint32_t>(kRadix), c.take<uint32_t>(kRadix)};  // alternate passes

    // (tile | depth)-shaped sort: LSD over the segment bits only, then per-segment LDS sorts
    // average pairs per segment: per tile of the caller's grid with ranges_out, else per segment-bit value
    const bool avg_ok = ranges_out ? n >= kTileSegmentedMinAvg * (long long)num_tiles
                                   : n >= (kSegmentedMinAvg << (end_bit - 32));
    const bool segmented = sizeof(K) == 8 && begin_bit == 0 && end_bit > 32 && end_bit - 32 <= kMaxSegmentBits &&
                           n >= kSegmentedMinN && avg_ok;
    const int lo_bit = segmented ? 32 : begin_bit;
    const int lsd_passes = segmented ? (end_bit - 32 + kRadixBits - 1) / kRadixBits : passes;

    // segmented path: the segment ranges (the caller's tile ranges with ranges_out: tile ids
    // < num_tiles <= 2^(end_bit-32) leave no bits above end_bit, so segment == tile) and the
    // hot-tile queue (its job slots are cleared by the last histogram pass)
    // with ranges_out the last pass hands segment_sort 8-byte {low key half, value} records in keys_out
    // (the high half is the segment id); generic keys keep whole pairs: bits above end_bit survive
    const bool packed = segmented && ranges_out != nullptr;
    int nseg = 0;
    uint32_t* seg_starts = nullptr;
    uint32_t* low_base = nullptr;
    BigQueue q{};
    if (segmented) {
        nseg = ranges_out ? num_tiles : 1 << (end_bit - 32);
        seg_starts = c.take<uint32_t>(((size_t)1 << kMaxSegmentBits) + 1);
        low_base = c.take<uint32_t>(kRadix);
        q = queue_caps(n);
        q.ctl = c.take<uint32_t>(Q_WORDS);  // the counters and the job slots are contiguous (1 KB + ...):
        q.job = c.take<uint4>(q.job_cap);   // the last histogram pass clears them as one range
        q.rec = c.take<BigSeg>(q.rec_cap);
        q.pool = c.take<uint32_t>(q.pool_cap);
        q.alt_k = reinterpret_cast<uint64_t*>(alt_k);
        q.alt_v = alt_v;
        q.piece = c.take<uint2>(q.piece_cap);
    }

    const K* src_k = keys_in;
    const uint32_t* src_v = vals_in;
    // balanced digit widths (13 tile bits: 7 + 6, not 8 + 5): fewer buckets per pass mean
    // longer runs per bucket in each tile's scatter, i.e. fuller write lines
    const int span = end_bit - lo_bit;
    int shift = lo_bit;
    int pass_bits[2] = {0, 0};
    for (int p = 0; p < lsd_passes; p++) {
        const int bits = (span * (p + 1)) / lsd_passes - (span * p) / lsd_passes;
        const uint32_t mask = (1u << bits) - 1u;
        const bool to_out = ((lsd_passes - 1 - p) % 2) == 0;
        K* dk = to_out ? keys_out : alt_k;
        uint32_t* dv = to_out ? vals_out : alt_v;
        uint32_t* totals = totals_pass[p & 1];
        const bool last = p == lsd_passes - 1;
        uint4* zero_jobs = segmented && last ? reinterpret_cast<uint4*>(q.ctl) : nullptr;
        static_assert(Q_WORDS * sizeof(uint32_t) % kAlign == 0, "ctl and job slots contiguous");
        // records (radix.h): the first of two passes also writes the second one's digit as a byte per pair
        // (into the value scratch), which is then all the second histogram reads
        const bool rec_in = packed && lsd_passes == 2 && last, rec_digit_out = packed && lsd_passes == 2 && !last;
        const int next_shift = shift + bits;
        const uint32_t next_mask = rec_digit_out ? (1u << (span - bits)) - 1u : 0u;  // two passes: the other one's bits
        const char* hist_name = sizeof(K) == 8 ? "radix_hist_u64" : "radix_hist_u32";
        if (rec_in)
            HIDEGS_LAUNCH(hist_name, (radix_hist_kernel<K, true>), dim3(nt), dim3(kBlock), 0, stream,
                          reinterpret_cast<const K*>(src_v), n, shift, mask, nt, counts, zero_jobs,
                          zero_jobs ? q.job_cap + Q_WORDS / 4 : 0u);
        else
            HIDEGS_LAUNCH(hist_name, radix_hist_kernel<K>, dim3(nt), dim3(kBlock), 0, stream, src_k, n, shift, mask, nt,
                          counts, zero_jobs, zero_jobs ? q.job_cap + Q_WORDS / 4 : 0u);
        // digits above `mask` never occur: their (stale) totals only follow the used digits in the
        // scatter's exclusive scan, and their counts are never read
        const bool low = segmented && last && lsd_passes == 2;  // the previous pass's digit bases, for the starts
        HIDEGS_LAUNCH("radix_digit_scan", radix_digit_scan_kernel, dim3(mask + 1), dim3(kBlock), 0, stream, counts,
                      nt, totals, low ? totals_pass[0] : nullptr, low ? 1 << pass_bits[0] : 0, low_base);
        if (p < 2) pass_bits[p] = bits;
        // narrow digits (and, for the starts, a narrower previous pass: the passes are balanced, so
        // pass_bits[0] <= bits) take the smaller-LDS instance
        const bool with_starts = segmented && last;  // also the segments' first positions (no pass over the sorted keys)
        const int b0 = with_starts && lsd_passes == 2 ? pass_bits[0] : 0;
        const bool narrow = (int)mask < kNarrowRadix && n <= kNarrowMaxN && (1 << b0) <= kNarrowRadix;
        const char* scatter_name = sizeof(K) == 8 ? "radix_scatter_u64" : "radix_scatter_u32";
#define HIDEGS_SCATTER(...)                                                                                            \
    HIDEGS_LAUNCH(scatter_name, (radix_scatter_kernel<K, __VA_ARGS__>), dim3(nt), dim3(kSBlock), 0, stream, src_k, src_v, \
                  dk, dv, n, shift, mask, nt, counts, totals, with_starts ? low_base : nullptr, b0,                       \
                  with_starts ? seg_starts : nullptr, next_shift, next_mask)
        if (rec_in) {  // tile ids are whole high key halves (the caller's guarantee): 8-byte records
            if (narrow) HIDEGS_SCATTER(true, kNarrowRadix, kOutRecords, true);
            else HIDEGS_SCATTER(true, kRadix, kOutRecords, true);
        } else if (rec_digit_out) {
            if (narrow) HIDEGS_SCATTER(false, kNarrowRadix, kOutRecordsDigit);
            else HIDEGS_SCATTER(false, kRadix, kOutRecordsDigit);
        } else if (with_starts && packed) {  // one pass
            if (narrow) HIDEGS_SCATTER(true, kNarrowRadix, kOutRecords);
            else HIDEGS_SCATTER(true, kRadix, kOutRecords);
        } else if (with_starts) {
            if (narrow) HIDEGS_SCATTER(true, kNarrowRadix);
            else HIDEGS_SCATTER(true, kRadix);
        } else {
            if (narrow) HIDEGS_SCATTER(false, kNarrowRadix);
            else HIDEGS_SCATTER(false, kRadix);
        }
#undef HIDEGS_SCATTER
        src_k = dk;
        src_v = dv;
        shift += bits;
    }
    if (segmented) {
        uint64_t* ko = reinterpret_cast<uint64_t*>(keys_out);
        if (packed && n <= kThroughMaxN)
            HIDEGS_LAUNCH("segment_sort", (segment_sort_kernel<true, kThrough>), dim3(nseg + kScouts), dim3(kBlock), 0,
                          stream, ko, vals_out, seg_starts, ranges_out, nseg, q);
        else if (packed)
            HIDEGS_LAUNCH("segment_sort", segment_sort_kernel<true>, dim3(nseg + kScouts), dim3(kBlock), 0, stream, ko,
                          vals_out, seg_starts, ranges_out, nseg, q);
        else
            HIDEGS_LAUNCH("segment_sort", segment_sort_kernel<false>, dim3(nseg + kScouts), dim3(kBlock), 0, stream, ko,
                          vals_out, seg_starts, ranges_out, nseg, q);
        HIDEGS_LAUNCH("big_segments", big_segment_kernel, dim3(kQueueBlocks), dim3(kBlock), 0, stream, ko, vals_out,
                      reinterpret_cast<uint64_t*>(alt_k), alt_v, q);
        // debug mode checks this call's queue itself (below); otherwise the last kernel hands a queue
        // error to the mapped host word, which fails the next entry-point call
        const bool debug = debug_enabled();
        uint32_t* async_err = debug ? nullptr : async_error_slot(stream);
        // piece_sort_kernel is the sort's last kernel: it reports the queue's error
        HIDEGS_LAUNCH("piece_sort", piece_sort_kernel, dim3(kPieceBlocks), dim3(kBlock), 0, stream, ko, vals_out,
                      reinterpret_cast<const uint64_t*>(alt_k), alt_v, q, async_err);
        if (debug) {  // debug mode: this call's own queue error word (in its scratch), after the grid has drained
            if (int rc = check_launch(what, stream, 1)) return rc;
            uint32_t err = 0;
            if (hipMemcpyAsync(&err, q.ctl + kCtlStride * Q_ERROR, sizeof(err), hipMemcpyDeviceToHost, stream) !=
                    hipSuccess ||
                hipStreamSynchronize(stream) != hipSuccess)
                return fail(HIDEGS_E_HIP, std::string(what) + ": queue error readback failed");
            if (err)
                return fail(HIDEGS_E_HIP, std::string(what) + ": hot-tile partition queue error " + std::to_string(err) +
                                              ((err & 1u) ? " (job slots exhausted)" : "") +
                                              ((err & 4u) ? " (a worker gave up waiting)" : "") +
                                              ": the output is not sorted");
        }
    } else if (ranges_out) {
        if (int rc = check_launch(what, stream, 0)) return rc;
        return identify_tile_ranges(reinterpret_cast<const uint64_t*>(keys_out), n,
                                    reinterpret_cast<uint32_t*>(ranges_out), num_tiles, stream);
    }
    return check_launch(what, stream, 0);
}

}  // namespace

// Reads (clear: exchanges with 0) the sticky word in one device-side atomic, so an error raised
// between a read and a separate clear cannot be lost.
__device__ uint32_t g_queue_error_read;
__global__ void queue_error_take_kernel(int clear)
{
    g_queue_error_read = clear ? __hip_atomic_exchange(&g_queue_error, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                               : __hip_atomic_load(&g_queue_error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int queue_error(hipStream_t stream, int clear, uint32_t* flags)
{
    // one reader at a time: g_queue_error_read is a single word per device
    static std::mutex m;
    std::lock_guard<std::mutex> lock(m);
    uint32_t v = 0;
    hipLaunchKernelGGL(queue_error_take_kernel, dim3(1), dim3(1), 0, stream, clear);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyFromSymbolAsync(&v, HIP_SYMBOL(g_queue_error_read), sizeof(v), 0, hipMemcpyDeviceToHost, stream) !=
            hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return fail(HIDEGS_E_HIP, "queue_error: readback failed");
    // the asynchronous copy of the same failures on this stream: reported here and taken with the clear
    if (clear) v |= take_async_bits(stream);
    *flags = v;
    return 0;
}

int inclusive_scan_u32(void* scratch, size_t scratch_bytes, const uint32_t* in, uint32_t* out, long long n,
                       hipStream_t stream)
{
    if (n < 0) return fail(HIDEGS_E_ARG, "inclusive_scan_u32: negative size");
    if (n == 0) return 0;
    if (!in || !out) return fail(HIDEGS_E_ARG, "inclusive_scan_u32: NULL pointer");
    if (!scratch || scratch_bytes < scan_scratch(n)) return fail(HIDEGS_E_ARG, "inclusive_scan_u32: scratch too small");
    const int nt = ceil_div(n, kDevScanTile);
    Carver c(scratch);
    uint32_t* sums = c.take<uint32_t>(nt);
    HIDEGS_LAUNCH("scan_reduce", scan_reduce_kernel, dim3(nt), dim3(kBlock), 0, stream, in, n, sums);
    const int own = nt <= kOwnOffsetTiles;
    if (!own)
        HIDEGS_LAUNCH("scan_small", scan_small_kernel, dim3(1), dim3(kBlock), 0, stream, sums, nt, (uint32_t*)nullptr);
    HIDEGS_LAUNCH("scan_downsweep", scan_downsweep_kernel, dim3(nt), dim3(kBlock), 0, stream, in, n, sums, own, out);
    return check_launch("inclusive_scan_u32", stream, 0);
}

size_t inclusive_scan_scratch(long long n) { return scan_scratch(n); }
size_t sort_u64_scratch(long long n) { return sort_scratch<uint64_t>(n); }
size_t sort_u32_scratch(long long n) { return sort_scratch<uint32_t>(n); }

int sort_pairs_u64(void* scratch, size_t bytes, const uint64_t* ki, uint64_t* ko, const uint32_t* vi, uint32_t* vo,
                   long long n, int b, int e, hipStream_t s)
{
    return sort_pairs<uint64_t>(scratch, bytes, ki, ko, vi, vo, n, b, e, s, "sort_pairs_u64");
}
int sort_pairs_u32(void* scratch, size_t bytes, const uint32_t* ki, uint32_t* ko, const uint32_t* vi, uint32_t* vo,
                   long long n, int b, int e, hipStream_t s)
{
    return sort_pairs<uint32_t>(scratch, bytes, ki, ko, vi, vo, n, b, e, s, "sort_pairs_u32");
}

int sort_tile_pairs(void* scratch, size_t bytes, const uint64_t* ki, uint64_t* ko, const uint32_t* vi, uint32_t* vo,
                    long long n, int num_tiles, uint32_t* ranges, hipStream_t s)
{
    if (num_tiles < 1) return fail(HIDEGS_E_ARG, "sort_tile_pairs: num_tiles must be >= 1");
    if (!ranges) return fail(HIDEGS_E_ARG, "sort_tile_pairs: NULL ranges");
    const int end = 32 + (int)(32u - (uint32_t)__builtin_clz((uint32_t)num_tiles | 1u));  // 32 + getHigherMsb
    if (end > 64) return fail(HIDEGS_E_ARG, "sort_tile_pairs: too many tiles");
    return sort_pairs<uint64_t>(scratch, bytes, ki, ko, vi, vo, n, 0, end, s, "sort_tile_pairs",
                                reinterpret_cast<uint2*>(ranges), num_tiles);
}

int identify_tile_ranges(const uint64_t* keys, long long n, uint32_t* ranges, int num_tiles, hipStream_t stream)
{
    if (n < 0 || num_tiles < 0) return fail(HIDEGS_E_ARG, "identify_tile_ranges: negative size");
    if (num_tiles > 0 && !ranges) return fail(HIDEGS_E_ARG, "identify_tile_ranges: NULL ranges");
    if (num_tiles > 0 && hipMemsetAsync(ranges, 0, (size_t)num_tiles * 2 * sizeof(uint32_t), stream) != hipSuccess)
        return fail(HIDEGS_E_HIP, "identify_tile_ranges: memset failed");
    if (n == 0) return check_launch("identify_tile_ranges", stream, 0);
    if (!keys) return fail(HIDEGS_E_ARG, "identify_tile_ranges: NULL keys");
    HIDEGS_LAUNCH("identify_ranges", identify_ranges_kernel, dim3(ceil_div(n, kBlock * kRangeKeys)), dim3(kBlock), 0, stream, keys, n,
                       reinterpret_cast<uint2*>(ranges), (uint32_t)num_tiles, 0xffffffffu);
    return check_launch("identify_tile_ranges", stream, 0);
}

}  // namespace hidegs

// ============================== C ABI ==========================================
extern "C" {

size_t hidegs_scan_scratch_bytes(long long n) { return n > 0 ? hidegs::inclusive_scan_scratch(n) : 0; }
int hidegs_inclusive_scan_u32(void* scratch, size_t scratch_bytes, const uint32_t* in, uint32_t* out, long long n,
                              void* stream)
{
    if (int rc = hidegs::take_async_error("hidegs_inclusive_scan_u32", hidegs::as_stream(stream))) return rc;
    return hidegs::inclusive_scan_u32(scratch, scratch_bytes, in, out, n, hidegs::as_stream(stream));
}

size_t hidegs_sort_pairs_u64_scratch_bytes(long long n) { return n > 0 ? hidegs::sort_u64_scratch(n) : 0; }
int hidegs_sort_pairs_u64(void* scratch, size_t scratch_bytes, const uint64_t* keys_in, uint64_t* keys_out,
                          const uint32_t* vals_in, uint32_t* vals_out, long long n, int begin_bit, int end_bit,
                          void* stream)
{
    if (int rc = hidegs::take_async_error("hidegs_sort_pairs_u64", hidegs::as_stream(stream))) return rc;
    return hidegs::sort_pairs_u64(scratch, scratch_bytes, keys_in, keys_out, vals_in, vals_out, n, begin_bit, end_bit,
                                  hidegs::as_stream(stream));
}

size_t hidegs_sort_pairs_u32_scratch_bytes(long long n) { return n > 0 ? hidegs::sort_u32_scratch(n) : 0; }
int hidegs_sort_pairs_u32(void* scratch, size_t scratch_bytes, const uint32_t* keys_in, uint32_t* keys_out,
                          const uint32_t* vals_in, uint32_t* vals_out, long long n, int begin_bit, int end_bit,
                          void* stream)
{
    if (int rc = hidegs::take_async_error("hidegs_sort_pairs_u32", hidegs::as_stream(stream))) return rc;
    return hidegs::sort_pairs_u32(scratch, scratch_bytes, keys_in, keys_out, vals_in, vals_out, n, begin_bit, end_bit,
                                  hidegs::as_stream(stream));
}

int hidegs_sort_tile_pairs(void* scratch, size_t scratch_bytes, const uint64_t* keys_in, uint64_t* keys_out,
                           const uint32_t* vals_in, uint32_t* vals_out, long long n, int num_tiles, uint32_t* ranges,
                           void* stream)
{
    if (int rc = hidegs::take_async_error("hidegs_sort_tile_pairs", hidegs::as_stream(stream))) return rc;
    return hidegs::sort_tile_pairs(scratch, scratch_bytes, keys_in, keys_out, vals_in, vals_out, n, num_tiles, ranges,
                                   hidegs::as_stream(stream));
}

int hidegs_identify_tile_ranges(const uint64_t* sorted_keys, long long n, uint32_t* ranges, int num_tiles,
                                void* stream)
{
    if (int rc = hidegs::take_async_error("hidegs_identify_tile_ranges", hidegs::as_stream(stream))) return rc;
    return hidegs::identify_tile_ranges(sorted_keys, n, ranges, num_tiles, hidegs::as_stream(stream));
}

int hidegs_queue_error(void* stream, int clear, uint32_t* flags)
{
    if (!flags) return hidegs::fail(HIDEGS_E_ARG, "hidegs_queue_error: NULL flags");
    return hidegs::queue_error(hidegs::as_stream(stream), clear, flags);
}

uint32_t hidegs_higher_msb(uint32_t n)
{
    // Number of bits needed to hold n, at least 1 -- the value getHigherMsb's
    // binary search (rasterizer_impl.cu:35-50) returns for every u32 input.
    uint32_t bits = 32u - (uint32_t)__builtin_clz(n | 1u);
    return bits;
}

#ifdef HIDEGS_QUEUE_TRACE
// experiments only: copy out (and reset) the partition queue's traces; each returns its job count
int hidegs_debug_wide_trace(unsigned long long* host, int max_jobs)
{
    return hidegs::trace_take(hidegs::g_wtrace, hidegs::g_wtrace_n, host, max_jobs);
}

int hidegs_debug_queue_trace(unsigned long long* host, int max_jobs)
{
    return hidegs::trace_take(hidegs::g_qtrace, hidegs::g_qtrace_n, host, max_jobs);
}
#endif
}  // extern "C"
