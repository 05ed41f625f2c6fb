// knn_stats.h -- HIDEGS_KNN_STATS builds only (tools/knn_stats.py): distCUDA2's phase-1 search statistics,
// one trace row per wave, and their copy-out and report.  The product build sees only the empty hooks at
// the end.  Included by knn.hip before its kernels.
#pragma once

#include "common.h"

#ifdef HIDEGS_KNN_STATS
#include <algorithm>
#include <cstdio>
#include <vector>
#endif

namespace hidegs {
namespace {

#ifdef HIDEGS_KNN_STATS
// The statistics block follows the counters in the caller's scratch, one carving step (kAlign) behind them
// (layout() in knn.hip): this header, then 4 u64 per leaf {start, end (s_memrealtime ticks), leaves, points}.
struct KnnStats {
    unsigned long long coarse;  // candidate leaves evaluated
    unsigned long long fine;    // candidate points evaluated
    uint32_t max_coarse, max_fine;
    uint32_t bailed;            // waves that took the bail-out
    uint32_t pad;
    uint32_t hist[8];           // waves by candidate leaves: <16, <32, <64, <128, <256, <512, <1024, more
};
static_assert(sizeof(KnnStats) <= kAlign, "the trace rows start one carving step behind the header");

inline size_t knn_stats_bytes(int nleaves) { return kAlign + sizeof(unsigned long long) * 4 * (size_t)nleaves; }

// One wave's tallies; lane 0 adds them to the block when the wave's walk is over.
struct WaveStats {
    unsigned long long t_start;
    uint32_t coarse = 0, fine = 0;
    bool bailed = false;
    __device__ WaveStats() : t_start(__builtin_amdgcn_s_memrealtime()) {}
    __device__ void leaf() { coarse++; }
    __device__ void points(uint64_t mask) { fine += (uint32_t)__popcll(mask); }
    __device__ void bail() { bailed = true; }
    __device__ void report(void* counters, int L, int lane) const
    {
        if (lane != 0) return;
        KnnStats* s = reinterpret_cast<KnnStats*>(static_cast<char*>(counters) + kAlign);
        unsigned long long* row = reinterpret_cast<unsigned long long*>(s) + kAlign / sizeof(unsigned long long) + 4 * (size_t)L;
        atomicAdd(&s->coarse, (unsigned long long)coarse);
        atomicAdd(&s->fine, (unsigned long long)fine);
        atomicMax(&s->max_coarse, coarse);
        atomicMax(&s->max_fine, fine);
        if (bailed) atomicAdd(&s->bailed, 1u);
        int bk = 0;
        while (bk < 7 && coarse >= (16u << bk)) bk++;
        atomicAdd(&s->hist[bk], 1u);
        row[0] = t_start;
        row[1] = __builtin_amdgcn_s_memrealtime();
        row[2] = coarse;
        row[3] = fine;
    }
};

// Waits for `stream`, copies the counters and the block out and prints the two reports to stderr.
inline void knn_stats_report(const void* counters, int P, int nleaves, int nsuper, hipStream_t stream)
{
    std::vector<unsigned long long> h((kAlign + knn_stats_bytes(nleaves)) / sizeof(unsigned long long));
    if (hipMemcpyAsync(h.data(), counters, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) {
        fprintf(stderr, "[hidegs knn] statistics copy-out failed\n");
        return;
    }
    const uint32_t hard = *reinterpret_cast<const uint32_t*>(h.data());
    const KnnStats& s = *reinterpret_cast<const KnnStats*>(h.data() + kAlign / sizeof(h[0]));
    const unsigned long long* rows = h.data() + 2 * kAlign / sizeof(h[0]);
    fprintf(stderr, "[hidegs knn] P=%d leaves=%d supers=%d hard=%u bailed=%u coarse_leaves/wave=%.2f (max %u) "
            "points/wave=%.2f (max %u) hist<16,32,64,128,256,512,1024,more: %u %u %u %u %u %u %u %u\n",
            P, nleaves, nsuper, hard, s.bailed, (double)s.coarse / nleaves, s.max_coarse, (double)s.fine / nleaves,
            s.max_fine, s.hist[0], s.hist[1], s.hist[2], s.hist[3], s.hist[4], s.hist[5], s.hist[6], s.hist[7]);
    // the memrealtime counter runs at 100 MHz: 100 ticks per microsecond
    unsigned long long t0 = ~0ull, t1 = 0;
    std::vector<double> dur;
    for (int i = 0; i < nleaves; i++)
        if (rows[4 * i + 1]) {
            t0 = std::min(t0, rows[4 * i]);
            t1 = std::max(t1, rows[4 * i + 1]);
            dur.push_back((double)(rows[4 * i + 1] - rows[4 * i]));
        }
    if (dur.empty()) return;
    std::sort(dur.begin(), dur.end());
    auto pct = [&](double q) { return dur[(size_t)(q * (dur.size() - 1))] / 100.0; };
    double sum = 0;
    for (double d : dur) sum += d;
    const double span = (double)std::max(1ull, t1 - t0);
    fprintf(stderr, "[hidegs knn trace] waves=%zu span=%.1f us sum=%.1f us avg-concurrency=%.1f "
            "dur us p50=%.2f p90=%.2f p99=%.2f p999=%.2f max=%.2f\n", dur.size(), span / 100.0, sum / 100.0, sum / span,
            pct(0.5), pct(0.9), pct(0.99), pct(0.999), pct(1.0));
    int bins[10] = {0};  // waves started per tenth of the span
    for (int i = 0; i < nleaves; i++)
        if (rows[4 * i + 1]) bins[std::min(9, (int)(10.0 * (rows[4 * i] - t0) / span))]++;
    fprintf(stderr, "[hidegs knn trace] starts per tenth: %d %d %d %d %d %d %d %d %d %d\n", bins[0], bins[1], bins[2],
            bins[3], bins[4], bins[5], bins[6], bins[7], bins[8], bins[9]);
}
#else
inline size_t knn_stats_bytes(int) { return 0; }
struct WaveStats {
    __device__ void leaf() {}
    __device__ void points(uint64_t) {}
    __device__ void bail() {}
    __device__ void report(void*, int, int) const {}
};
inline void knn_stats_report(const void*, int, int, int, hipStream_t) {}
#endif

}  // namespace
}  // namespace hidegs
