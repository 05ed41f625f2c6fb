// queue_trace.h -- HIDEGS_QUEUE_TRACE builds only (tools/queue_trace.py): the partition queue's per-job
// timestamps, WSTAMP for the WIDE job's phases, and their copy-out.
// Included by primitives.hip inside namespace hidegs::{anonymous}, before hot_queue.h.
#pragma once

#ifdef HIDEGS_QUEUE_TRACE
constexpr unsigned int kQTraceCap = 32768;
__device__ unsigned long long g_qtrace[kQTraceCap][4];  // (type | block << 8 | index << 32, claimed, started, ended)
__device__ unsigned int g_qtrace_n;
constexpr int kWTraceCap = 4096;
__device__ unsigned long long g_wtrace[kWTraceCap][9];  // WIDE jobs: m, then 8 phase timestamps
__device__ unsigned int g_wtrace_n;
#define WSTAMP(k) do { if (threadIdx.x == 0 && wslot < kWTraceCap) g_wtrace[wslot][1 + (k)] = wall_clock64(); } while (0)

// Copies a trace's first min(count, max_jobs) rows to host and resets the count; returns the number
// of rows copied, or -1.
template <typename Rows>
int trace_take(const Rows& rows, unsigned int& count, unsigned long long* host, int max_jobs)
{
    unsigned int n = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(&n, HIP_SYMBOL(count), sizeof(n)) != hipSuccess)
        return -1;
    const int m = (int)(n < (unsigned)max_jobs ? n : (unsigned)max_jobs);
    if (m > 0 && hipMemcpyFromSymbol(host, HIP_SYMBOL(rows), (size_t)m * sizeof(rows[0])) != hipSuccess) return -1;
    n = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(count), &n, sizeof(n)) != hipSuccess) return -1;
    return m;
}
#else
#define WSTAMP(k) do { } while (0)
#endif
