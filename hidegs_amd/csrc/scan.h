// scan.h -- the inclusive scan's kernels: load_tile_u32, scan_reduce_kernel, scan_downsweep_kernel.
// Included by primitives.hip inside namespace hidegs::{anonymous}, after block_scan.h, common.h and the shared
// constants (kBlock, kWavesPerBlock).
#pragma once

// ============================== scan ===========================================
constexpr int kDevScanItems = 16;  // u32 items per thread of a scan tile
constexpr int kDevScanTile = kBlock * kDevScanItems;

// Loads one tile of u32 (striped 16-byte loads) and leaves it in LDS.
__device__ __forceinline__ void load_tile_u32(const uint32_t* in, long long base, long long n,
                                              uint32_t* s_tile)
{
    const int t = threadIdx.x;
    if (base + kDevScanTile <= n && ((reinterpret_cast<uintptr_t>(in) & 15) == 0)) {
        const uint4* src = reinterpret_cast<const uint4*>(in + base);
#pragma unroll
        for (int j = 0; j < kDevScanItems / 4; j++) {
            uint4 v = src[j * kBlock + t];
            reinterpret_cast<uint4*>(s_tile)[j * kBlock + t] = v;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kDevScanItems; j++) {
            long long i = base + j * kBlock + t;
            s_tile[j * kBlock + t] = (i < n) ? in[i] : 0u;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kBlock) void scan_reduce_kernel(const uint32_t* __restrict__ in, long long n,
                                                             uint32_t* __restrict__ tile_sums)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_tile[kDevScanTile];
    __shared__ uint32_t s_wave[kWavesPerBlock];
    const long long base = (long long)blockIdx.x * kDevScanTile;
    load_tile_u32(in, base, n, s_tile);
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < kDevScanItems; j++) sum += s_tile[threadIdx.x * kDevScanItems + j];
    uint32_t total;
    block_exclusive_scan(sum, s_wave, &total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// in and out may alias (in-place scan): each workgroup reads its whole tile before writing it.
// With `sums_raw` the workgroup adds up the tile sums before it itself (up to kOwnOffsetTiles
// tiles: a few loads per thread), which saves the separate scan of the tile sums; otherwise
// tile_offsets holds that exclusive scan.
constexpr int kOwnOffsetTiles = 4096;
__global__ __launch_bounds__(kBlock) void scan_downsweep_kernel(const uint32_t* in, long long n,
                                                                const uint32_t* __restrict__ tile_offsets,
                                                                int sums_raw, uint32_t* out)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_tile[kDevScanTile];
    __shared__ uint32_t s_wave[kWavesPerBlock];
    const long long base = (long long)blockIdx.x * kDevScanTile;
    uint32_t tile_off;
    if (sums_raw) {
        uint32_t part = 0;
        for (int i = threadIdx.x; i < (int)blockIdx.x; i += kBlock) part += tile_offsets[i];
        block_exclusive_scan(part, s_wave, &tile_off);
    } else {
        tile_off = tile_offsets[blockIdx.x];
    }
    load_tile_u32(in, base, n, s_tile);
    uint32_t v[kDevScanItems];
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < kDevScanItems; j++) {
        v[j] = s_tile[threadIdx.x * kDevScanItems + j];
        sum += v[j];
    }
    uint32_t total;
    uint32_t run = block_exclusive_scan(sum, s_wave, &total) + tile_off;
#pragma unroll
    for (int j = 0; j < kDevScanItems; j++) {
        run += v[j];
        s_tile[threadIdx.x * kDevScanItems + j] = run;  // inclusive
    }
    __syncthreads();
    if (base + kDevScanTile <= n && ((reinterpret_cast<uintptr_t>(out) & 15) == 0)) {
        uint4* dst = reinterpret_cast<uint4*>(out + base);
#pragma unroll
        // (as kStream stream_stores: level, 149.3-149.8 against 149.2-150.8 us per step, profiles/r13_store_policy.md)
        for (int j = 0; j < kDevScanItems / 4; j++) dst[j * kBlock + threadIdx.x] = reinterpret_cast<uint4*>(s_tile)[j * kBlock + threadIdx.x];
    } else {
#pragma unroll
        for (int j = 0; j < kDevScanItems; j++) {
            long long i = base + j * kBlock + threadIdx.x;
            if (i < n) out[i] = s_tile[j * kBlock + threadIdx.x];
        }
    }
}
