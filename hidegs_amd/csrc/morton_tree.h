// morton_tree.h -- the structure that distCUDA2 (knn.hip) and the nearest-point index (nearest.hip) both build
// over a (P,3) fp32 cloud and search, written once:
//   1. bounding box (grid-stride partial min/max + one finishing workgroup), no host read;
//   2. 48-bit Morton keys, kMortonBits = 16 bits per axis, relative to the box (the frame);
//   3. stable radix sort of (key, row) pairs (sort_pairs_u64; SortLayout carves its arrays);
//   4. the rows gathered into sorted float4 {x, y, z, bits(row)} -- the gather kernels stay in their files,
//      since they write different things beside the points;
//   5. AABBs over leaves of kLeaf = 64 sorted points (one wave64) and super-boxes of kFan = 64 leaves.
// The searches prune with box_point_lb and box_box_lb: sqdist's own monotone expression applied to
// componentwise smaller gaps, so a bound never exceeds the distance of any point in the box, rounding included.
// Both files' exactness arguments rest on these three being one form; this is the only place they are written.
//
// The build kernels are templates over a tag type that each file defines in its own namespace:
//   static constexpr bool kNonFiniteLast
//       true (nearest): a row with a non-finite coordinate widens no box and takes kLastKey, which every other
//       row's key is kept below: such rows sort strictly last;
//       false (distCUDA2): every row is keyed and boxed as it is -- fminf/fmaxf drop a NaN, the key's clamp
//       sends it to 0 -- which reproduces the reference's behaviour.
// The tag also keeps the two instantiations' kernel symbols apart.
#pragma once
#include <float.h>

#include "common.h"

namespace hidegs {

constexpr int kLeaf = 64;  // points per leaf
constexpr int kFan = 64;   // leaves per super-box
// Per axis; the sort runs over all 3x these bits.  10 bits sort in 4 passes instead of 6 but the coarser
// order costs the search as much; a sort over the high bits only loses the dense region of a cloud whose
// outliers inflate the bounding box.
constexpr int kMortonBits = 16;
constexpr int kBoundBlocks = 1024;
constexpr int kTreeBlock = 256;                // threads of a build workgroup
constexpr int kTreeWaves = kTreeBlock / kWave;  // 4 waves = 4 leaves or super-boxes per workgroup
constexpr uint64_t kLastKey = 0xffffffffffffull;  // the largest key: kNonFiniteLast's non-finite rows
static_assert(kLeaf == kWave, "one lane per point of a leaf");

struct Box {
    float4 lo, hi;
};

// ---- geometry ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float sqdist(float4 q, float4 c)
{
    const float dx = c.x - q.x, dy = c.y - q.y, dz = c.z - q.z;
    return fmaf(dz, dz, fmaf(dx, dx, dy * dy));
}

// Lower bound of sqdist(q, c) over c in the box, same monotone expression as sqdist.
__device__ __forceinline__ float box_point_lb(const Box& b, float4 q)
{
    const float gx = fmaxf(fmaxf(b.lo.x - q.x, q.x - b.hi.x), 0.f);
    const float gy = fmaxf(fmaxf(b.lo.y - q.y, q.y - b.hi.y), 0.f);
    const float gz = fmaxf(fmaxf(b.lo.z - q.z, q.z - b.hi.z), 0.f);
    return fmaf(gz, gz, fmaf(gx, gx, gy * gy));
}

// Lower bound over every query in the AABB [qlo, qhi] and every point of the box.
__device__ __forceinline__ float box_box_lb(const Box& b, float4 qlo, float4 qhi)
{
    const float gx = fmaxf(fmaxf(b.lo.x - qhi.x, qlo.x - b.hi.x), 0.f);
    const float gy = fmaxf(fmaxf(b.lo.y - qhi.y, qlo.y - b.hi.y), 0.f);
    const float gz = fmaxf(fmaxf(b.lo.z - qhi.z, qlo.z - b.hi.z), 0.f);
    return fmaf(gz, gz, fmaf(gx, gx, gy * gy));
}

// ---- keys -------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t spread3(uint32_t v)
{
    // bit i of v -> bit 3i (v < 2^21)
    uint64_t x = v & 0x1fffffu;
    x = (x | (x << 32)) & 0x001f00000000ffffull;
    x = (x | (x << 16)) & 0x001f0000ff0000ffull;
    x = (x | (x << 8)) & 0x100f00f00f00f00full;
    x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

// Morton key of a position in the frame {lo.xyz, scale.xyz}, clamped into the box; a NaN goes to 0 (fmaxf).
// The key orders; it decides no result.
__device__ __forceinline__ uint64_t morton_key(float x, float y, float z, const float* __restrict__ frame)
{
    const float qmax = (float)((1u << kMortonBits) - 1u);
    const float v[3] = {x, y, z};
    uint64_t code = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        float t = (v[a] - frame[a]) * frame[3 + a];
        t = fminf(fmaxf(t, 0.f), qmax);
        code |= spread3((uint32_t)t) << a;
    }
    return code;
}

// ---- build kernels ----------------------------------------------------------------------------------------
// Workgroup minimum and maximum per axis: thread a < 3 receives axis a's in (l, h).  (Indexing lo[] and hi[]
// by the thread index instead would make the compiler move both arrays to LDS, 6 KiB a workgroup.)
__device__ __forceinline__ void block_minmax(float (&lo)[3], float (&hi)[3], float (*s)[6], float& l, float& h)
{
    const int wave = threadIdx.x / kWave;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = wave_min(lo[a]);
        hi[a] = wave_max(hi[a]);
    }
    if (lane_id() == 0)
        for (int a = 0; a < 3; a++) {
            s[wave][a] = lo[a];
            s[wave][3 + a] = hi[a];
        }
    __syncthreads();
    l = FLT_MAX, h = -FLT_MAX;
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        for (int w = 0; w < kTreeWaves; w++) {
            l = fminf(l, s[w][a]);
            h = fmaxf(h, s[w][3 + a]);
        }
    }
}

// partials[6 b ..] = {lo.xyz, hi.xyz} of the rows that workgroup b strides over.
template <class Tree>
__global__ __launch_bounds__(kTreeBlock) void tree_bounds_kernel(const float* __restrict__ pts, long long P,
                                                                 float* __restrict__ partials)
{
    __shared__ float s[kTreeWaves][6];
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (long long i = (long long)blockIdx.x * kTreeBlock + threadIdx.x; i < P; i += (long long)gridDim.x * kTreeBlock) {
        const float v[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        if (Tree::kNonFiniteLast && !finite3(v[0], v[1], v[2])) continue;  // no candidate: it widens nothing
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo[a] = fminf(lo[a], v[a]);
            hi[a] = fmaxf(hi[a], v[a]);
        }
    }
    float l, h;
    block_minmax(lo, hi, s, l, h);
    if (threadIdx.x < 3) {
        partials[blockIdx.x * 6 + threadIdx.x] = l;
        partials[blockIdx.x * 6 + 3 + threadIdx.x] = h;
    }
}

// frame = {lo.x, lo.y, lo.z, scale.x, scale.y, scale.z}
template <class Tree>
__global__ __launch_bounds__(kTreeBlock) void tree_frame_kernel(const float* __restrict__ partials, int nparts,
                                                                float* __restrict__ frame)
{
    __shared__ float s[kTreeWaves][6];
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int b = threadIdx.x; b < nparts; b += kTreeBlock)
        for (int a = 0; a < 3; a++) {
            lo[a] = fminf(lo[a], partials[b * 6 + a]);
            hi[a] = fmaxf(hi[a], partials[b * 6 + 3 + a]);
        }
    float l, h;
    block_minmax(lo, hi, s, l, h);
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        const float ext = h - l;  // negative without a row in the box
        const float q = (float)((1u << kMortonBits) - 1u);
        frame[a] = l;
        frame[3 + a] = (ext > 0.f && ext < INFINITY) ? q / ext : 0.f;
    }
}

template <class Tree>
__global__ __launch_bounds__(kTreeBlock) void tree_point_keys_kernel(const float* __restrict__ pts, long long P,
                                                                     const float* __restrict__ frame,
                                                                     uint64_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const long long i = (long long)blockIdx.x * kTreeBlock + threadIdx.x;
    if (i >= P) return;
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (Tree::kNonFiniteLast)
        keys[i] = finite3(x, y, z) ? min(morton_key(x, y, z, frame), kLastKey - 1) : kLastKey;
    else
        keys[i] = morton_key(x, y, z, frame);
    vals[i] = (uint32_t)i;
}

// One wave per super-box: the AABB of its kFan leaf boxes.
template <class Tree>
__global__ __launch_bounds__(kTreeBlock) void tree_super_kernel(const Box* __restrict__ leaves, long long nleaves, int nsuper,
                                                                Box* __restrict__ supers)
{
    const int S = blockIdx.x * kTreeWaves + threadIdx.x / kWave;
    if (S >= nsuper) return;
    const long long l = (long long)S * kFan + lane_id();
    const Box b = l < nleaves ? leaves[l]
                              : Box{make_float4(FLT_MAX, FLT_MAX, FLT_MAX, 0.f), make_float4(-FLT_MAX, -FLT_MAX, -FLT_MAX, 0.f)};
    Box r;
    r.lo = make_float4(wave_min(b.lo.x), wave_min(b.lo.y), wave_min(b.lo.z), 0.f);
    r.hi = make_float4(wave_max(b.hi.x), wave_max(b.hi.y), wave_max(b.hi.z), 0.f);
    if (lane_id() == 0) supers[S] = r;
}

// ---- sort layout ------------------------------------------------------------------------------------------
// The arrays of one sort of n (key, row) pairs, carved in this order.
struct SortLayout {
    uint64_t *keys, *keys_sorted;
    uint32_t *vals, *vals_sorted;
    void* sort_tmp;
    size_t sort_bytes;
};

inline void sort_layout(Carver& c, long long n, SortLayout& l)
{
    l.keys = c.take<uint64_t>(n);
    l.keys_sorted = c.take<uint64_t>(n);
    l.vals = c.take<uint32_t>(n);
    l.vals_sorted = c.take<uint32_t>(n);
    l.sort_bytes = sort_u64_scratch(n);
    l.sort_tmp = c.take<char>(l.sort_bytes);
}

}  // namespace hidegs
