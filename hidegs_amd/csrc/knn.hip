// knn.hip -- distCUDA2 for gfx950: mean of the squared distances to the 3 nearest
// OTHER points, for every point of a (P,3) fp32 cloud.
//
// Contract replaced: distCUDA2 / SimpleKNN::knn (submodules/simple-knn/spatial.cu:15-25,
// simple_knn.cu:186-221).  Its result is an exact 3-NN quantity -- the box pruning of
// boxMeanDist (simple_knn.cu:148-184) only discards boxes whose lower-bound distance
// exceeds an upper bound of the 3rd-best distance -- so this file computes the same
// value with its own search.  The arithmetic that fixes the result bits follows the
// reference's definition: squared distance of (candidate - query), the three best
// initialised to FLT_MAX (so P <= 3 yields FLT_MAX / inf terms exactly as there,
// simple_knn.cu:155), a point never matches itself by index (duplicates count as
// distance 0, :159,178), result ((b0 + b1) + b2) / 3.0f (:183).  The squared distance
// d.x*d.x + d.y*d.y + d.z*d.z (:136) is evaluated as fmaf(dz,dz, fmaf(dx,dx, dy*dy)) on device and
// in the oracle: the contraction an LLVM-based CUDA compiler gives that expression (the left product
// of `a*b + c*d` fused; DESIGN.md "Parity").
//
// Search (MI355X-first).  Steps 1, 2 and 4, the distance and the lower bounds are morton_tree.h's, which
// the nearest-point index (nearest.hip) builds and prunes with as well:
//   1. bounding box (grid-stride partial min/max + one finishing workgroup) -- no host
//      sync; the reference does two blocking D2H copies (simple_knn.cu:194-201);
//   2. 48-bit Morton codes (16 bits/axis), stable LSD radix sort (primitives.hip);
//   3. points gathered into a sorted float4 array {x, y, z, original index};
//   4. leaves = 64 consecutive sorted points = exactly one wave64 of queries,
//      super-boxes = 64 leaves; AABBs for both;
//   5. phase 1: one wave per leaf.  The wave seeds its 64 queries from its own leaf
//      (candidates broadcast from LDS), sends outliers (3rd-best far above the wave's
//      mean, or unseeded) to a hard list, then walks super-boxes and leaves with the
//      wave AABB / wave upper bound as a coarse filter and each lane's own bound as a
//      fine filter (skip a leaf unless some lane can still improve);
//   6. phase 2: one wave per hard query, lanes cooperate over candidate points and
//      merge lane-local top-3 lists.
// Pruning compares a lower bound computed with the same monotone fp expression as the
// point distance, and prunes only when strictly greater than an upper bound of the
// 3rd-best: the result is exact for any distribution; the heuristics affect speed only.
#include <float.h>

#include <algorithm>

#include "common.h"
#include "knn_stats.h"
#include "morton_tree.h"

namespace hidegs {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;  // 4 waves = 4 leaves per workgroup
constexpr int kSub = 4;                 // sub-boxes per leaf (16 points each): the fine filter
constexpr float kHardFactor = 8.0f;     // 3rd-best above 8x the wave mean -> phase 2

// distCUDA2 keys and boxes every row as it is, as the reference does (morton_tree.h).
struct KnnTree {
    static constexpr bool kNonFiniteLast = false;
};

inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// Keep the three smallest values seen (a multiset, as updateKBest<3> does).  NaN never enters.
// Every value here is a non-negative float (a sum of squares, FLT_MAX or +inf), whose bit
// patterns order like unsigned integers: the min/max network runs on the bits, which spares the
// NaN-quieting canonicalisation that fminf/fmaxf of loop-carried values costs on gfx950.
// No NaN test is needed (dropping it: knn_leaf frustum 959 -> 896 us at 2M): the three best only decrease
// from FLT_MAX, and every NaN pattern -- and +inf -- is above FLT_MAX as an unsigned integer, so such a
// d leaves them unchanged exactly as the reference's `dist < best` (false for NaN and inf) does.
__device__ __forceinline__ void kbest(float d, float& b0, float& b1, float& b2)
{
    const uint32_t x = __float_as_uint(d);
    const uint32_t c0 = __float_as_uint(b0), c1 = __float_as_uint(b1), c2 = __float_as_uint(b2);
    const uint32_t t0 = min(c0, x), u0 = max(c0, x);
    const uint32_t t1 = min(c1, u0), u1 = max(c1, u0);
    b2 = __uint_as_float(min(c2, u1));
    b1 = __uint_as_float(t1);
    b0 = __uint_as_float(t0);
}

constexpr int kChunk = kLeaf / kSub;  // points per sub-box

// Evaluates the kChunk candidates held by lanes k0 .. k0 + kChunk of `c` (one point per lane) against
// query p: each candidate is broadcast with v_readlane into scalar registers, so the loop has no
// memory latency at all.  Candidates at or past `nvalid` and the query itself (lane `self`) enter as
// FLT_MAX, which leaves the three best unchanged exactly as skipping them would.
__device__ __forceinline__ void eval_lanes(float4 c, int k0, int nvalid, int self, float4 p, float& b0, float& b1,
                                           float& b2)
{
#pragma unroll
    for (int j = 0; j < kChunk; j++) {
        const int k = k0 + j;
        const float4 q = make_float4(uniform_lane(c.x, k), uniform_lane(c.y, k), uniform_lane(c.z, k), 0.f);
        const float d = sqdist(p, q);
        kbest((k < nvalid && k != self) ? d : FLT_MAX, b0, b1, b2);
    }
}

// ---- 3./4. gather into sorted order; leaf and super boxes ---------------------------------------
// Leaf L's box and its kSub sub-boxes of kLeaf / kSub consecutive points (the fine filter), from the
// wave holding the leaf's points (lane = point in leaf).
__device__ __forceinline__ void store_leaf_boxes(const float4 p, const bool valid, const int L, const int lane,
                                                 Box* __restrict__ leaves, Box* __restrict__ subs)
{
    float v[6] = {valid ? p.x : FLT_MAX,  valid ? p.y : FLT_MAX,  valid ? p.z : FLT_MAX,
                  valid ? p.x : -FLT_MAX, valid ? p.y : -FLT_MAX, valid ? p.z : -FLT_MAX};
    // reduce inside groups of kLeaf / kSub lanes, store the sub-box, then finish across groups
#pragma unroll
    for (int m = 1; m < kLeaf / kSub; m <<= 1)
#pragma unroll
        for (int a = 0; a < 6; a++) {
            const float o = __shfl_xor(v[a], m, kWave);
            v[a] = a < 3 ? fminf(v[a], o) : fmaxf(v[a], o);
        }
    if ((lane % (kLeaf / kSub)) == 0)
        subs[L * kSub + lane / (kLeaf / kSub)] = Box{make_float4(v[0], v[1], v[2], 0.f), make_float4(v[3], v[4], v[5], 0.f)};
#pragma unroll
    for (int m = kLeaf / kSub; m < kWave; m <<= 1)
#pragma unroll
        for (int a = 0; a < 6; a++) {
            const float o = __shfl_xor(v[a], m, kWave);
            v[a] = a < 3 ? fminf(v[a], o) : fmaxf(v[a], o);
        }
    if (lane == 0) leaves[L] = Box{make_float4(v[0], v[1], v[2], 0.f), make_float4(v[3], v[4], v[5], 0.f)};
}

// Sorted point j = original point order[j] as {x, y, z, bits(original index)}.  Wave w of block b holds
// leaf 4b + w (kLeaf == kWave) and also writes its boxes, without reading the sorted array again (a
// launch of its own for the boxes: distCUDA2 frustum 1138/1125 -> 1143/1146 us, uniform 1056/1026 -> 1066/1063).
__global__ __launch_bounds__(kBlock) void gather_kernel(const float* __restrict__ pts, const uint32_t* __restrict__ order,
                                                        int P, float4* __restrict__ sp, int nleaves,
                                                        Box* __restrict__ leaves, Box* __restrict__ subs)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    bool valid = false;
    if (j < P) {
        const uint32_t i = order[j];
        if (i < (uint32_t)P) {  // a permutation of [0, P) by construction
            p = make_float4(pts[3ll * i], pts[3ll * i + 1], pts[3ll * i + 2], __uint_as_float(i));
            sp[j] = p;
            valid = true;
        }
    }
    const int L = j / kLeaf;  // wave-uniform
    if (L >= nleaves) return;  // whole wave
    store_leaf_boxes(p, valid, L, lane_id(), leaves, subs);
}

// ---- 5. phase 1: one wave per leaf ------------------------------------------------------------
constexpr int kGroups = 2;      // query groups per wave for the coarse filter (4 and 8: more box tests, slower)
constexpr int kSuperBatch = 2;  // super-boxes tested per lane per batch
constexpr int kLeafBatch = 2;   // passing super-boxes whose leaf boxes load together
constexpr int kListCap = 256;   // candidate leaves buffered per wave
constexpr int kFlushBatch = 4;  // candidate leaves loaded together
constexpr int kGroupLanes = kWave / kGroups;
constexpr int kBailout = 256;   // candidate leaves after which a wave hands its queries to phase 2
// The walk appends a leaf box test's `cnt` passing leaves to the list only while the list's total stays
// at or below kBailout, and bails otherwise.  So the list never holds more than kBailout <= kListCap
// leaves: it needs no emptying during the walk, and is filled once and evaluated once after it.
static_assert(kBailout <= kListCap, "the candidate list holds every leaf a wave that does not bail passes");

// Boxes of the active queries of each group of kGroupLanes lanes, broadcast to every lane.
__device__ __forceinline__ void group_boxes(float4 p, bool active, float4 (&lo)[kGroups], float4 (&hi)[kGroups])
{
    float v[6] = {active ? p.x : FLT_MAX,  active ? p.y : FLT_MAX,  active ? p.z : FLT_MAX,
                  active ? p.x : -FLT_MAX, active ? p.y : -FLT_MAX, active ? p.z : -FLT_MAX};
#pragma unroll
    for (int m = 1; m < kGroupLanes; m <<= 1)
#pragma unroll
        for (int a = 0; a < 6; a++) {
            const float o = __shfl_xor(v[a], m, kWave);
            v[a] = a < 3 ? fminf(v[a], o) : fmaxf(v[a], o);
        }
#pragma unroll
    for (int g = 0; g < kGroups; g++) {
        lo[g] = make_float4(uniform_lane(v[0], g * kGroupLanes), uniform_lane(v[1], g * kGroupLanes),
                            uniform_lane(v[2], g * kGroupLanes), 0.f);
        hi[g] = make_float4(uniform_lane(v[3], g * kGroupLanes), uniform_lane(v[4], g * kGroupLanes),
                            uniform_lane(v[5], g * kGroupLanes), 0.f);
    }
}

// Upper bound of the 3rd-best distance over each group's active queries (-FLT_MAX if none).
__device__ __forceinline__ void group_bounds(float b2, bool active, float (&ub)[kGroups])
{
    float v = active ? b2 : -FLT_MAX;
#pragma unroll
    for (int m = 1; m < kGroupLanes; m <<= 1) v = fmaxf(v, __shfl_xor(v, m, kWave));
#pragma unroll
    for (int g = 0; g < kGroups; g++) ub[g] = uniform_lane(v, g * kGroupLanes);
}

// ---- phase 1 kernel ------------------------------------------------------------
struct KnnCounters {
    uint32_t hard;  // number of queries sent to phase 2
};
static_assert(sizeof(KnnCounters) <= kAlign, "knn_stats.h finds its block one carving step behind the counters");

// Appends query `me` of every lane with `flag` to the hard list (phase 2's input): one atomic per wave.
__device__ __forceinline__ void push_hard(bool flag, int me, KnnCounters* __restrict__ counters,
                                          uint32_t* __restrict__ hard)
{
    const uint32_t at = wave_append(flag, &counters->hard);
    if (flag) hard[at] = (uint32_t)me;
}

// At least 7 waves per SIMD set the register budget: knn_leaf 792/790 -> 773/773 us frustum against the 6
// waves that the 79 VGPRs of a free allocation gave (profiles/r04_knn_waves.md).  The kernel now takes 64
// VGPRs and no scratch, so 8 waves fit (profiles/r08_knn_refactor.md).
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(7))) void knn_leaf_kernel(const float4* __restrict__ sp, int P, int nleaves, int nsuper,
                                                          const Box* __restrict__ leaves, const Box* __restrict__ subs,
                                                          const Box* __restrict__ supers,
                                                          float* __restrict__ out, uint32_t* __restrict__ hard,
                                                          KnnCounters* __restrict__ counters)
{
    __shared__ uint32_t s_list[kWaves][kListCap];
    WaveStats ws;  // statistics builds only (knn_stats.h): empty otherwise
    const int wave = threadIdx.x / kWave;
    const int lane = lane_id();
    const int L = xcd_swizzle(blockIdx.x, gridDim.x) * kWaves + wave;
    if (L >= nleaves) return;  // whole wave exits; no workgroup barrier below

    const int me = L * kLeaf + lane;
    const bool valid = me < P;
    const float4 p = valid ? sp[me] : make_float4(0.f, 0.f, 0.f, 0.f);
    float b0 = FLT_MAX, b1 = FLT_MAX, b2 = FLT_MAX;

    // seed from the own leaf and its two Morton neighbours (a query near its leaf's border finds a
    // tight bound there, which prunes the box walk below)
    {
        const int nc = min(kLeaf, P - L * kLeaf);
        for (int k0 = 0; k0 < nc; k0 += kChunk) eval_lanes(p, k0, nc, lane, p, b0, b1, b2);
        const int ln = L - 1, rn = L + 1;
        const float4 pl = ln >= 0 ? sp[ln * kLeaf + lane] : p;
        const float4 pr = rn < nleaves ? sp[min(rn * kLeaf + lane, P - 1)] : p;
        // A neighbour point is evaluated only if it lies within some query group's bound of that
        // group's box (boxes and bounds over every valid lane, so each lane's three best come out
        // exactly as from evaluating all 64: a skipped point is at least its bound from every query).
        // All 128 evaluated instead: knn_leaf frustum 815/814 -> 836/831 us, uniform 773/765 -> 784/787 (2M).
        float4 slo[kGroups], shi[kGroups];
        float sub[kGroups];
        group_boxes(p, valid, slo, shi);
        group_bounds(b2, valid, sub);
        auto seed_filtered = [&](const float4 pt, const int nc) {
            bool usable = false;
#pragma unroll
            for (int g = 0; g < kGroups; g++) usable |= box_point_lb(Box{slo[g], shi[g]}, pt) <= sub[g];
            uint64_t pm = __ballot(usable && lane < nc);
            while (pm) {
                const int k = __builtin_ctzll(pm);
                pm &= pm - 1;
                kbest(sqdist(p, make_float4(uniform_lane(pt.x, k), uniform_lane(pt.y, k), uniform_lane(pt.z, k), 0.f)),
                      b0, b1, b2);
            }
        };
        if (ln >= 0) seed_filtered(pl, kLeaf);
        if (rn < nleaves) seed_filtered(pr, min(kLeaf, P - rn * kLeaf));
    }

    // outliers -> phase 2
    bool active = valid;
    if (nleaves > 1) {
        const bool finite = valid && b2 < FLT_MAX;
        const float nfin = (float)__popcll(__ballot(finite));
        const float mean = wave_sum(finite ? b2 : 0.f) / fmaxf(nfin, 1.f);
        const bool is_hard = valid && (!finite || b2 > kHardFactor * mean);
        push_hard(is_hard, me, counters, hard);
        active = valid && !is_hard;
    } else {
        active = false;  // a single leaf holds every point: the seed is the answer
        if (valid) out[__float_as_uint(p.w)] = ((b0 + b1) + b2) / 3.0f;
        return;
    }

    if (__ballot(active)) {
        // Coarse filter against kGroups query groups (32 Morton-consecutive queries each, so a
        // leaf that straddles a Morton jump does not inflate one wave-wide box): a box passes
        // if it is within the group's upper bound of some group's box.  The walk is organised
        // for memory-level parallelism: super-boxes are tested kSuperBatch per lane at a time,
        // the leaf boxes of kLeafBatch passing super-boxes are loaded together, passing leaves
        // go to an LDS list, and after the walk the list is evaluated kFlushBatch leaves' loads
        // at a time.
        float4 glo[kGroups], ghi[kGroups];
        float gub[kGroups];
        group_boxes(p, active, glo, ghi);
        group_bounds(b2, active, gub);
        uint32_t* list = s_list[wave];
        int nnear = 0, nfar = 0;  // list[0, nnear) near leaves, list[cap - nfar, cap) far leaves
        bool bail = false;

        for (int s0 = 0; s0 < nsuper; s0 += kWave * kSuperBatch) {
            uint64_t smask[kSuperBatch];
            {
                Box sb[kSuperBatch];
#pragma unroll
                for (int j = 0; j < kSuperBatch; j++) {
                    const int sidx = s0 + j * kWave + lane;
                    if (sidx < nsuper) sb[j] = supers[sidx];
                }
#pragma unroll
                for (int j = 0; j < kSuperBatch; j++) {
                    const int sidx = s0 + j * kWave + lane;
                    bool pass = false;
                    if (sidx < nsuper) {
#pragma unroll
                        for (int g = 0; g < kGroups; g++) pass |= box_box_lb(sb[j], glo[g], ghi[g]) <= gub[g];
                    }
                    smask[j] = __ballot(pass);
                }
            }
            // passing super-boxes in ascending order, kLeafBatch at a time
            int j = 0;
            while (true) {
                int S[kLeafBatch];
                int ns = 0;
                while (ns < kLeafBatch && j < kSuperBatch) {
                    if (smask[j]) {
                        S[ns++] = s0 + j * kWave + __builtin_ctzll(smask[j]);
                        smask[j] &= smask[j] - 1;
                    } else {
                        j++;
                    }
                }
                if (ns == 0) break;
                Box lb[kLeafBatch];
#pragma unroll
                for (int q = 0; q < kLeafBatch; q++) {
                    const int l = (q < ns ? S[q] : 0) * kFan + lane;
                    if (q < ns && l < nleaves) lb[q] = leaves[l];
                }
#pragma unroll
                for (int q = 0; q < kLeafBatch; q++) {
                    if (q >= ns) break;
                    const int l = S[q] * kFan + lane;
                    bool lpass = false, near = false;
                    if (l < nleaves && l != L && l != L - 1 && l != L + 1) {  // those three were the seed
#pragma unroll
                        for (int g = 0; g < kGroups; g++) {
                            const float d = box_box_lb(lb[q], glo[g], ghi[g]);
                            lpass |= d <= gub[g];
                            near |= d == 0.f;
                        }
                    }
                    const uint64_t lm = __ballot(lpass);
                    const int cnt = __popcll(lm);
                    if (cnt == 0) continue;
                    if (nnear + nfar + cnt > kBailout) {  // a long-tail wave: its queries go to phase 2
                        bail = true;
                        break;
                    }
                    // leaves touching a query group's box go to the front and are evaluated first,
                    // so the bounds shrink before the farther leaves are filtered
                    const uint64_t nm = __ballot(lpass && near), fm = lm & ~nm;
                    const uint64_t lt = lanes_below(lane);
                    if (lpass && near) list[nnear + __popcll(nm & lt)] = (uint32_t)l;
                    if (lpass && !near) list[kListCap - 1 - nfar - __popcll(fm & lt)] = (uint32_t)l;
                    nnear += __popcll(nm);
                    nfar += __popcll(fm);
                    __builtin_amdgcn_wave_barrier();
                }
                if (bail) break;
            }
            if (bail) break;
        }
        if (bail) {
            // Waves whose coarse walk passes more than kBailout leaves (queries at the edge of a
            // sparse region inflate their group's bound) would run for milliseconds while the rest
            // of the grid idles; phase 2 searches each of their queries with its own bound instead.
            push_hard(active, me, counters, hard);
            active = false;
            ws.bail();
        } else {
            // Evaluate the candidate list, near leaves first, in batches of kFlushBatch leaves: every
            // point load of a batch is issued before any is used, so a batch costs one memory latency.
            // (A rotating prefetch across iterations measured no gain: the waitcnt pass drains all
            // loads at the loop header.)
            const int cnt = nnear + nfar;
            auto at = [&](int i) { return (int)list[i < nnear ? i : kListCap - 1 - (i - nnear)]; };
            for (int i0 = 0; i0 < cnt; i0 += kFlushBatch) {
                float4 pt[kFlushBatch];
                int Cb[kFlushBatch];
#pragma unroll
                for (int q = 0; q < kFlushBatch; q++) {
                    Cb[q] = at(min(i0 + q, cnt - 1));
                    pt[q] = sp[min(Cb[q] * kLeaf + lane, P - 1)];
                }
#pragma unroll
                for (int q = 0; q < kFlushBatch; q++) {
                    if (i0 + q >= cnt) break;
                    ws.leaf();
                    // The leaf's sub-boxes by scalar loads (the leaf index is wave-uniform) instead of a vector
                    // load and six readlanes each: 893 -> 840 us frustum, 848 -> 787 uniform, 448 -> 492 plane (2M).
                    // Without this per-lane sub-box test before the point filter: frustum 889 -> 1003 us.
                    const Box* sbp = subs + (size_t)__builtin_amdgcn_readfirstlane(Cb[q]) * kSub;
                    uint32_t smask4 = 0u;
#pragma unroll
                    for (int j = 0; j < kSub; j++) {
                        const Box sb = sbp[j];
                        if (__ballot(active && box_point_lb(sb, p) <= b2)) smask4 |= 1u << j;
                    }
                    const int nc = min(kLeaf, P - Cb[q] * kLeaf);
                    // point-level filter: lane c holds point c of the leaf; it is evaluated only if
                    // its sub-box passed some lane's own bound AND it lies within some query group's
                    // bound of that group's box (both skip only points that cannot improve any
                    // active query's three best)
                    uint64_t sm = 0;
#pragma unroll
                    for (int j = 0; j < kSub; j++)
                        if (smask4 >> j & 1u) sm |= 0xFFFFull << (kChunk * j);
                    bool usable = false;
#pragma unroll
                    for (int g = 0; g < kGroups; g++) usable |= box_point_lb(Box{glo[g], ghi[g]}, pt[q]) <= gub[g];
                    uint64_t pm = __ballot(usable && lane < nc) & sm;
                    ws.points(pm);
                    while (pm) {
                        const int k = __builtin_ctzll(pm);
                        pm &= pm - 1;
                        const float4 c = make_float4(uniform_lane(pt[q].x, k), uniform_lane(pt[q].y, k),
                                                     uniform_lane(pt[q].z, k), 0.f);
                        kbest(sqdist(p, c), b0, b1, b2);
                    }
                }
                group_bounds(b2, active, gub);  // tighter group bounds for the next batch
            }
        }
        ws.report(counters, L, lane);
    }
    if (active) out[__float_as_uint(p.w)] = ((b0 + b1) + b2) / 3.0f;
}

// ---- 6. phase 2: one wave per hard query ---------------------------------------------------------
// Three smallest of the wave's lane-local lists plus g; lane lists are reset.
__device__ __forceinline__ void wave_merge3(float& a0, float& a1, float& a2, float& g0, float& g1, float& g2)
{
    if (lane_id() == 0) {
        kbest(g0, a0, a1, a2);
        kbest(g1, a0, a1, a2);
        kbest(g2, a0, a1, a2);
    }
    float g[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float m = wave_min(a0);
        const uint64_t who = __ballot(a0 == m);
        const int w = __builtin_ctzll(who);
        if (lane_id() == w) {
            a0 = a1;
            a1 = a2;
            a2 = FLT_MAX;
        }
        g[r] = m;
    }
    g0 = g[0];
    g1 = g[1];
    g2 = g[2];
    a0 = a1 = a2 = FLT_MAX;
}

__global__ __launch_bounds__(kBlock) void knn_hard_kernel(const float4* __restrict__ sp, int P, int nleaves, int nsuper,
                                                          const Box* __restrict__ leaves, const Box* __restrict__ supers,
                                                          float* __restrict__ out, const uint32_t* __restrict__ hard,
                                                          const KnnCounters* __restrict__ counters)
{
    const int lane = lane_id();
    const uint32_t nhard = counters->hard;
    const int nw = gridDim.x * kWaves;
    for (uint32_t h = blockIdx.x * kWaves + threadIdx.x / kWave; h < nhard; h += nw) {
        const int me = (int)hard[h];
        const float4 p = sp[me];
        const int L = me / kLeaf;
        float a0 = FLT_MAX, a1 = FLT_MAX, a2 = FLT_MAX;
        float g0 = FLT_MAX, g1 = FLT_MAX, g2 = FLT_MAX;
        // seed: own leaf and its two neighbours, one candidate per lane
        for (int C = max(0, L - 1); C <= min(nleaves - 1, L + 1); C++) {
            const int j = C * kLeaf + lane;
            if (j < P && j != me) kbest(sqdist(p, sp[j]), a0, a1, a2);
        }
        wave_merge3(a0, a1, a2, g0, g1, g2);
        for (int s0 = 0; s0 < nsuper; s0 += kWave) {
            const int s = s0 + lane;
            bool pass = false;
            if (s < nsuper) pass = box_point_lb(supers[s], p) <= g2;
            uint64_t smask = __ballot(pass);
            while (smask) {
                const int S = s0 + __builtin_ctzll(smask);
                smask &= smask - 1;
                const int l = S * kFan + lane;
                bool lpass = false;
                if (l < nleaves && (l < L - 1 || l > L + 1)) lpass = box_point_lb(leaves[l], p) <= g2;
                uint64_t lmask = __ballot(lpass);
                if (!lmask) continue;
                while (lmask) {
                    const int C = S * kFan + __builtin_ctzll(lmask);
                    lmask &= lmask - 1;
                    const int j = C * kLeaf + lane;
                    if (j < P) kbest(sqdist(p, sp[j]), a0, a1, a2);
                }
                wave_merge3(a0, a1, a2, g0, g1, g2);
            }
        }
        if (lane == 0) out[__float_as_uint(p.w)] = ((g0 + g1) + g2) / 3.0f;
    }
}

struct KnnLayout {
    SortLayout sort;
    float4* sp;
    Box *leaves, *subs, *supers;
    uint32_t* hard;
    KnnCounters* counters;
    size_t counter_bytes;
    float *partials, *params;
    size_t total;
};

KnnLayout layout(void* base, int P)
{
    const int nleaves = ceil_div(P, kLeaf), nsuper = ceil_div(nleaves, kFan);
    Carver c(base);
    KnnLayout l;
    sort_layout(c, P, l.sort);
    l.sp = c.take<float4>(P);
    l.leaves = c.take<Box>(nleaves);
    l.subs = c.take<Box>((size_t)nleaves * kSub);
    l.supers = c.take<Box>(nsuper);
    l.hard = c.take<uint32_t>(P);
    const size_t counters_at = c.used;
    l.counters = c.take<KnnCounters>(1);
    c.take<char>(knn_stats_bytes(nleaves));  // statistics builds: their block follows the counters (knn_stats.h)
    l.counter_bytes = c.used - counters_at;  // zeroed before every call
    l.partials = c.take<float>(kBoundBlocks * 6);
    l.params = c.take<float>(8);
    l.total = c.used;
    return l;
}

}  // namespace

size_t knn_scratch_bytes(int P) { return P > 0 ? layout(nullptr, P).total : 0; }

int dist_cuda2(hidegs_alloc_fn alloc, void* user, int P, const float* points, float* mean_dists, hipStream_t stream)
{
    if (P < 0) return fail(HIDEGS_E_ARG, "distCUDA2: negative point count");
    if (P == 0) return 0;
    if (!points || !mean_dists) return fail(HIDEGS_E_ARG, "distCUDA2: NULL points or output");
    if (!alloc) return fail(HIDEGS_E_ARG, "distCUDA2: NULL scratch allocator");
    const size_t bytes = knn_scratch_bytes(P);
    char* base = alloc(user, bytes);
    if (!base) return fail(HIDEGS_E_ALLOC, "distCUDA2: scratch allocation of " + std::to_string(bytes) + " bytes failed");
    const KnnLayout l = layout(base, P);
    const int nleaves = ceil_div(P, kLeaf), nsuper = ceil_div(nleaves, kFan);
    const int nb = ceil_div(P, kBlock);
    const int nbound = std::min(kBoundBlocks, nb);

    if (hipMemsetAsync(l.counters, 0, l.counter_bytes, stream) != hipSuccess)
        return fail(HIDEGS_E_HIP, "distCUDA2: memset failed");
    HIDEGS_LAUNCH("bounds", tree_bounds_kernel<KnnTree>, dim3(nbound), dim3(kTreeBlock), 0, stream, points, P, l.partials);
    HIDEGS_LAUNCH("bounds_finalize", tree_frame_kernel<KnnTree>, dim3(1), dim3(kTreeBlock), 0, stream, l.partials, nbound,
                  l.params);
    HIDEGS_LAUNCH("morton", tree_point_keys_kernel<KnnTree>, dim3(nb), dim3(kTreeBlock), 0, stream, points, P, l.params,
                  l.sort.keys, l.sort.vals);
    int rc = sort_pairs_u64(l.sort.sort_tmp, l.sort.sort_bytes, l.sort.keys, l.sort.keys_sorted, l.sort.vals,
                            l.sort.vals_sorted, P, 0, 3 * kMortonBits, stream);
    if (rc) return rc;
    HIDEGS_LAUNCH("gather", gather_kernel, dim3(nb), dim3(kBlock), 0, stream, points, l.sort.vals_sorted, P, l.sp, nleaves,
                  l.leaves, l.subs);
    HIDEGS_LAUNCH("super_box", tree_super_kernel<KnnTree>, dim3(ceil_div(nsuper, kTreeWaves)), dim3(kTreeBlock), 0, stream,
                  l.leaves, nleaves, nsuper, l.supers);
    HIDEGS_LAUNCH("knn_leaf", knn_leaf_kernel, dim3(ceil_div(nleaves, kWaves)), dim3(kBlock), 0, stream, l.sp, P, nleaves,
                       nsuper, l.leaves, l.subs, l.supers, mean_dists, l.hard, l.counters);
    HIDEGS_LAUNCH("knn_hard", knn_hard_kernel, dim3(std::min(2048, ceil_div(nleaves, kWaves))), dim3(kBlock), 0, stream, l.sp,
                       P, nleaves, nsuper, l.leaves, l.supers, mean_dists, l.hard, l.counters);
    knn_stats_report(l.counters, P, nleaves, nsuper, stream);  // statistics builds only (knn_stats.h)
    return check_launch("distCUDA2", stream, 0);
}

}  // namespace hidegs

extern "C" {

int hidegs_dist_cuda2(hidegs_alloc_fn scratch_buffer, void* alloc_user, int P, const float* points, float* mean_dists,
                      void* stream)
{
    if (int rc = hidegs::take_async_error("hidegs_dist_cuda2", hidegs::as_stream(stream))) return rc;
    return hidegs::dist_cuda2(scratch_buffer, alloc_user, P, points, mean_dists, hidegs::as_stream(stream));
}

size_t hidegs_knn_scratch_bytes(int P) { return hidegs::knn_scratch_bytes(P); }

}  // extern "C"
