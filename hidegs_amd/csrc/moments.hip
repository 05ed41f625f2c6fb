// moments.hip -- moments of neighbour lists and the eigen-decomposition of symmetric 3x3 matrices
// (include/hidegs_moments.h).
//
// The rule cuts a list into blocks of 64 positions: a block's partial is a sequential sum from +0.0f, a total is
// block 0's partial plus the partials of the later blocks in block order.  Three kernels state it:
//   moments_lane   one lane per query, for lists of up to kLaneBlocks blocks: the lane sums its blocks one after
//                  the other (pass 1: W and S; the division; pass 2, which gathers the points again: C), sixteen
//                  entries' loads in flight.  A longer list is appended to the long list in scratch -- one
//                  ballot and one integer atomic per wave on a counter that the call clears -- and left alone;
//   moments_short  a table of at most kShort columns: one lane per query as above, but the list's points are
//                  gathered once, all loads in flight together, and stay in registers for the second pass;
//   moments_wave   one wave per long list over a fixed grid, the waves striding over the long list.  In round r
//                  lane l sums block 64 r + l; the wave then adds the 64 partials in lane order (v_readlane, the
//                  same addition in every lane) before the next round: the rule's order exactly.
// A table of more than kLaneBlocks * 64 columns has only long lists: moments_wave alone, over every query, with
// no long list.  With evals and evecs given, the lane (or the wave, every lane alike) that holds a query's
// covariance decomposes it before it writes: sym3_eigen, a cyclic Jacobi iteration in Rutishauser's form of
// kSweeps sweeps, which hidegs_sym3_eigen runs alone, one lane per matrix.
// There is no floating-point atomic and no workgroup waits on another; capped launches stride past their caps.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/hidegs_moments.h"
#include "common.h"
#include "neighbor_sum.h"  // kSum: the positions of a block of the rule

namespace hidegs {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;  // 4
constexpr long long kMomentsMax = 0x7fffffffLL;
constexpr uint32_t kLaneBlocks = 4;  // blocks of the longest list that one lane sums
constexpr int kLaneGridCap = 8192;   // workgroups of moments_short, moments_lane and sym3_eigen: 32 per CU, then by stride
constexpr int kWaveGrid = 2048;      // workgroups of moments_wave: 8 per CU
constexpr int kSweeps = 4;           // Jacobi sweeps of sym3_eigen
constexpr int kInFlight = 16;        // entries whose loads are issued together (4 waves per SIMD; measured against 4 and 8)
constexpr uint32_t kShort = 16;      // columns of the widest table whose lists a lane keeps in registers

struct Cloud {
    const float* points;
    const float* weights;
    uint32_t P;
};

struct Lists {
    const int32_t* table;  // (Q, k), or NULL: the list form
    const int32_t* starts;
    const int32_t* rows;
    uint32_t k, capacity, Q;
};

struct Out {
    int32_t* count;
    float *mean, *cov, *evals, *evecs;
};

// The entries of query j < Q: ent[0 .. L).  Nothing at or past capacity is inside it, whatever starts holds.
__device__ __forceinline__ void list_span(const Lists& ls, uint32_t j, const int32_t*& ent, uint32_t& L)
{
    if (ls.table) {
        ent = ls.table + (size_t)j * ls.k;
        L = ls.k;
    } else {
        const int32_t a = max(ls.starts[j], 0), e = min(ls.starts[j + 1], (int32_t)ls.capacity);
        ent = ls.rows + a;
        L = e > a ? (uint32_t)(e - a) : 0u;
    }
}

struct Entry {
    float x, y, z, w;
    bool ok;
};

__device__ __forceinline__ Entry load_entry(const Cloud& c, int32_t r)
{
    Entry e;
    e.ok = (uint32_t)r < c.P;  // a negative row is above every P
    e.x = e.y = e.z = 0.f;
    e.w = 1.f;
    if (e.ok) {
        const float* p = c.points + 3 * (size_t)r;
        e.x = p[0], e.y = p[1], e.z = p[2];
        if (c.weights) e.w = c.weights[r];
        e.ok = finite3(e.x, e.y, e.z);
    }
    return e;
}

// Pass 1 of one block: acc = {W, Sx, Sy, Sz}.
struct Pass1 {
    static constexpr int N = 4;
    __device__ __forceinline__ void add(const Entry& e, float (&acc)[N], uint32_t& cnt) const
    {
        acc[0] = acc[0] + e.w;
        acc[1] = fmaf(e.w, e.x, acc[1]);
        acc[2] = fmaf(e.w, e.y, acc[2]);
        acc[3] = fmaf(e.w, e.z, acc[3]);
        cnt++;
    }
};

// Pass 2 of one block: acc = {Cxx, Cxy, Cxz, Cyy, Cyz, Czz} about the mean.
struct Pass2 {
    static constexpr int N = 6;
    float mx, my, mz;
    __device__ __forceinline__ void add(const Entry& e, float (&acc)[N], uint32_t&) const
    {
        const float dx = e.x - mx, dy = e.y - my, dz = e.z - mz;
        const float tx = e.w * dx, ty = e.w * dy, tz = e.w * dz;
        acc[0] = fmaf(tx, dx, acc[0]);
        acc[1] = fmaf(tx, dy, acc[1]);
        acc[2] = fmaf(tx, dz, acc[2]);
        acc[3] = fmaf(ty, dy, acc[3]);
        acc[4] = fmaf(ty, dz, acc[4]);
        acc[5] = fmaf(tz, dz, acc[5]);
    }
};

// The partial of the n <= 64 entries ent[0 .. n): from +0.0f, the valid entries in ascending position.
template <typename Pass>
__device__ __forceinline__ void block_partial(const Cloud& c, const int32_t* __restrict__ ent, uint32_t n, const Pass& pass,
                                              float (&acc)[Pass::N], uint32_t& cnt)
{
#pragma unroll
    for (int s = 0; s < Pass::N; s++) acc[s] = 0.f;
    for (uint32_t i = 0; i < n; i += kInFlight) {
        int32_t r[kInFlight];
        Entry e[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; u++) r[u] = i + u < n ? ent[i + u] : -1;  // past the end: an invalid entry
#pragma unroll
        for (int u = 0; u < kInFlight; u++) e[u] = load_entry(c, r[u]);
#pragma unroll
        for (int u = 0; u < kInFlight; u++)
            if (e[u].ok) pass.add(e[u], acc, cnt);
    }
}

// One lane, the whole list: block 0's partial, plus the partials of the later blocks in block order.
template <typename Pass>
__device__ __forceinline__ void lane_total(const Cloud& c, const int32_t* __restrict__ ent, uint32_t L, const Pass& pass,
                                           float (&tot)[Pass::N], uint32_t& cnt)
{
#pragma unroll
    for (int s = 0; s < Pass::N; s++) tot[s] = 0.f;
    for (uint32_t b = 0; b * kSum < L; b++) {
        float part[Pass::N];
        block_partial(c, ent + b * kSum, min(kSum, L - b * kSum), pass, part, cnt);
#pragma unroll
        for (int s = 0; s < Pass::N; s++) tot[s] = b == 0 ? part[s] : tot[s] + part[s];
    }
}

// One wave, the whole list (ent and L wave-uniform, L > 0): lane l sums block 64 r + l in round r, then every
// lane adds the round's partials in lane order.  Every lane ends with the same totals; cnt is the lane's own.
template <typename Pass>
__device__ __forceinline__ void wave_total(const Cloud& c, const int32_t* __restrict__ ent, uint32_t L, const Pass& pass,
                                           float (&tot)[Pass::N], uint32_t& cnt)
{
    const uint32_t nb = (L + kSum - 1) / kSum, lane = lane_id();
#pragma unroll
    for (int s = 0; s < Pass::N; s++) tot[s] = 0.f;
    for (uint32_t b0 = 0; b0 < nb; b0 += kWave) {  // wave-uniform
        float part[Pass::N];
#pragma unroll
        for (int s = 0; s < Pass::N; s++) part[s] = 0.f;
        const uint32_t b = b0 + lane;
        if (b < nb) block_partial(c, ent + (size_t)b * kSum, min(kSum, L - b * kSum), pass, part, cnt);
        const uint32_t lanes = min((uint32_t)kWave, nb - b0);
        for (uint32_t l = 0; l < lanes; l++) {
#pragma unroll
            for (int s = 0; s < Pass::N; s++) {
                const float v = uniform_lane(part[s], (int)l);
                tot[s] = (b0 == 0 && l == 0) ? v : tot[s] + v;
            }
        }
    }
}

// ---- eigen-decomposition ------------------------------------------------------------------------------
// One Jacobi rotation in the (p, q) plane, Rutishauser's form: the diagonal moves by t * a_pq, a_pq becomes 0,
// the remaining off-diagonal pair (a_rp, a_rq) and the columns p and q of V turn by s and tau = s / (1 + c).
__device__ __forceinline__ void jacobi_rotate(float& dp, float& dq, float& zp, float& zq, float& apq, float& arp, float& arq,
                                              float (&v)[3][3], int p, int q)
{
    if (apq == 0.f) return;
    // halved before the subtraction: two finite diagonal entries of opposite sign near FLT_MAX must not overflow
    // to an infinite theta, which would drop a_pq without a rotation
    const float theta = (0.5f * dq - 0.5f * dp) / apq;
    // the smaller root of t^2 + 2 theta t - 1: |t| <= 1.  A theta beyond the float range (a_pq negligible next to
    // the difference) or an overflow of its square gives t = 0.
    float t = 1.0f / (fabsf(theta) + sqrtf(fmaf(theta, theta, 1.0f)));
    t = theta < 0.f ? -t : t;
    const float cs = 1.0f / sqrtf(fmaf(t, t, 1.0f)), sn = t * cs, tau = sn / (1.0f + cs);
    const float h = t * apq;
    zp -= h, zq += h, dp -= h, dq += h;
    apq = 0.f;
    const float g = arp, k = arq;
    arp = g - sn * (k + g * tau);
    arq = k + sn * (g - k * tau);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float a = v[j][p], b = v[j][q];
        v[j][p] = a - sn * (b + a * tau);
        v[j][q] = b + sn * (a - b * tau);
    }
}

// evals[3] ascending and evecs[9], row i the unit eigenvector of evals[i], of the symmetric matrix a =
// {xx, xy, xz, yy, yz, zz}; the signs as the header states them.  All NaN where an input is not finite.
__device__ __forceinline__ void sym3_eigen(const float (&a)[6], float (&evals)[3], float (&evecs)[9])
{
    bool finite = true;
#pragma unroll
    for (int s = 0; s < 6; s++) finite = finite && fabsf(a[s]) < INFINITY;
    if (!finite) {
        const float nan = __uint_as_float(0x7fc00000u);
#pragma unroll
        for (int s = 0; s < 3; s++) evals[s] = nan;
#pragma unroll
        for (int s = 0; s < 9; s++) evecs[s] = nan;
        return;
    }
    float d[3] = {a[0], a[3], a[5]}, b[3] = {a[0], a[3], a[5]}, z[3] = {0.f, 0.f, 0.f};
    float a01 = a[1], a02 = a[2], a12 = a[4];
    float v[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}};  // column i: the eigenvector of d[i]
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps; sweep++) {
        jacobi_rotate(d[0], d[1], z[0], z[1], a01, a02, a12, v, 0, 1);
        jacobi_rotate(d[0], d[2], z[0], z[2], a02, a01, a12, v, 0, 2);
        jacobi_rotate(d[1], d[2], z[1], z[2], a12, a01, a02, v, 1, 2);
#pragma unroll
        for (int i = 0; i < 3; i++) {  // the diagonal is the sum of the sweeps' updates, not of the rotations'
            b[i] += z[i];
            d[i] = b[i];
            z[i] = 0.f;
        }
    }
    float r[3][3];  // row i: eigenvector i
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) r[i][j] = v[j][i];
    auto order = [&](int i, int j) {  // d[i] <= d[j] afterwards; equal values stay
        if (d[j] < d[i]) {
            const float t = d[i];
            d[i] = d[j], d[j] = t;
#pragma unroll
            for (int s = 0; s < 3; s++) {
                const float u = r[i][s];
                r[i][s] = r[j][s], r[j][s] = u;
            }
        }
    };
    order(0, 1), order(1, 2), order(0, 1);
#pragma unroll
    for (int i = 0; i < 2; i++) {  // the component of largest magnitude positive, the lowest index among equals
        float lead = r[i][0];
        if (fabsf(r[i][1]) > fabsf(lead)) lead = r[i][1];
        if (fabsf(r[i][2]) > fabsf(lead)) lead = r[i][2];
        if (lead < 0.f)
#pragma unroll
            for (int s = 0; s < 3; s++) r[i][s] = -r[i][s];
    }
    const float cx = r[0][1] * r[1][2] - r[0][2] * r[1][1], cy = r[0][2] * r[1][0] - r[0][0] * r[1][2],
                cz = r[0][0] * r[1][1] - r[0][1] * r[1][0];  // row 0 x row 1
    if (cx * r[2][0] + cy * r[2][1] + cz * r[2][2] < 0.f)
#pragma unroll
        for (int s = 0; s < 3; s++) r[2][s] = -r[2][s];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        evals[i] = d[i];
#pragma unroll
        for (int s = 0; s < 3; s++) evecs[3 * i + s] = r[i][s];
    }
}

// What query j receives: the divisions, and the decomposition where it is wanted.
__device__ __forceinline__ void write_mean(const Out& o, uint32_t j, uint32_t cnt, const float (&s)[4], float (&m)[3])
{
    m[0] = s[1] / s[0], m[1] = s[2] / s[0], m[2] = s[3] / s[0];
    o.count[j] = (int32_t)cnt;
    for (int a = 0; a < 3; a++) o.mean[3 * (size_t)j + a] = m[a];
}

__device__ __forceinline__ void write_cov(const Out& o, uint32_t j, float W, const float (&c)[6])
{
    float cov[6];
#pragma unroll
    for (int a = 0; a < 6; a++) cov[a] = c[a] / W;
#pragma unroll
    for (int a = 0; a < 6; a++) o.cov[6 * (size_t)j + a] = cov[a];
    if (o.evals) {
        float evals[3], evecs[9];
        sym3_eigen(cov, evals, evecs);
#pragma unroll
        for (int a = 0; a < 3; a++) o.evals[3 * (size_t)j + a] = evals[a];
#pragma unroll
        for (int a = 0; a < 9; a++) o.evecs[9 * (size_t)j + a] = evecs[a];
    }
}

__global__ __launch_bounds__(kBlock) void moments_lane_kernel(Cloud c, Lists ls, Out o, uint32_t* __restrict__ long_list,
                                                              uint32_t* __restrict__ long_count)
{
    for (unsigned long long base = (unsigned long long)blockIdx.x * kBlock; base < ls.Q;
         base += (unsigned long long)gridDim.x * kBlock) {  // workgroup-uniform
        const unsigned long long j64 = base + threadIdx.x;
        const bool active = j64 < ls.Q;
        const uint32_t j = (uint32_t)j64;
        const int32_t* ent = nullptr;
        uint32_t L = 0;
        if (active) list_span(ls, j, ent, L);
        const bool is_long = L > kLaneBlocks * kSum;
        if (long_list) {  // the long lists of this wave: one atomic, then every lane its own slot
            const uint32_t at = wave_append(is_long, long_count);
            if (is_long) long_list[at] = j;
        }
        if (!active || is_long) continue;
        float s[4], m[3], cc[6];
        uint32_t cnt = 0, unused = 0;
        lane_total(c, ent, L, Pass1(), s, cnt);
        write_mean(o, j, cnt, s, m);
        lane_total(c, ent, L, Pass2{m[0], m[1], m[2]}, cc, unused);
        write_cov(o, j, s[0], cc);
    }
}

// A table of at most kShort columns: one lane per query, the list's points gathered once and kept in registers
// for both passes (the same additions in the same order as moments_lane, half its gathers, all of them in flight
// at once).
__global__ __launch_bounds__(kBlock) void moments_short_kernel(Cloud c, Lists ls, Out o)
{
    for (unsigned long long j64 = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; j64 < ls.Q;
         j64 += (unsigned long long)gridDim.x * kBlock) {
        const uint32_t j = (uint32_t)j64;
        const int32_t* __restrict__ ent = ls.table + (size_t)j * ls.k;
        int32_t r[kShort];
        Entry e[kShort];
        if (ls.k == kShort) {  // uniform: loads that can be merged
#pragma unroll
            for (uint32_t u = 0; u < kShort; u++) r[u] = ent[u];
        } else {
#pragma unroll
            for (uint32_t u = 0; u < kShort; u++) r[u] = u < ls.k ? ent[u] : -1;
        }
#pragma unroll
        for (uint32_t u = 0; u < kShort; u++) e[u] = load_entry(c, r[u]);
        float s[4] = {0.f, 0.f, 0.f, 0.f}, cc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, m[3];
        uint32_t cnt = 0, unused = 0;
        const Pass1 p1;
#pragma unroll
        for (uint32_t u = 0; u < kShort; u++)
            if (e[u].ok) p1.add(e[u], s, cnt);
        write_mean(o, j, cnt, s, m);
        const Pass2 p2{m[0], m[1], m[2]};
#pragma unroll
        for (uint32_t u = 0; u < kShort; u++)
            if (e[u].ok) p2.add(e[u], cc, unused);
        write_cov(o, j, s[0], cc);
    }
}

// long_list == NULL: every query of the call is a long list (a wide table).
__global__ __launch_bounds__(kBlock) void moments_wave_kernel(Cloud c, Lists ls, Out o, const uint32_t* __restrict__ long_list,
                                                              const uint32_t* __restrict__ long_count)
{
    const uint32_t n = long_list ? min(*long_count, ls.Q) : ls.Q;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kWaves + threadIdx.x / kWave; i < n;
         i += (unsigned long long)gridDim.x * kWaves) {  // wave-uniform
        uint32_t j = long_list ? long_list[i] : (uint32_t)i;
        j = (uint32_t)__builtin_amdgcn_readfirstlane((int)j);
        if (j >= ls.Q) continue;
        const int32_t* ent;
        uint32_t L;
        list_span(ls, j, ent, L);  // wave-uniform, like j
        float s[4], m[3], cc[6];
        uint32_t cnt = 0, unused = 0;
        wave_total(c, ent, L, Pass1(), s, cnt);
        cnt = wave_sum_u32(cnt);
        m[0] = s[1] / s[0], m[1] = s[2] / s[0], m[2] = s[3] / s[0];
        wave_total(c, ent, L, Pass2{m[0], m[1], m[2]}, cc, unused);
        if (lane_id() == 0) {  // every lane holds the same totals
            write_mean(o, j, cnt, s, m);
            write_cov(o, j, s[0], cc);
        }
    }
}

__global__ __launch_bounds__(kBlock) void sym3_eigen_kernel(const float* __restrict__ cov, float* __restrict__ evals,
                                                            float* __restrict__ evecs, uint32_t Q)
{
    for (unsigned long long j = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; j < Q;
         j += (unsigned long long)gridDim.x * kBlock) {
        float a[6], l[3], v[9];
#pragma unroll
        for (int s = 0; s < 6; s++) a[s] = cov[6 * j + s];
        sym3_eigen(a, l, v);
#pragma unroll
        for (int s = 0; s < 3; s++) evals[3 * j + s] = l[s];
#pragma unroll
        for (int s = 0; s < 9; s++) evecs[9 * j + s] = v[s];
    }
}

bool in_range(long long n) { return n >= 0 && n <= kMomentsMax; }

int lane_grid(long long Q) { return (int)std::min<long long>((Q + kBlock - 1) / kBlock, kLaneGridCap); }

int wave_grid(long long lists) { return (int)std::min<long long>((lists + kWaves - 1) / kWaves, kWaveGrid); }

size_t lists_scratch(long long Q) { return align_up((size_t)Q * sizeof(uint32_t)) + align_up(sizeof(uint32_t)); }

// The checks that the two forms share; `who` names the entry point.
int check_common(const std::string& who, const float* points, long long P, long long Q, const int32_t* count,
                 const float* mean, const float* cov, const float* evals, const float* evecs)
{
    if (!in_range(P)) return fail(HIDEGS_E_ARG, who + ": P must be in [0, 2^31)");
    if (!in_range(Q)) return fail(HIDEGS_E_ARG, who + ": Q must be in [0, 2^31)");
    if ((evals == nullptr) != (evecs == nullptr))
        return fail(HIDEGS_E_ARG, who + ": evals and evecs must both be given or both be NULL");
    if (Q == 0) return 0;
    if (P > 0 && !points) return fail(HIDEGS_E_ARG, who + ": NULL points");
    if (!count) return fail(HIDEGS_E_ARG, who + ": NULL count");
    if (!mean) return fail(HIDEGS_E_ARG, who + ": NULL mean");
    if (!cov) return fail(HIDEGS_E_ARG, who + ": NULL cov");
    return 0;
}

}  // namespace
}  // namespace hidegs

extern "C" size_t hidegs_neighbor_moments_scratch_bytes(long long Q)
{
    return Q > 0 && hidegs::in_range(Q) ? hidegs::lists_scratch(Q) : 0;
}

extern "C" int hidegs_neighbor_moments_table(const float* points, const float* weights, long long P, const int32_t* table,
                                             long long Q, int k, int32_t* count, float* mean, float* cov, float* evals,
                                             float* evecs, void* stream)
{
    using namespace hidegs;
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_neighbor_moments_table", s)) return rc;
    if (k < 1) return fail(HIDEGS_E_ARG, "neighbor_moments_table: k must be >= 1");
    if (int rc = check_common("neighbor_moments_table", points, P, Q, count, mean, cov, evals, evecs)) return rc;
    if (Q == 0) return 0;
    if (!table) return fail(HIDEGS_E_ARG, "neighbor_moments_table: NULL table");
    const Cloud c{points, weights, (uint32_t)P};
    const Lists ls{table, nullptr, nullptr, (uint32_t)k, 0u, (uint32_t)Q};
    const Out o{count, mean, cov, evals, evecs};
    if ((uint32_t)k <= kShort)
        HIDEGS_LAUNCH("moments_short", moments_short_kernel, dim3(lane_grid(Q)), dim3(kBlock), 0, s, c, ls, o);
    else if ((uint32_t)k <= kLaneBlocks * kSum)
        HIDEGS_LAUNCH("moments_lane", moments_lane_kernel, dim3(lane_grid(Q)), dim3(kBlock), 0, s, c, ls, o, (uint32_t*)nullptr,
                      (uint32_t*)nullptr);
    else
        HIDEGS_LAUNCH("moments_wave", moments_wave_kernel, dim3(wave_grid(Q)), dim3(kBlock), 0, s, c, ls, o,
                      (const uint32_t*)nullptr, (const uint32_t*)nullptr);
    return check_launch("neighbor_moments_table", s, 0);
}

extern "C" int hidegs_neighbor_moments_lists(void* scratch, size_t scratch_bytes, const float* points, const float* weights,
                                             long long P, const int32_t* starts, const int32_t* rows, long long capacity,
                                             long long Q, int32_t* count, float* mean, float* cov, float* evals,
                                             float* evecs, void* stream)
{
    using namespace hidegs;
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_neighbor_moments_lists", s)) return rc;
    if (!in_range(capacity)) return fail(HIDEGS_E_ARG, "neighbor_moments_lists: capacity must be in [0, 2^31)");
    if (int rc = check_common("neighbor_moments_lists", points, P, Q, count, mean, cov, evals, evecs)) return rc;
    if (Q == 0) return 0;
    if (!starts) return fail(HIDEGS_E_ARG, "neighbor_moments_lists: NULL starts");
    if (capacity > 0 && !rows) return fail(HIDEGS_E_ARG, "neighbor_moments_lists: NULL rows");
    if (!scratch || scratch_bytes < lists_scratch(Q))
        return fail(HIDEGS_E_ARG, "neighbor_moments_lists: scratch NULL or too small");
    Carver carve(scratch);
    uint32_t* long_list = carve.take<uint32_t>((size_t)Q);
    uint32_t* long_count = carve.take<uint32_t>(1);
    if (hipMemsetAsync(long_count, 0, sizeof(uint32_t), s) != hipSuccess)
        return fail(HIDEGS_E_HIP, "neighbor_moments_lists: clearing the long-list counter failed");
    const Cloud c{points, weights, (uint32_t)P};
    const Lists ls{nullptr, starts, rows, 0u, (uint32_t)capacity, (uint32_t)Q};
    const Out o{count, mean, cov, evals, evecs};
    HIDEGS_LAUNCH("moments_lane", moments_lane_kernel, dim3(lane_grid(Q)), dim3(kBlock), 0, s, c, ls, o, long_list, long_count);
    if ((unsigned long long)capacity > kLaneBlocks * kSum)  // no long list otherwise
        HIDEGS_LAUNCH("moments_wave", moments_wave_kernel, dim3(wave_grid(std::min(Q, capacity / (kLaneBlocks * kSum)))),
                      dim3(kBlock), 0, s, c, ls, o, (const uint32_t*)long_list, (const uint32_t*)long_count);
    return check_launch("neighbor_moments_lists", s, 0);
}

extern "C" int hidegs_sym3_eigen(const float* cov, float* evals, float* evecs, long long Q, void* stream)
{
    using namespace hidegs;
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_sym3_eigen", s)) return rc;
    if (!in_range(Q)) return fail(HIDEGS_E_ARG, "sym3_eigen: Q must be in [0, 2^31)");
    if (Q == 0) return 0;
    if (!cov) return fail(HIDEGS_E_ARG, "sym3_eigen: NULL cov");
    if (!evals) return fail(HIDEGS_E_ARG, "sym3_eigen: NULL evals");
    if (!evecs) return fail(HIDEGS_E_ARG, "sym3_eigen: NULL evecs");
    HIDEGS_LAUNCH("sym3_eigen", sym3_eigen_kernel, dim3(lane_grid(Q)), dim3(kBlock), 0, s, cov, evals, evecs, (uint32_t)Q);
    return check_launch("sym3_eigen", s, 0);
}
