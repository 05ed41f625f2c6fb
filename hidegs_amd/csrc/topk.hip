// topk.hip -- top-k row selection (include/hidegs_topk.h): a byte mask of the min(k, candidates) best-scored
// candidate rows, ties broken by row index.  A radix select over the scores' order keys, not a sort: nothing
// is moved, the scores are read six times and the mask is written once.
//
// Four digit passes of 8 bits, from the top.  topk_hist_kernel<P> counts, per value of digit P, the candidates
// whose higher digits equal the prefix chosen so far: workgroup histogram in LDS, then one global add per
// non-empty bin.  The digit that holds the k-th best key is picked by every workgroup of the NEXT launch in
// its prologue (next_state: a 256-bin scan from the top), redundantly and identically, so that no launch of
// its own and no hand-off between workgroups is needed; workgroup 0 also stores the state for the launch
// after that.  After the fourth digit the threshold key T and the tie quota r are known.
//
// Ties (key == T) are taken in row order, the two-pass shape of select_count / select_write in rows.hip:
// topk_tie_count_kernel writes each tile's number of ties, topk_write_kernel forms its tile's offset (adding
// up the counts before it, or from their scan above kOwnTiles tiles), ranks the ties inside the tile and
// writes flags_out and info.  Where every tie is selected (r == their number: tie-free scores, k >= c) both
// kernels skip the ranking; that is decided from the state alone, so it is the same in every workgroup.
//
// Launch boundaries are the only synchronisation.  The histograms are the only scratch that must start at
// zero and are cleared by a memset node of the call; the states and tile counts are written before they are
// read.
#include <stdint.h>

#include <string>

#include "../../include/hidegs_topk.h"
#include "block_scan.h"
#include "common.h"

namespace hidegs {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;  // 4
constexpr int kItems = 16;                      // rows per thread: four 16-byte score loads, one 16-byte mask load
constexpr int kTile = kBlock * kItems;          // 4096
constexpr int kOwnTiles = 512;                  // up to here topk_write_kernel adds the tie counts before it itself
constexpr long long kTopkMax = 0x7fffffffLL;    // counts and ranks are u32, tile counts fit the grid
constexpr int kRadix = 256;                     // kBlock == kRadix: one thread per bin
constexpr int kPasses = 4;
constexpr int kHistGrid = 2048;                 // workgroups of a digit pass: each flushes its bins once
static_assert(kBlock == kRadix, "one thread per bin");

// What is known after digit pass p; state[p] in scratch.
struct State {
    uint32_t prefix;  // the digits chosen so far, in place; after pass 3 the threshold key T
    uint32_t krem;    // how many are still to be taken among the candidates that match prefix; after pass 3: r
    uint32_t c;       // candidates
    uint32_t ksel;    // min(k, c)
    uint32_t ties;    // candidates in the chosen bin; after pass 3: those with key == T
    uint32_t pad[3];
};

__device__ __forceinline__ uint32_t ord_key(uint32_t b)
{
    if ((b & 0x7fffffffu) > 0x7f800000u) return 0u;  // NaN
    if (b == 0x80000000u) b = 0u;                    // -0.0
    return (b >> 31) ? ~b : b | 0x80000000u;
}

// The canonical score bits of a key (info[2]).
__device__ __forceinline__ uint32_t score_of_key(uint32_t key)
{
    if (key == 0u) return 0x7fc00000u;
    return (key >> 31) ? key & 0x7fffffffu : ~key;
}

// key[j] = order key of row base + threadIdx.x * kItems + j (0 past n); bit j of the result: that row is a
// candidate.  16-byte loads on a full tile of an aligned base (the tile base is a multiple of 16 rows).
__device__ __forceinline__ uint32_t load_keys(const uint32_t* __restrict__ scores, const uint8_t* among, long long base,
                                              long long n, int vec_s, int vec_a, uint32_t (&key)[kItems])
{
    const long long i0 = base + (long long)threadIdx.x * kItems;
    const bool full = base + kTile <= n;  // workgroup-uniform
    if (full && vec_s) {
        const uint4* p = reinterpret_cast<const uint4*>(scores + i0);
        uint4 v[kItems / 4];
#pragma unroll
        for (int q = 0; q < kItems / 4; q++) v[q] = p[q];
#pragma unroll
        for (int q = 0; q < kItems / 4; q++) {
            key[4 * q + 0] = ord_key(v[q].x);
            key[4 * q + 1] = ord_key(v[q].y);
            key[4 * q + 2] = ord_key(v[q].z);
            key[4 * q + 3] = ord_key(v[q].w);
        }
    } else {
#pragma unroll
        for (int j = 0; j < kItems; j++) key[j] = i0 + j < n ? ord_key(scores[i0 + j]) : 0u;
    }
    uint32_t cand = 0;
    if (!among) {
        if (full) {
            cand = 0xffffu;
        } else {
#pragma unroll
            for (int j = 0; j < kItems; j++)
                if (i0 + j < n) cand |= 1u << j;
        }
    } else if (full && vec_a) {
        const uint4 v = *reinterpret_cast<const uint4*>(among + i0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < kItems; j++) cand |= (((w[j / 4] >> (8 * (j % 4))) & 0xffu) != 0 ? 1u : 0u) << j;
    } else {
#pragma unroll
        for (int j = 0; j < kItems; j++)
            if (i0 + j < n && among[i0 + j] != 0) cand |= 1u << j;
    }
    return cand;
}

// s_hist[d]++ for every lane with ok.  Equal scores are a real input (every row that was never visible scores
// 0) and would send all 64 lanes to one bin, one LDS cycle each.  So the lanes are matched on the digit first:
// twice, the lanes that share the first pending lane's digit are counted by a ballot and their lowest lane
// adds the count.  What is left after two rounds (scores that spread over the bins) adds one by one.
__device__ __forceinline__ void wave_hist_add(uint32_t* s_hist, uint32_t d, bool ok)
{
    bool pending = ok;
#pragma unroll
    for (int round = 0; round < 2; round++) {
        if (pending) {
            const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
            const bool same = d == d0;
            const uint64_t m = __ballot(same);  // of the pending lanes
            if (same) {
                const uint32_t below =
                    __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (below == 0) atomicAdd(&s_hist[d0], (uint32_t)__popcll(m));
                pending = false;
            }
        }
    }
    if (pending) atomicAdd(&s_hist[d], 1u);
}

// The state after digit pass p, from pass p's histogram and the state before it (state[p - 1]; pass 0 starts
// from k).  Scanning the bins from the top, the chosen digit is the one at which the running count reaches
// krem; the bins above it are taken whole.  With nothing to take (krem == 0) no bin is chosen and the state
// stays at krem == 0 with digit 0.  Called by every thread of the workgroup; s_pick holds 3 words.
__device__ __forceinline__ State next_state(int p, const uint32_t* hist, const State* state,
                                            uint32_t k, uint32_t* s_wave, uint32_t* s_pick)
{
    const int t = threadIdx.x;
    const uint32_t v = hist[p * kRadix + (kRadix - 1 - t)];  // thread t holds bin 255 - t
    State st;
    if (p > 0) st = state[p - 1];
    if (t == 0) s_pick[0] = s_pick[1] = s_pick[2] = 0u;
    uint32_t total;
    const uint32_t above = block_exclusive_scan(v, s_wave, &total);
    if (p == 0) {
        st.prefix = 0u;
        st.c = total;
        st.ksel = k < total ? k : total;
        st.krem = st.ksel;
    }
    if (above < st.krem && above + v >= st.krem) {  // one thread at most
        s_pick[0] = (uint32_t)(kRadix - 1 - t);
        s_pick[1] = above;
        s_pick[2] = v;
    }
    __syncthreads();
    st.prefix |= s_pick[0] << (24 - 8 * p);
    st.krem -= s_pick[1];
    st.ties = s_pick[2];
    return st;
}

// Digit pass P: hist[P][d] += the candidates with digit d whose digits above P equal the prefix.  hist is
// zero on entry.  Workgroups stride over the tiles and flush their bins once.
template <int P>
__global__ __launch_bounds__(kBlock) void topk_hist_kernel(const uint32_t* __restrict__ scores, const uint8_t* among,
                                                           long long n, uint32_t k, int ntiles,
                                                           uint32_t* hist, State* state,
                                                           int vec_s, int vec_a)
{
    __shared__ uint32_t s_hist[kRadix];
    __shared__ uint32_t s_wave[kWavesPerBlock];
    __shared__ uint32_t s_pick[3];
    const int t = threadIdx.x;
    constexpr int kShift = 24 - 8 * P;
    s_hist[t] = 0u;
    State st = {};
    if (P > 0) {
        st = next_state(P - 1, hist, state, k, s_wave, s_pick);
        if (blockIdx.x == 0 && t == 0) state[P - 1] = st;
    }
    __syncthreads();
    if (P == 0 || st.krem > 0) {  // workgroup-uniform
        const uint32_t want = P > 0 ? st.prefix >> (kShift + 8) : 0u;
        for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
            uint32_t key[kItems];
            const uint32_t cand = load_keys(scores, among, (long long)tile * kTile, n, vec_s, vec_a, key);
#pragma unroll
            for (int j = 0; j < kItems; j++) {
                const bool ok = ((cand >> j) & 1u) && (P == 0 || (key[j] >> ((kShift + 8) & 31)) == want);
                wave_hist_add(s_hist, (key[j] >> kShift) & (kRadix - 1), ok);
            }
        }
    }
    __syncthreads();
    const uint32_t mine = s_hist[t];
    if (mine) atomicAdd(&hist[P * kRadix + t], mine);
}

// Bit j: candidate row j of the thread has key == T.
__device__ __forceinline__ uint32_t equal_bits(const uint32_t (&key)[kItems], uint32_t cand, uint32_t T)
{
    uint32_t eq = 0;
#pragma unroll
    for (int j = 0; j < kItems; j++) eq |= (key[j] == T ? 1u : 0u) << j;
    return eq & cand;
}

// Forms the final state (T, r) and, where the ties have to be ranked, each tile's number of ties.
__global__ __launch_bounds__(kBlock) void topk_tie_count_kernel(const uint32_t* __restrict__ scores, const uint8_t* among,
                                                                long long n, uint32_t k,
                                                                const uint32_t* hist, State* state,
                                                                uint32_t* __restrict__ tile_counts, int vec_s, int vec_a)
{
    __shared__ uint32_t s_wave[kWavesPerBlock];
    __shared__ uint32_t s_pick[3];
    const State st = next_state(kPasses - 1, hist, state, k, s_wave, s_pick);
    if (blockIdx.x == 0 && threadIdx.x == 0) state[kPasses - 1] = st;
    if (st.krem == st.ties) return;  // every tie is selected, or nothing is: no ranks (the same in every workgroup)
    uint32_t key[kItems];
    const uint32_t cand = load_keys(scores, among, (long long)blockIdx.x * kTile, n, vec_s, vec_a, key);
    uint32_t total;
    block_exclusive_scan((uint32_t)__popc(equal_bits(key, cand, st.prefix)), s_wave, &total);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}

// counts_raw: tile_counts holds the tie counts, and the workgroup adds up those before its own; otherwise
// their exclusive scan.  flags_out may be `among`: a thread reads its 16 mask bytes before it writes them,
// and no other thread touches them.
__global__ __launch_bounds__(kBlock) void topk_write_kernel(const uint32_t* __restrict__ scores, const uint8_t* among,
                                                            long long n, const State* __restrict__ state,
                                                            const uint32_t* __restrict__ tile_counts, int counts_raw,
                                                            uint8_t* flags_out, uint32_t* __restrict__ info, int vec_s,
                                                            int vec_a, int vec_o)
{
    __shared__ uint32_t s_wave[kWavesPerBlock];
    const State st = state[kPasses - 1];
    const uint32_t T = st.prefix, r = st.krem;
    const bool rank_ties = r != st.ties;  // then 0 < r < ties; workgroup-uniform
    uint32_t tile_off = 0;
    if (rank_ties) {
        if (counts_raw) {
            uint32_t part = 0;
            for (int i = threadIdx.x; i < (int)blockIdx.x; i += kBlock) part += tile_counts[i];
            block_exclusive_scan(part, s_wave, &tile_off);
        } else {
            tile_off = tile_counts[blockIdx.x];
        }
    }
    const long long base = (long long)blockIdx.x * kTile;
    uint32_t key[kItems];
    const uint32_t cand = load_keys(scores, among, base, n, vec_s, vec_a, key);
    uint32_t gt = 0;
#pragma unroll
    for (int j = 0; j < kItems; j++) gt |= (key[j] > T ? 1u : 0u) << j;
    gt &= cand;
    uint32_t eq = equal_bits(key, cand, T);
    if (st.ksel == 0) gt = eq = 0u;  // T is no key then
    if (rank_ties) {
        uint32_t total;
        uint32_t rank = tile_off + block_exclusive_scan((uint32_t)__popc(eq), s_wave, &total);
        uint32_t kept = 0;
#pragma unroll
        for (int j = 0; j < kItems; j++) {  // ascending inside the thread, threads in order: ascending rows
            const uint32_t bit = (eq >> j) & 1u;
            kept |= (bit & (rank < r ? 1u : 0u)) << j;
            rank += bit;
        }
        eq = kept;
    }
    const uint32_t sel = gt | eq;
    const long long i0 = base + (long long)threadIdx.x * kItems;
    if (vec_o && base + kTile <= n) {
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t s4 = sel >> (4 * q);
            w[q] = (s4 & 1u) | ((s4 & 2u) << 7) | ((s4 & 4u) << 14) | ((s4 & 8u) << 21);
        }
        *reinterpret_cast<uint4*>(flags_out + i0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kItems; j++)
            if (i0 + j < n) flags_out[i0 + j] = (uint8_t)((sel >> j) & 1u);
    }
    if (info && blockIdx.x == 0 && threadIdx.x == 0) {
        info[0] = st.ksel;
        info[1] = st.c;
        info[2] = st.ksel ? score_of_key(T) : 0u;
        info[3] = r;
    }
}

int topk_tiles(long long n) { return (int)((n + kTile - 1) / kTile); }
size_t topk_scratch(long long n)
{
    return align_up((size_t)kPasses * kRadix * sizeof(uint32_t)) + align_up((size_t)kPasses * sizeof(State)) +
           align_up((size_t)topk_tiles(n) * sizeof(uint32_t));
}

}  // namespace
}  // namespace hidegs

extern "C" size_t hidegs_top_k_scratch_bytes(long long n)
{
    return n > 0 && n <= hidegs::kTopkMax ? hidegs::topk_scratch(n) : 0;
}

extern "C" int hidegs_top_k_mask_f32(void* scratch, size_t scratch_bytes, const float* scores,
                                     const unsigned char* among, long long n, long long k, unsigned char* flags_out,
                                     uint32_t* info, void* stream)
{
    using namespace hidegs;
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_top_k_mask_f32", s)) return rc;
    if (n < 0 || n > kTopkMax) return fail(HIDEGS_E_ARG, "top_k_mask: n must be in [0, 2^31)");
    if (k < 0 || k > kTopkMax) return fail(HIDEGS_E_ARG, "top_k_mask: k must be in [0, 2^31)");
    if (n == 0) return 0;
    if (!scores) return fail(HIDEGS_E_ARG, "top_k_mask: NULL scores");
    if (!flags_out) return fail(HIDEGS_E_ARG, "top_k_mask: NULL flags_out");
    if (!scratch || scratch_bytes < topk_scratch(n)) return fail(HIDEGS_E_ARG, "top_k_mask: scratch too small");
    const int nt = topk_tiles(n);
    Carver c(scratch);
    uint32_t* hist = c.take<uint32_t>((size_t)kPasses * kRadix);
    State* state = c.take<State>(kPasses);
    uint32_t* counts = c.take<uint32_t>(nt);
    const uint32_t* keys = reinterpret_cast<const uint32_t*>(scores);
    const int vec_s = aligned16(scores), vec_a = aligned16(among), vec_o = aligned16(flags_out);
    const uint32_t kk = (uint32_t)k;
    const hipError_t e = hipMemsetAsync(hist, 0, (size_t)kPasses * kRadix * sizeof(uint32_t), s);
    if (e != hipSuccess) return fail(HIDEGS_E_HIP, std::string("top_k_mask: clearing the histograms: ") + hipGetErrorString(e));
    const dim3 hist_grid(nt < kHistGrid ? nt : kHistGrid), block(kBlock);
    HIDEGS_LAUNCH("topk_hist", topk_hist_kernel<0>, hist_grid, block, 0, s, keys, among, n, kk, nt, hist, state, vec_s, vec_a);
    HIDEGS_LAUNCH("topk_hist", topk_hist_kernel<1>, hist_grid, block, 0, s, keys, among, n, kk, nt, hist, state, vec_s, vec_a);
    HIDEGS_LAUNCH("topk_hist", topk_hist_kernel<2>, hist_grid, block, 0, s, keys, among, n, kk, nt, hist, state, vec_s, vec_a);
    HIDEGS_LAUNCH("topk_hist", topk_hist_kernel<3>, hist_grid, block, 0, s, keys, among, n, kk, nt, hist, state, vec_s, vec_a);
    HIDEGS_LAUNCH("topk_tie_count", topk_tie_count_kernel, dim3(nt), block, 0, s, keys, among, n, kk, hist, state, counts,
                  vec_s, vec_a);
    const int own = nt <= kOwnTiles;
    if (!own)
        HIDEGS_LAUNCH("topk_offsets", scan_small_kernel, dim3(1), dim3(kScanBlock), 0, s, counts, nt, (uint32_t*)nullptr);
    HIDEGS_LAUNCH("topk_write", topk_write_kernel, dim3(nt), block, 0, s, keys, among, n, state, counts, own, flags_out, info,
                  vec_s, vec_a, vec_o);
    return check_launch("top_k_mask", s, 0);
}
