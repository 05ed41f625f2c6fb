// common.h -- shared plumbing of the C-ABI library: error channel, stream handle,
// scratch carving, launch checks and a few wave64 helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/hidegs.h"

namespace hidegs {

// Last error message of the calling thread (hidegs_last_error()).
void set_error(const std::string& msg);
const std::string& last_error();

inline int fail(int code, const std::string& msg)
{
    set_error(msg);
    return code;
}

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Checks the launch queue after kernels were enqueued; with debug != 0 it also
// synchronises the stream so an asynchronous fault is reported at its stage
// (the reference's CHECK_CUDA(..., debug), auxiliary.h:23-30).
int check_launch(const char* stage, hipStream_t stream, int debug);

// Library-wide debug mode (hidegs_set_debug): every launch check synchronises, and the sort reads
// back the partition queue's error word.
bool debug_enabled();

// Sticky partition-queue error word of the current device (primitives.hip); synchronises `stream`.
// Reads and clears it in one device-side exchange.
int queue_error(hipStream_t stream, int clear, uint32_t* flags);

// Asynchronous error words: one u32 per stream in a page of mapped, coherent pinned host memory.  A
// sort's last kernel ORs its partition queue's error bits into its stream's word (system-scope vector
// stores), so that the failure surfaces without a host synchronisation.  The page is allocated by the
// first entry-point call of any kind that does not come from a stream being captured into a graph.
// async_error_slot() returns the device address of `stream`'s word -- of the graph word when `stream`
// is being captured (a graph may be replayed on any stream) -- or NULL if the page does not exist (it
// could not be allocated, or every call so far came from a capturing stream; then only the debug mode
// and hidegs_queue_error report that call's queue errors).
uint32_t* async_error_slot(hipStream_t stream);
// Called first by every compute entry point: if `stream`'s word (or the graph word) is set it is taken
// (exchanged with 0) and turned into HIDEGS_E_ASYNC with its message, so a call on the stream of a failed
// sort (any call, after a failed graph replay), made once that sort's last kernel has run, fails loudly
// instead of running.
int take_async_error(const char* what, hipStream_t stream);
// `stream`'s word's bits and the graph word's, taken (exchanged with 0); 0 when none are pending.
uint32_t take_async_bits(hipStream_t stream);

// The stable u64-key radix sort over key bits [b, e) (primitives.hip), as distCUDA2 (knn.hip) calls it.
size_t sort_u64_scratch(long long n);
int sort_pairs_u64(void* scratch, size_t bytes, const uint64_t* ki, uint64_t* ko, const uint32_t* vi, uint32_t* vo,
                   long long n, int b, int e, hipStream_t s);
// The same over u32 keys, as the neighbour-list transpose (neighbor_grad.hip) calls it.
size_t sort_u32_scratch(long long n);
int sort_pairs_u32(void* scratch, size_t bytes, const uint32_t* ki, uint32_t* ko, const uint32_t* vi, uint32_t* vo,
                   long long n, int b, int e, hipStream_t s);

// 256-byte aligned carving of one caller-provided scratch buffer.
constexpr size_t kAlign = 256;
inline size_t align_up(size_t n) { return (n + kAlign - 1) & ~(kAlign - 1); }

struct Carver {
    char* base;
    size_t used = 0;
    explicit Carver(void* b) : base(static_cast<char*>(b)) {}
    template <typename T>
    T* take(size_t count)
    {
        T* p = reinterpret_cast<T*>(base ? base + used : nullptr);
        used += align_up(count * sizeof(T));
        return p;
    }
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- wave64 helpers (device) --------------------------------------------------
constexpr int kWave = 64;

__device__ __forceinline__ int lane_id() { return __lane_id(); }

// Block b of nb -> a work index such that consecutive work indices run on one XCD: the dispatcher
// deals workgroups to the 8 XCDs round-robin (b, b+8, ... share an XCD's L2), so this hands each
// XCD a contiguous range of indices.
__device__ __forceinline__ int xcd_swizzle(int b, int nb)
{
    const int per = nb / 8, rem = nb % 8, x = b % 8, k = b / 8;
    return (x < rem) ? x * (per + 1) + k : rem * (per + 1) + (x - rem) * per + k;
}

template <typename T>
__device__ __forceinline__ T wave_shfl_xor(T v, int m)
{
    return __shfl_xor(v, m, kWave);
}

// Inclusive prefix sum over the 64 lanes with DPP moves (row_shr within rows of 16, then the
// row_bcast:15 / row_bcast:31 carries of GFX9): VALU-latency steps instead of LDS-path shuffles.
// Every lane of the wave must be active.
__device__ __forceinline__ uint32_t wave_inclusive_scan_u32(uint32_t v)
{
    const int lane = lane_id(), rl = lane & 15;
    int x = (int)v, t;
    t = __builtin_amdgcn_mov_dpp(x, 0x111, 0xf, 0xf, false);  // row_shr:1
    if (rl >= 1) x += t;
    t = __builtin_amdgcn_mov_dpp(x, 0x112, 0xf, 0xf, false);  // row_shr:2
    if (rl >= 2) x += t;
    t = __builtin_amdgcn_mov_dpp(x, 0x114, 0xf, 0xf, false);  // row_shr:4
    if (rl >= 4) x += t;
    t = __builtin_amdgcn_mov_dpp(x, 0x118, 0xf, 0xf, false);  // row_shr:8
    if (rl >= 8) x += t;
    t = __builtin_amdgcn_mov_dpp(x, 0x142, 0xf, 0xf, false);  // row_bcast:15
    if ((lane & 31) >= 16) x += t;
    t = __builtin_amdgcn_mov_dpp(x, 0x143, 0xf, 0xf, false);  // row_bcast:31
    if (lane >= 32) x += t;
    return (uint32_t)x;
}

// Reduction of one u32 per lane over the 64 lanes by an idempotent operation (min, max, and, or), with
// the same DPP moves: row_shr:1/2/4/8 leave each row's result in its lane 15, row_bcast:15 and
// row_bcast:31 carry it on to lane 63, which is read back as a wave-uniform value.  A lane with no
// source keeps its own value (op(x, x) == x), so no identity is needed.  Seven VALU steps and a
// v_readlane where the __shfl_xor chain takes six ds_bpermute round trips.  Every lane of the wave must
// be active.
#define HIDEGS_DPP_SELF(x, ctrl, rows) ((uint32_t)__builtin_amdgcn_update_dpp((int)(x), (int)(x), ctrl, rows, 0xf, false))
template <typename Op>
__device__ __forceinline__ uint32_t wave_reduce_u32(uint32_t x, Op op)
{
    x = op(x, HIDEGS_DPP_SELF(x, 0x111, 0xf));  // row_shr:1
    x = op(x, HIDEGS_DPP_SELF(x, 0x112, 0xf));  // row_shr:2
    x = op(x, HIDEGS_DPP_SELF(x, 0x114, 0xf));  // row_shr:4
    x = op(x, HIDEGS_DPP_SELF(x, 0x118, 0xf));  // row_shr:8
    x = op(x, HIDEGS_DPP_SELF(x, 0x142, 0xa));  // row_bcast:15 into rows 1 and 3
    x = op(x, HIDEGS_DPP_SELF(x, 0x143, 0xc));  // row_bcast:31 into rows 2 and 3
    return (uint32_t)__builtin_amdgcn_readlane((int)x, kWave - 1);
}
#undef HIDEGS_DPP_SELF
struct OpMinU32 {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; }
};
struct OpMaxU32 {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
};
struct OpAndU32 {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a & b; }
};
struct OpOrU32 {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a | b; }
};
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { return wave_reduce_u32(v, OpMinU32()); }
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { return wave_reduce_u32(v, OpMaxU32()); }
__device__ __forceinline__ uint32_t wave_and_u32(uint32_t v) { return wave_reduce_u32(v, OpAndU32()); }
__device__ __forceinline__ uint32_t wave_or_u32(uint32_t v) { return wave_reduce_u32(v, OpOrU32()); }

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, kWave));
    return v;
}
__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, kWave));
    return v;
}
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// Value of lane `src` (wave-uniform) as a wave-uniform (scalar-register) float.
__device__ __forceinline__ float uniform_lane(float v, int src)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// Mask of the lanes below `lane`: its popcount with a ballot is the lane's rank among the set lanes.
__device__ __forceinline__ uint64_t lanes_below(int lane) { return (lane == 0) ? 0ull : (~0ull >> (64 - lane)); }

// Appends one entry per lane with `flag` to a list whose length is *counter: one ballot, one atomic by lane 0,
// the base handed on by readfirstlane, every flagged lane its own slot in lane order.  Returns the caller's
// slot, valid where `flag` holds.  Every lane of the wave must be active.
__device__ __forceinline__ uint32_t wave_append(bool flag, uint32_t* counter)
{
    const uint64_t m = __ballot(flag);
    if (!m) return 0;
    const int lane = lane_id();
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    return base + (uint32_t)__popcll(m & lanes_below(lane));
}

// A global store with a cache policy, for output that is streamed out and not read again by its kernel
// (its counterpart on the load side is __builtin_nontemporal_load):
//   kPlain    an ordinary write-back store;
//   kStream   global_store_* ... nt: the line is marked for early eviction from the L2;
//   kThrough  global_store_dword/dwordx2 ... sc1: written through the L2 at agent scope.  4- and 8-byte
//             values only; other sizes take the stream policy.
// T is a scalar or a native ext_vector_type (for 16 bytes 4 x uint32_t: the builtin does not take uint4).
enum StorePolicy { kPlain = 0, kStream = 1, kThrough = 2 };
template <StorePolicy P, typename T>
__device__ __forceinline__ void stream_store(T* p, const T v)
{
    if constexpr (P == kPlain) {
        *p = v;
    } else if constexpr (P == kThrough && (sizeof(T) == 4 || sizeof(T) == 8)) {
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        __builtin_nontemporal_store(v, p);
    }
}

__device__ __forceinline__ bool finite3(float x, float y, float z)
{
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;  // false for a NaN
}

}  // namespace hidegs

namespace hidegs {

// Per-kernel device timing (hidegs_kernel_timing in include/hidegs.h): when enabled, each
// launch made through HIDEGS_LAUNCH is bracketed by two hipEvents recorded on its stream;
// the durations are resolved and accumulated per kernel name when they are queried.
bool kernel_timing_enabled();
struct LaunchTimer {
    const char* name;
    hipStream_t stream;
    hipEvent_t start = nullptr, stop = nullptr;
    LaunchTimer(const char* n, hipStream_t s);
    ~LaunchTimer();
};

}  // namespace hidegs

#define HIDEGS_LAUNCH(NAME, KERNEL, GRID, BLOCK, SHMEM, STREAM, ...)                        \
    do {                                                                                   \
        if (::hidegs::kernel_timing_enabled()) {                                           \
            ::hidegs::LaunchTimer _t(NAME, STREAM);                                        \
            hipLaunchKernelGGL(KERNEL, GRID, BLOCK, SHMEM, STREAM, __VA_ARGS__);           \
        } else {                                                                           \
            hipLaunchKernelGGL(KERNEL, GRID, BLOCK, SHMEM, STREAM, __VA_ARGS__);           \
        }                                                                                  \
    } while (0)
