// neighbor_grad.hip -- transposed neighbour lists and the backward of the SUM and MEAN field reductions
// (include/hidegs_neighbor_grad.h).
//
// The transpose is a stable sort, not a count / cursor / fill: emit (row or P, position) per position, sort_pairs_u32
// over the bit_length(P) key bits, then
//   transpose_starts  one thread per row r in [0, P]: the first position of the sorted keys that is not below r is
//                     starts_t[r], empty rows included; the lengths' maximum and the named rows go into info with
//                     one integer atomic each per wave;
//   transpose_decode  one thread per sorted position: its query (position / k, or a search of starts), and -1 from
//                     the first invalid key on.
// The field gradient and the row-weight gradient are reductions over the transposed lists and run through
// hidegs_neighbor_reduce_lists itself -- its kernels, its rule, its bits.  What is new for them is the gather of
// the coefficients c[entry_t] and, for the weight gradients, the per-entry dot product
//   ngrad_dot         one entry per group of G lanes, the columns across the lanes (16-byte loads where every width
//                     of the launch is a multiple of 4 and every base is aligned), a butterfly over the group, lane
//                     0 writes.  No (E, w) temporary.
// No floating-point atomic, no workgroup waits on another; capped launches stride past their caps.
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/hidegs_neighbor_grad.h"
#include "../../include/hidegs_neighbor_reduce.h"
#include "common.h"

namespace hidegs {
namespace {

constexpr int kBlock = 256;
constexpr long long kGradMax = 0x7fffffffLL;
constexpr int kGridCap = 8192;  // workgroups of the per-position kernels: 32 per CU, then by stride
constexpr int kMaxFields = 8;   // fields of one ngrad_dot launch

// The forward structure: a (Q, k) table, or starts (Q + 1) and rows (E).
struct Forward {
    const int32_t* table;
    const int32_t* starts;
    const int32_t* rows;
    uint32_t k, E, Q, P;
};

__device__ __forceinline__ const int32_t* entries(const Forward& fw) { return fw.table ? fw.table : fw.rows; }

// The query whose list holds position pos < E; false where no list does.  List form: the number of starts[1 .. Q]
// at or below pos, by bisection -- nothing outside starts[0 .. Q] is read, whatever starts holds.
__device__ __forceinline__ bool query_of(const Forward& fw, uint32_t pos, uint32_t& j)
{
    if (fw.table) {
        j = pos / fw.k;
        return true;
    }
    uint32_t lo = 0, hi = fw.Q;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (fw.starts[mid + 1] <= (int32_t)pos)
            lo = mid + 1;
        else
            hi = mid;
    }
    j = lo;
    return lo < fw.Q && fw.starts[lo] <= (int32_t)pos;
}

__global__ __launch_bounds__(kBlock) void transpose_emit_kernel(Forward fw, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const int32_t* __restrict__ ent = entries(fw);
    for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < fw.E;
         i += (unsigned long long)gridDim.x * kBlock) {
        const uint32_t pos = (uint32_t)i;
        const uint32_t r = (uint32_t)ent[pos];  // a negative row is above every P
        uint32_t j;
        keys[pos] = (r < fw.P && query_of(fw, pos, j)) ? r : fw.P;
        vals[pos] = pos;
    }
}

// The first position of keys[0 .. n) that is not below r.
__device__ __forceinline__ uint32_t first_not_below(const uint32_t* __restrict__ keys, uint32_t n, uint32_t r)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < r)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// info is cleared by the call; every wave is whole (the loop is workgroup-uniform).
__global__ __launch_bounds__(kBlock) void transpose_starts_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t P,
                                                                  int32_t* __restrict__ starts_t, int32_t* __restrict__ info)
{
    for (unsigned long long base = (unsigned long long)blockIdx.x * kBlock; base <= P; base += (unsigned long long)gridDim.x * kBlock) {
        const unsigned long long r64 = base + threadIdx.x;
        const bool active = r64 <= P;
        const uint32_t r = (uint32_t)r64;
        const uint32_t a = active ? first_not_below(keys, n, r) : 0u;
        uint32_t b = (uint32_t)__shfl_down((int)a, 1, kWave);
        const bool row = active && r < P;
        if (row && lane_id() == kWave - 1) b = first_not_below(keys, n, r + 1);
        if (active) starts_t[r] = (int32_t)a;
        const uint32_t len = row ? b - a : 0u;
        const uint32_t longest = wave_max_u32(len);
        const uint32_t named = (uint32_t)__popcll(__ballot(len > 0));
        if (lane_id() == 0 && named) {
            atomicMax(&info[2], (int32_t)longest);
            atomicAdd(&info[3], (int32_t)named);
        }
        if (active && r == P) info[0] = (int32_t)a;
    }
}

// keys == NULL: every position is tail (P == 0, or lists without a query).  entry_t holds the sorted positions and gets its tail here.
__global__ __launch_bounds__(kBlock) void transpose_decode_kernel(Forward fw, const uint32_t* __restrict__ keys,
                                                                  int32_t* __restrict__ query_t, int32_t* __restrict__ entry_t)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < fw.E;
         i += (unsigned long long)gridDim.x * kBlock) {
        uint32_t j = 0;
        const bool valid = keys && keys[i] < fw.P && query_of(fw, (uint32_t)entry_t[i], j);
        if (!valid) entry_t[i] = -1;
        query_t[i] = valid ? (int32_t)j : -1;
    }
}

// c[i] for the transposed position i: the entry weight of its forward position (1.0f without), for c_mean divided
// by its query's weight total.  0 in the tail, which no list holds.
__global__ __launch_bounds__(kBlock) void ngrad_coef_kernel(uint32_t E, uint32_t Q, const int32_t* __restrict__ query_t,
                                                            const int32_t* __restrict__ entry_t, const float* __restrict__ ew,
                                                            const float* __restrict__ wsum, float* __restrict__ c_sum,
                                                            float* __restrict__ c_mean)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < E;
         i += (unsigned long long)gridDim.x * kBlock) {
        const uint32_t e = (uint32_t)entry_t[i], j = (uint32_t)query_t[i];
        const bool held = e < E && j < Q;  // anything else is no transposed entry of this structure: nothing is read for it
        const float w = !held ? 0.f : (ew ? ew[e] : 1.f);
        if (c_sum) c_sum[i] = w;
        if (c_mean) c_mean[i] = !held ? 0.f : w / wsum[j];
    }
}

// grad[r, :] *= weights[r] for every row that is named at least once.
__global__ __launch_bounds__(kBlock) void ngrad_scale_kernel(float* __restrict__ grad, uint32_t width, unsigned long long n,
                                                             const float* __restrict__ weights, const int32_t* __restrict__ starts_t)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * kBlock) {
        const uint32_t r = (uint32_t)(i / width);
        if (starts_t[r + 1] > starts_t[r]) grad[i] = grad[i] * weights[r];
    }
}

struct DotField {
    const float* src;
    const float* out;
    const float* g;
    uint32_t width;
    int mean;
};

struct DotFields {
    DotField f[kMaxFields];
    int n, any_mean;
};

template <int G, int V>
__global__ __launch_bounds__(kBlock) void ngrad_dot_kernel(Forward fw, DotFields fs, const float* __restrict__ weights,
                                                           const float* __restrict__ ew, const float* __restrict__ wsum,
                                                           float* __restrict__ gew, float* __restrict__ per_entry, int accumulate)
{
    constexpr int kGroups = kBlock / G;
    const uint32_t g = threadIdx.x % G;
    const int32_t* __restrict__ ent = entries(fw);
    for (unsigned long long base = (unsigned long long)blockIdx.x * kGroups; base < fw.E;
         base += (unsigned long long)gridDim.x * kGroups) {  // workgroup-uniform
        const unsigned long long p64 = base + threadIdx.x / G;
        const bool active = p64 < fw.E;
        const uint32_t pos = (uint32_t)p64;
        int32_t r = -1;
        uint32_t j = 0;
        if (active) {
            r = ent[pos];
            if ((uint32_t)r >= fw.P || !query_of(fw, pos, j)) r = -1;
        }
        float ds = 0.f, dm = 0.f;
        if (r >= 0) {  // the same in every lane of the group
            for (int i = 0; i < fs.n; i++) {
                const DotField fd = fs.f[i];
                const float* __restrict__ x = fd.src + (size_t)r * fd.width;
                const float* __restrict__ o = fd.out + (size_t)j * fd.width;
                const float* __restrict__ go = fd.g + (size_t)j * fd.width;
                float acc = 0.f;
                if constexpr (V == 4) {
                    for (uint32_t c = 4 * g; c < fd.width; c += 4 * G) {
                        const float4 xv = *reinterpret_cast<const float4*>(x + c);
                        const float4 gv = *reinterpret_cast<const float4*>(go + c);
                        float4 ov = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (fd.mean) ov = *reinterpret_cast<const float4*>(o + c);
                        acc = fmaf(gv.x, fd.mean ? xv.x - ov.x : xv.x, acc);
                        acc = fmaf(gv.y, fd.mean ? xv.y - ov.y : xv.y, acc);
                        acc = fmaf(gv.z, fd.mean ? xv.z - ov.z : xv.z, acc);
                        acc = fmaf(gv.w, fd.mean ? xv.w - ov.w : xv.w, acc);
                    }
                } else {
                    for (uint32_t c = g; c < fd.width; c += G) acc = fmaf(go[c], fd.mean ? x[c] - o[c] : x[c], acc);
                }
                if (fd.mean)
                    dm += acc;
                else
                    ds += acc;
            }
        }
#pragma unroll
        for (int m = 1; m < G; m <<= 1) {  // every lane of the wave is here
            ds += __shfl_xor(ds, m, kWave);
            dm += __shfl_xor(dm, m, kWave);
        }
        if (!active || g != 0) continue;
        float d = 0.f, wr = 1.f;
        if (r >= 0) {
            d = fs.any_mean ? ds + dm / wsum[j] : ds;
            if (weights) wr = weights[r];
        }
        if (gew) {
            const float v = r >= 0 ? wr * d : 0.f;
            gew[pos] = accumulate ? gew[pos] + v : v;
        }
        if (per_entry) {
            const float v = r >= 0 ? (ew ? ew[pos] * d : d) : 0.f;
            per_entry[pos] = accumulate ? per_entry[pos] + v : v;
        }
    }
}

bool in_range(long long n) { return n >= 0 && n <= kGradMax; }

int bit_length(long long n)
{
    int b = 0;
    while (n >> b) b++;
    return b;
}

int flat_grid(unsigned long long n) { return (int)std::max<unsigned long long>(1, std::min<unsigned long long>((n + kBlock - 1) / kBlock, kGridCap)); }

size_t transpose_scratch(long long E) { return 3 * align_up((size_t)E * sizeof(uint32_t)) + align_up(sort_u32_scratch(E)); }

// The checks of the two transposes, in the order of the header.
int check_transpose(const std::string& who, long long P, long long Q, long long E, const void* ent, const int32_t* starts, bool lists,
                    const void* scratch, size_t scratch_bytes, const int32_t* starts_t, const int32_t* query_t,
                    const int32_t* entry_t, const int32_t* info)
{
    if (!in_range(P)) return fail(HIDEGS_E_ARG, who + ": P must be in [0, 2^31)");
    if (!in_range(Q)) return fail(HIDEGS_E_ARG, who + ": Q must be in [0, 2^31)");
    if (!in_range(E)) return fail(HIDEGS_E_ARG, who + ": at most 2^31 - 1 entry positions");
    if (E > 0 && !ent) return fail(HIDEGS_E_ARG, who + (lists ? ": NULL rows" : ": NULL table"));
    if (lists && Q > 0 && !starts) return fail(HIDEGS_E_ARG, who + ": NULL starts");
    if (!starts_t || !info) return fail(HIDEGS_E_ARG, who + ": NULL starts_t or info");
    if (E > 0 && (!query_t || !entry_t)) return fail(HIDEGS_E_ARG, who + ": NULL query_t or entry_t");
    if (E > 0 && P > 0 && (!lists || Q > 0) && (!scratch || scratch_bytes < transpose_scratch(E)))
        return fail(HIDEGS_E_ARG, who + ": scratch NULL or too small");
    return 0;
}

int transpose(const char* who, void* scratch, size_t scratch_bytes, const Forward& fw, int32_t* starts_t, int32_t* query_t,
              int32_t* entry_t, int32_t* info, hipStream_t s)
{
    if (hipMemsetAsync(info, 0, 4 * sizeof(int32_t), s) != hipSuccess) return fail(HIDEGS_E_HIP, std::string(who) + ": clearing info failed");
    const bool sorted = fw.E > 0 && fw.P > 0 && (fw.table || fw.Q > 0);  // otherwise no entry is valid: zero starts_t, all tail
    uint32_t* keys_sorted = nullptr;
    if (sorted) {
        Carver carve(scratch);
        uint32_t* keys = carve.take<uint32_t>(fw.E);
        keys_sorted = carve.take<uint32_t>(fw.E);
        uint32_t* vals = carve.take<uint32_t>(fw.E);
        void* sort_tmp = carve.take<char>(sort_u32_scratch(fw.E));
        HIDEGS_LAUNCH("transpose_emit", transpose_emit_kernel, dim3(flat_grid(fw.E)), dim3(kBlock), 0, s, fw, keys, vals);
        if (int rc = sort_pairs_u32(sort_tmp, scratch_bytes - (size_t)((char*)sort_tmp - (char*)scratch), keys, keys_sorted, vals,
                                    reinterpret_cast<uint32_t*>(entry_t), fw.E, 0, bit_length(fw.P), s))
            return rc;
    }
    HIDEGS_LAUNCH("transpose_starts", transpose_starts_kernel, dim3(flat_grid((unsigned long long)fw.P + 1)), dim3(kBlock), 0, s,
                  (const uint32_t*)keys_sorted, sorted ? fw.E : 0u, fw.P, starts_t, info);
    if (fw.E > 0)
        HIDEGS_LAUNCH("transpose_decode", transpose_decode_kernel, dim3(flat_grid(fw.E)), dim3(kBlock), 0, s, fw,
                      (const uint32_t*)keys_sorted, query_t, entry_t);
    return check_launch(who, s, 0);
}

struct BackwardScratch {
    float *c_sum, *c_mean, *per_entry;
    void* reduce;
    size_t reduce_bytes, total;
    BackwardScratch(void* base, long long P, long long E)
    {
        Carver carve(base);
        c_sum = carve.take<float>((size_t)E);
        c_mean = carve.take<float>((size_t)E);
        per_entry = carve.take<float>((size_t)E);
        reduce_bytes = hidegs_neighbor_reduce_scratch_bytes(P, 1);
        reduce = carve.take<char>(reduce_bytes);
        total = carve.used;
    }
};

int zero(const char* who, void* p, size_t bytes, hipStream_t s)
{
    if (p && bytes && hipMemsetAsync(p, 0, bytes, s) != hipSuccess) return fail(HIDEGS_E_HIP, std::string(who) + ": zero fill failed");
    return 0;
}

template <int G, int V>
void launch_dot(const Forward& fw, const DotFields& fs, const float* weights, const float* ew, const float* wsum, float* gew,
                float* per_entry, int accumulate, hipStream_t s)
{
    const unsigned long long groups = kBlock / G;
    const int grid = (int)std::max<unsigned long long>(1, std::min<unsigned long long>((fw.E + groups - 1) / groups, 4 * kGridCap));
    HIDEGS_LAUNCH("ngrad_dot", (ngrad_dot_kernel<G, V>), dim3(grid), dim3(kBlock), 0, s, fw, fs, weights, ew, wsum, gew, per_entry,
                  accumulate);
}

template <int V>
void launch_dot_lanes(int lanes, const Forward& fw, const DotFields& fs, const float* weights, const float* ew, const float* wsum,
                      float* gew, float* per_entry, int accumulate, hipStream_t s)
{
    if (lanes <= 1)
        launch_dot<1, V>(fw, fs, weights, ew, wsum, gew, per_entry, accumulate, s);
    else if (lanes <= 4)
        launch_dot<4, V>(fw, fs, weights, ew, wsum, gew, per_entry, accumulate, s);
    else if (lanes <= 16)
        launch_dot<16, V>(fw, fs, weights, ew, wsum, gew, per_entry, accumulate, s);
    else
        launch_dot<64, V>(fw, fs, weights, ew, wsum, gew, per_entry, accumulate, s);
}

int backward(const std::string& who, void* scratch, size_t scratch_bytes, const hidegs_neighbor_grad_field* fields, int nfields,
             const Forward& fw, long long P, long long Q, long long E, const float* weights, const float* ew, const float* wsum,
             const int32_t* starts_t, const int32_t* query_t, const int32_t* entry_t, float* grad_weights, float* gew, hipStream_t s)
{
    if (nfields < 0) return fail(HIDEGS_E_ARG, who + ": negative field count");
    if (nfields > 0 && !fields) return fail(HIDEGS_E_ARG, who + ": NULL field list");
    bool any_mean = false, any_grad_src = false;
    for (int i = 0; i < nfields; i++) {
        const std::string what = who + ": field " + std::to_string(i);
        if (fields[i].width < 1) return fail(HIDEGS_E_ARG, what + ": width must be >= 1");
        if (fields[i].op != HIDEGS_NEIGHBOR_SUM && fields[i].op != HIDEGS_NEIGHBOR_MEAN)
            return fail(HIDEGS_E_ARG, what + ": op must be HIDEGS_NEIGHBOR_SUM or HIDEGS_NEIGHBOR_MEAN");
        if (P > 0 && !fields[i].src) return fail(HIDEGS_E_ARG, what + ": NULL src");
        if (Q > 0 && (!fields[i].out || !fields[i].grad_out)) return fail(HIDEGS_E_ARG, what + ": NULL out or grad_out");
        any_mean |= fields[i].op == HIDEGS_NEIGHBOR_MEAN;
        any_grad_src |= fields[i].grad_src != nullptr;
    }
    const bool empty = P == 0 || Q == 0 || E == 0;
    if (!empty) {
        if (any_mean && !wsum) return fail(HIDEGS_E_ARG, who + ": a MEAN field needs wsum");
        if ((any_grad_src || grad_weights) && (!starts_t || !query_t || !entry_t))
            return fail(HIDEGS_E_ARG, who + ": the gradient of a field or of weights needs the transposed lists");
        if (grad_weights && !weights) return fail(HIDEGS_E_ARG, who + ": grad_weights without weights");
        if (gew && !ew) return fail(HIDEGS_E_ARG, who + ": grad_entry_weights without entry_weights");
        if (!scratch || scratch_bytes < BackwardScratch(nullptr, P, E).total) return fail(HIDEGS_E_ARG, who + ": scratch NULL or too small");
    }
    const char* name = who.c_str();
    if (empty || nfields == 0) {
        for (int i = 0; i < nfields; i++)
            if (int rc = zero(name, fields[i].grad_src, (size_t)P * fields[i].width * sizeof(float), s)) return rc;
        if (int rc = zero(name, grad_weights, (size_t)P * sizeof(float), s)) return rc;
        return zero(name, gew, (size_t)E * sizeof(float), s);
    }
    const BackwardScratch sc(scratch, P, E);

    if (any_grad_src) {  // the fields' gradients: the forward's reduction over the transposed lists
        std::vector<hidegs_neighbor_field> of_sum, of_mean;
        for (int i = 0; i < nfields; i++)
            if (fields[i].grad_src)
                (fields[i].op == HIDEGS_NEIGHBOR_MEAN ? of_mean : of_sum)
                    .push_back(hidegs_neighbor_field{fields[i].grad_out, fields[i].grad_src, fields[i].width, HIDEGS_NEIGHBOR_SUM});
        float* c_sum = ew && !of_sum.empty() ? sc.c_sum : nullptr;
        float* c_mean = !of_mean.empty() ? sc.c_mean : nullptr;
        if (c_sum || c_mean)
            HIDEGS_LAUNCH("ngrad_coef", ngrad_coef_kernel, dim3(flat_grid(E)), dim3(kBlock), 0, s, (uint32_t)E, (uint32_t)Q, query_t, entry_t, ew,
                          wsum, c_sum, c_mean);
        if (!of_sum.empty())
            if (int rc = hidegs_neighbor_reduce_lists(sc.reduce, sc.reduce_bytes, of_sum.data(), (int)of_sum.size(), Q, nullptr, starts_t,
                                                      query_t, c_sum, E, P, nullptr, s))
                return rc;
        if (!of_mean.empty())
            if (int rc = hidegs_neighbor_reduce_lists(sc.reduce, sc.reduce_bytes, of_mean.data(), (int)of_mean.size(), Q, nullptr,
                                                      starts_t, query_t, c_mean, E, P, nullptr, s))
                return rc;
        if (weights)
            for (int i = 0; i < nfields; i++)
                if (fields[i].grad_src) {
                    const unsigned long long n = (unsigned long long)P * fields[i].width;
                    HIDEGS_LAUNCH("ngrad_scale", ngrad_scale_kernel, dim3(flat_grid(n)), dim3(kBlock), 0, s, fields[i].grad_src,
                                  (uint32_t)fields[i].width, n, weights, starts_t);
                }
    }

    if (gew || grad_weights) {  // the per-entry dot products, kMaxFields fields to a launch
        float* per_entry = grad_weights ? sc.per_entry : nullptr;
        for (int at = 0; at < nfields; at += kMaxFields) {
            DotFields fs;
            fs.n = std::min(kMaxFields, nfields - at);
            fs.any_mean = 0;
            int widest = 1;
            bool vec = true;
            for (int i = 0; i < fs.n; i++) {
                const hidegs_neighbor_grad_field& f = fields[at + i];
                fs.f[i] = DotField{f.src, f.out, f.grad_out, (uint32_t)f.width, f.op == HIDEGS_NEIGHBOR_MEAN};
                fs.any_mean |= fs.f[i].mean;
                widest = std::max(widest, f.width);
                vec = vec && f.width % 4 == 0 && aligned16(f.src) && aligned16(f.out) && aligned16(f.grad_out);
            }
            if (vec)
                launch_dot_lanes<4>((widest + 3) / 4, fw, fs, weights, ew, wsum, gew, per_entry, at > 0, s);
            else
                launch_dot_lanes<1>(widest, fw, fs, weights, ew, wsum, gew, per_entry, at > 0, s);
        }
        if (grad_weights) {  // the per-entry values summed over the transposed lists: entry_t names them
            const hidegs_neighbor_field f{sc.per_entry, grad_weights, 1, HIDEGS_NEIGHBOR_SUM};
            if (int rc = hidegs_neighbor_reduce_lists(sc.reduce, sc.reduce_bytes, &f, 1, E, nullptr, starts_t, entry_t, nullptr, E, P,
                                                      nullptr, s))
                return rc;
        }
    }
    return check_launch(name, s, 0);
}

}  // namespace
}  // namespace hidegs

extern "C" size_t hidegs_neighbor_transpose_scratch_bytes(long long E)
{
    return E > 0 && hidegs::in_range(E) ? hidegs::transpose_scratch(E) : 0;
}

extern "C" int hidegs_neighbor_transpose_table(void* scratch, size_t scratch_bytes, long long P, const int32_t* table, long long Q,
                                               int k, int32_t* starts_t, int32_t* query_t, int32_t* entry_t, int32_t* info,
                                               void* stream)
{
    using namespace hidegs;
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_neighbor_transpose_table", s)) return rc;
    if (k < 1) return fail(HIDEGS_E_ARG, "neighbor_transpose_table: k must be >= 1");
    const long long E = in_range(Q) ? Q * (long long)k : -1;
    if (int rc = check_transpose("neighbor_transpose_table", P, Q, E, table, nullptr, false, scratch, scratch_bytes, starts_t, query_t,
                                 entry_t, info))
        return rc;
    const Forward fw{table, nullptr, nullptr, (uint32_t)k, (uint32_t)E, (uint32_t)Q, (uint32_t)P};
    return transpose("neighbor_transpose_table", scratch, scratch_bytes, fw, starts_t, query_t, entry_t, info, s);
}

extern "C" int hidegs_neighbor_transpose_lists(void* scratch, size_t scratch_bytes, long long P, const int32_t* starts,
                                               const int32_t* rows, long long capacity, long long Q, int32_t* starts_t,
                                               int32_t* query_t, int32_t* entry_t, int32_t* info, void* stream)
{
    using namespace hidegs;
    hipStream_t s = as_stream(stream);
    if (int rc = take_async_error("hidegs_neighbor_transpose_lists", s)) return rc;
    if (int rc = check_transpose("neighbor_transpose_lists", P, Q, capacity, rows, starts, true, scratch, scratch_bytes, starts_t,
                                 query_t, entry_t, info))
        return rc;
    const Forward fw{nullptr, starts, rows, 0u, (uint32_t)capacity, (uint32_t)Q, (uint32_t)P};
    return transpose("neighbor_transpose_lists", scratch, scratch_bytes, fw, starts_t, query_t, entry_t, info, s);
}

extern "C" size_t hidegs_neighbor_reduce_backward_scratch_bytes(long long P, long long E)
{
    using namespace hidegs;
    return P > 0 && E > 0 && in_range(P) && in_range(E) ? BackwardScratch(nullptr, P, E).total : 0;
}

extern "C" int hidegs_neighbor_reduce_backward_table(void* scratch, size_t scratch_bytes, const hidegs_neighbor_grad_field* fields,
                                                     int nfields, long long P, const float* weights, const int32_t* table,
                                                     const float* entry_weights, long long Q, int k, const float* wsum,
                                                     const int32_t* starts_t, const int32_t* query_t, const int32_t* entry_t,
                                                     float* grad_weights, float* grad_entry_weights, void* stream)
{
    using namespace hidegs;
    hipStream_t s = as_stream(stream);
    const std::string who = "neighbor_reduce_backward_table";
    if (int rc = take_async_error("hidegs_neighbor_reduce_backward_table", s)) return rc;
    if (k < 1) return fail(HIDEGS_E_ARG, who + ": k must be >= 1");
    if (!in_range(P)) return fail(HIDEGS_E_ARG, who + ": P must be in [0, 2^31)");
    if (!in_range(Q)) return fail(HIDEGS_E_ARG, who + ": Q must be in [0, 2^31)");
    const long long E = Q * (long long)k;
    if (!in_range(E)) return fail(HIDEGS_E_ARG, who + ": at most 2^31 - 1 entry positions");
    if (E > 0 && !table) return fail(HIDEGS_E_ARG, who + ": NULL table");
    const Forward fw{table, nullptr, nullptr, (uint32_t)k, (uint32_t)E, (uint32_t)Q, (uint32_t)P};
    return backward(who, scratch, scratch_bytes, fields, nfields, fw, P, Q, E, weights, entry_weights, wsum, starts_t, query_t, entry_t,
                    grad_weights, grad_entry_weights, s);
}

extern "C" int hidegs_neighbor_reduce_backward_lists(void* scratch, size_t scratch_bytes, const hidegs_neighbor_grad_field* fields,
                                                     int nfields, long long P, const float* weights, const int32_t* starts,
                                                     const int32_t* rows, const float* entry_weights, long long capacity, long long Q,
                                                     const float* wsum, const int32_t* starts_t, const int32_t* query_t,
                                                     const int32_t* entry_t, float* grad_weights, float* grad_entry_weights,
                                                     void* stream)
{
    using namespace hidegs;
    hipStream_t s = as_stream(stream);
    const std::string who = "neighbor_reduce_backward_lists";
    if (int rc = take_async_error("hidegs_neighbor_reduce_backward_lists", s)) return rc;
    if (!in_range(P)) return fail(HIDEGS_E_ARG, who + ": P must be in [0, 2^31)");
    if (!in_range(Q)) return fail(HIDEGS_E_ARG, who + ": Q must be in [0, 2^31)");
    if (!in_range(capacity)) return fail(HIDEGS_E_ARG, who + ": at most 2^31 - 1 entry positions");
    if (capacity > 0 && !rows) return fail(HIDEGS_E_ARG, who + ": NULL rows");
    if (Q > 0 && !starts) return fail(HIDEGS_E_ARG, who + ": NULL starts");
    const Forward fw{nullptr, starts, rows, 0u, (uint32_t)capacity, (uint32_t)Q, (uint32_t)P};
    return backward(who, scratch, scratch_bytes, fields, nfields, fw, P, Q, capacity, weights, entry_weights, wsum, starts_t, query_t,
                    entry_t, grad_weights, grad_entry_weights, s);
}
