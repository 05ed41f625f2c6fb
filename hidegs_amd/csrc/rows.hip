// rows.hip -- stream compaction of a byte mask and indexed row moves (include/hidegs_rows.h): the
// local steps of the compacted view-DP exchange (hidegs_amd/view_dp.py).  Where few rows are visible
// to any rank, only those rows travel: they are selected from the union mask, packed field-major
// ([field][j][col], the layout the exchange always had), summed by the collectives and written back.
// These kernels replace union.sum() + nonzero() (two host synchronisations, int64 indices) and the
// index_select / index_copy_ launch per field.  Every move is a bit copy.
//
// Select: two passes over the flags, the shape of scan.h.  select_count writes each 4096-flag tile's
// number of set flags; select_write forms its tile's base offset (by adding up the counts before it,
// or from their scan above kSelectOwnTiles tiles), ranks the flags inside the tile with
// block_exclusive_scan and writes the positions through LDS, so the global stores are contiguous.
// No workgroup waits on another.
//
// Gather / scatter: one launch moves every field of a batch of up to kMaxFields.  Consecutive lanes
// take consecutive floats (or 16-byte quads, where width, bases and therefore every row start allow)
// of the packed side, which is thus fully coalesced; the row side is contiguous inside a row and, for
// ascending indices, ascending across rows.  A thread owns kUnroll units a workgroup-stride apart and
// steps (packed row, column) from one to the next with host-computed increments: one division per
// thread, not per element.
//
// Resize (include/hidegs_resize.h): the row surgery of densification -- prune by a keep list, append new
// rows -- on every per-Gaussian tensor in one launch per kMaxFields.  The same unit stepping over the dense
// destination, which is written from three sources: kept rows gathered, appended rows copied, or zeros.
// With include/hidegs_clone.h a fourth: appended rows gathered from the source by a second index list, the
// clone and the split of densification (resize_rows_cloned_kernel).
#include <stdint.h>

#include <string>

#include "../../include/hidegs_rows.h"
#include "block_scan.h"
#include "common.h"

namespace hidegs {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;  // 4

// ============================== select =========================================
constexpr int kSelectItems = 16;                      // flags per thread: one 16-byte load
constexpr int kSelectTile = kBlock * kSelectItems;    // 4096
constexpr int kSelectOwnTiles = 4096;                 // up to here a workgroup adds the counts before it itself
constexpr long long kSelectMax = 0x7fffffffLL;        // positions are u32, tile counts fit the grid

// Bit j of the result: flag j of this thread's kSelectItems consecutive flags is non-zero.
__device__ __forceinline__ uint32_t load_flag_bits(const uint8_t* __restrict__ flags, long long base, long long n,
                                                   int vec)
{
    const long long i0 = base + (long long)threadIdx.x * kSelectItems;
    uint32_t bits = 0;
    if (vec && base + kSelectTile <= n) {  // workgroup-uniform; the tile base is a multiple of 16
        const uint4 v = *reinterpret_cast<const uint4*>(flags + i0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < kSelectItems; j++)
            bits |= (((w[j / 4] >> (8 * (j % 4))) & 0xffu) != 0 ? 1u : 0u) << j;
    } else {
#pragma unroll
        for (int j = 0; j < kSelectItems; j++)
            if (i0 + j < n && flags[i0 + j] != 0) bits |= 1u << j;
    }
    return bits;
}

__global__ __launch_bounds__(kBlock) void select_count_kernel(const uint8_t* __restrict__ flags, long long n,
                                                              uint32_t* __restrict__ tile_counts, int vec)
{
    __shared__ uint32_t s_wave[kWavesPerBlock];
    const long long base = (long long)blockIdx.x * kSelectTile;
    const uint32_t bits = load_flag_bits(flags, base, n, vec);
    uint32_t total;
    block_exclusive_scan((uint32_t)__popc(bits), s_wave, &total);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}

// counts_raw: tile_counts holds the counts, and the workgroup adds up those before its own; otherwise
// their exclusive scan.  The last tile's offset and total are the count.
__global__ __launch_bounds__(kBlock) void select_write_kernel(const uint8_t* __restrict__ flags, long long n,
                                                              const uint32_t* __restrict__ tile_counts, int counts_raw,
                                                              uint32_t* __restrict__ indices,
                                                              uint32_t* __restrict__ count, int vec)
{
    __shared__ uint32_t s_pos[kSelectTile];
    __shared__ uint32_t s_wave[kWavesPerBlock];
    const long long base = (long long)blockIdx.x * kSelectTile;
    uint32_t tile_off;
    if (counts_raw) {
        uint32_t part = 0;
        for (int i = threadIdx.x; i < (int)blockIdx.x; i += kBlock) part += tile_counts[i];
        block_exclusive_scan(part, s_wave, &tile_off);
    } else {
        tile_off = tile_counts[blockIdx.x];
    }
    uint32_t bits = load_flag_bits(flags, base, n, vec);
    uint32_t total;
    uint32_t rank = block_exclusive_scan((uint32_t)__popc(bits), s_wave, &total);
    const uint32_t i0 = (uint32_t)base + threadIdx.x * kSelectItems;
    while (bits) {  // ascending inside the thread, threads in order: ascending in the tile
        const int j = __ffs((int)bits) - 1;
        bits &= bits - 1;
        s_pos[rank++] = i0 + (uint32_t)j;
    }
    __syncthreads();
    // tile_off + total <= n while the flags are those the first pass counted; the check keeps a caller
    // that changed them in between inside the buffer
    for (uint32_t i = threadIdx.x; i < total; i += kBlock) {
        const long long pos = (long long)tile_off + i;
        if (pos < n) indices[pos] = s_pos[i];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *count = tile_off + total;
}

int select_tiles(long long n) { return (int)((n + kSelectTile - 1) / kSelectTile); }
size_t select_scratch(long long n) { return align_up((size_t)select_tiles(n) * sizeof(uint32_t)); }

// ============================== gather / scatter ===============================
constexpr int kMaxFields = 8;  // fields per launch
constexpr int kUnroll = 8;     // units per thread, all in flight
constexpr int kUnitsPerBlock = kBlock * kUnroll;

struct RowField {
    uint32_t* rows;
    uint32_t* packed;
    long long n_rows;
    long long units;   // k * width / unit
    uint32_t width;
    uint32_t unit;     // floats per access: 4 (16-byte accesses on both sides) or 1
    uint32_t step_j;   // (kBlock * unit) / width: packed rows between a thread's consecutive units
    uint32_t step_c;   // (kBlock * unit) % width: columns
    double inv_w;
};

// Workgroups [first[f], first[f + 1]) own field f.
struct RowBatch {
    int count;
    int first[kMaxFields + 1];
    RowField f[kMaxFields];
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// e / w for e < 2^52: double estimate, exact after the correction.
__device__ __forceinline__ long long row_of(long long e, uint32_t w, double inv_w)
{
    long long r = (long long)((double)e * inv_w);
    if (r * (long long)w > e) r--;
    if ((r + 1) * (long long)w <= e) r++;
    return r;
}

template <bool kScatter, typename V>
__device__ __forceinline__ void move_units(const RowField& F, long long u0, const uint32_t* __restrict__ indices)
{
    constexpr uint32_t kUnit = sizeof(V) / sizeof(uint32_t);
    const long long e0 = u0 * kUnit;  // the workgroup's first packed element
    const long long j0 = row_of(e0, F.width, F.inv_w);
    const uint32_t r = (uint32_t)(e0 - j0 * (long long)F.width) + threadIdx.x * kUnit;  // < width + 1024
    const uint32_t q = r / F.width;
    long long j = j0 + q;            // packed row and column of this thread's first unit
    uint32_t c = r - q * F.width;
    size_t at[kUnroll];              // element offset on the row side
    bool ok[kUnroll];
#pragma unroll
    for (int i = 0; i < kUnroll; i++) {  // every index load issued before any is used
        const long long u = u0 + i * kBlock + threadIdx.x;
        ok[i] = u < F.units;         // then j < k
        const uint32_t idx = indices[ok[i] ? j : 0];  // (entry 0 exists: k >= 1)
        ok[i] = ok[i] && (long long)idx < F.n_rows;  // an index past the rows is never dereferenced
        at[i] = (size_t)idx * F.width + c;
        c += F.step_c;
        j += F.step_j;
        if (c >= F.width) {
            c -= F.width;
            j++;
        }
    }
    V v[kUnroll];
    const V* src = reinterpret_cast<const V*>(kScatter ? F.packed : F.rows);
    V* dst = reinterpret_cast<V*>(kScatter ? F.rows : F.packed);
#pragma unroll
    for (int i = 0; i < kUnroll; i++) {
        const size_t p = (size_t)(u0 + i * kBlock + threadIdx.x);  // unit on the packed side
        v[i] = src[ok[i] ? (kScatter ? p : at[i] / kUnit) : 0];  // unit 0 exists on both sides: loads without branches
    }
#pragma unroll
    for (int i = 0; i < kUnroll; i++) {
        const size_t p = (size_t)(u0 + i * kBlock + threadIdx.x);
        if (ok[i]) dst[kScatter ? at[i] / kUnit : p] = v[i];
    }
}

template <bool kScatter>
__global__ __launch_bounds__(kBlock) void move_rows_kernel(const RowBatch batch, const uint32_t* __restrict__ indices)
{
    // workgroup-uniform selects over constant indices: the descriptors stay in scalar registers
    RowField F = batch.f[0];
    int first = batch.first[0];
#pragma unroll
    for (int i = 1; i < kMaxFields; i++) {
        if (i < batch.count && (int)blockIdx.x >= batch.first[i]) {
            F = batch.f[i];
            first = batch.first[i];
        }
    }
    const long long u0 = (long long)((int)blockIdx.x - first) * kUnitsPerBlock;
    if (F.unit == 4)
        move_units<kScatter, u32x4>(F, u0, indices);
    else
        move_units<kScatter, uint32_t>(F, u0, indices);
}


int move_rows(bool scatter, const hidegs_row_field* fields, int nfields, const uint32_t* indices, long long k,
              hipStream_t stream)
{
    const char* name = scatter ? "scatter_rows" : "gather_rows";
    const std::string who = name;
    if (nfields < 0) return fail(HIDEGS_E_ARG, who + ": negative field count");
    if (k < 0 || k > kSelectMax) return fail(HIDEGS_E_ARG, who + ": k must be in [0, 2^31)");
    if (nfields > 0 && !fields) return fail(HIDEGS_E_ARG, who + ": NULL field list");
    for (int i = 0; i < nfields; i++) {
        if (fields[i].width < 1) return fail(HIDEGS_E_ARG, who + ": field " + std::to_string(i) + ": width < 1");
        if (fields[i].n_rows < 0) return fail(HIDEGS_E_ARG, who + ": field " + std::to_string(i) + ": negative n_rows");
    }
    if (k == 0 || nfields == 0) return 0;
    if (!indices) return fail(HIDEGS_E_ARG, who + ": NULL indices");
    for (int i = 0; i < nfields; i++)
        if (!fields[i].packed || (fields[i].n_rows > 0 && !fields[i].rows))
            return fail(HIDEGS_E_ARG, who + ": field " + std::to_string(i) + ": NULL pointer");
    for (int i0 = 0; i0 < nfields; i0 += kMaxFields) {  // kMaxFields per launch
        RowBatch batch;
        batch.count = 0;
        long long blocks = 0;
        for (int i = i0; i < nfields && i < i0 + kMaxFields; i++) {
            const hidegs_row_field& a = fields[i];
            if (a.n_rows == 0) continue;  // every index is past the rows
            RowField F;
            F.rows = reinterpret_cast<uint32_t*>(a.rows);
            F.packed = reinterpret_cast<uint32_t*>(a.packed);
            F.n_rows = a.n_rows;
            F.width = (uint32_t)a.width;
            // width a multiple of 4 and both bases on 16 bytes: every row start and every quad is aligned
            F.unit = (a.width % 4 == 0 && aligned16(a.rows) && aligned16(a.packed)) ? 4u : 1u;
            F.units = k * (long long)a.width / F.unit;
            F.step_j = (uint32_t)(kBlock * F.unit) / F.width;
            F.step_c = (uint32_t)(kBlock * F.unit) % F.width;
            F.inv_w = 1.0 / (double)a.width;
            batch.first[batch.count] = (int)blocks;
            batch.f[batch.count++] = F;
            blocks += (F.units + kUnitsPerBlock - 1) / kUnitsPerBlock;
            if (blocks > 0x7fffffffLL) return fail(HIDEGS_E_ARG, who + ": fields too large for one launch");
        }
        if (batch.count == 0) continue;
        batch.first[batch.count] = (int)blocks;
        if (scatter)
            HIDEGS_LAUNCH("scatter_rows", move_rows_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, batch,
                          indices);
        else
            HIDEGS_LAUNCH("gather_rows", move_rows_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, batch,
                          indices);
    }
    return check_launch(name, stream, 0);
}

// ============================== resize =========================================
// One field of a resize: dst = [src rows named by keep | append rows or zeros], dense.
struct ResizeField {
    const uint32_t* src;
    const uint32_t* append;  // NULL: the appended rows are zeros
    const uint32_t* safe;    // one readable unit for the lanes that write zeros (src or append); NULL: all zeros
    uint32_t* dst;
    long long n_rows;
    long long kept;    // k * width / unit: the units gathered from src
    long long units;   // (k + n_append) * width / unit
    uint32_t width;
    uint32_t unit;     // floats per access: 4 (16-byte accesses on all three sides) or 1
    uint32_t step_j;   // as RowField's
    uint32_t step_c;
    double inv_w;
};

// Workgroups [first[f], first[f + 1]) own field f.
struct ResizeBatch {
    int count;
    int first[kMaxFields + 1];
    ResizeField f[kMaxFields];
};

// Consecutive lanes take consecutive units of dst.  A unit below F.kept is gathered (dst row j from src row
// keep[j], or row j itself without a keep array; zeros if that row is past the source); one at or after it
// comes from append at unit - F.kept, or is zeros.  Which of the two is workgroup-uniform except in the one
// workgroup that holds unit F.kept.
// kClone (include/hidegs_clone.h): the field's appended rows are rows of src too, dst row k + i from src row
// from[i].  Every unit of dst is then a gathered one; only the index array and the entry differ on the two
// sides of unit F.kept, so the pointer is selected and one load is issued, as for the data.
template <typename V, bool kKeep, bool kClone = false>
__device__ __forceinline__ void resize_units(const ResizeField& F, long long u0, const uint32_t* __restrict__ keep,
                                             const uint32_t* __restrict__ from_list = nullptr, long long k = 0)
{
    constexpr uint32_t kUnit = sizeof(V) / sizeof(uint32_t);
    const long long e0 = u0 * kUnit;  // the workgroup's first dst element
    const long long j0 = row_of(e0, F.width, F.inv_w);
    const uint32_t r = (uint32_t)(e0 - j0 * (long long)F.width) + threadIdx.x * kUnit;  // < width + 1024
    const uint32_t q = r / F.width;
    long long j = j0 + q;            // dst row and column of this thread's first unit
    uint32_t c = r - q * F.width;
    uint32_t idx[kUnroll], col[kUnroll];
#pragma unroll
    for (int i = 0; i < kUnroll; i++) {  // every index load issued before any is used
        const long long u = u0 + i * kBlock + threadIdx.x;
        // a gathered unit (u < F.kept) has j < k; entry 0 exists (keep is passed only where k >= 1)
        if constexpr (kClone) {
            // an appended unit (F.kept <= u < F.units) has k <= j < k + n_append; entry 0 of from_list exists
            // (a field is cloned only where n_append >= 1) and serves the lanes past the last unit
            const bool gathered = kKeep && u < F.kept;
            const uint32_t* list = gathered ? keep : from_list;
            const long long entry = gathered ? j : (u >= F.kept && u < F.units ? j - k : 0);
            const uint32_t got = list[entry];
            idx[i] = (!kKeep && u < F.kept) ? (uint32_t)j : got;
        } else {
            idx[i] = kKeep ? keep[u < F.kept ? j : 0] : (uint32_t)j;
        }
        col[i] = c;
        c += F.step_c;
        j += F.step_j;
        if (c >= F.width) {
            c -= F.width;
            j++;
        }
    }
    const V* from[kUnroll];          // where the unit is read: F.safe where it is zeros, so the loads need no branch
    bool zero[kUnroll];
#pragma unroll
    for (int i = 0; i < kUnroll; i++) {
        const long long u = u0 + i * kBlock + threadIdx.x;
        // an index past the rows is never dereferenced
        const bool in_src = (u < (kClone ? F.units : F.kept)) & ((long long)idx[i] < F.n_rows);
        const bool in_append = !kClone & (u >= F.kept) & (u < F.units) & (F.append != nullptr);
        const uint32_t* base = in_src ? F.src : (in_append ? F.append : F.safe);
        const size_t at = in_src ? ((size_t)idx[i] * F.width + col[i]) / kUnit : (in_append ? (size_t)(u - F.kept) : 0);
        from[i] = reinterpret_cast<const V*>(base) + at;
        zero[i] = !(in_src | in_append);
    }
    V v[kUnroll];
#pragma unroll
    for (int i = 0; i < kUnroll; i++) v[i] = *from[i];  // every load issued before the first store
    V* dst = reinterpret_cast<V*>(F.dst);
#pragma unroll
    for (int i = 0; i < kUnroll; i++) {
        const long long u = u0 + i * kBlock + threadIdx.x;
        if (u < F.units) dst[u] = zero[i] ? V{} : v[i];
    }
}

// A field with nothing to read (no source row and no appended rows given): zeros.
template <typename V>
__device__ __forceinline__ void zero_units(const ResizeField& F, long long u0)
{
    V* dst = reinterpret_cast<V*>(F.dst);
#pragma unroll
    for (int i = 0; i < kUnroll; i++) {
        const long long u = u0 + i * kBlock + threadIdx.x;
        if (u < F.units) dst[u] = V{};
    }
}

__global__ __launch_bounds__(kBlock) void resize_rows_kernel(const ResizeBatch batch, const uint32_t* __restrict__ keep)
{
    // workgroup-uniform selects over constant indices: the descriptors stay in scalar registers
    ResizeField F = batch.f[0];
    int first = batch.first[0];
#pragma unroll
    for (int i = 1; i < kMaxFields; i++) {
        if (i < batch.count && (int)blockIdx.x >= batch.first[i]) {
            F = batch.f[i];
            first = batch.first[i];
        }
    }
    const long long u0 = (long long)((int)blockIdx.x - first) * kUnitsPerBlock;
    if (!F.safe) {
        if (F.unit == 4)
            zero_units<u32x4>(F, u0);
        else
            zero_units<uint32_t>(F, u0);
    } else if (keep) {
        if (F.unit == 4)
            resize_units<u32x4, true>(F, u0, keep);
        else
            resize_units<uint32_t, true>(F, u0, keep);
    } else {
        if (F.unit == 4)
            resize_units<u32x4, false>(F, u0, keep);
        else
            resize_units<uint32_t, false>(F, u0, keep);
    }
}

// resize_rows_kernel with a third source for the appended rows (include/hidegs_clone.h): bit f of `cloned` says
// that field f of the batch takes them from src, row from[i] for dst row k + i.  The mode is workgroup-uniform
// like the descriptor; the other fields run the code of resize_rows_kernel.
__global__ __launch_bounds__(kBlock) void resize_rows_cloned_kernel(const ResizeBatch batch,
                                                                    const uint32_t* __restrict__ keep,
                                                                    const uint32_t* __restrict__ from, long long k,
                                                                    uint32_t cloned)
{
    ResizeField F = batch.f[0];
    int first = batch.first[0];
    bool clone = cloned & 1u;
#pragma unroll
    for (int i = 1; i < kMaxFields; i++) {
        if (i < batch.count && (int)blockIdx.x >= batch.first[i]) {
            F = batch.f[i];
            first = batch.first[i];
            clone = (cloned >> i) & 1u;
        }
    }
    const long long u0 = (long long)((int)blockIdx.x - first) * kUnitsPerBlock;
    if (!F.safe) {
        if (F.unit == 4)
            zero_units<u32x4>(F, u0);
        else
            zero_units<uint32_t>(F, u0);
    } else if (clone) {
        if (keep) {
            if (F.unit == 4)
                resize_units<u32x4, true, true>(F, u0, keep, from, k);
            else
                resize_units<uint32_t, true, true>(F, u0, keep, from, k);
        } else {
            if (F.unit == 4)
                resize_units<u32x4, false, true>(F, u0, keep, from, k);
            else
                resize_units<uint32_t, false, true>(F, u0, keep, from, k);
        }
    } else if (keep) {
        if (F.unit == 4)
            resize_units<u32x4, true>(F, u0, keep);
        else
            resize_units<uint32_t, true>(F, u0, keep);
    } else {
        if (F.unit == 4)
            resize_units<u32x4, false>(F, u0, keep);
        else
            resize_units<uint32_t, false>(F, u0, keep);
    }
}

// The descriptor of one field; src and append are NULL where the launch reads no row of theirs.
ResizeField resize_field(const float* src, const float* append, float* dst, long long n_rows, int width, long long k,
                         long long n_append)
{
    ResizeField F;
    F.src = reinterpret_cast<const uint32_t*>(src);
    F.append = reinterpret_cast<const uint32_t*>(append);
    F.safe = F.src ? F.src : F.append;
    F.dst = reinterpret_cast<uint32_t*>(dst);
    F.n_rows = n_rows;
    F.width = (uint32_t)width;
    // width a multiple of 4 and every base on 16 bytes: every row start and every quad is aligned, and
    // k * width is a multiple of 4, so no quad holds both gathered and appended floats
    F.unit = (width % 4 == 0 && aligned16(F.src) && aligned16(F.append) && aligned16(dst)) ? 4u : 1u;
    F.kept = k * (long long)width / F.unit;
    F.units = (k + n_append) * (long long)width / F.unit;
    F.step_j = (uint32_t)(kBlock * F.unit) / F.width;
    F.step_c = (uint32_t)(kBlock * F.unit) % F.width;
    F.inv_w = 1.0 / (double)width;
    return F;
}

int resize_rows(const hidegs_resize_field* fields, int nfields, const uint32_t* keep, long long k, long long n_append,
                hipStream_t stream)
{
    const std::string who = "resize_rows";
    if (nfields < 0) return fail(HIDEGS_E_ARG, who + ": negative field count");
    if (k < 0 || n_append < 0 || k > kSelectMax || n_append > kSelectMax || k + n_append > kSelectMax)
        return fail(HIDEGS_E_ARG, who + ": k, n_append and k + n_append must be in [0, 2^31)");
    if (nfields > 0 && !fields) return fail(HIDEGS_E_ARG, who + ": NULL field list");
    for (int i = 0; i < nfields; i++) {
        if (fields[i].width < 1) return fail(HIDEGS_E_ARG, who + ": field " + std::to_string(i) + ": width < 1");
        if (fields[i].n_rows < 0) return fail(HIDEGS_E_ARG, who + ": field " + std::to_string(i) + ": negative n_rows");
    }
    if (k + n_append == 0 || nfields == 0) return 0;
    for (int i = 0; i < nfields; i++) {
        if (!fields[i].dst || (k > 0 && fields[i].n_rows > 0 && !fields[i].src))
            return fail(HIDEGS_E_ARG, who + ": field " + std::to_string(i) + ": NULL pointer");
        if (!keep && k > fields[i].n_rows)
            return fail(HIDEGS_E_ARG, who + ": field " + std::to_string(i) + ": without keep, k must not exceed n_rows");
    }
    if (k == 0) keep = nullptr;  // no row is gathered: the kernel reads no entry
    for (int i0 = 0; i0 < nfields; i0 += kMaxFields) {  // kMaxFields per launch
        ResizeBatch batch;
        batch.count = 0;
        long long blocks = 0;
        for (int i = i0; i < nfields && i < i0 + kMaxFields; i++) {
            const hidegs_resize_field& a = fields[i];
            const ResizeField F = resize_field(k > 0 && a.n_rows > 0 ? a.src : nullptr, n_append > 0 ? a.append : nullptr,
                                               a.dst, a.n_rows, a.width, k, n_append);
            batch.first[batch.count] = (int)blocks;
            batch.f[batch.count++] = F;
            blocks += (F.units + kUnitsPerBlock - 1) / kUnitsPerBlock;
            if (blocks > 0x7fffffffLL) return fail(HIDEGS_E_ARG, who + ": fields too large for one launch");
        }
        batch.first[batch.count] = (int)blocks;
        HIDEGS_LAUNCH("resize_rows", resize_rows_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, batch, keep);
    }
    return check_launch("resize_rows", stream, 0);
}

// hidegs_resize_rows_cloned.  A batch without a cloned field is a launch of resize_rows_kernel itself.
int resize_rows_cloned(const hidegs_clone_field* fields, int nfields, const uint32_t* keep, long long k,
                       const uint32_t* from, long long n_append, hipStream_t stream)
{
    const std::string who = "resize_rows_cloned";
    if (nfields < 0) return fail(HIDEGS_E_ARG, who + ": negative field count");
    if (k < 0 || n_append < 0 || k > kSelectMax || n_append > kSelectMax || k + n_append > kSelectMax)
        return fail(HIDEGS_E_ARG, who + ": k, n_append and k + n_append must be in [0, 2^31)");
    if (nfields > 0 && !fields) return fail(HIDEGS_E_ARG, who + ": NULL field list");
    bool any_cloned = false;
    for (int i = 0; i < nfields; i++) {
        const std::string field = who + ": field " + std::to_string(i);
        if (fields[i].width < 1) return fail(HIDEGS_E_ARG, field + ": width < 1");
        if (fields[i].n_rows < 0) return fail(HIDEGS_E_ARG, field + ": negative n_rows");
        if (fields[i].cloned && fields[i].append) return fail(HIDEGS_E_ARG, field + ": cloned, but append is given");
        any_cloned = any_cloned || fields[i].cloned;
    }
    if (k + n_append == 0 || nfields == 0) return 0;
    const bool cloning = any_cloned && n_append > 0;
    for (int i = 0; i < nfields; i++) {
        const hidegs_clone_field& a = fields[i];
        const bool reads_src = a.n_rows > 0 && (k > 0 || (a.cloned && n_append > 0));
        if (!a.dst || (reads_src && !a.src))
            return fail(HIDEGS_E_ARG, who + ": field " + std::to_string(i) + ": NULL pointer");
        if (!keep && k > a.n_rows)
            return fail(HIDEGS_E_ARG, who + ": field " + std::to_string(i) + ": without keep, k must not exceed n_rows");
    }
    if (cloning && !from) return fail(HIDEGS_E_ARG, who + ": NULL from with a cloned field");
    if (k == 0) keep = nullptr;  // no row is gathered by keep: the kernel reads no entry
    for (int i0 = 0; i0 < nfields; i0 += kMaxFields) {  // kMaxFields per launch
        ResizeBatch batch;
        batch.count = 0;
        long long blocks = 0;
        uint32_t cloned = 0;
        for (int i = i0; i < nfields && i < i0 + kMaxFields; i++) {
            const hidegs_clone_field& a = fields[i];
            const bool clone = a.cloned && n_append > 0;
            // a cloned field has no append side: 16-byte units where src and dst allow
            const ResizeField F = resize_field((k > 0 || clone) && a.n_rows > 0 ? a.src : nullptr,
                                               n_append > 0 ? a.append : nullptr, a.dst, a.n_rows, a.width, k, n_append);
            if (clone) cloned |= 1u << batch.count;
            batch.first[batch.count] = (int)blocks;
            batch.f[batch.count++] = F;
            blocks += (F.units + kUnitsPerBlock - 1) / kUnitsPerBlock;
            if (blocks > 0x7fffffffLL) return fail(HIDEGS_E_ARG, who + ": fields too large for one launch");
        }
        batch.first[batch.count] = (int)blocks;
        if (cloned)
            HIDEGS_LAUNCH("resize_rows_cloned", resize_rows_cloned_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream,
                          batch, keep, from, k, cloned);
        else
            HIDEGS_LAUNCH("resize_rows", resize_rows_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, batch, keep);
    }
    return check_launch("resize_rows_cloned", stream, 0);
}

}  // namespace
}  // namespace hidegs

extern "C" size_t hidegs_select_scratch_bytes(long long n)
{
    return n > 0 && n <= hidegs::kSelectMax ? hidegs::select_scratch(n) : 0;
}

extern "C" int hidegs_select_flagged(void* scratch, size_t scratch_bytes, const unsigned char* flags, long long n,
                                     uint32_t* indices, uint32_t* count, void* stream)
{
    using namespace hidegs;
    if (int rc = take_async_error("hidegs_select_flagged", as_stream(stream))) return rc;
    if (n < 0 || n > kSelectMax) return fail(HIDEGS_E_ARG, "select_flagged: n must be in [0, 2^31)");
    if (n == 0) return 0;
    if (!flags || !indices || !count) return fail(HIDEGS_E_ARG, "select_flagged: NULL pointer");
    if (!scratch || scratch_bytes < select_scratch(n)) return fail(HIDEGS_E_ARG, "select_flagged: scratch too small");
    const int nt = select_tiles(n);
    Carver c(scratch);
    uint32_t* counts = c.take<uint32_t>(nt);
    const int vec = (reinterpret_cast<uintptr_t>(flags) & 15) == 0;
    hipStream_t s = as_stream(stream);
    HIDEGS_LAUNCH("select_count", select_count_kernel, dim3(nt), dim3(kBlock), 0, s, flags, n, counts, vec);
    const int own = nt <= kSelectOwnTiles;
    if (!own)
        HIDEGS_LAUNCH("select_offsets", scan_small_kernel, dim3(1), dim3(kBlock), 0, s, counts, nt, (uint32_t*)nullptr);
    HIDEGS_LAUNCH("select_write", select_write_kernel, dim3(nt), dim3(kBlock), 0, s, flags, n, counts, own, indices,
                  count, vec);
    return check_launch("select_flagged", s, 0);
}

extern "C" int hidegs_gather_rows(const hidegs_row_field* fields, int nfields, const uint32_t* indices, long long k,
                                  void* stream)
{
    if (int rc = hidegs::take_async_error("hidegs_gather_rows", hidegs::as_stream(stream))) return rc;
    return hidegs::move_rows(false, fields, nfields, indices, k, hidegs::as_stream(stream));
}

extern "C" int hidegs_scatter_rows(const hidegs_row_field* fields, int nfields, const uint32_t* indices, long long k,
                                   void* stream)
{
    if (int rc = hidegs::take_async_error("hidegs_scatter_rows", hidegs::as_stream(stream))) return rc;
    return hidegs::move_rows(true, fields, nfields, indices, k, hidegs::as_stream(stream));
}

extern "C" int hidegs_resize_rows(const hidegs_resize_field* fields, int nfields, const uint32_t* keep, long long k,
                                  long long n_append, void* stream)
{
    if (int rc = hidegs::take_async_error("hidegs_resize_rows", hidegs::as_stream(stream))) return rc;
    return hidegs::resize_rows(fields, nfields, keep, k, n_append, hidegs::as_stream(stream));
}

extern "C" int hidegs_resize_rows_cloned(const hidegs_clone_field* fields, int nfields, const uint32_t* keep, long long k,
                                         const uint32_t* from, long long n_append, void* stream)
{
    if (int rc = hidegs::take_async_error("hidegs_resize_rows_cloned", hidegs::as_stream(stream))) return rc;
    return hidegs::resize_rows_cloned(fields, nfields, keep, k, from, n_append, hidegs::as_stream(stream));
}
