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
// Gather / scatter and resize share the walk over the units of a dense side and the batching of fields.
// One launch serves a Batch of up to kMaxFields field descriptors (place_field gives each its range of
// workgroups).  Consecutive lanes take consecutive floats (or 16-byte quads, where width, bases and
// therefore every row start allow) of the dense side, which is thus fully coalesced.  A thread owns
// kUnroll units a workgroup-stride apart: first_unit finds the (row, column) of its first with one
// division per thread, not per element, and next_unit steps to the next with the increments make_walk
// computed on the host (Walk, the tail of both descriptors).
//
// Gather / scatter (move_rows, move_rows_kernel<kScatter>, move_units): the dense side is the packed one;
// the row side is contiguous inside a row and, for ascending indices, ascending across rows.
//
// Resize (include/hidegs_resize.h, include/hidegs_clone.h): the row surgery of densification -- prune by a
// keep list, append new rows -- on every per-Gaussian tensor.  The dense side is the destination, written
// from four sources (resize_units): kept rows gathered, appended rows copied, zeros, or appended rows gathered
// from the source by a second index list, the clone and the split of densification.  One host function,
// resize_rows, serves both entry points, and one kernel template both launches: resize_kernel<true> where
// the batch has a cloned field, resize_kernel<false>, without that branch, where it has none.
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

// ============================== fields, batches and the unit walk ==============
constexpr int kMaxFields = 8;  // fields per launch
constexpr int kUnroll = 8;     // units per thread, all in flight
constexpr int kUnitsPerBlock = kBlock * kUnroll;

// How a thread steps through the units of a dense side of rows `width` floats wide (the packed side of a
// move, the dst of a resize): the last members of both field descriptors.
struct Walk {
    uint32_t width;
    uint32_t unit;     // floats per access: 4 (16-byte accesses on every side) or 1
    uint32_t step_j;   // (kBlock * unit) / width: dense rows between a thread's consecutive units
    uint32_t step_c;   // (kBlock * unit) % width: columns
    double inv_w;
};

Walk make_walk(int width, uint32_t unit)
{
    Walk w;
    w.width = (uint32_t)width;
    w.unit = unit;
    w.step_j = (uint32_t)(kBlock * unit) / w.width;
    w.step_c = (uint32_t)(kBlock * unit) % w.width;
    w.inv_w = 1.0 / (double)width;
    return w;
}

struct RowField {
    uint32_t* rows;
    uint32_t* packed;
    long long n_rows;
    long long units;   // k * width / unit
    Walk w;
};

// The fields of one launch: workgroups [first[f], first[f + 1]) own field f.
template <typename Field>
struct Batch {
    int count = 0;
    int first[kMaxFields + 1] = {0};
    Field f[kMaxFields];
};

// Appends F to the batch, after the workgroups of the fields before it.
template <typename Field>
int place_field(Batch<Field>& batch, const Field& F, const std::string& who)
{
    const long long blocks = batch.first[batch.count] + (F.units + kUnitsPerBlock - 1) / kUnitsPerBlock;
    if (blocks > 0x7fffffffLL) return fail(HIDEGS_E_ARG, who + ": fields too large for one launch");
    batch.f[batch.count++] = F;
    batch.first[batch.count] = (int)blocks;
    return 0;
}

// The checks of one entry of a field list that every entry point makes.
template <typename Field>
int check_shape(const std::string& who, int i, const Field& a)
{
    if (a.width < 1) return fail(HIDEGS_E_ARG, who + ": field " + std::to_string(i) + ": width < 1");
    if (a.n_rows < 0) return fail(HIDEGS_E_ARG, who + ": field " + std::to_string(i) + ": negative n_rows");
    return 0;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// e / w for e < 2^52: double estimate, exact after the correction.
__device__ __forceinline__ long long row_of(long long e, uint32_t w, double inv_w)
{
    long long r = (long long)((double)e * inv_w);
    if (r * (long long)w > e) r--;
    if ((r + 1) * (long long)w <= e) r++;
    return r;
}

// Where a unit starts on the dense side: row j, column c.
struct UnitAt {
    long long j;
    uint32_t c;
};

// This thread's first unit in the workgroup whose first unit is u0.
template <uint32_t kUnit>
__device__ __forceinline__ UnitAt first_unit(const Walk& w, long long u0)
{
    const long long e0 = u0 * kUnit;  // the workgroup's first dense element
    const long long j0 = row_of(e0, w.width, w.inv_w);
    const uint32_t r = (uint32_t)(e0 - j0 * (long long)w.width) + threadIdx.x * kUnit;  // < width + 1024
    const uint32_t q = r / w.width;
    return {j0 + q, r - q * w.width};
}

// From one of a thread's units to its next, kBlock units on.
__device__ __forceinline__ void next_unit(const Walk& w, UnitAt& p)
{
    p.c += w.step_c;
    p.j += w.step_j;
    if (p.c >= w.width) {
        p.c -= w.width;
        p.j++;
    }
}

// ============================== gather / scatter ===============================
template <bool kScatter, typename V>
__device__ __forceinline__ void move_units(const RowField& F, long long u0, const uint32_t* __restrict__ indices)
{
    constexpr uint32_t kUnit = sizeof(V) / sizeof(uint32_t);
    UnitAt here = first_unit<kUnit>(F.w, u0);  // on the packed side
    size_t at[kUnroll];                        // element offset on the row side
    bool ok[kUnroll];
#pragma unroll
    for (int i = 0; i < kUnroll; i++) {  // every index load issued before any is used
        const long long u = u0 + i * kBlock + threadIdx.x;
        ok[i] = u < F.units;         // then here.j < k
        const uint32_t idx = indices[ok[i] ? here.j : 0];  // (entry 0 exists: k >= 1)
        ok[i] = ok[i] && (long long)idx < F.n_rows;  // an index past the rows is never dereferenced
        at[i] = (size_t)idx * F.w.width + here.c;
        next_unit(F.w, here);
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
__global__ __launch_bounds__(kBlock) void move_rows_kernel(const Batch<RowField> batch,
                                                           const uint32_t* __restrict__ indices)
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
    if (F.w.unit == 4)
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
    for (int i = 0; i < nfields; i++)
        if (int rc = check_shape(who, i, fields[i])) return rc;
    if (k == 0 || nfields == 0) return 0;
    if (!indices) return fail(HIDEGS_E_ARG, who + ": NULL indices");
    for (int i = 0; i < nfields; i++)
        if (!fields[i].packed || (fields[i].n_rows > 0 && !fields[i].rows))
            return fail(HIDEGS_E_ARG, who + ": field " + std::to_string(i) + ": NULL pointer");
    for (int i0 = 0; i0 < nfields; i0 += kMaxFields) {  // kMaxFields per launch
        Batch<RowField> batch;
        for (int i = i0; i < nfields && i < i0 + kMaxFields; i++) {
            const hidegs_row_field& a = fields[i];
            if (a.n_rows == 0) continue;  // every index is past the rows
            RowField F;
            F.rows = reinterpret_cast<uint32_t*>(a.rows);
            F.packed = reinterpret_cast<uint32_t*>(a.packed);
            F.n_rows = a.n_rows;
            // width a multiple of 4 and both bases on 16 bytes: every row start and every quad is aligned
            F.w = make_walk(a.width, (a.width % 4 == 0 && aligned16(a.rows) && aligned16(a.packed)) ? 4u : 1u);
            F.units = k * (long long)a.width / F.w.unit;
            if (int rc = place_field(batch, F, who)) return rc;
        }
        if (batch.count == 0) continue;
        const dim3 grid((unsigned)batch.first[batch.count]);
        if (scatter)
            HIDEGS_LAUNCH("scatter_rows", move_rows_kernel<true>, grid, dim3(kBlock), 0, stream, batch, indices);
        else
            HIDEGS_LAUNCH("gather_rows", move_rows_kernel<false>, grid, dim3(kBlock), 0, stream, batch, indices);
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
    Walk w;
};

// Consecutive lanes take consecutive units of dst.  A unit below F.kept is gathered (dst row j from src row
// keep[j], or row j itself without a keep array; zeros if that row is past the source); one at or after it
// comes from append at unit - F.kept, or is zeros.  Which of the two is workgroup-uniform except in the one
// workgroup that holds unit F.kept.
// kClone (include/hidegs_clone.h): the field's appended rows are rows of src too, dst row k + i from src row
// from[i].  Every unit of dst is then a gathered one; only the index array and the entry differ on the two
// sides of unit F.kept, so the pointer is selected and one load is issued, as for the data.
template <typename V, bool kKeep, bool kClone>
__device__ __forceinline__ void resize_units(const ResizeField& F, long long u0, const uint32_t* __restrict__ keep,
                                             const uint32_t* __restrict__ from_list, long long k)
{
    constexpr uint32_t kUnit = sizeof(V) / sizeof(uint32_t);
    UnitAt here = first_unit<kUnit>(F.w, u0);  // in dst
    uint32_t idx[kUnroll], col[kUnroll];
#pragma unroll
    for (int i = 0; i < kUnroll; i++) {  // every index load issued before any is used
        const long long u = u0 + i * kBlock + threadIdx.x;
        // a gathered unit (u < F.kept) has here.j < k; entry 0 exists (keep is passed only where k >= 1)
        if constexpr (kClone) {
            // an appended unit (F.kept <= u < F.units) has k <= here.j < k + n_append; entry 0 of from_list exists
            // (a field is cloned only where n_append >= 1) and serves the lanes past the last unit
            const bool gathered = kKeep && u < F.kept;
            const uint32_t* list = gathered ? keep : from_list;
            const long long entry = gathered ? here.j : (u >= F.kept && u < F.units ? here.j - k : 0);
            const uint32_t got = list[entry];
            idx[i] = (!kKeep && u < F.kept) ? (uint32_t)here.j : got;
        } else {
            idx[i] = kKeep ? keep[u < F.kept ? here.j : 0] : (uint32_t)here.j;
        }
        col[i] = here.c;
        next_unit(F.w, here);
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
        const size_t at =
            in_src ? ((size_t)idx[i] * F.w.width + col[i]) / kUnit : (in_append ? (size_t)(u - F.kept) : 0);
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

// The instance of resize_units for the launch's keep list (workgroup-uniform: given or not) and the field's unit.
template <bool kClone>
__device__ __forceinline__ void resize_field_units(const ResizeField& F, long long u0,
                                                   const uint32_t* __restrict__ keep,
                                                   const uint32_t* __restrict__ from, long long k)
{
    if (keep) {
        if (F.w.unit == 4)
            resize_units<u32x4, true, kClone>(F, u0, keep, from, k);
        else
            resize_units<uint32_t, true, kClone>(F, u0, keep, from, k);
    } else {
        if (F.w.unit == 4)
            resize_units<u32x4, false, kClone>(F, u0, keep, from, k);
        else
            resize_units<uint32_t, false, kClone>(F, u0, keep, from, k);
    }
}

// kCloning (include/hidegs_clone.h): the launch has cloned fields.  Bit f of `cloned` says that field f of the
// batch takes its appended rows from src, row from[i] for dst row k + i; the mode is workgroup-uniform like the
// descriptor.  Without kCloning there is no such field and from, k and cloned are not read.
template <bool kCloning>
__global__ __launch_bounds__(kBlock) void resize_kernel(const Batch<ResizeField> batch,
                                                        const uint32_t* __restrict__ keep,
                                                        const uint32_t* __restrict__ from, long long k, uint32_t cloned)
{
    // workgroup-uniform selects over constant indices: the descriptors stay in scalar registers
    ResizeField F = batch.f[0];
    int first = batch.first[0];
    bool clone = kCloning && (cloned & 1u);
#pragma unroll
    for (int i = 1; i < kMaxFields; i++) {
        if (i < batch.count && (int)blockIdx.x >= batch.first[i]) {
            F = batch.f[i];
            first = batch.first[i];
            if (kCloning) clone = (cloned >> i) & 1u;
        }
    }
    const long long u0 = (long long)((int)blockIdx.x - first) * kUnitsPerBlock;
    if (!F.safe) {
        if (F.w.unit == 4)
            zero_units<u32x4>(F, u0);
        else
            zero_units<uint32_t>(F, u0);
    } else if (clone) {
        resize_field_units<kCloning>(F, u0, keep, from, k);
    } else {
        resize_field_units<false>(F, u0, keep, from, k);
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
    // width a multiple of 4 and every base on 16 bytes: every row start and every quad is aligned, and
    // k * width is a multiple of 4, so no quad holds both gathered and appended floats
    F.w = make_walk(width, (width % 4 == 0 && aligned16(F.src) && aligned16(F.append) && aligned16(dst)) ? 4u : 1u);
    F.kept = k * (long long)width / F.w.unit;
    F.units = (k + n_append) * (long long)width / F.w.unit;
    return F;
}

bool is_cloned(const hidegs_resize_field&) { return false; }
bool is_cloned(const hidegs_clone_field& a) { return a.cloned != 0; }

// hidegs_resize_rows and hidegs_resize_rows_cloned, `name` without its prefix; the first has no cloned field
// and no `from`.  A batch without a cloned field is a launch of resize_kernel<false>, whichever entry was called.
template <typename Field>
int resize_rows(const char* name, const Field* fields, int nfields, const uint32_t* keep, long long k,
                const uint32_t* from, long long n_append, hipStream_t stream)
{
    const std::string who = name;
    if (nfields < 0) return fail(HIDEGS_E_ARG, who + ": negative field count");
    if (k < 0 || n_append < 0 || k > kSelectMax || n_append > kSelectMax || k + n_append > kSelectMax)
        return fail(HIDEGS_E_ARG, who + ": k, n_append and k + n_append must be in [0, 2^31)");
    if (nfields > 0 && !fields) return fail(HIDEGS_E_ARG, who + ": NULL field list");
    bool any_cloned = false;
    for (int i = 0; i < nfields; i++) {
        if (int rc = check_shape(who, i, fields[i])) return rc;
        if (is_cloned(fields[i]) && fields[i].append)
            return fail(HIDEGS_E_ARG, who + ": field " + std::to_string(i) + ": cloned, but append is given");
        any_cloned = any_cloned || is_cloned(fields[i]);
    }
    if (k + n_append == 0 || nfields == 0) return 0;
    // the source of field `a` is read: for its kept rows, or for its cloned ones
    const auto reads_src = [&](const Field& a) { return a.n_rows > 0 && (k > 0 || (is_cloned(a) && n_append > 0)); };
    for (int i = 0; i < nfields; i++) {
        const Field& a = fields[i];
        if (!a.dst || (reads_src(a) && !a.src))
            return fail(HIDEGS_E_ARG, who + ": field " + std::to_string(i) + ": NULL pointer");
        if (!keep && k > a.n_rows)
            return fail(HIDEGS_E_ARG, who + ": field " + std::to_string(i) + ": without keep, k must not exceed n_rows");
    }
    if (any_cloned && n_append > 0 && !from) return fail(HIDEGS_E_ARG, who + ": NULL from with a cloned field");
    if (k == 0) keep = nullptr;  // no row is gathered by keep: the kernel reads no entry
    for (int i0 = 0; i0 < nfields; i0 += kMaxFields) {  // kMaxFields per launch
        Batch<ResizeField> batch;
        uint32_t cloned = 0;
        for (int i = i0; i < nfields && i < i0 + kMaxFields; i++) {
            const Field& a = fields[i];
            if (is_cloned(a) && n_append > 0) cloned |= 1u << batch.count;
            // a cloned field has no append side: 16-byte units where src and dst allow
            const ResizeField F = resize_field(reads_src(a) ? a.src : nullptr, n_append > 0 ? a.append : nullptr, a.dst,
                                               a.n_rows, a.width, k, n_append);
            if (int rc = place_field(batch, F, who)) return rc;
        }
        const dim3 grid((unsigned)batch.first[batch.count]);
        if (cloned)
            HIDEGS_LAUNCH("resize_rows_cloned", resize_kernel<true>, grid, dim3(kBlock), 0, stream, batch, keep, from,
                          k, cloned);
        else
            HIDEGS_LAUNCH("resize_rows", resize_kernel<false>, grid, dim3(kBlock), 0, stream, batch, keep,
                          (const uint32_t*)nullptr, 0LL, 0u);
    }
    return check_launch(name, stream, 0);
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
    return hidegs::resize_rows("resize_rows", fields, nfields, keep, k, nullptr, n_append, hidegs::as_stream(stream));
}

extern "C" int hidegs_resize_rows_cloned(const hidegs_clone_field* fields, int nfields, const uint32_t* keep, long long k,
                                         const uint32_t* from, long long n_append, void* stream)
{
    if (int rc = hidegs::take_async_error("hidegs_resize_rows_cloned", hidegs::as_stream(stream))) return rc;
    return hidegs::resize_rows("resize_rows_cloned", fields, nfields, keep, k, from, n_append,
                               hidegs::as_stream(stream));
}
