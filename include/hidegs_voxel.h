/*
 * hidegs_voxel.h -- voxel grid over a point cloud: group the rows that share a cell, then reduce rows per
 * group.  A primitive family next to hidegs_rows.h and hidegs_topk.h, whose conventions hold here: device
 * pointers unless marked [host], stream-ordered on `stream`, 0 or a negative HIDEGS_E_* code with
 * hidegs_last_error(), no allocation, no host read (both calls can be captured into a graph), every
 * argument error reported before the first launch.  Scratch is the caller's and may hold anything.  Launch
 * boundaries are the only synchronisation; no workgroup waits on another.
 *
 * No reference counterpart: this is the voxel-grid filter of point-cloud libraries (thinning a dense cloud,
 * fusing coincident rows, per-cell statistics).  Kernels: hidegs_amd/csrc/voxel.hip.
 */
#ifndef HIDEGS_VOXEL_H_INCLUDED
#define HIDEGS_VOXEL_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Grouping.  Every step below is one fp32 operation, so that it can be restated bit for bit.
 *
 * Eligible rows: row i < P is eligible iff (among == NULL or among[i] != 0, any non-zero byte counts) and
 * its three coordinates are finite.
 *
 * Origin: with origin != NULL the three floats it points to.  With origin == NULL the componentwise minimum
 * over the eligible rows, computed by the call on the device; a minimum that is a zero is taken as +0.0
 * (min + 0.0f), and with no eligible row the origin is (0, 0, 0).  frame receives {origin.x, origin.y,
 * origin.z, cell}.
 *
 * Cell index: inv = 1.0f / cell, formed once on the host in fp32.  Per axis t = (p - origin) * inv: one fp32
 * subtraction, then one fp32 multiplication (no fused multiply-add).  c = floorf(t).
 *
 * Candidates: an eligible row is a candidate iff 0 <= t && t < 2^21 on all three axes (a NaN t, from a
 * non-finite origin or an overflow, fails both).  An eligible row that is no candidate is counted in info[2]
 * and belongs to no group; it is never clamped into a border cell.
 *
 * Key of a candidate: cx << 42 | cy << 21 | cz, below 2^63.
 *
 * Groups: the distinct keys, numbered 0 .. G-1 in ascending key.  With m candidates,
 *   order[0 .. m)      the candidate rows ascending by (key, row);
 *   starts[0 .. G]     group g is order[starts[g] .. starts[g+1]); starts[0] = 0, starts[G] = m;
 *   group_of[i]        the group of row i, or -1 where row i is no candidate; every element is written;
 *   first_flags[i]     1 iff row i is the lowest row of its group, else 0; every byte is written (may be NULL:
 *                      not wanted).  It is the keep mask of resize_rows and hidegs_select_flagged that leaves
 *                      one row per occupied cell.
 * order[m .. P) and starts[G+1 .. P] are not written.
 * info = {G, m, eligible rows that are no candidates, rows in the largest group (0 without a group)}.
 *
 * cell [host] must be finite and > 0 and 1.0f / cell must be finite; 0 <= P < 2^31.  P == 0 writes
 * info = {0, 0, 0, 0} and starts[0] = 0 and needs no points, group_of, order or scratch.  scratch holds at
 * least hidegs_voxel_group_scratch_bytes(P) bytes (0 at P <= 0 and past the range; it does not shrink as P
 * grows).  The outputs must not overlap the inputs, one another or scratch; points, among and origin must
 * not change until the call's kernels have run.  The result is a function of (points, among, cell, origin)
 * alone.
 */
size_t hidegs_voxel_group_scratch_bytes(long long P);
int hidegs_voxel_group(void* scratch, size_t scratch_bytes, const float* points, const unsigned char* among,
                       long long P, float cell, const float* origin, int32_t* group_of, uint32_t* order,
                       uint32_t* starts, unsigned char* first_flags, float* frame, uint32_t* info, void* stream);

/*
 * Reduction.  One field is a (n_rows, width) fp32 matrix src and a (max_groups, width) fp32 matrix out; every
 * field of a call is reduced over the same groups.
 */
typedef struct hidegs_voxel_field {
    const float* src; /* (n_rows, width) */
    float* out;       /* (max_groups, width) */
    long long n_rows;
    int width; /* >= 1 */
    int op;    /* HIDEGS_VOXEL_* */
} hidegs_voxel_field;

enum { HIDEGS_VOXEL_SUM = 0, HIDEGS_VOXEL_MEAN = 1, HIDEGS_VOXEL_MIN = 2, HIDEGS_VOXEL_MAX = 3, HIDEGS_VOXEL_FIRST = 4 };

/*
 * order, starts and info are the outputs of hidegs_voxel_group over a cloud of P rows (G = info[0] and
 * m = info[1] are read on the device; the launches are sized from P and max_groups, both [host]).  For every
 * group g < min(G, max_groups), every field and every column c, out[g * width + c] is the reduction of
 * src[row * width + c] over the rows of the group.  Rows of out from min(G, max_groups) on are not written,
 * and groups from max_groups on are skipped.  A row index in order that is >= n_rows of a field (>= P with
 * weights) is skipped for that field and never dereferenced; over no row at all SUM is 0, MEAN is 0/0,
 * MIN and MAX are NaN and FIRST is 0.
 *
 *   FIRST   the bits of the group's first row in order (its lowest row) that is not skipped;
 *   MIN/MAX as numbers: a NaN is ignored unless every value is a NaN; the sign of a zero result is unspecified;
 *   SUM     the sum of x, or with weights (P floats, or NULL) of w * x, the product rounded to fp32 first;
 *   MEAN    that sum divided by the number of rows as fp32, or with weights by the sum of w: one IEEE
 *           division, so 0/0 is a NaN.
 * weights does not enter MIN, MAX and FIRST.
 *
 * Determinism: there is no floating-point atomic anywhere.  The order in which a group's values are added
 * (a fixed split of the rows over lanes, a fixed tree over the lanes, fixed chunks of rows added in chunk
 * order) is a function of the group's size and the field's width alone, so the same call gives the same bits
 * every time and a group's result does not depend on which other groups exist.  That order is not the
 * sequential one and is not promised to stay what it is: the sum is within the bound that holds for every
 * order, |error| <= gamma(n) * sum |w * x| with gamma(k) = k u / (1 - k u), u = 2^-24.  A MEAN of n equal
 * values x is x itself where n * x has at most 24 significant bits (every partial sum is then exact).
 *
 * Any nfields >= 0 (one set of launches per 8 fields) and any width >= 1.  0 <= P < 2^31, max_groups >= 0;
 * with P == 0, nfields == 0 or max_groups == 0 nothing is launched.  scratch holds at least
 * hidegs_voxel_reduce_scratch_bytes(P, max_groups, max_width) bytes, max_width the widest field (0 at
 * P <= 0, max_width < 1 or past the range; it does not shrink as P or max_width grow).  out must not overlap
 * any input or scratch.
 */
size_t hidegs_voxel_reduce_scratch_bytes(long long P, long long max_groups, int max_width);
int hidegs_voxel_reduce_rows(void* scratch, size_t scratch_bytes, const hidegs_voxel_field* fields, int nfields,
                             const uint32_t* order, const uint32_t* starts, const uint32_t* info, long long P,
                             long long max_groups, const float* weights, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HIDEGS_VOXEL_H_INCLUDED */
