/*
 * hidegs_nearest_lists.h -- variable-length neighbour lists from the nearest-point index of hidegs_nearest.h:
 * every row within a radius of arbitrary positions, in CSR form (offsets, rows, distances), exactly and with no
 * limit on a list's length.  The conventions of hidegs_nearest_within.h hold: device pointers, stream-ordered on
 * `stream`, 0 or a negative HIDEGS_E_* code with hidegs_last_error(), no allocation, no host read, no host
 * synchronisation, no state kept between calls, capturable in a graph, every argument error before the first
 * launch, and a scratch buffer that may hold anything.
 *
 * The index is the one hidegs_nearest_build wrote, unchanged; nothing is added to the build.
 * Kernels: hidegs_amd/csrc/nearest_lists.h, a stage of nearest.hip.
 *
 * Candidates of query j, the distance d and "in range" are hidegs_nearest_within.h's: the rows i < P whose three
 * coordinates are finite, without row exclude[j] when `exclude` is given and 0 <= exclude[j] < P;
 * d(q, p) = fmaf(dz, dz, fmaf(dx, dx, dy * dy)) of (p - q), every rounding as written; a candidate is in range
 * iff r2[j] >= 0 and bits(d) <= bits(r2[j] + 0.0f), both as u32.  The boundary is inclusive, r2[j] = +inf takes
 * every candidate, nothing is in range of a negative or NaN radius, and a query with a NaN or infinite coordinate
 * has an empty list.
 *
 * The list of query j holds every candidate in range, each exactly once, at positions starts[j] .. starts[j+1])
 * of `rows` and of `d2`; starts[0] = 0 and starts[Q] = M, the number of entries of all lists.  d2 holds the bits
 * of d that hidegs_nearest_query_within reports for the same pair.  Inside a list the entries ascend by their
 * position in the index (hidegs_nearest_index_order), which is a function of the points alone.  Hence the list of
 * a query is a function of (points, that query, its r2, its exclude) alone: not of the other queries of the call,
 * not of how often it is asked.  The lists are not sorted by distance; where the nearest come first and 64
 * suffice, hidegs_nearest_query_within serves.
 *
 * Two calls make the lists: hidegs_nearest_list_offsets counts and scans, hidegs_nearest_list_fill writes.  The
 * caller sizes `rows` and `d2` between them (M is in info_out), or gives a capacity chosen beforehand.
 */
#ifndef HIDEGS_NEAREST_LISTS_H_INCLUDED
#define HIDEGS_NEAREST_LISTS_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * order_out: (P) int32.  order_out[i] = the row stored at position i of the index: a permutation of 0 .. P-1 in
 * which the rows with a non-finite coordinate come behind every candidate.  It is the order in which
 * hidegs_nearest_build stored the points (ascending Morton key in the cloud's own frame, rows of equal keys in
 * ascending row order), the same for every build over the same points.  0 <= P < 2^31; P == 0 returns 0 without
 * a launch.  order_out may not overlap the index.
 */
int hidegs_nearest_index_order(const void* index, size_t index_bytes, long long P, int32_t* order_out, void* stream);

/*
 * queries: (Q, 3) fp32, row-major.  r2: (Q) fp32, the squared radius of every query.  exclude: (Q) int32 or
 * NULL.  starts_out: (Q + 1) int32.  info_out: 4 u32, 8-byte aligned.  0 <= P, Q < 2^31.
 *
 * starts_out[0] = 0 and starts_out[j + 1] = starts_out[j] + the exact number of candidates in range of query j
 * (hidegs_nearest_query_within's count with k = 0 and max_count = 2^31 - 1, by that call's own kernels, scanned by
 * hidegs_inclusive_scan_u32).  info_out = {M mod 2^32, M / 2^32, the longest list, the number of non-empty
 * lists}; M is summed in 64 bits.  starts_out is exact iff M <= 2^31 - 1; above that its content is unspecified
 * (every element is still written) and a caller must not fill.
 *
 * starts_out and info_out are required at every P and Q.  Q == 0 writes starts_out[0] = 0 and a zero info;
 * P == 0 writes zeros, and index and scratch may then be NULL.  The scratch buffer is
 * hidegs_nearest_list_offsets_scratch_bytes(P, Q) bytes, 16-byte aligned.  No output may overlap the other, the
 * queries, `r2`, `exclude`, the index or the scratch.
 */
size_t hidegs_nearest_list_offsets_scratch_bytes(long long P, long long Q);
int hidegs_nearest_list_offsets(const void* index, size_t index_bytes, long long P, void* scratch, size_t scratch_bytes,
                                const float* queries, long long Q, const float* r2, const int32_t* exclude,
                                int32_t* starts_out, uint32_t* info_out, void* stream);

/*
 * starts: (Q + 1) int32, as hidegs_nearest_list_offsets wrote it for the same index, queries, r2 and exclude.
 * rows_out: (capacity) int32.  dist2_out: (capacity) fp32 or NULL (no distances).  capacity >= 0; a negative one
 * returns HIDEGS_E_ARG before any launch, at Q == 0 as well.  Positions are below 2^31, so a capacity above
 * 2^31 - 1 is that.  rows_out may be NULL iff capacity == 0.
 *
 * For every query j, entry i of its list (in the order above) goes to position starts[j] + i of rows_out and of
 * dist2_out iff 0 <= starts[j] and that position is below min(starts[j + 1], capacity).  Nothing else is written:
 * whatever `starts` holds, no byte outside rows_out[0 .. capacity) and dist2_out[0 .. capacity) is touched.  So
 * capacity < M cuts the lists at a fixed position -- every position below the cut holds what the full call would
 * have put there -- and capacity == 0 writes nothing; a `starts` that disagrees with the counts loses entries and
 * never writes out of bounds.  A query with starts[j] == starts[j + 1] is not searched, and a search ends with
 * its last position.
 *
 * The call keeps no state from hidegs_nearest_list_offsets: it keys and sorts its queries itself, for coherence
 * only.  The scratch buffer is hidegs_nearest_list_fill_scratch_bytes(P, Q) bytes, 16-byte aligned
 * (hidegs_nearest_query_scratch_bytes's).  Q == 0 and P == 0 return 0 without writing; index and scratch may
 * then be NULL.  No output may overlap the other, the queries, `r2`, `exclude`, `starts`, the index or the
 * scratch.
 */
size_t hidegs_nearest_list_fill_scratch_bytes(long long P, long long Q);
int hidegs_nearest_list_fill(const void* index, size_t index_bytes, long long P, void* scratch, size_t scratch_bytes,
                             const float* queries, long long Q, const float* r2, const int32_t* exclude,
                             const int32_t* starts, long long capacity, int32_t* rows_out, float* dist2_out,
                             void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HIDEGS_NEAREST_LISTS_H_INCLUDED */
