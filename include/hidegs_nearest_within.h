/*
 * hidegs_nearest_within.h -- the fixed-radius query of the nearest-point index of hidegs_nearest.h: how many
 * points lie within a radius of arbitrary positions, and the k nearest of them with rows and distances, both
 * exactly.  The conventions of that header hold: device pointers, stream-ordered on `stream`, 0 or a negative
 * HIDEGS_E_* code with hidegs_last_error(), no allocation, no host read, no host synchronisation, no state kept
 * between calls, capturable in a graph.
 *
 * The index is the one hidegs_nearest_build wrote, unchanged; nothing is added to the build.
 * Kernels: hidegs_amd/csrc/nearest_within.h, a stage of nearest.hip.
 */
#ifndef HIDEGS_NEAREST_WITHIN_H_INCLUDED
#define HIDEGS_NEAREST_WITHIN_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * queries: (Q, 3) fp32, row-major.  r2: (Q) fp32, the squared radius of every query.  exclude: (Q) int32 or
 * NULL.  count_out: (Q) int32.  idx_out, dist2_out: (Q, k) row-major; both may be NULL iff k == 0.
 * 0 <= P, Q < 2^31, 0 <= k <= 64 and max(k, 1) <= max_count <= 2^31 - 1; any other k or max_count returns
 * HIDEGS_E_ARG before any launch, at Q == 0 as well.
 *
 * Candidates of query j and the distance d are hidegs_nearest_k.h's: the rows i < P whose three coordinates are
 * finite, without row exclude[j] when `exclude` is given and 0 <= exclude[j] < P, and
 * d(q, p) = fmaf(dz, dz, fmaf(dx, dx, dy * dy)) of (p - q), every rounding as written.
 *
 * A candidate is in range of query j iff r2[j] >= 0 and bits(d) <= bits(r2[j] + 0.0f), both as u32: the boundary
 * is inclusive and -0 is 0.  r2[j] = +inf takes every candidate, one whose d overflowed to +inf included; with
 * r2[j] negative or a NaN nothing is in range.
 *
 * count_out[j] = min(number of candidates in range, max_count).  idx_out[j*k + i] and dist2_out[j*k + i] for
 * i = 0 .. k-1 receive the candidates in range in ascending order of the pair (bits(d) as u32, row): the k
 * smallest such pairs.  The slots past them receive -1 and +inf.  A query with a NaN or infinite coordinate
 * receives the count 0 and -1 / +inf in every slot.  Every element of the three outputs is written.  The result
 * is a function of (points, queries, r2, k, max_count, exclude) alone.  Hence max_count changes count_out only,
 * never a slot; columns 0 .. k'-1 of a k-call are the k'-call's slots; with r2 = +inf the slots are
 * hidegs_nearest_query_k's, bit for bit; and where count_out[j] < max_count it is the exact count.
 *
 * max_count is what lets a caller ask "at least m within r" cheaply: a query that has counted max_count and
 * filled its k slots with the k nearest is searched no further.
 *
 * The scratch buffer (hidegs_nearest_query_within_scratch_bytes bytes, 16-byte aligned; the size does not depend
 * on P or k and is hidegs_nearest_query_scratch_bytes's) may hold anything: what must start at zero is cleared
 * by the call on `stream`.  After the call's kernels have run, its first u32 holds how many queries were
 * searched by one wave each rather than by one lane each (every finite query with a radius that is no NaN and
 * not negative when k > 16): a diagnostic the library never reads on the host.
 *
 * Q == 0 returns 0 without a launch.  P == 0 writes zeros and -1 / +inf; index and scratch may then be NULL.
 * No output may overlap another output, the queries, `r2`, `exclude`, the index or the scratch.
 */
size_t hidegs_nearest_query_within_scratch_bytes(long long P, long long Q, int k);
int hidegs_nearest_query_within(const void* index, size_t index_bytes, long long P, void* scratch, size_t scratch_bytes,
                                const float* queries, long long Q, const float* r2, int k, int max_count,
                                const int32_t* exclude, int32_t* count_out, int32_t* idx_out, float* dist2_out,
                                void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HIDEGS_NEAREST_WITHIN_H_INCLUDED */
