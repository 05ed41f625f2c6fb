/*
 * hidegs_nearest_k.h -- the k nearest points of arbitrary positions, with rows and distances, answered exactly
 * from the nearest-point index of hidegs_nearest.h.  The conventions of that header hold: device pointers,
 * stream-ordered on `stream`, 0 or a negative HIDEGS_E_* code with hidegs_last_error(), no allocation, no host
 * read, no host synchronisation, no state kept between calls, capturable in a graph.
 *
 * The index is the one hidegs_nearest_build wrote, unchanged; nothing is added to the build.
 * Kernels: hidegs_amd/csrc/nearest_k.h, a stage of nearest.hip.
 */
#ifndef HIDEGS_NEAREST_K_H_INCLUDED
#define HIDEGS_NEAREST_K_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * queries: (Q, 3) fp32, row-major.  exclude: (Q) int32 or NULL.  idx_out, dist2_out: (Q, k) row-major.
 * 0 <= P, Q < 2^31 and 1 <= k <= 64; any other k returns HIDEGS_E_ARG before any launch.
 *
 * Candidates of query j: the rows i < P whose three coordinates are finite, without row exclude[j] when
 * `exclude` is given and 0 <= exclude[j] < P.  Any other value of exclude[j] excludes nothing.
 *
 * Distance: hidegs_nearest.h's d(q, p) = fmaf(dz, dz, fmaf(dx, dx, dy * dy)) of (p - q), every rounding as
 * written.
 *
 * A query j whose three coordinates are finite receives, in idx_out[j*k + i] and dist2_out[j*k + i] for
 * i = 0 .. k-1, its candidates in ascending order of the pair (bits(d) as u32, row): the k smallest such pairs.
 * A distance of +inf through overflow is ordered by its bits and returned with its row, as for k = 1.  The
 * slots past the number of candidates receive -1 and +inf; so do all k slots of a query with a NaN or infinite
 * coordinate.  Every one of the Q*k elements of both outputs is written.  The result is a function of
 * (points, queries, k, exclude) alone.  Hence columns 0 .. k'-1 of a k-query are the k'-query, bit for bit,
 * and k = 1 without exclusion is hidegs_nearest_query, bit for bit.
 *
 * The scratch buffer (hidegs_nearest_query_k_scratch_bytes bytes, 16-byte aligned; the size does not depend on
 * P) may hold anything: what must start at zero is cleared by the call on `stream`.  After the call's kernels
 * have run, its first u32 holds how many queries were searched by one wave each rather than by one lane each
 * (every finite query when k > 16): a diagnostic the library never reads on the host.
 *
 * Q == 0 returns 0 without a launch.  P == 0 writes -1 / +inf; index and scratch may then be NULL.  idx_out
 * and dist2_out must not overlap each other, the queries, `exclude`, the index or the scratch.
 */
size_t hidegs_nearest_query_k_scratch_bytes(long long P, long long Q, int k);
int hidegs_nearest_query_k(const void* index, size_t index_bytes, long long P, void* scratch, size_t scratch_bytes,
                           const float* queries, long long Q, int k, const int32_t* exclude, int32_t* idx_out,
                           float* dist2_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HIDEGS_NEAREST_K_H_INCLUDED */
