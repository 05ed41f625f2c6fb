/*
 * hidegs_nearest.h -- nearest-point index: an index over a (P,3) fp32 point cloud that is built once and then
 * asked, for arbitrary query positions, which point is nearest.  A primitive next to those of hidegs.h,
 * hidegs_rows.h and hidegs_topk.h, whose conventions hold here: device pointers, stream-ordered on `stream`,
 * 0 or a negative HIDEGS_E_* code with hidegs_last_error(), no allocation, no host read, no host
 * synchronisation, no state kept between calls (the caller provides every buffer).
 *
 * No reference formula: the reference maps world points to their nearest Gaussian with a dense distance matrix
 * (scene/gaussian_model.py:801-829), which cannot be formed at the project's sizes.  The definition here is
 * "nearest point, lowest index among equals", answered exactly.  Kernels: hidegs_amd/csrc/nearest.hip.
 */
#ifndef HIDEGS_NEAREST_H_INCLUDED
#define HIDEGS_NEAREST_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * points: (P, 3) fp32, row-major.  queries: (Q, 3) fp32, row-major.  0 <= P, Q < 2^31.
 *
 * Candidates: row i < P is a candidate iff its three coordinates are finite.
 *
 * Distance: d(q, p) = fmaf(dz, dz, fmaf(dx, dx, dy * dy)) with dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z,
 * in fp32 with every rounding as written (distCUDA2's expression).
 *
 * A query j whose three coordinates are finite receives the candidate i that minimises the pair
 * (bits(d) as u32, i) lexicographically -- the smallest distance, then the lowest row index:
 * idx_out[j] = i (int32) and dist2_out[j] = d.  d may be +inf through overflow; it is still ordered by its bits.
 * A query with a NaN or infinite coordinate, and every query when there is no candidate (P == 0 included),
 * receives idx_out[j] = -1 and dist2_out[j] = +inf.  Every output element is written.  The result is a function
 * of (points, queries) alone: grid size, dispatch order, scratch contents and the order of the queries have no
 * part in it.
 *
 * The index buffer (hidegs_nearest_index_bytes(P) bytes, 16-byte aligned) belongs to the caller and is
 * self-contained: it holds its own Morton-ordered copy of the points, so `points` may change or be freed once
 * the build's kernels have run.  Queries only read it, so several streams may query one index at once, each
 * with a scratch buffer of its own.  P at the query must be the build's P.
 *
 * Scratch buffers (16-byte aligned) may hold anything: what must start at zero is cleared by the call on
 * `stream`.  After a query's kernels have run, the first u32 of its scratch holds how many queries took the
 * second search phase (a diagnostic; the library never reads it on the host).
 *
 * Q == 0 returns 0 without a launch.  P == 0 builds nothing (index and scratch may then be NULL); its queries
 * write -1 / +inf.  idx_out and dist2_out must not overlap each other, the queries, the index or the scratch.
 * Both calls can be captured into a graph.  Launch boundaries are their only synchronisation of their own; the
 * Morton sort inside them is hidegs_sort_pairs_u64.
 */
size_t hidegs_nearest_index_bytes(long long P);
size_t hidegs_nearest_build_scratch_bytes(long long P);
int hidegs_nearest_build(void* index, size_t index_bytes, void* scratch, size_t scratch_bytes, const float* points,
                         long long P, void* stream);
size_t hidegs_nearest_query_scratch_bytes(long long P, long long Q);
int hidegs_nearest_query(const void* index, size_t index_bytes, long long P, void* scratch, size_t scratch_bytes,
                         const float* queries, long long Q, int32_t* idx_out, float* dist2_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HIDEGS_NEAREST_H_INCLUDED */
