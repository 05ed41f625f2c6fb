/*
 * hidegs_moments.h -- moments of neighbour lists: the weighted mean and covariance of the points that every
 * query's list names, and the eigen-decomposition of symmetric 3x3 matrices.  A primitive family next to
 * hidegs_voxel.h, whose conventions hold here: device pointers unless marked [host], stream-ordered on
 * `stream`, 0 or a negative HIDEGS_E_* code with hidegs_last_error(), no allocation, no host read (every call
 * can be captured into a graph), every argument error reported before the first launch.  Scratch is the
 * caller's and may hold anything.  Launch boundaries are the only synchronisation; no workgroup waits on
 * another, and there is no floating-point atomic anywhere.
 *
 * No reference counterpart: these are the local frames a point-cloud library derives from a neighbour search
 * (normals, planarity, an oriented anisotropic scale).  Kernels: hidegs_amd/csrc/moments.hip.
 */
#ifndef HIDEGS_MOMENTS_H_INCLUDED
#define HIDEGS_MOMENTS_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The lists.  Query j < Q has a list of L entries, each the row of a point:
 *   table form   table is (Q, k) int32, k >= 1 (hidegs_nearest_query_k, hidegs_nearest_query_within): the list
 *                of query j is its k slots, L = k;
 *   list form    starts is (Q + 1) int32 and rows is (capacity) int32, as hidegs_nearest_list_offsets and
 *                hidegs_nearest_list_fill write them: the list of query j is the positions from
 *                max(starts[j], 0) up to, not including, min(starts[j + 1], capacity) of rows, and is empty
 *                where that range is empty.  A list that the capacity cut is reduced over the part that was
 *                written; no position at or past capacity is read, whatever starts holds.
 *
 * The rule.  Every step below is one fp32 operation, so that it can be restated bit for bit.
 *
 * Validity: an entry with row r is valid iff 0 <= r < P and the three coordinates of row r of points are
 * finite.  Invalid entries (-1, rows past P, non-finite points) are skipped wherever they stand; a row that
 * occurs twice counts twice.  count[j] is the number of valid entries, with or without weights.
 *
 * Weight: w = weights[r], or 1.0f with weights == NULL.  Weights enter as they are: a NaN or negative weight
 * is no error, it propagates.
 *
 * Order of additions: the list's positions 0 .. L-1 are cut into blocks of 64 consecutive positions.  A block's
 * partial starts at +0.0f and takes the block's valid entries in ascending position.  A total is block 0's
 * partial plus the partials of blocks 1, 2, ... in block order (plain fp32 additions; a block without a valid
 * entry contributes its +0.0f; an empty list's totals are +0.0f).  For L <= 64 the total is one sequential sum.
 * The order depends on the list's length and on where its valid entries stand, not on Q or on the other lists.
 *
 * Pass 1:  W accumulates acc + w;  S_c accumulates fmaf(w, p_c, acc) for c = x, y, z;  mean_c = S_c / W, one
 *          IEEE division (an empty list gives 0/0 = NaN).
 * Pass 2:  d_c = p_c - mean_c (one subtraction);  t_x = w * d_x (one rounded product), C_xx = fmaf(t_x, d_x, acc),
 *          C_xy = fmaf(t_x, d_y, acc), C_xz = fmaf(t_x, d_z, acc);  t_y = w * d_y, C_yy = fmaf(t_y, d_y, acc),
 *          C_yz = fmaf(t_y, d_z, acc);  t_z = w * d_z, C_zz = fmaf(t_z, d_z, acc);  the same blocks as pass 1;
 *          cov = C / W: the population covariance.
 * With weights == NULL and with weights all 1.0f the outputs are the same bits (W = n is exact below 2^24).
 *
 * Outputs: count (Q) int32, mean (Q, 3), cov (Q, 6) in the order xx, xy, xz, yy, yz, zz, and evals (Q, 3) and
 * evecs (Q, 3, 3) as hidegs_sym3_eigen gives them for cov -- both NULL (not wanted) or both given.  Every
 * element of every given output is written.
 *
 * 0 <= P, Q < 2^31, 0 <= capacity < 2^31; points may be NULL where P == 0 (every entry is then invalid).
 * Q == 0 launches nothing and needs no pointer.  scratch holds at least hidegs_neighbor_moments_scratch_bytes(Q)
 * bytes (0 at Q <= 0 and past the range; it does not shrink as Q grows); the table form needs none and takes
 * none.  The outputs must not overlap the inputs, one another or scratch.
 */
size_t hidegs_neighbor_moments_scratch_bytes(long long Q);
int hidegs_neighbor_moments_table(const float* points, const float* weights, long long P, const int32_t* table,
                                  long long Q, int k, int32_t* count, float* mean, float* cov, float* evals,
                                  float* evecs, void* stream);
int hidegs_neighbor_moments_lists(void* scratch, size_t scratch_bytes, const float* points, const float* weights,
                                  long long P, const int32_t* starts, const int32_t* rows, long long capacity,
                                  long long Q, int32_t* count, float* mean, float* cov, float* evals, float* evecs,
                                  void* stream);

/*
 * Eigen-decomposition of Q symmetric 3x3 matrices, cov (Q, 6) in the order xx, xy, xz, yy, yz, zz.
 *   evals (Q, 3)     ascending: l0 <= l1 <= l2;
 *   evecs (Q, 3, 3)  row i is a unit eigenvector of l_i: row 0 is the normal of a planar neighbourhood, row 2
 *                    its main direction.  In rows 0 and 1 the component of largest magnitude is positive (the
 *                    lowest index among equal magnitudes); row 2 has the sign that makes det(evecs[j]) = +1,
 *                    so the matrix is a rotation.
 * Where any of the six inputs is not finite all twelve outputs are NaN.  The zero matrix gives zeros and the
 * identity.  The method is a cyclic Jacobi iteration of a fixed number of sweeps (no data-dependent loop
 * bound); its results are specified by residuals against single-precision LAPACK, not by bits.
 * Supported magnitudes: matrices whose Frobenius norm is at most 2^126, so that no eigenvalue and no intermediate
 * diagonal entry leaves the float range; above that a finite input may give infinite or NaN outputs.
 * 0 <= Q < 2^31; Q == 0 launches nothing.  evals and evecs must not overlap cov.
 */
int hidegs_sym3_eigen(const float* cov, float* evals, float* evecs, long long Q, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HIDEGS_MOMENTS_H_INCLUDED */
