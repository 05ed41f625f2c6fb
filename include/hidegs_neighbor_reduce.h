/*
 * hidegs_neighbor_reduce.h -- per-row fields reduced over neighbour lists: for every query, the sum, weighted
 * mean, minimum or maximum of the rows of arbitrary (P, width) float fields that the query's list names.  The
 * third member of the family of hidegs_voxel.h (rows that share a cell) and hidegs_moments.h (positions over
 * neighbour lists), whose conventions hold here: device pointers unless marked [host], stream-ordered on
 * `stream`, 0 or a negative HIDEGS_E_* code with hidegs_last_error(), no allocation, no host read (every call
 * can be captured into a graph), every argument error reported before the first launch.  Scratch is the
 * caller's and may hold anything.  Launch boundaries are the only synchronisation; no workgroup waits on
 * another, and there is no floating-point atomic anywhere.
 *
 * No reference counterpart: this is the gather-and-combine behind attribute transfer, inverse-distance
 * (Shepard) interpolation, neighbourhood smoothing and local extrema.  Kernels: hidegs_amd/csrc/neighbor_reduce.hip.
 */
#ifndef HIDEGS_NEIGHBOR_REDUCE_H_INCLUDED
#define HIDEGS_NEIGHBOR_REDUCE_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One field: src (P, width) is reduced into out (Q, width) by `op`. */
typedef struct hidegs_neighbor_field {
    const float* src; /* (P, width) */
    float* out;       /* (Q, width) */
    int width;        /* >= 1 */
    int op;           /* HIDEGS_NEIGHBOR_* */
} hidegs_neighbor_field;
enum { HIDEGS_NEIGHBOR_SUM = 0, HIDEGS_NEIGHBOR_MEAN = 1, HIDEGS_NEIGHBOR_MIN = 2, HIDEGS_NEIGHBOR_MAX = 3 };

/*
 * The lists are those of hidegs_moments.h.  Query j < Q has a list of L entries, each the row of a point:
 *   table form   table is (Q, k) int32, k >= 1: the list of query j is its k slots, L = k, and the entry at slot i
 *                stands at position j * k + i;
 *   list form    starts is (Q + 1) int32 and rows is (capacity) int32: the list of query j is the positions from
 *                max(starts[j], 0) up to, not including, min(starts[j + 1], capacity) of rows, and is empty where
 *                that range is empty.  No position at or past capacity is read, of rows or of entry_weights,
 *                whatever starts holds.
 * entry_weights is NULL or one float per entry position, laid out like the entries: (Q, k) for a table,
 * (capacity) for lists -- the d2 of a k-nearest query or of neighbour lists, or anything derived from it.
 * weights is NULL or (P) floats, one per row.
 *
 * The rule.  Every step below is one fp32 operation, so that it can be restated bit for bit.
 *
 * Validity: an entry with row r is valid iff 0 <= r < P.  Invalid entries (-1, rows past P) are skipped wherever
 * they stand, and their entry weight never enters; a row that occurs twice counts twice.  count[j] is the number
 * of valid entries.  Field values that are not finite are not skipped: they propagate.
 *
 * Weight of a valid entry at position pos with row r: w = 1.0f with neither weight given; w = weights[r] or
 * w = entry_weights[pos] with one of them given; w = weights[r] * entry_weights[pos], one rounded product, with
 * both.  Weights enter as they are: a NaN or negative weight is no error, it propagates.
 *
 * Order of additions (that of hidegs_moments.h): the list's positions 0 .. L-1 are cut into blocks of 64
 * consecutive positions.  A block's partial starts at +0.0f and takes the block's valid entries in ascending
 * position.  A total is block 0's partial plus the partials of blocks 1, 2, ... in block order (plain fp32
 * additions; a block without a valid entry contributes its +0.0f; an empty list's totals are +0.0f).
 *   SUM   per column c, S_c accumulates fmaf(w, x_c, acc) with x_c the field's value in row r;  out_c = S_c;
 *   MEAN  W accumulates acc + w in the same order;  out_c = S_c / W, one IEEE division (a list without a valid
 *         entry gives 0/0 = NaN).
 * With no weights and with weights that are all 1.0f the outputs are the same bits.
 *   MIN / MAX  as numbers: a NaN is ignored unless every value is a NaN; the sign of a zero result is
 *         unspecified.  Weights do not enter.
 * Over no valid entry SUM is +0.0f and MEAN, MIN and MAX are NaN.
 *
 * A list's result depends on that list, its weights and the field alone: not on Q, on the other lists, on the
 * other fields of the call, or on which kernel served it.  With the (P, 3) points as the field, op MEAN and no
 * entry_weights, out is the mean of hidegs_neighbor_moments_* in every bit wherever every point is finite.
 *
 * Any nfields >= 0 (one set of launches per 8 fields), every field with its own width >= 1 and op.  0 <= P, Q,
 * capacity < 2^31; offsets into src and out are 64-bit.  src may be NULL where P == 0 (every entry is then
 * invalid).  count (Q) int32 may be NULL (not wanted).  Q == 0 launches nothing and looks at no pointer;
 * nfields == 0 writes count alone (and launches nothing where count is NULL).  Every element of every out and of
 * a given count is written.  The outputs must not overlap the inputs, one another or scratch.
 *
 * scratch: the list form needs hidegs_neighbor_reduce_scratch_bytes(Q, max_width) bytes, max_width the widest
 * field of the call (0 at Q <= 0 and past the range; it does not shrink as Q or max_width grows).  The table form
 * needs no scratch: its scratch and scratch_bytes are not looked at and may be NULL and 0.
 */
size_t hidegs_neighbor_reduce_scratch_bytes(long long Q, int max_width);

int hidegs_neighbor_reduce_table(void* scratch, size_t scratch_bytes, const hidegs_neighbor_field* fields /*[host]*/,
                                 int nfields, long long P, const float* weights, const int32_t* table,
                                 const float* entry_weights, long long Q, int k, int32_t* count, void* stream);

int hidegs_neighbor_reduce_lists(void* scratch, size_t scratch_bytes, const hidegs_neighbor_field* fields /*[host]*/,
                                 int nfields, long long P, const float* weights, const int32_t* starts,
                                 const int32_t* rows, const float* entry_weights, long long capacity, long long Q,
                                 int32_t* count, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HIDEGS_NEIGHBOR_REDUCE_H_INCLUDED */
