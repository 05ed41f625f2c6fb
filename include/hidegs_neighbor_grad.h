/*
 * hidegs_neighbor_grad.h -- what the gradients of hidegs_neighbor_reduce.h need: the transpose of neighbour lists
 * ("who named me": for every row, the queries and forward positions of the entries that name it) and the backward
 * of the SUM and MEAN reductions with respect to the fields, the row weights and the entry weights.  The
 * conventions are those of hidegs_neighbor_reduce.h: device pointers unless marked [host], stream-ordered on
 * `stream`, 0 or a negative HIDEGS_E_* code with hidegs_last_error(), the caller's scratch (it may hold anything),
 * no allocation and no host read (every call can be captured into a graph), every argument error reported before
 * the first launch.  Launch boundaries are the only synchronisation; no workgroup waits on another, and there is
 * no floating-point atomic anywhere: every result is a function of the inputs alone.
 *
 * No reference counterpart.  Kernels: hidegs_amd/csrc/neighbor_grad.hip.
 */
#ifndef HIDEGS_NEIGHBOR_GRAD_H_INCLUDED
#define HIDEGS_NEIGHBOR_GRAD_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Transposed neighbour lists.
 *
 * The forward structure is that of hidegs_neighbor_reduce_*: a (Q, k) table, or starts (Q + 1) and rows
 * (capacity) with every span clamped to [0, capacity) as there; the list form takes starts that do not decrease
 * (those of hidegs_nearest_list_*), and a position belongs to the one list whose span holds it.  It has E
 * positions, E = Q * k or E = capacity; the entry of the table's slot (j, i) stands at position j * k + i, a CSR
 * entry at its position in rows.  An entry is valid iff it lies inside a list and its row r is in [0, P).
 * E must be at most 2^31 - 1, like P and Q: otherwise the call fails and launches nothing.
 *
 * Outputs: starts_t (P + 1) int32, query_t (E) and entry_t (E) int32, info (4) int32.  The transposed list of row
 * r is the positions starts_t[r] .. starts_t[r + 1] of query_t and entry_t: the query and the forward position of
 * every valid entry that names r, in ascending forward position -- a row that a query lists twice stands twice.
 * starts_t[P] == V, the number of valid entries; query_t and entry_t hold -1 from V on.  info is {V, 0, the
 * longest transposed list, the rows named at least once}.  Every element of every output is written, at Q == 0,
 * E == 0 (starts_t all 0) and P == 0 (starts_t = {0}) too.  (starts_t, query_t) are neighbour lists over the Q
 * queries as rows: hidegs_neighbor_reduce_lists takes them as they are, with capacity E.
 *
 * Method: one pass emits (row, or P for an invalid entry; position) per position, the stable sort_pairs_u32 of
 * hidegs.h sorts them over the bit_length(P) key bits -- its stability is the ascending-position order -- one
 * pass finds every row's first position in the sorted keys, one decodes every position's query (position / k, or
 * a search of starts).  info is accumulated with integer atomics.
 *
 * scratch: hidegs_neighbor_transpose_scratch_bytes(E) bytes (0 at E <= 0 and past the range).
 */
size_t hidegs_neighbor_transpose_scratch_bytes(long long E);

int hidegs_neighbor_transpose_table(void* scratch, size_t scratch_bytes, long long P, const int32_t* table, long long Q,
                                    int k, int32_t* starts_t, int32_t* query_t, int32_t* entry_t, int32_t* info,
                                    void* stream);

int hidegs_neighbor_transpose_lists(void* scratch, size_t scratch_bytes, long long P, const int32_t* starts,
                                    const int32_t* rows, long long capacity, long long Q, int32_t* starts_t,
                                    int32_t* query_t, int32_t* entry_t, int32_t* info, void* stream);

/*
 * The backward of SUM and MEAN.
 *
 * One field of the forward call: src (P, width) was reduced into out (Q, width) by op, HIDEGS_NEIGHBOR_SUM or
 * HIDEGS_NEIGHBOR_MEAN; grad_out (Q, width) is the gradient of out.  grad_src (P, width) receives the gradient of
 * src, or is NULL (not wanted).
 */
typedef struct hidegs_neighbor_grad_field {
    const float* src;      /* (P, width) */
    const float* out;      /* (Q, width), as the forward wrote it */
    const float* grad_out; /* (Q, width) */
    float* grad_src;       /* (P, width) or NULL */
    int width;             /* >= 1 */
    int op;                /* HIDEGS_NEIGHBOR_SUM or HIDEGS_NEIGHBOR_MEAN */
} hidegs_neighbor_grad_field;

/*
 * Notation: a valid entry at position pos belongs to query j and names row r; g is grad_out; W_j = wsum[j] is the
 * weight total of query j as the forward's rule gives it (the SUM of a field of ones with the same weights);
 * m = 1 for MEAN and 0 for SUM.  wsum (Q) may be NULL where no field is a MEAN.
 *
 * grad_src, every bit:  c[pos] = entry_weights[pos], or 1.0f without entry weights, for MEAN divided by W_j (one
 * IEEE division).  S[r, col] is the SUM rule of hidegs_neighbor_reduce.h over row r's transposed list with g as
 * the field, c[entry] as every entry's weight and no row weights.  grad_src[r, col] = S[r, col], times weights[r]
 * (one multiplication) where weights are given and r is named at least once; a row that nobody names gets +0.0f.
 * It is computed by hidegs_neighbor_reduce_lists itself over (starts_t, query_t).
 *
 * grad_entry_weights (laid out like the entries) or NULL: with D[pos] the sum over the fields and columns of
 * g[j, col] * (x[r, col] - m * out[j, col]), taken apart for the SUM and the MEAN fields,
 *   grad_entry_weights[pos] = weights[r] * (D_sum[pos] + D_mean[pos] / W_j),
 * and 0 at an invalid position and outside every list.  The order of the additions inside D is the kernel's.
 *
 * grad_weights (P) or NULL: the SUM rule over row r's transposed list of the per-entry values
 * entry_weights[pos] * (D_sum[pos] + D_mean[pos] / W_j), unweighted; +0.0f for a row that nobody names.
 *
 * starts_t, query_t and entry_t are the transposed structure of the same forward structure and P; they may be
 * NULL where neither a grad_src nor grad_weights is wanted.  Any nfields >= 0.  The outputs must not overlap the
 * inputs, one another or scratch.  Q == 0 or P == 0 or E == 0: the outputs are zero-filled.
 *
 * scratch: hidegs_neighbor_reduce_backward_scratch_bytes(P, E) bytes, E as above.
 */
size_t hidegs_neighbor_reduce_backward_scratch_bytes(long long P, long long E);

int hidegs_neighbor_reduce_backward_table(void* scratch, size_t scratch_bytes,
                                          const hidegs_neighbor_grad_field* fields /*[host]*/, int nfields, long long P,
                                          const float* weights, const int32_t* table, const float* entry_weights,
                                          long long Q, int k, const float* wsum, const int32_t* starts_t,
                                          const int32_t* query_t, const int32_t* entry_t, float* grad_weights,
                                          float* grad_entry_weights, void* stream);

int hidegs_neighbor_reduce_backward_lists(void* scratch, size_t scratch_bytes,
                                          const hidegs_neighbor_grad_field* fields /*[host]*/, int nfields, long long P,
                                          const float* weights, const int32_t* starts, const int32_t* rows,
                                          const float* entry_weights, long long capacity, long long Q, const float* wsum,
                                          const int32_t* starts_t, const int32_t* query_t, const int32_t* entry_t,
                                          float* grad_weights, float* grad_entry_weights, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HIDEGS_NEIGHBOR_GRAD_H_INCLUDED */
