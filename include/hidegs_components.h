/*
 * hidegs_components.h -- connected components of a graph over rows: the transitive step after the neighbour
 * queries.  Edges come from neighbour tables and CSR neighbour lists (hidegs_nearest_k.h, hidegs_nearest_within.h,
 * hidegs_nearest_lists.h) or, fused, from the nearest-point index's own walk within a radius.  A primitive family
 * next to hidegs_moments.h, whose conventions hold here: device pointers, stream-ordered on `stream`, 0 or a
 * negative HIDEGS_E_* code with hidegs_last_error(), no allocation, no host read, no host synchronisation (every
 * call can be captured into a graph), every argument error, overlaps included, reported before the first launch.
 * Scratch is the caller's and may hold anything.  There is no floating-point atomic anywhere.
 *
 * No reference counterpart.  What it is for: "this component has fewer than S rows" removes a floater, a small
 * clump of Gaussians that are each other's neighbours and so pass every per-row neighbour count.
 * Kernels: hidegs_amd/csrc/components.hip, hidegs_amd/csrc/nearest_components.h (a stage of nearest.hip), and the
 * device header they share, hidegs_amd/csrc/union_find.h.
 */
#ifndef HIDEGS_COMPONENTS_H_INCLUDED
#define HIDEGS_COMPONENTS_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The state is a forest, parent: N int32 owned by the caller, 0 <= N < 2^31.  Row i is a node iff parent[i] >= 0;
 * the other rows hold -1 and take part in nothing.
 *
 * The rule.  A node's parent is never above it (parent[i] <= i); a root is a node whose parent is not below it.
 * Every write lowers a parent: a link is a compare-and-swap on a root, a compression moves a row to an ancestor.
 * So the root of a tree is its lowest row, and the label of a component is its lowest row whatever the order in
 * which the threads ran: the result is a function of the set of edges alone, the same bits on every call and for
 * every order of the queries, with no sort and no tie rule.
 *
 * Termination.  find stands on one row at a time; each step moves to a parent that is >= 0 and strictly below the
 * row it stands on and stops at the first parent that is negative or not below it: at most N steps on any content
 * of parent, reading only [0, N).  unite(a, b) finds both roots and swaps the higher root's word from the value
 * find read there to the lower root; after a failed swap it continues from the value the swap returned.  A swap
 * fails only because another thread lowered that word, words only go down and never below -1, so a launch makes
 * finitely many writes and finitely many retries.  No thread waits for another: no flag, no queue, no poll.
 * Inside a linking kernel every access to parent is an agent-scope relaxed atomic; a stale read is an earlier
 * parent, still an ancestor, and only the compare-and-swap decides.  Launch boundaries are the only
 * synchronisation between linking and finishing.
 *
 * hidegs_components_begin: parent[i] = i where among == NULL or among[i] != 0, and -1 elsewhere.  among is N
 * bytes; any non-zero byte counts (hidegs_voxel.h).  N == 0 launches nothing and needs no pointer.
 */
int hidegs_components_begin(int32_t* parent, long long N, const unsigned char* among, void* stream);

/*
 * Edges from neighbour lists.  Query j < Q has a list (hidegs_moments.h's two forms):
 *   table form   table is (Q, k) int32, k >= 1: the list of query j is its k slots;
 *   list form    starts is (Q + 1) int32 and rows is (capacity) int32: the list of query j is the positions from
 *                max(starts[j], 0) up to, not including, min(starts[j + 1], capacity) of rows, and is empty where
 *                that range is empty.  No position at or past capacity is read, whatever starts holds.
 * Every valid entry r of query j's list adds the undirected edge {s, r}, s = sources[j], or s = j with
 * sources == NULL, which needs Q <= N.  An entry is valid iff 0 <= s < N, 0 <= r < N and both are nodes; everything
 * else (-1, rows past N, rows that are no nodes) is skipped where it stands.  Self-edges, repeated edges and an
 * edge given in one direction or in both all mean the same; no symmetry of the input is assumed.  Calls
 * accumulate: the forest after several calls is that of the union of their edges.
 * 0 <= Q < 2^31, 0 <= capacity < 2^31; Q == 0 launches nothing and needs no pointer but is still checked.
 * sources, table, starts and rows must not overlap parent.
 */
int hidegs_components_add_table(int32_t* parent, long long N, const int32_t* sources, const int32_t* table, long long Q,
                                int k, void* stream);
int hidegs_components_add_lists(int32_t* parent, long long N, const int32_t* sources, const int32_t* starts,
                                const int32_t* rows, long long capacity, long long Q, void* stream);

/*
 * Edges within a radius, fused with the search.  index is what hidegs_nearest_build wrote over a cloud of P rows,
 * and parent holds P words.  For every row j of the cloud that is a node, every candidate in range of point j adds
 * the edge {j, candidate}.  Candidates, the distance and "in range" are hidegs_nearest_within.h's, word for word,
 * with no row excluded (a self-edge means nothing).  r2 points to one float for all rows (r2_is_per_row == 0) or
 * to P floats, one per row; with one per row the edge exists if either end reaches the other.  A row with a
 * non-finite coordinate is no candidate and makes no edge.  No list is written and nothing is searched twice.
 * The walk needs no scratch: hidegs_nearest_components_within_scratch_bytes is 0 for every P, and scratch may be
 * NULL.  P == 0 launches nothing.  parent must not overlap the index, r2 or scratch.
 */
size_t hidegs_nearest_components_within_scratch_bytes(long long P);
int hidegs_nearest_components_within(const void* index, size_t index_bytes, long long P, void* scratch,
                                     size_t scratch_bytes, const float* r2, int r2_is_per_row, int32_t* parent,
                                     void* stream);

/*
 * Flattens parent in place: afterwards parent[i] is the lowest row of i's component for a node, and -1 for the
 * others.  parent is the label array; more edges may be added afterwards, and it may be finished again.
 *   size_out (N) int32 or NULL   the number of nodes of i's component, 0 for a row that is no node;
 *   ids_out  (N) int32 or NULL   the rank of i's component among the components in ascending order of label,
 *                                0 .. C-1, and -1 for a row that is no node;
 *   info_out 4 int32, required   {C, the number of nodes, the size of the largest component, the lowest label among
 *                                the components of that size}; all four are 0 where there is no node.
 * scratch holds at least hidegs_components_finish_scratch_bytes(N) bytes, 16-byte aligned (0 at N <= 0 and past
 * the range; it does not shrink as N grows).  N == 0 clears info_out and launches nothing else.  The outputs must
 * not overlap parent, one another or scratch.  On a parent of arbitrary content the call terminates, touches only
 * its own buffers and writes labels in [-1, N); what they mean is then unspecified.
 */
size_t hidegs_components_finish_scratch_bytes(long long N);
int hidegs_components_finish(void* scratch, size_t scratch_bytes, int32_t* parent, long long N, int32_t* size_out,
                             int32_t* ids_out, int32_t* info_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HIDEGS_COMPONENTS_H_INCLUDED */
