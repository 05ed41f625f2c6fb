/*
 * hidegs_rows.h -- stream compaction and indexed row moves, the third primitive family of the library
 * next to the scan and the sort of hidegs.h, whose conventions hold here: device pointers unless marked
 * [host], stream-ordered on `stream`, 0 or a negative HIDEGS_E_* code with hidegs_last_error(), no host
 * synchronisation, no state kept between calls (the caller provides every buffer).
 *
 * No reference counterpart (the reference trains on one GPU): the compacted branch of the view-DP
 * exchange (hidegs_amd/view_dp.py) runs on them -- the rows visible to some rank are selected, packed
 * field-major for the collectives and written back after them.  Kernels: hidegs_amd/csrc/rows.hip.
 */
#ifndef HIDEGS_ROWS_H_INCLUDED
#define HIDEGS_ROWS_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Stream compaction of a byte mask.  indices[0 .. *count) = the ascending positions i < n with
 * flags[i] != 0 (any non-zero byte counts); *count = how many.  Entries of indices at and after *count
 * are not written; indices holds n entries.  scratch holds at least hidegs_select_scratch_bytes(n)
 * bytes.  n < 2^31.  Two passes over the flags (per-tile counts, then ranks and writes); no workgroup
 * waits on another.  flags must not change between the call and the completion of its kernels.
 */
size_t hidegs_select_scratch_bytes(long long n);
int hidegs_select_flagged(void* scratch, size_t scratch_bytes, const unsigned char* flags, long long n,
                          uint32_t* indices, uint32_t* count, void* stream);

/* One field of a row move: `rows` is the indexed side, `packed` the dense one. */
typedef struct hidegs_row_field {
    float* rows;      /* (n_rows, width) row-major */
    float* packed;    /* (k, width) row-major */
    long long n_rows;
    int width;        /* >= 1, any value */
} hidegs_row_field;

/*
 * gather:  packed[j] = rows[indices[j]] for j < k, for every field (a bit copy).
 * scatter: rows[indices[j]] = packed[j]; rows not named keep their bits.  Scatter needs ascending,
 *          unique indices (two packed rows with one index would race).
 * An index >= n_rows is skipped and never dereferenced (gather leaves that packed row unwritten).
 * `fields` is a [host] array of `nfields` descriptors; any count is accepted, one launch per 8 fields.
 * k < 2^31.  A field's two sides must not overlap.
 */
int hidegs_gather_rows(const hidegs_row_field* fields, int nfields, const uint32_t* indices, long long k, void* stream);
int hidegs_scatter_rows(const hidegs_row_field* fields, int nfields, const uint32_t* indices, long long k, void* stream);

#ifdef __cplusplus
}
#endif

/* Resizing tensors by rows (prune and append, hidegs_resize_rows): declared in hidegs_resize.h, next to this file. */
#include "hidegs_resize.h"
/* The same with appended rows cloned from the tensor itself (hidegs_resize_rows_cloned): hidegs_clone.h. */
#include "hidegs_clone.h"

#endif /* HIDEGS_ROWS_H_INCLUDED */
