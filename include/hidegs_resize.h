/*
 * hidegs_resize.h -- resizing per-Gaussian tensors by rows: prune by a keep list and append new rows, the
 * row surgery of densification, for many tensors at once.  Part of the row family of hidegs_rows.h, which
 * includes this file and whose conventions hold: device pointers unless marked [host], stream-ordered on
 * `stream`, 0 or a negative HIDEGS_E_* code with hidegs_last_error(), no host synchronisation, no state kept
 * between calls.  Defined by torch semantics (t[mask], torch.cat); no reference counterpart.
 * Kernel: hidegs_amd/csrc/rows.hip.
 */
#ifndef HIDEGS_RESIZE_H_INCLUDED
#define HIDEGS_RESIZE_H_INCLUDED

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One field of a resize: dst = [the kept rows of src | the appended rows]. */
typedef struct hidegs_resize_field {
    const float* src;     /* (n_rows, width) row-major: the old rows */
    const float* append;  /* (n_append, width), or NULL: the appended rows are zero-filled */
    float* dst;           /* (k + n_append, width) */
    long long n_rows;
    int width;            /* >= 1, any value */
} hidegs_resize_field;

/*
 * For every field: dst[j] = src[keep[j]] for j < k, and dst[k + a] = append[a] for a < n_append (+0.0f bits
 * where append is NULL).  A bit copy: NaN payloads and -0.0f survive.
 * keep == NULL is the identity (rows [0, k) are copied; k <= n_rows of every field is required): the pure
 * append, with no index array.  A keep entry >= n_rows is never dereferenced and its dst row is written as
 * zeros, so every dst row is always defined.  src and append are not modified; dst overlaps neither.
 * `fields` is a [host] array of `nfields` descriptors; any count is accepted, one launch per 8 fields.
 * k + n_append < 2^31.  k + n_append == 0 or nfields == 0 returns 0 without a launch.
 */
int hidegs_resize_rows(const hidegs_resize_field* fields, int nfields, const uint32_t* keep, long long k,
                       long long n_append, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIDEGS_RESIZE_H_INCLUDED */
