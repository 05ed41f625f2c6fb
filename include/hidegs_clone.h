/*
 * hidegs_clone.h -- resizing per-Gaussian tensors by rows where the appended rows are rows of the tensor
 * itself: the clone and the split of densification in one call.  hidegs_resize.h with a third source for
 * the appended rows.  Part of the row family of hidegs_rows.h, which includes this file and whose
 * conventions hold: device pointers unless marked [host], stream-ordered on `stream`, 0 or a negative
 * HIDEGS_E_* code with hidegs_last_error(), no host synchronisation, no state kept between calls.  Defined
 * by torch semantics (t[mask], t[index], torch.cat); no reference counterpart.
 * Kernel: hidegs_amd/csrc/rows.hip.
 */
#ifndef HIDEGS_CLONE_H_INCLUDED
#define HIDEGS_CLONE_H_INCLUDED

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One field of a resize: dst = [the kept rows of src | the appended rows], which are given, zero or cloned. */
typedef struct hidegs_clone_field {
    const float* src;     /* (n_rows, width) row-major: the old rows */
    const float* append;  /* (n_append, width), or NULL: the appended rows are zero-filled, or cloned */
    float* dst;           /* (k + n_append, width) */
    long long n_rows;
    int width;            /* >= 1, any value */
    int cloned;           /* != 0: appended row i is src[from[i]]; append must be NULL */
} hidegs_clone_field;

/*
 * For every field: dst[j] = src[keep[j]] for j < k, as hidegs_resize_rows (keep == NULL is the identity and
 * requires k <= n_rows).  Then, for i < n_append, by the field's mode:
 *   cloned != 0      dst[k + i] = src[from[i]]
 *   append != NULL   dst[k + i] = append[i]
 *   neither          dst[k + i] = +0.0f bits
 * A bit copy: NaN payloads and -0.0f survive.  `from` holds n_append entries in any order, repeats allowed
 * (a split tiles its list); it may be NULL only if no field is cloned or n_append == 0.  A keep or from entry
 * >= n_rows is never dereferenced and its dst row is written as zeros, so every dst row is always defined.
 * src, append, keep and from are not modified; dst overlaps none of them.
 * `fields` is a [host] array of `nfields` descriptors; any count is accepted, one launch per 8 fields.
 * k + n_append < 2^31.  k + n_append == 0 or nfields == 0 returns 0 without a launch.
 */
int hidegs_resize_rows_cloned(const hidegs_clone_field* fields, int nfields, const uint32_t* keep, long long k,
                              const uint32_t* from, long long n_append, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIDEGS_CLONE_H_INCLUDED */
