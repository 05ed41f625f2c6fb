/*
 * hidegs_topk.h -- top-k row selection, a primitive next to the scan and the sort of hidegs.h and the
 * compaction of hidegs_rows.h, whose conventions hold here: device pointers unless marked [host],
 * stream-ordered on `stream`, 0 or a negative HIDEGS_E_* code with hidegs_last_error(), no host
 * synchronisation, no state kept between calls (the caller provides every buffer).
 *
 * No reference counterpart: the reference carries a point budget (max_all_points) and no code that holds
 * it.  Given fp32 scores, an optional candidate mask and a host-known k, the call writes a byte mask of
 * exactly the min(k, candidates) best rows -- the mask that resize_rows(keep= / clone=) and
 * hidegs_select_flagged take.  A radix select, not a sort.  Kernels: hidegs_amd/csrc/topk.hip.
 */
#ifndef HIDEGS_TOPK_H_INCLUDED
#define HIDEGS_TOPK_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Candidates: row i < n is a candidate iff among == NULL or among[i] != 0 (any non-zero byte counts);
 * c = how many.
 *
 * Order key of a score with bits b, a u32: a NaN of any sign or payload has key 0; -0.0 is taken as +0.0;
 * otherwise key = (b >> 31) ? ~b : b | 0x80000000.  Keys ascend with the scores, -inf has 0x007FFFFF, so a
 * NaN ranks strictly below every number.
 *
 * Selected: the first min(k, c) candidates in descending key, then ascending row index.  That is, with a
 * threshold key T and a tie quota r: every candidate with key > T, and of the candidates with key == T the r
 * lowest row indices.  flags_out[i] = 1 for a selected row and 0 for every other i < n, non-candidates
 * included; every byte is written.  k == 0 selects nothing, k >= c every candidate.  The result is a function
 * of (scores, among, n, k) alone.
 *
 * info, if not NULL, receives four words: info[0] = min(k, c), info[1] = c, info[2] = the bits of the
 * threshold score (the score of key T in canonical form: +0.0 for a zero, 0x7FC00000 for a NaN; 0 when nothing
 * is selected), info[3] = r (0 when nothing is selected).
 *
 * 0 <= n < 2^31, 0 <= k < 2^31; n == 0 returns 0 without a launch.  scratch holds at least
 * hidegs_top_k_scratch_bytes(n) bytes and may hold anything: what must start at zero is cleared by the call
 * on `stream`.  flags_out may be `among` itself (capping a selection in place); it must not overlap `among` in
 * part, nor `scores`, nor `scratch`.  scores and among must not change between the call and the completion of
 * its kernels.  No allocation and no host read: the call can be captured into a graph.  Launch boundaries are
 * its only synchronisation; no workgroup waits on another.
 */
size_t hidegs_top_k_scratch_bytes(long long n);
int hidegs_top_k_mask_f32(void* scratch, size_t scratch_bytes, const float* scores, const unsigned char* among,
                          long long n, long long k, unsigned char* flags_out, uint32_t* info, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HIDEGS_TOPK_H_INCLUDED */
