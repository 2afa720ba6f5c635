/*
 * gb_chain_extd2.h -- base-level alignment between and beyond the anchors of a chain (minimap2's
 * ksw_extd2_sse, tools/minimap2/ksw2_extd2_sse.c).
 *
 * gb_chain_extd2 is a batch form of ksw_extd2_sse with m = 5 and the matrix of ksw_gen_simple_mat(5, mat, a, b,
 * sc_ambi) (tools/minimap2/align.c:9-22): the dual-affine-gap, banded, z-dropped extension or global alignment
 * with CIGAR traceback that mm_align1 runs between consecutive anchors and past both ends of a chain. Every
 * field of ksw_extz_t and every CIGAR word equals the reference's: the call keeps the reference's row arrays,
 * their initial bytes, its 16-byte block updates and its wrapping 8-bit arithmetic ("chain
 * (extd2)"), so cells outside the band hold what the reference's hold and no parameter domain is assumed.
 */
#ifndef GB_CHAIN_EXTD2_H
#define GB_CHAIN_EXTD2_H

#include <stdint.h>

#include "gb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GB_EXTD2_MAX_LEN 32768 /* qlen and tlen of an item, at most */

/* the reference's KSW_EZ_* values that the call accepts, in any combination */
#define GB_EXTD2_RIGHT 0x02       /* right-align gaps */
#define GB_EXTD2_APPROX_MAX 0x08  /* follow one cell instead of the exact row maximum */
#define GB_EXTD2_APPROX_DROP 0x10 /* z-drop on that cell (only with APPROX_MAX) */
#define GB_EXTD2_EXTZ_ONLY 0x40   /* extension: the walk starts at the best end, not at the corner */
#define GB_EXTD2_REV_CIGAR 0x80   /* leave the CIGAR in walk order (last operation first) */
#define GB_EXTD2_FLAGS 0xda

/* match a, mismatch -b, a base against N -sc_ambi (0: the reference then scores it -e2), gap pairs (q, e) and
 * (q2, e2): a gap of length l costs min(q + l * e, q2 + l * e2). */
typedef struct gb_chain_extd2_params { int8_t a, b, sc_ambi, q, e, q2, e2, pad; } gb_chain_extd2_params;
/* query = seqs[q_off .. q_off + qlen), target = seqs[t_off .. t_off + tlen), bases as codes 0..4 (4 is N). w < 0
 * is no band, zdrop < 0 no z-drop. */
typedef struct gb_chain_extd2_item {
  int64_t q_off, t_off;
  int32_t qlen, tlen, w, zdrop, end_bonus, flag;
} gb_chain_extd2_item;
/* ksw_extz_t without m_cigar and the pointer */
typedef struct gb_chain_extd2_result {
  int32_t max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, reach_end, n_cigar, pad;
} gb_chain_extd2_result;

/*
 * Item i owns cigar[cigar_off[i] .. cigar_off[i + 1]): the reference's ez->cigar[0 .. n_cigar) words
 * (len << 4 | op, op 0 = M, 1 = I, 2 = D). *cigar_used is cigar_off[n_items]. res[i].pad is zero.
 *
 * cigar_cap must be at least the sum over the items of qlen + tlen; below that the call returns GB_ERR_ARG
 * before any device work with *cigar_used set to that sum and nothing else written.
 *
 * qlen == 0 or tlen == 0 gives the reset record (ksw_reset_extz) and no CIGAR, and so does every item of a
 * call whose parameters take the reference's `-min_sc > 2 * (q + e)` return. n_items == 0 succeeds without a
 * device (cigar_off[0] and *cigar_used are set to 0).
 *
 * GB_ERR_ARG before any device work, with the item named in gb_last_error() and every output untouched: a
 * flag bit outside GB_EXTD2_FLAGS (SCORE_ONLY, GENERIC_SC, the splice flags); a negative length or one above
 * GB_EXTD2_MAX_LEN; a sequence outside seqs; a base code above 4; an item whose workspace share alone passes
 * the budget.
 *
 * Environment: GB_CHAIN_EXTD2_WS=<bytes> is the budget of device workspace of one chunk of items (default
 * 4 GiB); a call's items are cut, in order, into as many chunks as it takes. An item's share is the
 * reference's (qlen + tlen - 1) * n_col_ * 16 bytes of backtrack codes, 4 bytes per CIGAR word of its bound
 * qlen + tlen, and, for an item whose row state does not fit the LDS (more than 64 KiB), that state. The band
 * bounds of a row (the reference's off[] pairs) are recomputed by the walk and take no workspace.
 * GB_CHAIN_EXTD2_HOST=1 runs the same arithmetic on the host, on GB_CHAIN_THREADS threads, and touches no
 * device.
 */
int gb_chain_extd2(const gb_chain_extd2_params *p, const uint8_t *seqs, int64_t seq_bytes,
                   const gb_chain_extd2_item *items, int64_t n_items, gb_chain_extd2_result *res, uint32_t *cigar,
                   int64_t cigar_cap, int64_t *cigar_off /* n_items + 1 */, int64_t *cigar_used);
/* Of the calling thread's last device call: the fill kernels' time and the walk and pack kernels' summed over
 * the chunks, and the number of in-band cells the sweeps visited before they stopped (en0 - st0 + 1 summed
 * over the rows reached). GB_ERR_STATE before the first. */
int gb_chain_extd2_timing(float *fill_ms, float *walk_ms, int64_t *cells);
/* Of the same call: the number of chunks and the largest chunk's workspace. */
int gb_chain_extd2_plan(int64_t *chunks, int64_t *workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GB_CHAIN_EXTD2_H */
