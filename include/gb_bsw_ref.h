/*
 * gb_bsw_ref.h -- bwa's 2-bit packed reference (.pac) resident on the device.
 *
 * Reference interface this stands for (paths relative to the reference repo):
 *   _get_pac(pac, l) = pac[l >> 2] >> ((~l & 3) << 1) & 3        tools/bwa/bntseq.c:43
 *   bns_get_seq(l_pac, pac, beg, end, &len)                      tools/bwa/bntseq.c:404-425
 *   the .pac file as bns_fasta2bntseq writes it                  tools/bwa/bntseq.c:317-325
 *   and bns_restore_core reads its length back                   tools/bwa/bntseq.c:100-105
 * Coordinates live in bwa's doubled space [0, 2 l_pac): [0, l_pac) is the forward strand and
 * position x >= l_pac the complement of forward base 2 l_pac - 1 - x. The .ann / .amb side
 * (bns_fetch_seq's clipping to contig ends, bns_depos) is not part of this.
 */
#ifndef GB_BSW_REF_H
#define GB_BSW_REF_H

#include <stdint.h>

#include "gb.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gb_ref gb_ref;

/* pac holds (l_pac + 3) / 4 bytes in bwa's layout, l_pac >= 1. The bytes are copied; no device is
 * touched here. The first call that uses the reference on a device uploads it to the device current
 * then and releases the host copy; from then on the reference belongs to that device (GB_ERR_STATE on
 * another). */
int gb_ref_create(const uint8_t *pac, int64_t l_pac, gb_ref **out);
/* A bwa .pac file: the packed bytes, one zero byte if l_pac % 4 == 0, then a byte equal to l_pac % 4.
 * GB_ERR_ARG for a file that cannot be read or is not of this form. */
int gb_ref_load_pac(const char *path, gb_ref **out);
int gb_ref_info(const gb_ref *ref, int64_t *l_pac);
int gb_ref_destroy(gb_ref *ref);

/* bns_get_seq for n regions: beg and end are swapped when end < beg, then clamped to [0, 2 l_pac]; a
 * forward region gives its bases, a reverse-strand region (beg >= l_pac) the complement read
 * backwards, a region bridging l_pac length 0. len[r] (may be NULL) receives region r's length and
 * off[r] (may be NULL) where its bytes start in out[]; the bytes are packed in region order. With
 * out_cap below the total the call returns GB_ERR_ARG before any device work, having written len[]
 * and off[]. A region longer than 2^31 - 1 bases is refused. This is the testable face of the fetch
 * kernel gb_bsw_gen_cigar runs, not a fast path: the bytes come back through the host. */
int gb_ref_fetch(const gb_ref *ref, const int64_t *beg, const int64_t *end, int64_t n, uint8_t *out, int64_t out_cap,
                 int64_t *off, int32_t *len);

#ifdef __cplusplus
}
#endif
#endif /* GB_BSW_REF_H */
