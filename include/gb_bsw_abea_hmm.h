/*
 * gb_bsw_abea_hmm.h -- methylation profile-HMM scores (GenomicsBench abea: f5c / nanopolish profile_hmm_score).
 *
 * gb_abea_hmm_score is a batch form of profile_hmm_score (benchmarks/abea/src/hmm.c:620-727), the forward
 * algorithm that calculate_methylation_for_read (src/meth.c:501-658) runs twice per group of CpG sites: once
 * over the unmethylated sequence and once over the methylated one (CG turned into MG). Every item's score is
 * the CPU function's return value bit for bit: f32 throughout, every log-sum the table-driven p7_FLogsum
 * (src/logsum.h, ESL_LOG_SUM), the six terms of a cell folded in the reference's order, the K (skip) state
 * reading its own row, the end updates in row order.
 *
 * The file is named with the banded-alignment leg's prefix for the reason gb_bsw_abea.h gives.
 */
#ifndef GB_BSW_ABEA_HMM_H
#define GB_BSW_ABEA_HMM_H

#include <stdint.h>

#include "gb.h"
#include "gb_bsw_abea.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GB_ABEA_HMM_MODEL_SIZE 15625  /* 5^6 entries over ACGMT, indexed by k-mer rank (A=0 C=1 G=2 M=3 T=4) */
#define GB_ABEA_HMM_MAX_KMERS  256    /* the reference's callers stop at span 200: 216 k-mers */
#define GB_ABEA_HMM_MAX_EVENTS 65536  /* rows of one item */
#define GB_ABEA_HMM_LOGSUM_TBL 16000  /* p7_LOGSUM_TBL */
#define GB_ABEA_HMM_PRE_CLIP   1      /* HAF_ALLOW_PRE_CLIP */
#define GB_ABEA_HMM_POST_CLIP  2      /* HAF_ALLOW_POST_CLIP */

/* A read: its events are event_mean[event_off .. event_off + n_events); scale, shift, var and log_var are
 * scalings_t under CACHED_LOG, events_per_base the read's (it sets the ten transition log-probabilities). */
typedef struct gb_abea_hmm_read { int64_t event_off; int32_t n_events; float scale, shift, var, log_var;
                                  int32_t pad; double events_per_base; } gb_abea_hmm_read;
/* One call of profile_hmm_score. The string seqs[seq_off .. seq_off + seq_len) is the one the reference would
 * read: m_seq for rc == 0, m_rc_seq for rc == 1 (k-mer ki is then taken at seq_len - ki - 6). Row r = 1 ..
 * |event_stop - event_start| + 1 uses the read's event event_start + (r - 1) * stride, with stride +1 for
 * rc == 0 and -1 for rc == 1 (the reference asserts that pairing). flags is the hmm_flags bit set. */
typedef struct gb_abea_hmm_item { int64_t seq_off; int32_t seq_len, read, event_start, event_stop;
                                  uint8_t rc, flags, pad[2]; } gb_abea_hmm_item;

/*
 * scores[i] is profile_hmm_score's return value for item i. A byte other than ACGMT has rank 0, and no warning
 * is printed.
 *
 * GB_ERR_ARG before any device work, with the item, read or model entry named in gb_last_error() and scores
 * untouched: seq_len < 6 or more than GB_ABEA_HMM_MAX_KMERS k-mers; more than GB_ABEA_HMM_MAX_EVENTS rows; an
 * event index outside the read; rc == 0 with event_start > event_stop or rc == 1 with event_start <
 * event_stop; rc > 1; flags > 3; a read index or an offset out of range; events_per_base not finite or < 1
 * (the reference takes the logarithm of a negative number there); p_mm_next <= 0; var not finite or <= 0;
 * log_var, scale, shift, an event mean or a model value not finite; level_stdv <= 0. n_items == 0 succeeds
 * without a device.
 *
 * Environment: GB_ABEA_HOST=1 runs the same arithmetic on the host, on GB_ABEA_THREADS threads, and touches no
 * device.
 */
int gb_abea_hmm_score(const gb_abea_model *cpg_model /* 15625 entries */, const char *seqs, int64_t seq_bytes,
                      const float *event_mean, int64_t n_event_total, const gb_abea_hmm_read *reads, int64_t n_reads,
                      const gb_abea_hmm_item *items, int64_t n_items, float *scores);
/* Of the calling thread's last device call: the kernels' time and the number of cells (rows x k-mers summed
 * over the items). GB_ERR_STATE before the first device call. */
int gb_abea_hmm_timing(float *kernel_ms, int64_t *cells);
/* The 16 000 entries of the log-sum table the library built with the host's libm. */
int gb_abea_hmm_logsum_table(float *out /* 16000 */);

#ifdef __cplusplus
}
#endif
#endif /* GB_BSW_ABEA_HMM_H */
