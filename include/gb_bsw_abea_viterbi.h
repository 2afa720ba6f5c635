/*
 * gb_bsw_abea_viterbi.h -- Viterbi event alignment with traceback (GenomicsBench abea: f5c / nanopolish
 * profile_hmm_align).
 *
 * gb_abea_hmm_align is a batch form of profile_hmm_align (benchmarks/abea/src/eventalign.c:703-911), which
 * align_read_to_ref runs once per window of about 100 reference bases of every read that `eventalign` writes
 * out. It is the profile HMM of gb_abea_hmm_score (three states K, B, M per k-mer) with the maximum in place of
 * the log-sum, over the 4096-entry nucleotide model of gb_abea_align, and it returns the path: for every
 * item the records of the reference's std::vector<HMMAlignmentState>, bit for bit.
 *
 * The file is named with the banded-alignment leg's prefix for the reason gb_bsw_abea.h gives.
 */
#ifndef GB_BSW_ABEA_VITERBI_H
#define GB_BSW_ABEA_VITERBI_H

#include <stdint.h>

#include "gb.h"
#include "gb_bsw_abea.h"
#include "gb_bsw_abea_hmm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GB_ABEA_VITERBI_MODEL_SIZE 4096  /* 4^6 entries, indexed by k-mer rank (A=0 C=1 G=2 T=3, any other byte 0) */

/* One HMMAlignmentState: the event's index in its read, the k-mer's index in the order the strand visits them,
 * the Viterbi value of the cell (the reference widens it to double, which is exact) and 'M', 'B' or 'K'. The
 * reference's l_posterior and log_transition_probability are constants (-infinity) and are not returned. */
typedef struct gb_abea_path_rec { int32_t event_idx, kmer_idx; float l_fm; uint8_t state; uint8_t pad[3]; } gb_abea_path_rec;

/*
 * Reads and items are gb_abea_hmm_score's records: an item's string is the one the reference would read
 * (fwd_subseq for rc == 0, rc_subseq for rc == 1), row r = 1 .. |event_stop - event_start| + 1 uses the read's
 * event event_start + (r - 1) * stride. Item i owns path[path_off[i] .. path_off[i + 1]) in the reference's final
 * order (rows ascending): the first record is (event_start, 0, 'M'), the last (event_stop, last k-mer, 'M'), and
 * there are rows + (number of 'K' records) of them. *path_used is path_off[n_items]. pad is zero.
 *
 * path_cap must be at least the sum over the items of rows + k-mers - 1; below that the call returns GB_ERR_ARG
 * before any device work with *path_used set to that sum and nothing else written.
 *
 * GB_ERR_ARG before any device work, with the item, read or model entry named in gb_last_error() and every
 * output untouched: what gb_abea_hmm_score refuses (over a model of 4096 entries), and flags != 0; fewer than 2
 * rows (the reference asserts it); an item of one k-mer and two rows in a read with events_per_base == 1 (no
 * path reaches its last cell: the reference would return a value of -infinity); an item whose backtrack codes
 * and records alone pass the workspace budget. n_items == 0 succeeds without a device (path_off[0] and
 * *path_used are set to 0).
 *
 * Environment: GB_ABEA_VITERBI_WS=<bytes> is the budget of device workspace of one chunk of items (default
 * 1 GiB); a call's items are cut into as many chunks as it takes. An item's share is 2 B per cell of its sweep
 * (rows + (k-mers - 1) / NK steps of k-mers rounded up to NK codes, NK = 1, 1, 2, 4 k-mers per lane up to 16, 64,
 * 128, 256 k-mers) and twice 16 B per record of its bound rows + k-mers - 1. GB_ABEA_HOST=1 runs the same
 * arithmetic on the host, on GB_ABEA_THREADS threads, and touches no device; on the device path those threads
 * copy the records into path.
 */
int gb_abea_hmm_align(const gb_abea_model *model /* 4096 entries */, const char *seqs, int64_t seq_bytes,
                      const float *event_mean, int64_t n_event_total, const gb_abea_hmm_read *reads, int64_t n_reads,
                      const gb_abea_hmm_item *items, int64_t n_items, gb_abea_path_rec *path, int64_t path_cap,
                      int64_t *path_off /* n_items + 1 */, int64_t *path_used);
/* Of the calling thread's last device call: the fill kernels' time and the walk and pack kernels' summed over
 * the chunks, and the number of cells (rows x k-mers summed over the items). GB_ERR_STATE before the first. */
int gb_abea_hmm_align_timing(float *fill_ms, float *walk_ms, int64_t *cells);
/* Of the same call: the number of chunks and the largest chunk's workspace (backtrack codes and records). */
int gb_abea_hmm_align_plan(int64_t *chunks, int64_t *workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GB_BSW_ABEA_VITERBI_H */
