/*
 * gb_bsw_abea.h -- adaptive banded event alignment (GenomicsBench abea: f5c / nanopolish align()).
 *
 * gb_abea_align is a batch form of align() (benchmarks/abea/src/align.c:169-548): every read's events are
 * aligned to the k-mers of its base-called sequence in a band of GB_ABEA_BANDWIDTH cells that follows the
 * best scores (Suzuki-Kasahara), and the alignment is walked back from the best (event, last k-mer) cell.
 * Every read follows the CPU align() bit for bit, with one exception: where no such cell lies inside its
 * band with a score above -infinity the reference has undefined behaviour, and the library reports
 * no_end_cell = 1, n_raw = n_pairs = 0 and walks nothing.
 *
 * The file is named with the banded-alignment leg's prefix (as is csrc/bsw_abea.hip): the benchmark's map
 * of sources to legs knows phmm, fmi, chain and bsw, and every source file belongs to one of them.
 */
#ifndef GB_BSW_ABEA_H
#define GB_BSW_ABEA_H

#include <stdint.h>

#include "gb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GB_ABEA_K 6           /* KMER_SIZE (f5c.h:24) */
#define GB_ABEA_BANDWIDTH 100 /* ALN_BANDWIDTH (f5c.h:28) */
#define GB_ABEA_MODEL_SIZE 4096 /* 4^GB_ABEA_K model entries, indexed by k-mer rank */
/* Limits per read. A read's trace is 32 bytes per band and its pair region 8, with n_events + n_kmers + 2
 * bands: at both limits that is 96 MiB + 24 MiB, so the default workspace (GB_ABEA_WS_BYTES, 1 GiB, one half
 * for traces and one for pair regions) still holds five such reads in flight and a chunk of twenty. */
#define GB_ABEA_MAX_SEQ_LEN (1 << 20)
#define GB_ABEA_MAX_EVENTS (1 << 21)

typedef struct gb_abea_model { float level_mean, level_stdv, level_log_stdv; } gb_abea_model; /* model_t under CACHED_LOG, 4096 entries */
typedef struct gb_abea_read  { int64_t seq_off; int64_t event_off; int32_t seq_len, n_events; float scale, shift; } gb_abea_read;
typedef struct gb_abea_pair  { int32_t ref_pos, read_pos; } gb_abea_pair;            /* AlignedPair */
typedef struct gb_abea_stat  { int32_t n_pairs;   /* align()'s return value: 0 when the QC fails */
                               int32_t n_raw;     /* pairs before the QC */
                               int32_t max_gap, spanned, end_event, no_end_cell, fills, pad;
                               float end_score; float pad2; double sum_emission; } gb_abea_stat;

/*
 * seqs holds ASCII bases (a base other than ACGT has rank 0, and no warning is printed), event_mean one
 * float per event (align() reads nothing else of an event). Read r uses seqs[seq_off .. seq_off + seq_len)
 * and event_mean[event_off .. event_off + n_events), with its scale and shift.
 *
 * Read r owns pairs[pair_off[r] .. pair_off[r] + stats[r].n_raw), in the reference's final (reversed)
 * order; pair_off has n_reads + 1 entries and pair_off[n_reads] == *pairs_used. The pairs are written even
 * when the QC fails (stats[r].n_pairs == 0): the reference leaves exactly that in its caller's buffer.
 * n_raw <= n_events + n_kmers, so that sum over the reads always suffices for pair_cap. With a pair_cap
 * that does not suffice the call returns GB_ERR_ARG, sets *pairs_used to the need, fills pair_off and
 * stats, and leaves pairs[] untouched.
 *
 * GB_ERR_ARG before any device work, with the read named in gb_last_error(): seq_len < GB_ABEA_K or above
 * GB_ABEA_MAX_SEQ_LEN, n_events < 1 or above GB_ABEA_MAX_EVENTS, offsets outside the buffers, a
 * level_stdv that is not finite or <= 0, a model value, scaling or event mean that is not finite.
 * n_reads == 0 succeeds without a device.
 *
 * Environment: GB_ABEA_WS_BYTES (default 1 GiB) bounds the device workspace: half for the waves' trace
 * slices (the grid shrinks to fit, down to one wave), half for a chunk's pair regions (a call is cut into
 * chunks of reads, down to one read). GB_ABEA_HOST=1 runs the same arithmetic on the host, on
 * GB_ABEA_THREADS threads, and touches no device.
 */
int gb_abea_align(const gb_abea_model *model, const char *seqs, int64_t seq_bytes, const float *event_mean,
                  int64_t n_event_total, const gb_abea_read *reads, int64_t n_reads, gb_abea_pair *pairs,
                  int64_t pair_cap, int64_t *pair_off, gb_abea_stat *stats, int64_t *pairs_used);
/* Of the calling thread's last device call: the kernel's time, split between band fill and walk by the
 * waves' own cycle counts, and the number of cells filled. GB_ERR_STATE before the first device call. */
int gb_abea_align_timing(float *fill_ms, float *trace_ms, int64_t *cells);
/* Of the calling thread's last device call: chunks it was cut into, waves of the (largest) grid, and
 * device workspace bytes (trace slices and pair regions). GB_ERR_STATE before the first device call. */
int gb_abea_align_plan(int64_t *chunks, int64_t *waves, int64_t *ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GB_BSW_ABEA_H */
