/*
 * gb_fmi_kmer.h -- k-mer counting and the solid k-mer index (Flye's KmerCounter::count and
 * VertexIndex::buildIndexUnevenCoverage, tools/Flye/src/sequence/vertex_index.cpp).
 *
 * Reads are ASCII bytes (A/a C/c G/g T/t) in container order. A k-mer is its 2k-bit big-endian code, its
 * canonical form the smaller of the code and its reverse complement (a palindrome stays forward). Only forward
 * reads are walked, and as the reference's IterKmers does, the walk of a read of L bases covers the offsets
 * 0 .. L - k - 1: the last k-mer of a read is not counted and a read of k bases or fewer has none. The reverse strand
 * exists through canonical forms and through positions. The global position
 * of offset p of forward read i is 2 * (L_0 + .. + L_{i-1}) + p, of its reverse complement the same plus L_i.
 *
 * gb_kmer_count keeps the 2-bit packed reads, the read offsets and the sorted distinct canonical codes with their
 * uint32 counts resident (on the device, or on the host under GB_KMER_HOST=1). gb_kmer_index builds the index of
 * the kept positions from such a handle. Every result is deterministic: two runs give identical bytes.
 */
#ifndef GB_FMI_KMER_H
#define GB_FMI_KMER_H

#include <stdint.h>

#include "gb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GB_KMER_MAX_K 31
/* keys of one sort tile (one workgroup of 256 lanes, 16 keys a lane) */
#define GB_KMER_TILE 4096
/* k-mer occurrences of one call, at most: offsets within a call are 32-bit and a slot table of twice the
 * occurrences is scanned in uint32. No count can pass uint32 below it. */
#define GB_KMER_MAX_OCC 2147483647ll

typedef struct gb_kmer_counts gb_kmer_counts;
typedef struct gb_kmer_idx gb_kmer_idx;

/*
 * Read i is bytes[seq_off[i] .. seq_off[i + 1]). GB_ERR_ARG before any device work, with *out untouched and the
 * item named in gb_last_error(): k outside 1..31; offsets that decrease or leave [0, n_bytes]; a byte that is no
 * base (read and position named); more than GB_KMER_MAX_OCC occurrences (a count could pass uint32); a workspace
 * need above the budget (the bytes needed are stated). n_seqs == 0, or no read longer than k, succeeds with empty
 * results and touches no device.
 *
 * Environment: GB_KMER_WS=<bytes> is the budget of device workspace of one call (default 32 GiB; one pass only).
 * GB_KMER_HOST=1 computes the same results on the host on GB_KMER_THREADS threads and touches no device; a handle
 * made on the host stays on the host.
 */
int gb_kmer_count(int k, const uint8_t *bytes, int64_t n_bytes, const int64_t *seq_off /* n_seqs + 1 */,
                  int64_t n_seqs, gb_kmer_counts **out);
void gb_kmer_free(gb_kmer_counts *h);

/* distinct canonical codes (Flye's "Total k-mers"), occurrences, codes with count >= 16 (Flye's "Hash size" under
 * the flat counter), the largest count. Any pointer may be null. */
int gb_kmer_counts_stats(const gb_kmer_counts *h, int64_t *n_distinct, int64_t *n_occurrences, int64_t *n_over15,
                         int64_t *max_count);
/* The distinct codes in ascending order with their counts. cap (in codes) below n_distinct is GB_ERR_ARG with
 * *used set to n_distinct and nothing else written. */
int gb_kmer_counts_export(gb_kmer_counts *h, uint64_t *codes, uint32_t *counts, int64_t cap, int64_t *used);
/* KmerCounter::getFreq of each code as given: 0 for an absent code and for a non-canonical one. */
int gb_kmer_counts_freq(gb_kmer_counts *h, const uint64_t *codes, int64_t n, uint32_t *freq_out);
/* hist[f] = number of codes with count f, for f < n_bins - 1; the last bin collects everything at or above it. */
int gb_kmer_counts_hist(gb_kmer_counts *h, int64_t *hist, int64_t n_bins);

/*
 * buildIndexUnevenCoverage(min_freq, select_rate, tandem_freq) with repeat_kmer_rate = repeat_rate. Both rate
 * products are f32 multiplies, as the reference's. min_freq >= 1, select_rate in (0, 1) and repeat_rate >= 0, or
 * GB_ERR_ARG. A code is listed when its list is not empty, which is what the reference's kmerFreq and iterKmerPos
 * show of it.
 */
int gb_kmer_index(gb_kmer_counts *h, int32_t min_freq, float select_rate, int32_t tandem_freq, float repeat_rate,
                  gb_kmer_idx **out);
void gb_kmer_idx_free(gb_kmer_idx *x);
int gb_kmer_idx_stats(const gb_kmer_idx *x, int64_t *n_codes, int64_t *n_entries, int64_t *n_rep_codes,
                      int64_t *repetitive_frequency);
/* codes[n_codes] ascending, off[n_codes + 1], pos[n_entries] (global positions, ascending within a code),
 * rep_codes[n_rep_codes] ascending. A capacity below the need is GB_ERR_ARG with nothing written. Any array may be
 * null with its capacity 0 to skip it. */
int gb_kmer_idx_export(const gb_kmer_idx *x, uint64_t *codes, int64_t *off, int64_t code_cap, int64_t *pos,
                       int64_t pos_cap, uint64_t *rep_codes, int64_t rep_cap);

/* Of the calling thread's last gb_kmer_count (pack, extract, sort, reduce) and gb_kmer_index (lookup, select,
 * fill): kernel times in ms, 0 on the host path, and the occurrences of the count. GB_ERR_STATE before the first. */
int gb_kmer_timing(float *pack_ms, float *extract_ms, float *sort_ms, float *reduce_ms, float *lookup_ms,
                   float *select_ms, float *fill_ms, int64_t *occurrences);
/* The sort's tile in keys, the passes of the last count's sort, and the device workspace of the last count or
 * index call on this thread (0 on the host path). */
int gb_kmer_plan(int64_t *tile_keys, int64_t *sort_passes, int64_t *workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GB_FMI_KMER_H */
