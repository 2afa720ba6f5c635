/*
 * gb_bsw.h -- C ABI of the MI355X banded Smith-Waterman extension (drop-in boundary for benchmarks/bsw).
 *
 * Reference interface this replaces (paths relative to the reference repo):
 *   BandedPairWiseSW::BandedPairWiseSW(o_del, e_del, o_ins, e_ins, zdrop, end_bonus, mat, w_match,
 *        w_mismatch, numThreads)                               benchmarks/bsw/bandedSWA.h:120-124
 *   void BandedPairWiseSW::getScores16(SeqPair *pairArray, uint8_t *seqBufRef, uint8_t *seqBufQer,
 *        int32_t numPairs, uint16_t numThreads, int32_t w)     bandedSWA.h:195-200, bandedSWA.cpp:3521
 *        semantics == scalarBandedSWA                          bandedSWA.cpp:130-251
 *   SeqPair                                                    bandedSWA.h:92-101
 *   bwa_fill_scmat                                             benchmarks/bsw/main_banded.cpp:77-88
 * Pair p's target (the reference's "ref", len1) is seqBufRef[idr .. idr+len1) and its query
 * (len2) is seqBufQer[idq .. idq+len2), codes 0..4 (main_banded.cpp:186-195). Results go into the
 * SeqPair fields score, tle, gtle, qle, gscore, max_off exactly as getScores16 writes them.
 * Limits: len2 <= GB_BSW_MAX_QLEN, len1 < 2^31. 0 on success, negative gb_status on failure.
 */
#ifndef GB_BSW_H
#define GB_BSW_H

#include <stdint.h>

#include "gb.h"
#include "gb_bsw_ref.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GB_BSW_MAX_QLEN 255 /* >= MAX_SEQ_LEN_QER - 1 (main_banded.cpp:61) */

/* Same layout as SeqPair (bandedSWA.h:92-101); 72 bytes. */
typedef struct gb_seqpair {
  int64_t idr, idq, id;
  int32_t len1, len2;
  int32_t h0;
  int32_t seqid, regid;
  int32_t score, tle, gtle, qle;
  int32_t gscore, max_off;
} gb_seqpair;

/* Constructor arguments of BandedPairWiseSW (bandedSWA.h:120-124) plus getScores16's w. */
typedef struct gb_bsw_params {
  int32_t o_del, e_del, o_ins, e_ins;
  int32_t zdrop, end_bonus;
  int32_t w;
  int8_t mat[25]; /* 5x5, row = target base, column = query base (bandedSWA.cpp:150-154, :180) */
} gb_bsw_params;

/* bwa_fill_scmat (main_banded.cpp:77-88) and the benchmark defaults (main_banded.cpp:53-57,846):
 * match 1, mismatch 4, ambig -1, gap open 6, extend 1, zdrop 100, end_bonus 5, w 100. */
void gb_bsw_fill_scmat(int a, int b, int ambig, int8_t mat[25]);
void gb_bsw_default_params(gb_bsw_params *p);

typedef struct gb_bsw_batch gb_bsw_batch;

/* Upload numPairs pairs and the two sequence buffers (ref_bytes / qer_bytes long) to the device. */
int gb_bsw_batch_create(const gb_bsw_params *params, const gb_seqpair *pairs, int64_t num_pairs,
                        const uint8_t *seq_buf_ref, int64_t ref_bytes, const uint8_t *seq_buf_qer,
                        int64_t qer_bytes, gb_bsw_batch **out);
/* Extend every pair (asynchronous on the batch's stream). */
int gb_bsw_batch_run(gb_bsw_batch *b);
int gb_bsw_batch_sync(gb_bsw_batch *b);
/* Write score/tle/gtle/qle/gscore/max_off into pairs[0..num_pairs) (other fields untouched; may be
 * NULL); out6 (may be NULL) receives {score, qle, tle, gtle, gscore, max_off} per pair; cells
 * (may be NULL) the DP cells each pair evaluated (the reference's inner-loop iterations,
 * bandedSWA.cpp:189); total_cells (may be NULL) their sum. */
int gb_bsw_batch_results(gb_bsw_batch *b, gb_seqpair *pairs, int32_t *out6, int32_t *cells,
                         int64_t *total_cells);
int gb_bsw_batch_timing(gb_bsw_batch *b, float *kernel_ms);
int gb_bsw_batch_destroy(gb_bsw_batch *b);

/* One-shot getScores16: results written into pairs in place. Reuses one cached device batch per
 * (calling thread, device), so calling it once per batch of pairs (main_banded.cpp:896-909) does
 * not create streams or buffers per call. */
int gb_bsw_get_scores16(const gb_bsw_params *params, gb_seqpair *pairs, int64_t num_pairs,
                        const uint8_t *seq_buf_ref, int64_t ref_bytes, const uint8_t *seq_buf_qer,
                        int64_t qer_bytes);
/* The same, also returning the DP cells evaluated (SW_cells accounting of BandedPairWiseSW). */
int gb_bsw_get_scores16_ex(const gb_bsw_params *params, gb_seqpair *pairs, int64_t num_pairs,
                           const uint8_t *seq_buf_ref, int64_t ref_bytes, const uint8_t *seq_buf_qer,
                           int64_t qer_bytes, int64_t *total_cells);
/* getScores8 (bandedSWA.cpp:426-725): the 8-bit kernel's domain is the one its bwa-mem2 caller
 * routes to it (bwamem.cpp:2152-2155): len1 < 128, len2 < 128, h0 + min(len1, len2) * w_match < 128.
 * Pairs in it get the exact (16-bit) results; any pair outside it fails the call with GB_ERR_ARG and
 * nothing is written. */
int gb_bsw_get_scores8(const gb_bsw_params *params, int32_t w_match, gb_seqpair *pairs, int64_t num_pairs,
                       const uint8_t *seq_buf_ref, int64_t ref_bytes, const uint8_t *seq_buf_qer,
                       int64_t qer_bytes, int64_t *total_cells);

/* ---- banded global alignment with CIGAR traceback: bwa's ksw_global2 (tools/bwa/ksw.c:504-606),
 * the step bwa_gen_cigar2 (tools/bwa/bwa.c:121-208) runs on a region getScores16 chose. Per pair:
 * score, CIGAR (len << 4 | op, M = 0, I = 1, D = 2, as ksw_global2 returns it) and NM, each bit for
 * bit what the reference computes. NM is bwa_gen_cigar2's count (bwa.c:169-200): mismatching
 * positions inside M runs plus the lengths of the I runs and of the D runs that are neither the
 * first nor the last operation (bwa.c:187 leaves those out).
 *
 * Accepted domain, per pair: 1 <= len2 <= GB_BSW_MAX_QLEN, 1 <= len1 <= GB_BSW_GLOBAL_MAX_TLEN,
 * w >= |len1 - len2| (bwa_gen_cigar2 always passes at least |len1 - len2| + 3), offsets inside the
 * sequence buffers; o_del, e_del, o_ins, e_ins in [0, 32768). Anything else fails the whole call
 * with GB_ERR_ARG before any device work, nothing is written, and gb_last_error() names the pair.
 * params->zdrop, end_bonus and w are ignored: the band is per pair. */
#define GB_BSW_GLOBAL_MAX_TLEN 2047 /* the reference driver's target buffer (main_banded.cpp:59-62) */

typedef struct gb_bsw_gpair { /* 48 bytes */
  int64_t idr, idq;           /* target / query offsets, as in gb_seqpair */
  int32_t len1, len2;         /* target, query length */
  int32_t w;                  /* band half-width for this pair */
  int32_t score, n_cigar, nm; /* out */
  int64_t cigar_off;          /* out: index of this pair's first op in cigar[] */
} gb_bsw_gpair;

/* Operations are packed in pair order: pair p owns cigar[cigar_off .. cigar_off + n_cigar), and
 * *cigar_used (may be NULL) receives their total. The sum of len1 + len2 over the pairs is always
 * enough for cigar_cap. With cigar_cap smaller than the total the call returns GB_ERR_ARG, sets
 * *cigar_used to the count required, fills the per-pair fields and leaves cigar[] untouched.
 * cigar == NULL asks for scores only (no direction matrix, no walk): n_cigar = 0, nm = -1,
 * cigar_off = 0, *cigar_used = 0. num_pairs == 0 succeeds. Device buffers are cached per (calling
 * thread, device), as for gb_bsw_get_scores16. GB_ERR_STATE reports a traceback that did not end
 * within len1 + len2 steps (an internal error; it cannot happen on a correct direction matrix). */
int gb_bsw_global(const gb_bsw_params *params, gb_bsw_gpair *pairs, int64_t num_pairs,
                  const uint8_t *seq_buf_ref, int64_t ref_bytes, const uint8_t *seq_buf_qer,
                  int64_t qer_bytes, uint32_t *cigar, int64_t cigar_cap, int64_t *cigar_used);

/* bwa_gen_cigar2's band rule (bwa.c:151-160) for a query of len2 against a target of len1; w_cap
 * is its w_ argument. Needs e_del > 0 and e_ins > 0; GB_ERR_ARG (negative) otherwise. */
int gb_bsw_global_band(const gb_bsw_params *params, int32_t len2, int32_t len1, int32_t w_cap);

/* Device time of the calling thread's last gb_bsw_global on the current device, summed over its
 * chunks: the DP fill kernel and the traceback kernel (0 for a scores-only call). */
int gb_bsw_global_timing(float *fill_ms, float *walk_ms);

/* ---- CIGAR, NM and MD from reference coordinates: all of bwa_gen_cigar2 (tools/bwa/bwa.c:121-208)
 * over a device-resident packed reference (gb_bsw_ref.h). Per pair the result is what
 *   bwa_gen_cigar2(params->mat, o_del, e_del, o_ins, e_ins, w, l_pac, pac, len2, query, rb, re,
 *                  &score, &n_cigar, &NM)
 * yields, bit for bit: the region [rb, re) is fetched from the pac (bns_get_seq); for a reverse-strand
 * region (rb >= l_pac) query and target are both reversed before the alignment, so that indels land
 * leftmost on the forward strand (bwa.c:135-140), and the MD letters come from "TGCAN", which turns the
 * complemented target bytes back into the forward strand's letters (bwa.c:172);
 * len2 == re - rb with w == 0 takes the reference's shortcut, one len2 M operation scored as the plain
 * sum of mat with no DP (bwa.c:141-149; a DP can score higher); every other pair gets the band of
 * gb_bsw_global_band and ksw_global2. NM is as in gb_bsw_global. MD follows bwa.c:169-198. The
 * caller's query bytes are never written.
 *
 * The reference's own rejections are per-pair results: rb >= re, a region bridging l_pac, and a region
 * bns_get_seq's clamps shorten (rb < 0 or re > 2 l_pac) give n_cigar = 0, nm = -1, md_len = 0 and
 * leave score as the caller set it (the reference does not write *score there).
 *
 * Refused for the whole call with GB_ERR_ARG before any device work, nothing written, the pair named
 * in gb_last_error(): len2 outside [1, GB_BSW_MAX_QLEN]; w < 0; a query outside seq_buf_qer;
 * re - rb > GB_BSW_GLOBAL_MAX_TLEN on a pair that is not rejected as above; gap penalties outside
 * [0, 32768); e_del == 0 or e_ins == 0 (the band rule divides by them); md without cigar.
 * params->zdrop, end_bonus and w are ignored. */
typedef struct gb_bsw_cpair { /* 64 bytes */
  int64_t rb, re;        /* region in the doubled coordinate space [0, 2 l_pac) */
  int64_t idq;           /* query offset in seq_buf_qer */
  int32_t len2, w;       /* query length; bwa_gen_cigar2's w_ argument */
  int32_t score, n_cigar, nm, md_len; /* out */
  int64_t cigar_off, md_off;          /* out */
} gb_bsw_cpair;

/* Pair p owns cigar[cigar_off .. cigar_off + n_cigar) and md[md_off .. md_off + md_len), both packed in
 * pair order; md_len excludes the reference's terminating NUL and none is stored. *cigar_used and
 * *md_used (may be NULL) receive the totals. The sum of (re - rb) + len2 over the pairs always suffices
 * for cigar_cap and the sum of GB_BSW_MD_CAP(re - rb) for md_cap (every target base adds at most three
 * characters, "0^A" for a one-base deletion between two insertions, and one final count follows). With
 * either capacity below its total the call returns GB_ERR_ARG, sets both totals, fills the per-pair
 * fields and leaves cigar[] and md[] untouched. cigar == NULL asks for scores only (mem_patch_reg's
 * call, tools/bwa/bwamem.c:428): n_cigar = 0, nm = -1, md_len = 0, offsets 0; md must then be NULL.
 * With cigar given and md == NULL, CIGAR and NM are produced without MD (md_len = 0, md_off = 0).
 * num_pairs == 0 succeeds without a device. */
#define GB_BSW_MD_CAP(len1) (3 * (int64_t)(len1) + 1)
int gb_bsw_gen_cigar(const gb_bsw_params *params, const gb_ref *ref, gb_bsw_cpair *pairs, int64_t num_pairs,
                     const uint8_t *seq_buf_qer, int64_t qer_bytes, uint32_t *cigar, int64_t cigar_cap,
                     int64_t *cigar_used, char *md, int64_t md_cap, int64_t *md_used);

/* mem_reg2aln's re-banding loop (tools/bwa/bwamem.c:1154-1163) around gb_bsw_gen_cigar: each pair
 * starts from its own w capped at params->w << 2; it is final when its score equals that of its previous
 * try, when w == params->w << 2, after three tries, or when score >= truesc[p] - params->mat[0];
 * otherwise w doubles (capped again) and the pair is redone. A pair the reference rejects is final after
 * one try. pairs[p].w receives the w of the pair's last try and tries[p] (may be NULL) their number. Each
 * round is one gb_bsw_gen_cigar over the pairs still open. Needs 0 <= params->w < 2^28 in addition.
 * infer_bw, the squeezing of leading and trailing deletions and the clipping (bwamem.c:1149-1153,
 * 1166-1192) stay with the caller. */
int gb_bsw_gen_cigar_retry(const gb_bsw_params *params, const gb_ref *ref, gb_bsw_cpair *pairs, int64_t num_pairs,
                           const uint8_t *seq_buf_qer, int64_t qer_bytes, const int32_t *truesc, uint32_t *cigar,
                           int64_t cigar_cap, int64_t *cigar_used, char *md, int64_t md_cap, int64_t *md_used,
                           int32_t *tries);

/* Device time of the calling thread's last gb_bsw_gen_cigar (or the rounds of a _retry) on the current
 * device: the fetch kernel, the DP fill and traceback kernels summed over the chunks, the MD kernel. */
int gb_bsw_gen_cigar_timing(float *fetch_ms, float *fill_ms, float *walk_ms, float *md_ms);

/* ---- unbanded local alignment with sub-optimal score and start: bwa's ksw_align2 (tools/bwa/ksw.c:
 * 63-365), the call mem_matesw makes for mate rescue (tools/bwa/bwamem_pair.c:150-151). Per pair the
 * seven fields of kswr_t, each bit for bit what ksw_align2(len2, query, len1, target, 5, mat, o_del,
 * e_del, o_ins, e_ins, xtra, 0) returns: score, te, qe (best local score and the target / query
 * positions where it ends), score2, te2 (the best row maximum >= xtra & 0xffff that ends more than
 * ceil(score / max(mat)) rows away from te; -1, -1 without GB_KSW_XSUBO or when there is none) and tb,
 * qb (where the best alignment starts; -1, -1 without GB_KSW_XSTART or when score lies below the
 * GB_KSW_XSUBO threshold). The reference pads the query with columns that score 0 up to a multiple of
 * 16 (GB_KSW_XBYTE) or 8; those columns take part in the row maxima behind score2 / te2, and they do
 * here. One more property of the reference is reproduced: with o_ins == 0 its lazy-F loop ends after
 * the first step, so an insertion no longer crosses more than one boundary between the p stripes of
 * L/p query columns, and scores can lie below the ordinary DP's ("bsw (local)").
 *
 * Accepted domain, per pair: 1 <= len2 <= GB_BSW_MAX_QLEN, 1 <= len1 <= GB_BSW_LOCAL_MAX_TLEN, offsets
 * inside the sequence buffers, no bit of xtra above bit 15 other than the four GB_KSW_X* flags;
 * max(mat) >= 1 and min(mat) <= 0; o_del, e_del, o_ins, e_ins >= 0 with o_del + e_del < 32768 and
 * o_ins + e_ins < 32768. With GB_KSW_XBYTE additionally o_del + e_del <= 255, o_ins + e_ins <= 255
 * (the reference truncates them to a byte) and len2 * max(mat) - min(mat) < 255, so that the
 * reference's byte kernel cannot saturate (bwa's own rule, len2 * a < 250, lies inside this). Anything
 * else fails the whole call with GB_ERR_ARG before any device work, nothing is written, and
 * gb_last_error() names the pair. params->zdrop, end_bonus and w are ignored. */
#define GB_KSW_XBYTE 0x10000  /* tools/bwa/ksw.h:6-9 */
#define GB_KSW_XSTOP 0x20000  /* stop once score >= xtra & 0xffff */
#define GB_KSW_XSUBO 0x40000  /* track score2 / te2 among row maxima >= xtra & 0xffff */
#define GB_KSW_XSTART 0x80000 /* find tb / qb */
#define GB_BSW_LOCAL_MAX_TLEN 16383 /* bwa caps the insert size that bounds a mate-rescue window at 10 000 */

typedef struct gb_bsw_lpair { /* 56 bytes */
  int64_t idr, idq;           /* target / query offsets, as in gb_seqpair */
  int32_t len1, len2, xtra;   /* target, query length; GB_KSW_X* flags | threshold */
  int32_t score, te, qe, score2, te2, tb, qb; /* out */
} gb_bsw_lpair;

/* num_pairs == 0 succeeds without a device. Device and pinned buffers are cached per (calling
 * thread, device); a large call runs in chunks of pairs. */
int gb_bsw_local(const gb_bsw_params *params, gb_bsw_lpair *pairs, int64_t num_pairs,
                 const uint8_t *seq_buf_ref, int64_t ref_bytes, const uint8_t *seq_buf_qer,
                 int64_t qer_bytes);

/* mem_matesw's xtra (bwamem_pair.c:150) for a mate of len2 bases with a = params->mat[0]:
 * XSUBO | XSTART | (len2 * a < 250 ? XBYTE : 0) | (min_seed_len * a). GB_ERR_ARG (negative) when
 * min_seed_len * a does not fit the 16 threshold bits. */
int gb_bsw_local_xtra(const gb_bsw_params *params, int32_t len2, int32_t min_seed_len);

/* Device time of the calling thread's last gb_bsw_local on the current device, summed over its chunks. */
int gb_bsw_local_timing(float *kernel_ms);

/* ---- seed extension from chains: all of bwa's mem_chain2aln (tools/bwa/bwamem.c:632-824) over a
 * device-resident packed reference. In go the seeds an SA lookup produces, grouped into chains and the
 * chains into reads (gb_bsw_seeds2chains, below, does that); out come the alignment regions
 * mem_chain2aln would push, bit for bit, in its order:
 * the chains of a read in the order given into one region list (mem_align1_core passes the same regs for
 * every chain of a read), the seeds of a chain by decreasing score << 32 | index. rb, re, qb, qe, truesc
 * and w are what gb_bsw_gen_cigar_retry consumes. rid and frac_rep come from the chain
 * (gb_bsw_alnreg_from_regions joins them); what follows mem_chain2aln, mem_sort_dedup_patch up to the MAPQ,
 * is gb_bsw_finish_regs, below.
 *
 * params gives mat, the gap penalties, zdrop and w = opt->w; params->end_bonus is ignored: left
 * extensions pass pen_clip5 as ksw_extend2's end_bonus, right extensions pen_clip3. contig_end (may be
 * NULL: one contig) holds the n_contigs cumulative end offsets of the contigs on the forward strand, the
 * last equal to l_pac: all of .ann that bns_fetch_seq (bntseq.c:427-446) needs to clip a chain's window
 * to the contig, or its reverse-strand mirror, that holds seeds[0].rbeg.
 *
 * Three CSR levels: read r has the query seq_buf_qer[idq[r] .. idq[r] + l_query[r]) (codes 0..4) and the
 * chains read_chain_off[r] .. read_chain_off[r + 1); chain c the seeds chain_seed_off[c] ..
 * chain_seed_off[c + 1). read_chain_off[0] == 0 and chain_seed_off[0] == 0; the number of chains is
 * read_chain_off[n_reads], the number of seeds chain_seed_off[that].
 *
 * Every seed is extended (a seed's extension depends on the seed, the read and its chain's window
 * only); the containment test against the read's earlier regions (bwamem.c:671-703) is applied
 * afterwards over the finished results, so the regions are the reference's.
 *
 * Refused for the whole call with GB_ERR_ARG before any device work, nothing written, the read, chain or
 * seed named in gb_last_error(): l_query < 1; an extension's query part (qbeg, or l_query - qbeg - len)
 * above GB_BSW_MAX_QLEN; len < 1, score < 1, qbeg < 0, qbeg + len > l_query; rbeg < 0 or
 * rbeg + len > 2 l_pac; a seed bridging l_pac; seeds of one chain on both strands; a seed that does not
 * lie inside its chain's window after the clip to the contig of seeds[0] (bwa never builds such a chain);
 * a window of 2^31 bases or more; gap penalties outside [0, 32768); e_del == 0 or e_ins == 0; w outside
 * [0, 2^28); an empty chain (the reference returns on c->n == 0; refused so that indices stay aligned);
 * offsets that decrease; a query outside seq_buf_qer; contig_end not increasing or not ending at l_pac;
 * 2^31 seeds or more. n_reads == 0 succeeds without a device. */
typedef struct gb_bsw_seed { /* mem_seed_t (bwamem.h), 24 bytes */
  int64_t rbeg;
  int32_t qbeg, len, score;
  int32_t pad;
} gb_bsw_seed;

typedef struct gb_bsw_region { /* 56 bytes */
  int64_t rb, re;
  int32_t qb, qe, score, truesc, w, seedcov, seedlen0;
  int32_t chain, seed; /* the chain's and the seed's index in the call */
  int32_t pad;
} gb_bsw_region;

/* What every extension returned, kept or not. Side 0 is the left extension, side 1 the right one.
 * out6[side] = {score, qle, tle, gtle, gscore, max_off} of that side's last try; tries[side] is 0 when the
 * side had nothing to extend (out6 is then all zero), else 1 or 2; skipped = 1 when the containment test
 * dropped the seed. */
typedef struct gb_bsw_c2a_raw { /* 64 bytes */
  int32_t out6[2][6];
  int32_t tries[2];
  int32_t skipped, pad;
} gb_bsw_c2a_raw;

/* Read r owns regs[reg_off[r] .. reg_off[r] + n_reg[r]), packed in read order; *reg_used (may be NULL)
 * receives the total. The number of seeds always suffices for reg_cap. With reg_cap below the total the
 * call returns GB_ERR_ARG, sets *reg_used to the count required, fills reg_off and n_reg and leaves
 * regs[] untouched. raw (may be NULL) has one record per seed. The reads are cut into chunks when the
 * gathered bytes (twice the windows plus twice the queries) pass 256 MiB (GB_BSW_C2A_BYTES overrides).
 * Buffers are cached per (calling thread, device). */
int gb_bsw_chain2aln(const gb_bsw_params *params, int32_t pen_clip5, int32_t pen_clip3, const gb_ref *ref,
                     const int64_t *contig_end, int64_t n_contigs, const uint8_t *seq_buf_qer, int64_t qer_bytes,
                     int64_t n_reads, const int64_t *idq, const int32_t *l_query, const int64_t *read_chain_off,
                     const int64_t *chain_seed_off, const gb_bsw_seed *seeds, gb_bsw_region *regs, int64_t reg_cap,
                     int64_t *reg_off, int32_t *n_reg, int64_t *reg_used, gb_bsw_c2a_raw *raw);

/* Device time of the calling thread's last gb_bsw_chain2aln on the current device, summed over its
 * chunks: the gather kernel; the extension launches of the four rounds, ext_ms[0] left at w, [1] left at
 * 2 w, [2] right at w, [3] right at 2 w (0 for a round that had no seed and launched nothing); the finish
 * kernel; the filter, scan and emit kernels. */
int gb_bsw_chain2aln_timing(float *gather_ms, float ext_ms[4], float *finish_ms, float *filter_ms);

/* ---- chains from seeds: bwa's mem_chain after mem_collect_intv (tools/bwa/bwamem.c:265-310, with
 * test_and_merge :190-211, bns_intv2rid / bns_pos2rid bntseq.c:355-379 and kbtree.h at t = 5) and
 * mem_chain_flt (:327-385, with mem_chain_weight :213-232 and ks_introsort ksort.h:176-226), bit for bit
 * and in the reference's order. In go the SMEMs of gb_fmi_results and the coordinates of
 * gb_fmi_sa_entries, unchanged; out come the CSR arguments of gb_bsw_chain2aln.
 *
 * mems are grouped by read in read order, in any order within a read; the call puts each read's SMEMs
 * into mem_chain's order (m << 32 | n + 1 ascending; equal keys are the same substring and interval) and
 * each SMEM's coordinates move with it. coords holds the coordinates concatenated in SMEM order, n_coord
 * of them per SMEM: what mem_chain's loop takes for that s and max_occ (step = s > max_occ ? s / max_occ
 * : 1; rows k, k + step, ... below s, at most max_occ). contig_end / n_contigs as in gb_bsw_chain2aln
 * (NULL: one contig), contig_is_alt (may be NULL: none) one byte per contig.
 *
 * stage 0 returns mem_chain's output: per read the chains in the B-tree's in-order traversal, each
 * chain's seeds in insertion order (score == len), info with pos, rid, is_alt, l_rep, frac_rep and w =
 * kept = 0. stage 1 additionally applies mem_chain_flt: the chains in the order the filter leaves them
 * (by weight as ks_introsort leaves ties, kept == 0 removed), info.w the weight and info.kept 1, 2 or 3.
 * mem_flt_chained_seeds (:598-615) is not applied: the call refuses a read with SMEMs and l_query >=
 * min_seed_len for which it would not be the identity, i.e. unless min_l > MEM_SEEDSW_COEF * l_query in
 * the reference's types (min_l = 1.1f * min_chain_weight, or 5.5f * log(l_query) when that is 0).
 *
 * read_chain_off has n_reads + 1 entries, chain_seed_off chains + 1. n_coords always suffices for
 * chain_cap and seed_cap. With a smaller cap that does not suffice the call returns GB_ERR_ARG, sets
 * *chains_used and *seeds_used (may be NULL) to the counts needed, fills read_chain_off (and
 * chain_seed_off when chain_cap suffices) and leaves seeds[] and info[] untouched.
 *
 * Refused for the whole call with GB_ERR_ARG before any device work, nothing written, the read or SMEM
 * named in gb_last_error(): read decreasing or outside [0, n_reads); m < 0, n < m, n >= l_query, s < 1;
 * n_coord not the number above; the sum of n_coord != n_coords; a coordinate outside [0, 2 l_pac);
 * max_occ < 1, w < 0, max_chain_gap < 0, max_chain_extend < 1; mask_level or drop_ratio not finite;
 * contig_end not increasing or not ending at l_pac; stage not 0 or 1; 2^31 coordinates or more; the
 * mem_flt_chained_seeds case above. n_reads == 0 succeeds without a device.
 *
 * The chains are built on the device, one read per lane. GB_BSW_MKCHAIN_HOST=1 sends every read through
 * the library's host path instead (no device is touched; GB_BSW_MKCHAIN_THREADS host threads, a number
 * from 1 up, default up to 16; anything else is refused), and a read with more than
 * GB_BSW_MKCHAIN_DEV_COORDS coordinates takes it in any case: a read has at most as many chains as
 * coordinates, so every read of up to that many chains stays on the device. Equal-pos ties are no reason
 * for the host path. An environment variable of the same name overrides the bound (a count from 0 up;
 * the tests reach a call served by both paths with it). No exception leaves the call: running out of
 * host memory returns GB_ERR_NOMEM. */
#define GB_BSW_MKCHAIN_DEV_COORDS 65536

typedef struct gb_bsw_chain_opt { /* the mem_opt_t fields mem_chain / mem_chain_flt read */
  int32_t w, max_chain_gap, max_occ, min_seed_len, min_chain_weight, max_chain_extend;
  float mask_level, drop_ratio;
} gb_bsw_chain_opt;
/* 100, 10000, 500, 19, 0, 1 << 30, 0.50f, 0.50f (bwamem.c:50-86) */
void gb_bsw_chain_default_opt(gb_bsw_chain_opt *o);

typedef struct gb_bsw_mem { /* one SMEM of one read, 24 bytes */
  int32_t read, m, n; /* gb_smem's rid, m, n: the seed is query [m, n] inclusive */
  int32_t n_coord;    /* coordinates it owns (counts[i] of gb_fmi_sa_entries) */
  int64_t s;          /* interval size */
} gb_bsw_mem;

typedef struct gb_bsw_chain_info { /* one per output chain, 32 bytes */
  int64_t pos;
  int32_t rid, is_alt, w, kept; /* w, kept: 0 at stage 0 */
  int32_t l_rep;
  float frac_rep; /* (float)l_rep / l_query */
} gb_bsw_chain_info;

int gb_bsw_seeds2chains(const gb_bsw_chain_opt *opt, int32_t stage, int64_t l_pac, const int64_t *contig_end,
                        const uint8_t *contig_is_alt, int64_t n_contigs, int64_t n_reads, const int32_t *l_query,
                        const gb_bsw_mem *mems, int64_t n_mems, const int64_t *coords, int64_t n_coords,
                        int64_t *read_chain_off, int64_t *chain_seed_off, gb_bsw_seed *seeds, gb_bsw_chain_info *info,
                        int64_t chain_cap, int64_t seed_cap, int64_t *chains_used, int64_t *seeds_used);

/* Of the calling thread's last gb_bsw_seeds2chains: the device time of the build kernel, the filter kernel
 * and the emit group (count, scans, scatter), 0 for a call that ran on the host alone, and the number of
 * reads that took the host path. emit_ms is the span between two events around the group, so it includes
 * the one read-back inside it (the chain count, which sizes the second scan) and the host's wait for it. */
int gb_bsw_seeds2chains_timing(float *build_ms, float *filter_ms, float *emit_ms, int64_t *host_reads);

/* ---- from regions to primaries: what bwa does with a read's regions between mem_chain2aln and
 * mem_reg2aln's re-banding loop (tools/bwa/bwamem.c), bit for bit and in the reference's order, for a batch
 * of single-end reads.
 *
 * stage 0 is the tail of mem_align1_core (:1114-1126): mem_sort_dedup_patch (:437-489) with mem_patch_reg
 * (:406-435) and its score-only global alignments (bwa_gen_cigar2 without a CIGAR, bwa.c:121-167), then is_alt
 * becomes 1 for a region on an ALT contig (the reference leaves it as given otherwise). A read with fewer
 * than two regions is returned as it came (n_comp included), as the reference's early return leaves it.
 * stage 1 adds the single-end worker's steps (:1235-1236): mem_mark_primary_se (:521-558, hash =
 * hash_64(id0 + read index + i), utils.h:98), mem_reorder_primary5 (:1019-1041) when opt->primary5 is set,
 * and mapq = secondary < 0 ? mem_approx_mapq_se (:993-1017) : 0, the value mem_reg2aln assigns (:1147).
 * At stage 0 mapq is 0 and secondary, secondary_all, alt_sc and hash are left as given.
 *
 * sub, csub and sub_n are inputs as well as outputs: a merge takes the larger sub and csub, csub feeds the
 * MAPQ, and the reference never resets sub_n, so stage 1 adds to what is there (twice for a hit counted by
 * both passes of mem_mark_primary_se_core). Regions from gb_bsw_chain2aln carry 0 in all three.
 *
 * mem_reg2sam's selection loop (T, drop_ratio, the supplementary MAPQ cap), XA, infer_bw, the SAM text and, of
 * the paired-end side, mem_pair and the paired MAPQ stay with the caller (mate rescue: gb_bsw_mate_rescue). The
 * stage-1 primaries go into gb_bsw_gen_cigar_retry as they are (rb, re, qb, qe, w, truesc).
 *
 * params gives mat; the gap penalties of mem_patch_reg's alignment are opt's, as in the reference.
 * Read r has the query seq_buf_qer[idq[r] .. idq[r] + l_query[r]) and the regions regs[reg_off[r] ..
 * reg_off[r + 1]). The result is written in place: the survivors of read r are regs[reg_off[r] ..
 * reg_off[r] + n_out[r]) in the reference's final order and the read's remaining slots are zeroed.
 * contig_is_alt (may be NULL: none) has one byte per contig; n_contigs bounds rid in either case.
 *
 * Refused for the whole call with GB_ERR_ARG before any work, nothing written, the read or region
 * named in gb_last_error(): stage not 0 or 1; offsets that decrease or do not start at 0; l_query outside
 * [1, GB_BSW_MAX_QLEN] or a query outside seq_buf_qer on a read that has regions; a region without
 * 0 <= qb < qe <= l_query or 0 <= rb < re <= 2 l_pac, or one bridging l_pac; rid outside [0, n_contigs);
 * score < 1; seedcov < 1; sub, csub or sub_n < 0; w outside [0, 2^28) (a region's or opt's);
 * max_chain_gap < 0; a < 1 or a + b < 1 (the MAPQ divides by both) or either at 32768 or above; |min_seed_len|
 * at 32768 or above; n_contigs < 1; mask_level, mask_level_redun or mapQ_coef_len not finite; gap penalties
 * outside [0, 32768) or an extension penalty of 0; 2^31 regions or more. One refusal is found during the
 * work: a mem_patch_reg alignment whose target b.re - a.rb exceeds GB_BSW_GLOBAL_MAX_TLEN fails the call
 * with GB_ERR_ARG naming the read; regs is untouched then too, because the library works on a copy and
 * writes the caller's arrays only at the end. n_reads == 0 succeeds. No exception leaves the call
 * (GB_ERR_NOMEM).
 *
 * The call runs on the host (GB_BSW_REGS_THREADS threads, a number from 1 up, default up to 16; anything
 * else is refused) and touches no device: the per-read routines are written for one read per lane, with
 * the alignment handed out as a request and the read resumed with its score, but the kernels around them
 * are not part of the library yet ("bsw (regions to primaries)"). The alignments are a plain
 * banded DP over the reference's host copy. That copy is released at the first device use of ref
 * (gb_bsw_gen_cigar, gb_bsw_chain2aln, gb_ref_fetch): a call with a read of two regions or more then
 * returns GB_ERR_ARG and says so, so a caller that runs those stages keeps a second gb_ref for this one. */
typedef struct gb_bsw_alnreg { /* mem_alnreg_t's fields (bwamem.h:60-78) plus mapq, 96 bytes */
  int64_t rb, re;
  int32_t qb, qe, rid, score, truesc, sub, alt_sc, csub, sub_n, w, seedcov;
  int32_t secondary, secondary_all, seedlen0, n_comp, is_alt;
  float frac_rep;
  int32_t mapq; /* out */
  uint64_t hash;
} gb_bsw_alnreg;

typedef struct gb_bsw_reg_opt { /* the mem_opt_t fields these functions read */
  int32_t a, b, o_del, e_del, o_ins, e_ins, w, max_chain_gap, min_seed_len;
  float mask_level, mask_level_redun, mapQ_coef_len;
  int32_t mapQ_coef_fac; /* an int in the reference: log(50) truncated */
  int32_t T, primary5;   /* primary5: MEM_F_PRIMARY5 */
} gb_bsw_reg_opt;
/* 1, 4, 6, 1, 6, 1, 100, 10000, 19, 0.50f, 0.95f, 50.f, 3, 30, 0 (bwamem.c:50-86) */
void gb_bsw_reg_default_opt(gb_bsw_reg_opt *o);

int gb_bsw_finish_regs(const gb_bsw_params *params, const gb_bsw_reg_opt *opt, int32_t stage, const gb_ref *ref,
                       const uint8_t *contig_is_alt, int64_t n_contigs, const uint8_t *seq_buf_qer, int64_t qer_bytes,
                       int64_t n_reads, const int64_t *idq, const int32_t *l_query, int64_t id0, const int64_t *reg_off,
                       gb_bsw_alnreg *regs, int32_t *n_out);

/* The join between gb_bsw_chain2aln / gb_bsw_seeds2chains and gb_bsw_finish_regs: out[k] takes rb, re, qb,
 * qe, score, truesc, w, seedcov and seedlen0 from regions[k], rid and frac_rep from
 * chain_info[regions[k].chain], and 0 everywhere else. GB_ERR_ARG for a chain index outside [0, n_chains). */
int gb_bsw_alnreg_from_regions(const gb_bsw_region *regions, int64_t n, const gb_bsw_chain_info *chain_info,
                               int64_t n_chains, gb_bsw_alnreg *out);

/* Of the calling thread's last gb_bsw_finish_regs: three device times, 0 while the call runs on the host
 * (kept so that the signature need not change when kernels arrive: dedup, alignments, mark); the largest
 * number of alignments one read needed (the rounds a one-read-per-lane device path would take), the number
 * of alignments, and the reads served on the host (all of them). */
int gb_bsw_finish_regs_timing(float *dedup_ms, float *dp_ms, float *mark_ms, int32_t *dp_rounds, int64_t *dp_requests,
                              int64_t *host_reads);

/* ---- mate rescue: the paired-end steps around ksw_align2 (tools/bwa/bwamem_pair.c), bit for bit and in
 * the reference's order. Reads 2p and 2p + 1 are pair p.
 *
 * gb_bsw_pestat is mem_pestat (:46-109, with mem_infer_dir :23-30 and cal_sub :32-44) over the stage-0 regions
 * of gb_bsw_finish_regs: per orientation (FF, FR, RF, RR) the bounds of a proper pair's distance, the mean and
 * the deviation, or failed. It runs on the host, touches no device and prints nothing. avg and std carry
 * the reference's bits (double arithmetic in its order, (int)(x + .499) truncating toward zero).
 *
 * gb_bsw_mate_rescue is the rescue loop of mem_sam_pe (:265-276) around mem_matesw (:111-180). Per pair the
 * anchors of read i are its regions with score >= its best score - pen_unpaired, at most max_matesw of them,
 * taken before any rescue; anchor j of read i looks for read !i in the windows the four orientations give,
 * unless the orientation failed or read !i already has a region at a proper distance from the anchor. The
 * window arithmetic, bns_fetch_seq's clip to the contig (or its reverse-strand mirror) holding the window's
 * middle, the fetch from the pac, the mate's reverse complement, ksw_align2 and the region it gives run on
 * the device, one round per anchor index j over all pairs, and the windows never leave it. The test above,
 * the sorted insertion and mem_sort_dedup_patch without mem_patch_reg (the reference passes a null bns) run
 * on the host between the rounds (GB_BSW_MATESW_THREADS threads, a number from 1 up, default up to 16).
 * A window that is empty after the clamps to [0, 2 l_pac] does nothing (the reference reads an
 * uninitialised rid there and then fails its length test).
 *
 * params gives mat; the gap penalties are opt's, as in gb_bsw_finish_regs, and xtra is gb_bsw_local_xtra's
 * value with a = opt->a. Read r has the query seq_buf_qer[idq[r] .. idq[r] + l_query[r]) and the regions
 * regs[reg_off[r] .. reg_off[r + 1]), which are never written. Read r's final list is out_regs[out_off[r] ..
 * out_off[r] + n_out[r]), packed in read order; a rescued region has rid and is_alt of its anchor, secondary
 * -1 and 0 in every field the reference leaves 0. n_sw[p] (may be NULL) is the sum of mem_matesw's return
 * values for pair p: the alignments performed. The sum over the reads of n + 4 * min(anchors of the mate,
 * max_matesw) always suffices for out_cap. With out_cap below the total the call returns GB_ERR_ARG, sets
 * *out_used (may be NULL) to the count required, fills out_off and n_out and leaves out_regs untouched.
 * n_pairs == 0 succeeds without a device. contig_end / n_contigs as in gb_bsw_chain2aln (NULL: one contig);
 * n_contigs bounds rid in either case.
 *
 * Refused for the whole call with GB_ERR_ARG before any device work, nothing written, the read or the
 * orientation named in gb_last_error(): what gb_bsw_finish_regs refuses about offsets, regions and rid;
 * min_seed_len < 1, max_matesw < 0, pen_unpaired < 0, a < 1, min_seed_len * a above 65535; for an orientation
 * that has not failed low < 0, high < low or high - low + the longest mate > GB_BSW_LOCAL_MAX_TLEN; a read
 * whose mate has regions and that lies outside gb_bsw_local's domain for its xtra (l_query outside [1,
 * GB_BSW_MAX_QLEN], a query outside seq_buf_qer, the GB_KSW_XBYTE rules, the penalties, the matrix);
 * contig_end not increasing or not ending at l_pac. No exception leaves the call (GB_ERR_NOMEM).
 *
 * The requests of a round are cut into chunks whose windows stay under 256 MiB; GB_BSW_MATESW_CHUNK
 * (requests per chunk, from 1 up) overrides that. */
struct gb_bsw_pestat { /* mem_pestat_t (bwamem.h), 32 bytes; a tag only: the function has the name */
  int32_t low, high, failed, pad;
  double avg, std;
};

typedef struct gb_bsw_pe_opt { /* the mem_opt_t fields mem_pestat and mem_matesw read */
  int32_t a, b, o_del, e_del, o_ins, e_ins, min_seed_len, max_chain_gap, pen_unpaired, max_matesw, max_ins;
  float mask_level, mask_level_redun;
} gb_bsw_pe_opt;
/* 1, 4, 6, 1, 6, 1, 19, 10000, 17, 50, 10000, 0.50f, 0.95f (bwamem.c:50-86) */
void gb_bsw_pe_default_opt(gb_bsw_pe_opt *o);

/* n_reads is even; reg_off has n_reads + 1 entries. Refused with GB_ERR_ARG, pes untouched: n_reads odd or
 * negative, offsets that decrease or do not start at 0, null arguments, mask_level not finite. */
int gb_bsw_pestat(const gb_bsw_pe_opt *opt, int64_t l_pac, int64_t n_reads, const int64_t *reg_off,
                  const gb_bsw_alnreg *regs, struct gb_bsw_pestat pes[4]);

int gb_bsw_mate_rescue(const gb_bsw_params *params, const gb_bsw_pe_opt *opt, const struct gb_bsw_pestat pes[4],
                       const gb_ref *ref, const int64_t *contig_end, int64_t n_contigs, const uint8_t *seq_buf_qer,
                       int64_t qer_bytes, int64_t n_pairs, const int64_t *idq, const int32_t *l_query,
                       const int64_t *reg_off, const gb_bsw_alnreg *regs, gb_bsw_alnreg *out_regs, int64_t out_cap,
                       int64_t *out_off, int32_t *n_out, int32_t *n_sw, int64_t *out_used);

/* Of the calling thread's last gb_bsw_mate_rescue: the device time of the window and fetch kernels (with the
 * reverse complements), of the local DP and of the region kernel, summed over rounds and chunks; the host
 * time of the bookkeeping between the rounds; the rounds that had a request, and the requests. */
int gb_bsw_mate_rescue_timing(float *fetch_ms, float *dp_ms, float *region_ms, float *host_ms, int32_t *rounds,
                              int64_t *requests);

#ifdef __cplusplus
}
#endif
#endif /* GB_BSW_H */
