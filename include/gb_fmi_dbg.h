/*
 * gb_fmi_dbg.h -- de Bruijn graph assembly of regions (Platypus' assembleReadsAndDetectVariants, benchmarks/dbg/
 * debruijn.cpp, with the k loop the reference keeps as a comment). DESIGN.md, "dbg", has the contract.
 *
 * A region is a reference string and a range of reads of one shared pool. Its graph at k: the reference is walked
 * over i = 0 .. len - k - 2 and adds the edge (k-mer at i) -> (k-mer at i + 1), both nodes colour 1 (REF), position
 * ref_start + i / + i + 1, weight 1, edge weight 1; then every read of the range with flag & 512 clear, in pool
 * order, over i = 0 .. len - k - 2: q is the smallest quality of the k + 1 bases i .. i + k, and where q >= min_qual
 * and none of those bases is 'N' the edge is added with both nodes colour 2 (READ), position -1, weight q and edge
 * weight q. An edge visits its start node and then its end node: the first visit of a k-mer makes the node (colour,
 * position, weight and text offset of that visit), a later one ORs the colour and adds the weight. Nodes are listed
 * in order of first visit. K-mers are compared as k bytes: lower case, IUPAC letters and '=' are ordinary symbols.
 * A node keeps the first 4 distinct out-edges in order of first appearance and the weights added to those; a fifth
 * successor's edge is dropped with its weights while its end node is still visited.
 *
 * The graph is cyclic when, leaving out every edge whose end node has colour 2 alone and whose weight is below
 * min_weight, a directed cycle remains (detectCyclesInGraph_Recursive). The k loop: k = k0; while the graph at k is
 * cyclic and k <= k_max, k += k_step and the graph is built again. Every result is an integer and deterministic:
 * two runs give identical bytes, on the device and on the host.
 */
#ifndef GB_FMI_DBG_H
#define GB_FMI_DBG_H

#include <stdint.h>

#include "gb.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest k a call may reach: k0 when k0 > k_max, otherwise the first k0 + m * k_step above k_max */
#define GB_DBG_MAX_K 64
/* edges (walk positions) of one region at k0 plus its texts, at most: a visit index (two an edge) and a table of
 * twice that many slots stay inside 32 bits */
#define GB_DBG_MAX_EDGES 536870911ll

typedef struct gb_dbg gb_dbg;

typedef struct {
  int32_t k0, k_step, k_max, min_qual, min_weight;
} gb_dbg_params; /* a null pointer means {15, 5, 50, 20, 40} */

typedef struct {
  int32_t k;              /* of the final graph */
  int32_t n_graphs;       /* graphs built */
  int32_t cyclic;         /* of the final graph */
  int32_t n_nodes, n_edges;
  int32_t n_ref_and_read; /* nodes of colour 3 */
  int32_t redone;         /* 1: a graph of this region was built again on the host (the device marked it) */
  int32_t reserved;
  int64_t node_weight_sum, edge_weight_sum;
} gb_dbg_region_summary;

/*
 * Region r: reference bytes ref_bytes[ref_off[r] .. ref_off[r + 1]), ref_start[r], reads [read_first[r],
 * read_last[r]) of the pool. Read j: seq / qual [read_off[j] .. read_off[j + 1]) and flag[j]. keep = 1 keeps the
 * final graph of every region for gb_dbg_export; keep = 0 keeps the summaries only.
 *
 * GB_ERR_ARG before any device work, with *out untouched and the item named in gb_last_error(): offsets that
 * decrease or leave their array; a read range outside the pool or reversed; k0 < 1, k_step < 1 or a largest k above
 * GB_DBG_MAX_K; a region with more than GB_DBG_MAX_EDGES edges and texts (its visits cannot be indexed in 32 bits);
 * a NUL byte in a reference or in a read of some region's range (the reference's strlen and strncmp stop there); a
 * region whose workspace alone is above the budget. n_regions == 0 succeeds and touches no device.
 *
 * Environment: GB_DBG_HOST=1 computes the same results on the host on GB_DBG_THREADS threads and touches no
 * device. GB_DBG_WS=<bytes> bounds the device workspace of a call (default 8 GiB): the batch runs in chunks of
 * consecutive regions that fit. GB_DBG_FP_BITS=<1..64> (tests only) keeps that many bits of the k-mer fingerprint.
 */
int gb_dbg_assemble(const uint8_t *ref_bytes, int64_t n_ref_bytes, const int64_t *ref_off /* n_regions + 1 */,
                    const int32_t *ref_start, const int64_t *read_first, const int64_t *read_last, int64_t n_regions,
                    const uint8_t *seq, const uint8_t *qual, int64_t n_read_bytes,
                    const int64_t *read_off /* n_reads + 1 */, const uint32_t *flag, int64_t n_reads,
                    const gb_dbg_params *params, int keep, gb_dbg **out);
void gb_dbg_free(gb_dbg *h);

/* n_regions entries; cap (in regions) below that is GB_ERR_ARG with nothing written. */
int gb_dbg_summary(const gb_dbg *h, gb_dbg_region_summary *out, int64_t cap);

/*
 * The final graph of one region, a node per entry in order of first visit: src (-1 the reference, otherwise the
 * read's index in the pool) and off (offset in that text) of the first visit, colours, position (of a reference
 * node ref_start + off, summed in 64 bits and cut to int32), weight, n_edges,
 * edge_to[4 * i ..] (node ids, -1 padded) and edge_weight[4 * i ..] (0 padded). *n_nodes is always set; node_cap
 * below it, or a handle made with keep = 0, is GB_ERR_ARG with no array written. Any array may be null.
 */
int gb_dbg_export(const gb_dbg *h, int64_t region, int64_t node_cap, int32_t *src, int32_t *off, int32_t *colours,
                  int32_t *position, int64_t *weight, int32_t *n_edges, int32_t *edge_to, int64_t *edge_weight,
                  int64_t *n_nodes);

/* Of the calling thread's last gb_dbg_assemble, summed over its rounds and chunks: host preparation and upload
 * (pack), the kernels (build: tables; rank: identity check and node ids; edges; cycle), the host's redo of marked
 * regions, in ms (kernel times are 0 on the host path); walk positions (edges) of every graph built and those of
 * them that passed the quality and 'N' test. GB_ERR_STATE before the first call. */
int gb_dbg_timing(float *pack_ms, float *build_ms, float *rank_ms, float *edges_ms, float *cycle_ms, float *redo_ms,
                  int64_t *positions, int64_t *valid_positions);
/* Of the same call: table slots of its largest region, device workspace bytes of its largest chunk, chunks, and
 * rounds (launch sets) in all. Zeros on the host path. */
int gb_dbg_plan(int64_t *max_table_slots, int64_t *workspace_bytes, int64_t *chunks, int64_t *rounds);

#ifdef __cplusplus
}
#endif
#endif /* GB_FMI_DBG_H */
