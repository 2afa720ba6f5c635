/*
 * gb_bsw_poa.h -- partial order alignment and window consensus (spoa as vendored under tools/racon/vendor/spoa:
 * SisdAlignmentEngine, Graph::add_alignment, Graph::generate_consensus()).
 *
 * gb_poa_align is a batch form of SisdAlignmentEngine::align for the global type (kNW): a sequence against a
 * partial-order graph given in rank order, with the reference's linear, affine or convex gap cost chosen by its
 * own rule from (m, n, g, e, q, c). Every pair of the alignment and the score equal the reference's: the call
 * keeps the reference's int32 matrices H, F, E, O and Q at the reference's values and restates its walk over
 * them ("poa"). gb_poa_consensus builds each window's graph read by read, with the alignments of a
 * round done in one device pass over all windows and the graph update on the host, and returns the
 * heaviest-bundle consensus.
 */
#ifndef GB_POA_H
#define GB_POA_H

#include <stdint.h>

#include "gb.h"

#ifdef __cplusplus
extern "C" {
#endif

/* With both limits every score stays below 2^28 in magnitude ((nodes + length + 2) * 128), so no int32 sum of
 * the fill or of its scans wraps, and none comes near the reference's kNegativeInfinity (INT32_MIN + 1024). */
#define GB_POA_MAX_LEN 65536      /* bases of one sequence, at most */
#define GB_POA_MAX_NODES 1048576  /* nodes of one graph view, at most */

/* spoa's AlignmentType values. Only GB_POA_NW is accepted. */
#define GB_POA_SW 0
#define GB_POA_NW 1
#define GB_POA_OV 2

/* spoa's AlignmentSubtype values, as gb_poa_subtype reports them */
#define GB_POA_LINEAR 0
#define GB_POA_AFFINE 1
#define GB_POA_CONVEX 2

/* the size classes of the fill kernel: a wave per item up to GB_POA_WAVE_MAX_LEN bases, a workgroup of four
 * waves per item above, with a row's values in registers up to GB_POA_GROUP_MAX_LEN bases and read back from
 * the workspace above that */
#define GB_POA_CLASS_WAVE 0
#define GB_POA_CLASS_GROUP 1
#define GB_POA_CLASS_LONG 2
#define GB_POA_WAVE_MAX_LEN 256
#define GB_POA_GROUP_MAX_LEN 1024

/* match m, mismatch n, and a gap of length l costs max(g + (l - 1) e, q + (l - 1) c); all four gap values are
 * <= 0. type is GB_POA_NW. */
typedef struct gb_poa_params { int8_t m, n, g, e, q, c, type, pad; } gb_poa_params;

/*
 * Graph views, concatenated. A view is the graph in rank order (Graph::rank_to_node_id): for rank r of the view
 * that starts at node k0 and edge e0, node_base[k0 + r] is the node's byte, node_id[k0 + r] its node id,
 * node_out[k0 + r] non-zero if it has out-edges, and its in-edges, in the order of Node::in_edges(), are the
 * predecessor ranks pred_rank[e0 + b .. e0 + in_end[k0 + r]) where b is in_end[k0 + r - 1], or 0 for r = 0.
 */
typedef struct gb_poa_graphs {
  const uint8_t *node_base;
  const int32_t *node_id;
  const uint8_t *node_out;
  const int32_t *in_end;
  const int32_t *pred_rank;
  int64_t n_nodes, n_edges;
} gb_poa_graphs;

/* the view [node_off, node_off + n_nodes) with the edges [edge_off, edge_off + n_edges), against
 * seqs[seq_off .. seq_off + seq_len) */
typedef struct gb_poa_item {
  int64_t node_off, edge_off, seq_off;
  int32_t n_nodes, n_edges, seq_len, pad;
} gb_poa_item;

/* The subtype spoa's createAlignmentEngine chooses: linear if g >= e, affine if g <= q || e >= c, convex
 * otherwise. GB_ERR_ARG with spoa's message for a positive gap value. */
int gb_poa_subtype(const gb_poa_params *p, int32_t *subtype);

/* cells * 4 * (1, 3 or 5 by subtype) rounded up to 16, plus 8 bytes per pair of the bound n_nodes + seq_len,
 * where cells = (n_nodes + 1) * (seq_len + 1): an item's share of the device workspace. 0 for an item with no
 * node or no base. */
int64_t gb_poa_item_bytes(int32_t subtype, int32_t n_nodes, int32_t seq_len);

/*
 * Item i owns pairs[2 * pair_off[i] .. 2 * pair_off[i + 1]): (node id or -1, sequence position or -1) in the
 * reference's order. scores[i] is the final H value the walk starts from. *pair_used is pair_off[n_items]. An item
 * with no node or no base owns no pair and has score 0.
 *
 * pair_cap (in pairs) must be at least the sum of n_nodes + seq_len over the items with a node and a base; below
 * that the call returns GB_ERR_ARG before any device work with *pair_used set to that sum and nothing else
 * written. n_items == 0 succeeds without a device.
 *
 * GB_ERR_ARG before any device work, with the item named in gb_last_error() and every output untouched: a type
 * other than GB_POA_NW (kSW and kOV by name); a positive gap value; a negative length or count, or one above
 * the limits; a view, its edges or a sequence outside the arrays; an in_end that decreases, or whose last value
 * is not n_edges; n_nodes == 0 with n_edges != 0; a predecessor rank that is negative or not below its node's
 * own; an item whose workspace share alone passes the budget; budget text that is not a number of bytes > 0.
 *
 * Environment: GB_POA_WS=<bytes> is the budget of device workspace of one chunk of items (default 4 GiB); a
 * call's items are cut, in order, into as many chunks as it takes. GB_POA_HOST=1 runs the same arithmetic on the
 * host, on GB_POA_THREADS threads, and touches no device.
 */
int gb_poa_align(const gb_poa_params *p, const gb_poa_graphs *g, const uint8_t *seqs, int64_t seq_bytes,
                 const gb_poa_item *items, int64_t n_items, int32_t *scores, int32_t *pairs, int64_t pair_cap,
                 int64_t *pair_off /* n_items + 1 */, int64_t *pair_used);

/*
 * Window w holds the sequences win_off[w] .. win_off[w + 1); sequence s is bytes[seq_off[s] .. seq_off[s + 1])
 * and weights, if not null, gives one weight per byte (spoa's quality form is the quality byte minus 33); null
 * is weight 1. Round j aligns sequence j of every window that has one against that window's graph (one
 * gb_poa_align pass over all of them; round 0 needs none) and then adds it to the graph on the host, on
 * GB_POA_THREADS threads. An empty sequence adds nothing. Window w's consensus
 * (Graph::generate_consensus()) is cons[cons_off[w] .. cons_off[w + 1]), node_count[w] its graph's final number
 * of nodes; a window with no non-empty sequence has an empty consensus and no node. *n_alignments counts the
 * alignments done (a sequence with a base against a graph with a node).
 *
 * cons_cap must be at least seq_off[n_seqs] - seq_off[0], the bound of the consensus bytes; below that the call
 * returns GB_ERR_ARG before any device work with *cons_used set to that bound and nothing else written.
 * Refusals as gb_poa_align's, with the window or sequence named. The budget is checked round by round, so a
 * window whose graph outgrows it is refused in that round, still with every output untouched.
 */
int gb_poa_consensus(const gb_poa_params *p, const int64_t *win_off /* n_windows + 1 */, int64_t n_windows,
                     const int64_t *seq_off /* n_seqs + 1 */, int64_t n_seqs, const uint8_t *bytes,
                     int64_t n_bytes, const uint32_t *weights, uint8_t *cons, int64_t cons_cap,
                     int64_t *cons_off /* n_windows + 1 */, int64_t *cons_used, int32_t *node_count,
                     int64_t *n_alignments);

/* Of the calling thread's last gb_poa_align or gb_poa_consensus: the fill kernels' and the walk kernels' time
 * summed over chunks and rounds (0 on the host path), the host time of the graph updates and re-flattened views
 * (0 for gb_poa_align), and the cells: n_nodes * seq_len summed over the alignments done. GB_ERR_STATE before
 * the first. */
int gb_poa_timing(float *fill_ms, float *walk_ms, float *host_ms, int64_t *cells);
/* Of the same call: the number of chunks, over all rounds, and the largest chunk's workspace (both 0 on the
 * host path). */
int gb_poa_plan(int64_t *chunks, int64_t *workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GB_POA_H */
