// poa_live_shim.cpp -- a C face over the reference's spoa (createAlignmentEngine, createGraph, align,
// add_alignment, generate_consensus and the accessors of Graph and Node), for ctypes. make_poa_golden.py compiles
// it, with the reference's own sources, in a temporary directory; nothing of the reference is kept here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "spoa/spoa.hpp"

namespace {
struct Engine { std::unique_ptr<spoa::AlignmentEngine> p; };
struct Graph { std::unique_ptr<spoa::Graph> p; };
}  // namespace

extern "C" {

// null if createAlignmentEngine throws; the message goes to err
void *poa_live_engine(int type, int m, int n, int g, int e, int q, int c, char *err, int err_cap) {
  try {
    auto *E = new Engine;
    E->p = spoa::createAlignmentEngine(static_cast<spoa::AlignmentType>(type), (std::int8_t)m, (std::int8_t)n,
                                       (std::int8_t)g, (std::int8_t)e, (std::int8_t)q, (std::int8_t)c);
    return E;
  } catch (const std::exception &x) {
    if (err && err_cap > 0) std::snprintf(err, (size_t)err_cap, "%s", x.what());
    return nullptr;
  }
}
void poa_live_engine_free(void *e) { delete static_cast<Engine *>(e); }

void *poa_live_graph() {
  auto *G = new Graph;
  G->p = spoa::createGraph();
  return G;
}
void poa_live_graph_free(void *g) { delete static_cast<Graph *>(g); }

// the pairs of align(seq, graph), two int32 each; returns their number, or -1 - number if cap is too small
int poa_live_align(void *e, void *g, const char *seq, int len, int32_t *pairs, int cap) {
  const auto a = static_cast<Engine *>(e)->p->align(seq, (std::uint32_t)len, static_cast<Graph *>(g)->p);
  if ((int)a.size() > cap) return -1 - (int)a.size();
  for (size_t k = 0; k < a.size(); ++k) pairs[2 * k] = a[k].first, pairs[2 * k + 1] = a[k].second;
  return (int)a.size();
}

// add_alignment with per-base weights, or with the default weight 1 if weights is null
void poa_live_add(void *g, const int32_t *pairs, int n_pairs, const char *seq, int len, const uint32_t *weights) {
  spoa::Alignment a;
  for (int k = 0; k < n_pairs; ++k) a.emplace_back(pairs[2 * k], pairs[2 * k + 1]);
  auto &G = static_cast<Graph *>(g)->p;
  if (weights) {
    G->add_alignment(a, seq, (std::uint32_t)len, std::vector<std::uint32_t>(weights, weights + len));
  } else {
    G->add_alignment(a, seq, (std::uint32_t)len);
  }
}
// add_alignment with a quality string
void poa_live_add_quality(void *g, const int32_t *pairs, int n_pairs, const char *seq, int len, const char *quality) {
  spoa::Alignment a;
  for (int k = 0; k < n_pairs; ++k) a.emplace_back(pairs[2 * k], pairs[2 * k + 1]);
  static_cast<Graph *>(g)->p->add_alignment(a, seq, (std::uint32_t)len, quality, (std::uint32_t)len);
}

int poa_live_consensus(void *g, char *dst, int cap) {
  const std::string s = static_cast<Graph *>(g)->p->generate_consensus();
  if ((int)s.size() > cap) return -1 - (int)s.size();
  std::memcpy(dst, s.data(), s.size());
  return (int)s.size();
}

int poa_live_nodes(void *g) { return (int)static_cast<Graph *>(g)->p->nodes().size(); }
int poa_live_edges(void *g) {
  int n = 0;
  for (const auto &nd : static_cast<Graph *>(g)->p->nodes()) n += (int)nd->in_edges().size();
  return n;
}

// the graph in rank order: per rank the node's byte, id, whether it has out-edges and the end of its in-edge
// range; per in-edge, in in_edges() order, the predecessor's rank
void poa_live_view(void *g, uint8_t *base, int32_t *id, uint8_t *out, int32_t *in_end, int32_t *pred) {
  const auto &G = static_cast<Graph *>(g)->p;
  const auto &order = G->rank_to_node_id();
  std::vector<int32_t> rank(order.size());
  for (size_t r = 0; r < order.size(); ++r) rank[order[r]] = (int32_t)r;
  int32_t e = 0;
  for (size_t r = 0; r < order.size(); ++r) {
    const auto &nd = G->nodes()[order[r]];
    base[r] = G->decoder((std::uint8_t)nd->code()), id[r] = (int32_t)order[r], out[r] = !nd->out_edges().empty();
    for (const auto &ed : nd->in_edges()) pred[e++] = rank[ed->begin_node_id()];
    in_end[r] = e;
  }
}

// per node id, the number of nodes aligned to it
void poa_live_aligned_counts(void *g, int32_t *dst) {
  const auto &G = static_cast<Graph *>(g)->p;
  for (size_t k = 0; k < G->nodes().size(); ++k) dst[k] = (int32_t)G->nodes()[k]->aligned_nodes_ids().size();
}

}  // extern "C"
