// dbg_live_shim.cpp -- drives the reference's benchmarks/dbg/debruijn.cpp, included unmodified, over a binary set of
// regions and writes what it built. Compiled by make_dbg_golden.py into a temporary directory, together with the
// reference's common.cpp (setWindowPointers); the reference driver's own main is renamed and, being unreferenced, is
// dropped by the linker with its htslib calls.
//
//   dbg_live_shim graphs in.bin out.bin     the k loop of assembleReadsAndDetectVariants (the loop the reference
//                                           keeps as a comment) for every region; per region the cycle flag of every
//                                           k tried and every node and edge of the final graph
//   dbg_live_shim windows in.bin out.bin    setWindowPointers for a list of (start, end) over reads given by pos, end
//   dbg_live_shim time in.bin out.bin       seconds of one thread for the k loop over every region
#define main reference_driver_main
#include "debruijn.cpp"
#undef main

#include <chrono>
#include <map>
#include <string>

namespace {

template <typename T>
T rd(FILE *f) {
  T v;
  if (fread(&v, sizeof v, 1, f) != 1) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
  return v;
}
template <typename T>
void wr(FILE *f, T v) {
  fwrite(&v, sizeof v, 1, f);
}

struct Region {
  std::vector<char> ref;
  int ref_start, read_first, read_last;
};

struct Set {
  int k0, k_step, k_max, min_qual, min_weight;
  std::vector<alignedRead> reads;
  std::vector<Region> regions;
};

void load(FILE *f, Set *s) {
  const int n_regions = rd<int32_t>(f), n_reads = rd<int32_t>(f);
  s->k0 = rd<int32_t>(f), s->k_step = rd<int32_t>(f), s->k_max = rd<int32_t>(f);
  s->min_qual = rd<int32_t>(f), s->min_weight = rd<int32_t>(f);
  s->reads.resize(n_reads);
  for (auto &r : s->reads) {
    memset(&r, 0, sizeof r);
    const int len = rd<int32_t>(f);
    r.flag = rd<uint32_t>(f);
    if (len >= MAX_READ_LEN) {
      fprintf(stderr, "read of %d bases\n", len);
      exit(2);
    }
    if (len && (fread(r.seq, 1, len, f) != (size_t)len || fread(r.qual, 1, len, f) != (size_t)len)) exit(2);
    r.rlen = len;
  }
  s->regions.resize(n_regions);
  for (auto &g : s->regions) {
    const int len = rd<int32_t>(f);
    g.ref_start = rd<int32_t>(f), g.read_first = rd<int32_t>(f), g.read_last = rd<int32_t>(f);
    g.ref.assign(len + 1, 0);
    if (len && fread(g.ref.data(), 1, len, f) != (size_t)len) exit(2);
  }
}

DeBruijnGraph *build(Set &s, Region &g, int k) {
  DeBruijnGraph *graph = createDeBruijnGraph(k, 5000);
  loadReferenceIntoGraph(graph, g.ref.data(), g.ref_start, k);
  loadBAMDataIntoGraph(graph, s.reads.data() + g.read_first, s.reads.data() + g.read_last, 1, 0, s.min_qual, k);
  return graph;
}

// the loop of assembleReadsAndDetectVariants; the final graph is returned and the flags of every k appended
DeBruijnGraph *k_loop(Set &s, Region &g, std::vector<int> *tried) {
  int k = s.k0;
  DeBruijnGraph *graph = build(s, g, k);
  for (;;) {
    const int cyclic = detectCyclesInGraph_Recursive(graph, s.min_weight);
    if (tried) tried->push_back(k), tried->push_back(cyclic);
    if (!cyclic || k > s.k_max) break;
    k += s.k_step;
    destroyDeBruijnGraph(graph);
    graph = build(s, g, k);
  }
  return graph;
}

int graphs(FILE *in, FILE *out) {
  Set s;
  load(in, &s);
  for (auto &g : s.regions) {
    std::vector<int> tried;
    DeBruijnGraph *graph = k_loop(s, g, &tried);
    wr<int32_t>(out, (int32_t)(tried.size() / 2));
    for (int v : tried) wr<int32_t>(out, v);
    const int n = graph->allNodes->top + 1;
    Node **nodes = graph->allNodes->elements;
    std::map<Node *, int> id;
    for (int i = 0; i < n; ++i) id[nodes[i]] = i;
    wr<int32_t>(out, n);
    for (int i = 0; i < n; ++i) {
      Node *x = nodes[i];
      int src = -1, off;
      if (x->sequence >= g.ref.data() && x->sequence < g.ref.data() + g.ref.size()) {
        off = (int)(x->sequence - g.ref.data());
      } else {
        src = (int)((x->sequence - (char *)s.reads.data()) / (ptrdiff_t)sizeof(alignedRead));
        off = (int)(x->sequence - s.reads[src].seq);
      }
      wr<int32_t>(out, src), wr<int32_t>(out, off), wr<int32_t>(out, x->colours), wr<int32_t>(out, x->position);
      wr<int64_t>(out, (int64_t)x->weight), wr<int32_t>(out, x->nEdges);
      for (int j = 0; j < 4; ++j) wr<int32_t>(out, j < x->nEdges ? id.at(x->edges[j]->endNode) : -1);
      for (int j = 0; j < 4; ++j) wr<int64_t>(out, j < x->nEdges ? (int64_t)x->edges[j]->weight : 0);
    }
    destroyDeBruijnGraph(graph);
  }
  return 0;
}

int timed(FILE *in, FILE *out) {
  Set s;
  load(in, &s);
  const auto t0 = std::chrono::steady_clock::now();
  for (auto &g : s.regions) destroyDeBruijnGraph(k_loop(s, g, nullptr));
  wr<double>(out, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  return 0;
}

int windows(FILE *in, FILE *out) {
  const int n = rd<int32_t>(in), longest = rd<int32_t>(in), n_q = rd<int32_t>(in);
  std::vector<alignedRead> reads(n ? n : 1);
  for (int i = 0; i < n; ++i) reads[i].pos = rd<uint32_t>(in), reads[i].end = rd<uint32_t>(in);
  ReadArray a;
  a.array = a.windowStart = a.windowEnd = reads.data();
  a.__size = n, a.__capacity = (int)reads.size(), a.__longestRead = longest;
  for (int i = 0; i < n_q; ++i) {
    const int start = rd<int32_t>(in), end = rd<int32_t>(in);
    setWindowPointers(&a, start, end);
    wr<int32_t>(out, (int32_t)(a.windowStart - a.array)), wr<int32_t>(out, (int32_t)(a.windowEnd - a.array));
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
  if (!in || !out) return 2;
  const std::string mode = argv[1];
  const int st = mode == "graphs" ? graphs(in, out) : mode == "windows" ? windows(in, out) : mode == "time" ? timed(in, out) : 2;
  fclose(in), fclose(out);
  return st;
}
