// dbg_host_check.cpp -- stand-alone host program over the host path of gb_dbg_assemble (csrc/fmi_dbg.hip), meant to
// be built with the address and undefined-behaviour sanitizers on the host side (`make dbg-sanitize` builds it
// together with the library's two source files and runs it). It touches no device: GB_DBG_HOST=1 is set before the
// first call. The stored k = 3 case with the live reference's graph, random regions over a shared read pool through
// every export with buffers of exactly the need (texts shorter than k + 2, 'N's, low qualities, QC-fail reads,
// tandem repeats that run the k loop to its end), every refusal and the empty batch. Values are checked on the stored
// case, shapes and sums elsewhere (the fixture checks values). Prints "ok" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/gb_fmi_dbg.h"

static int fail(const char *what, int trial) {
  printf("trial %d: %s: %s\n", trial, what, gb_last_error());
  return 1;
}

struct Batch {
  std::vector<uint8_t> ref, seq, qual;
  std::vector<int64_t> ref_off{0}, read_off{0}, first, last;
  std::vector<int32_t> start;
  std::vector<uint32_t> flag;
  void read(const std::string &s, const std::vector<uint8_t> &q, uint32_t f) {
    seq.insert(seq.end(), s.begin(), s.end()), qual.insert(qual.end(), q.begin(), q.end());
    read_off.push_back((int64_t)seq.size()), flag.push_back(f);
  }
  void region(const std::string &s, int32_t at, int64_t a, int64_t b) {
    ref.insert(ref.end(), s.begin(), s.end()), ref_off.push_back((int64_t)ref.size());
    start.push_back(at), first.push_back(a), last.push_back(b);
  }
  int assemble(const gb_dbg_params *p, int keep, gb_dbg **h) const {
    return gb_dbg_assemble(ref.data(), (int64_t)ref.size(), ref_off.data(), start.data(), first.data(), last.data(),
                           (int64_t)start.size(), seq.data(), qual.data(), (int64_t)seq.size(), read_off.data(),
                           flag.data(), (int64_t)flag.size(), p, keep, h);
  }
};

static int run(const Batch &B, const gb_dbg_params *p, int trial) {
  gb_dbg *h = nullptr, *h0 = nullptr;
  if (B.assemble(p, 1, &h) || B.assemble(p, 0, &h0)) return fail("gb_dbg_assemble", trial);
  const size_t n = B.start.size();
  std::vector<gb_dbg_region_summary> sum(n), sum0(n);
  if (gb_dbg_summary(h, sum.data(), (int64_t)n) || gb_dbg_summary(h0, sum0.data(), (int64_t)n))
    return fail("summary", trial);
  if (n && memcmp(sum.data(), sum0.data(), n * sizeof sum[0])) return fail("keep changes the summary", trial);
  for (size_t r = 0; r < n; ++r) {
    int64_t nn = -1;
    const size_t N = (size_t)sum[r].n_nodes;
    std::vector<int32_t> src(N), off(N), col(N), pos(N), ne(N), to(4 * N);
    std::vector<int64_t> w(N), ew(4 * N);
    if (gb_dbg_export(h, (int64_t)r, (int64_t)N, src.data(), off.data(), col.data(), pos.data(), w.data(), ne.data(),
                      to.data(), ew.data(), &nn) || nn != (int64_t)N)
      return fail("export", trial);
    if (gb_dbg_export(h0, (int64_t)r, (int64_t)N, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                      nullptr, &nn) != GB_ERR_ARG)
      return fail("export of a keep = 0 handle", trial);
    int64_t edges = 0, ws = 0, es = 0, both = 0;
    for (size_t i = 0; i < N; ++i) {
      edges += ne[i], ws += w[i], both += col[i] == 3;
      if (ne[i] < 0 || ne[i] > 4 || col[i] < 1 || col[i] > 3 || (src[i] < 0 ? pos[i] != B.start[r] + off[i] : pos[i] != -1))
        return fail("node record", trial);
      for (int j = 0; j < 4; ++j) {
        es += ew[4 * i + (size_t)j];
        if (j < ne[i] ? to[4 * i + (size_t)j] < 0 || to[4 * i + (size_t)j] >= (int32_t)N : to[4 * i + (size_t)j] != -1)
          return fail("edge record", trial);
      }
    }
    if (edges != sum[r].n_edges || ws != sum[r].node_weight_sum || es != sum[r].edge_weight_sum ||
        both != sum[r].n_ref_and_read)
      return fail("summary and export disagree", trial);
  }
  gb_dbg_free(h), gb_dbg_free(h0);
  return 0;
}

int main() {
  setenv("GB_DBG_HOST", "1", 1);
  setenv("GB_DBG_THREADS", "3", 1);
  std::mt19937_64 rng(29);
  {  // the stored case: the live reference gives 17 nodes, AAA with weight 11 and edges to AAC (2), AAG, AAT, AAN
    Batch B;
    B.region("AAAC.AAAG.AAAT.AAAN.AAAa.AAAC..", 100, 0, 0);
    const gb_dbg_params p{3, 5, 2, 20, 40};
    gb_dbg *h = nullptr;
    if (B.assemble(&p, 1, &h)) return fail("stored", 0);
    int32_t off[17], ne[17], to[68];
    int64_t w[17], ew[68], n = 0;
    if (gb_dbg_export(h, 0, 17, nullptr, off, nullptr, nullptr, w, ne, to, ew, &n) || n != 17) return fail("stored", 0);
    const int64_t want_ew[4] = {2, 1, 1, 1};
    const int32_t want_to[4] = {1, 5, 8, 11};  // AAC, AAG, AAT, AAN in order of first visit
    if (off[0] != 0 || w[0] != 11 || ne[0] != 4 || memcmp(ew, want_ew, sizeof want_ew) || memcmp(to, want_to, sizeof want_to))
      return fail("stored case differs", 0);
    gb_dbg_free(h);
  }
  int trial = 1;
  const char al[] = "ACGTNacM=";
  for (int rep = 0; rep < 12; ++rep, ++trial) {
    Batch B;
    const int k0 = rep % 3 == 0 ? 3 : rep % 3 == 1 ? 15 : 31;
    const gb_dbg_params p{k0, 1 + rep % 5, rep % 2 ? 50 : k0 + 4, 20, 40};
    std::string genome((size_t)(400 + rng() % 400), 'A');
    for (auto &c : genome) c = al[rng() % (rep % 4 == 3 ? 2 : 4)];
    if (rep % 4 == 1)
      for (size_t i = 100; i < 220; ++i) genome[i] = "ACGGT"[i % 5];  // cyclic at every k
    for (int j = 0; j < 40; ++j) {
      const size_t len = j % 9 == 0 ? (size_t)(k0 + j % 3) : 20 + rng() % 130;
      const size_t at = rng() % (genome.size() - 160);
      std::string s = genome.substr(at, len);
      std::vector<uint8_t> q(s.size());
      for (auto &c : s)
        if (rng() % 50 == 0) c = al[rng() % 9];
      for (auto &x : q) x = (uint8_t)(rng() % 20 == 0 ? rng() % 25 : 20 + rng() % 21);
      B.read(s, q, rng() % 10 == 0 ? 512u : (uint32_t)(rng() % 4));
    }
    for (int r = 0; r < 6; ++r) {
      const size_t at = rng() % 200, len = r == 5 ? (size_t)(k0 + 1) : 100 + rng() % (genome.size() - 300);
      const int64_t a = (int64_t)(rng() % 30);
      B.region(genome.substr(at, len), r == 4 ? 2000000000 : (int32_t)at, a, r == 3 ? a : a + 1 + (int64_t)(rng() % 10));
    }
    if (run(B, &p, trial)) return 1;
  }
  {  // refusals leave the handle pointer alone
    Batch B;
    B.read("ACGTACGTACGTACGTACGT", std::vector<uint8_t>(20, 30), 0);
    B.region("ACGTACGTTTGCACGTACGTAAA", 0, 0, 1);
    gb_dbg *h = (gb_dbg *)0x10;
    gb_dbg_params p{15, 5, 50, 20, 40};
    Batch C = B;
    C.ref[5] = 0;
    if (C.assemble(&p, 0, &h) != GB_ERR_ARG || h != (gb_dbg *)0x10) return fail("NUL in a reference accepted", trial);
    C = B, C.seq[7] = 0;
    if (C.assemble(&p, 0, &h) != GB_ERR_ARG || h != (gb_dbg *)0x10) return fail("NUL in a read accepted", trial);
    C = B, C.last[0] = 2;
    if (C.assemble(&p, 0, &h) != GB_ERR_ARG) return fail("range accepted", trial);
    C = B, C.read_off[1] = 21;
    if (C.assemble(&p, 0, &h) != GB_ERR_ARG) return fail("offsets accepted", trial);
    p.k_max = 60;
    if (B.assemble(&p, 0, &h) != GB_ERR_ARG) return fail("k = 65 accepted", trial);
    p.k_max = 50, p.k0 = 0;
    if (B.assemble(&p, 0, &h) != GB_ERR_ARG || h != (gb_dbg *)0x10) return fail("k0 = 0 accepted", trial);
    if (gb_dbg_assemble(nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0,
                        nullptr, 1, &h))
      return fail("empty", trial);
    if (gb_dbg_summary(h, nullptr, 0)) return fail("empty summary", trial);
    gb_dbg_free(h);
  }
  printf("ok\n");
  return 0;
}
