// poa_host_check.cpp -- stand-alone host program over the host path of gb_poa_align and gb_poa_consensus
// (csrc/bsw_poa.hip), meant to be built with the address and undefined-behaviour sanitizers on the host side
// (`make poa-sanitize` builds it together with the library's two source files and runs it). It touches no device:
// GB_POA_HOST=1 is set before the first call. Random windows of noisy reads of a template (substitutions, short
// and long indels, clipped ends, empty reads, with and without weights) at a linear, an affine and two convex
// parameter sets go through gb_poa_consensus; chains and forks built by hand go through gb_poa_align with a pair
// buffer of exactly the need, one of one pair less, and a refused item. The outputs are checked for shape only
// (the fixture checks values). Prints "ok" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../include/gb_bsw_poa.h"

static int fail(const char *what, int trial) {
  printf("trial %d: %s: %s\n", trial, what, gb_last_error());
  return 1;
}

int main() {
  setenv("GB_POA_HOST", "1", 1);
  setenv("GB_POA_THREADS", "3", 1);
  std::mt19937_64 rng(31);
  const gb_poa_params sets[] = {{2, -4, -6, -2, -25, -1, GB_POA_NW, 0}, {5, -4, -8, -8, -8, -8, GB_POA_NW, 0},
                                {5, -4, -8, -6, -8, -6, GB_POA_NW, 0},  {5, -4, -8, -6, -10, -2, GB_POA_NW, 0}};
  const char al[] = "ACGTNa";
  for (int trial = 0; trial < 24; ++trial) {
    const gb_poa_params P = sets[trial % 4];
    const int n_windows = 1 + (int)(rng() % 6);
    std::vector<int64_t> win_off{0}, seq_off{0};
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> weights;
    for (int w = 0; w < n_windows; ++w) {
      const int tlen = 1 + (int)(rng() % 120), n_reads = (int)(rng() % 9);
      std::vector<uint8_t> t((size_t)tlen);
      for (auto &b : t) b = (uint8_t)al[rng() % (trial % 3 ? 4 : 6)];
      for (int r = 0; r < n_reads; ++r) {
        size_t i = rng() % 4 ? 0 : rng() % (size_t)tlen, end = rng() % 4 ? (size_t)tlen : rng() % (size_t)(tlen + 1);
        if (rng() % 11) {
          for (; i < end; ++i) {
            const unsigned u = (unsigned)(rng() % 100);
            if (u < 1) {
              for (int k = 25 + (int)(rng() % 10); k > 0; --k) bytes.push_back((uint8_t)al[rng() % 4]);
            } else if (u < 2) {
              i += 25 + rng() % 10;
            } else if (u < 7) {
              bytes.push_back((uint8_t)al[rng() % 4]), --i;
            } else if (u < 12) {
              bytes.push_back((uint8_t)al[rng() % 4]);
            } else if (u >= 17) {
              bytes.push_back(t[i]);
            }
          }
        }  // else an empty read
        seq_off.push_back((int64_t)bytes.size());
      }
      win_off.push_back((int64_t)seq_off.size() - 1);
    }
    weights.resize(bytes.size());
    for (auto &x : weights) x = (uint32_t)(rng() % 41);
    const int64_t n_seqs = (int64_t)seq_off.size() - 1, need = (int64_t)bytes.size();
    std::vector<uint8_t> cons((size_t)need);  // exactly the need: a byte past it is the sanitizer's to find
    std::vector<int64_t> cons_off((size_t)n_windows + 1, -5);
    std::vector<int32_t> nodes((size_t)n_windows, -5);
    int64_t used = -1, done = -1;
    if (gb_poa_consensus(&P, win_off.data(), n_windows, seq_off.data(), n_seqs, bytes.data(), need,
                         trial % 2 ? weights.data() : nullptr, cons.data(), need, cons_off.data(), &used, nodes.data(), &done))
      return fail("gb_poa_consensus", trial);
    if (cons_off[0] != 0 || cons_off[(size_t)n_windows] != used || used > need || done < 0) return fail("offsets", trial);
    for (int w = 0; w < n_windows; ++w)
      if (cons_off[(size_t)w + 1] - cons_off[(size_t)w] > nodes[(size_t)w]) return fail("consensus longer than the graph", trial);
    if (need > 0) {
      used = -1;
      if (gb_poa_consensus(&P, win_off.data(), n_windows, seq_off.data(), n_seqs, bytes.data(), need, nullptr, cons.data(),
                           need - 1, cons_off.data(), &used, nodes.data(), &done) != GB_ERR_ARG ||
          used != need)
        return fail("a cap one short was not refused", trial);
    }
  }
  // gb_poa_align on graphs made by hand: a chain with skip edges, and a fork of two sinks
  for (int trial = 0; trial < 24; ++trial) {
    const gb_poa_params P = sets[trial % 4];
    std::vector<uint8_t> base, out, seqs;
    std::vector<int32_t> id, in_end, pred;
    std::vector<gb_poa_item> items;
    int64_t need = 0;
    const int n_items = 1 + (int)(rng() % 6);
    for (int k = 0; k < n_items; ++k) {
      gb_poa_item it{};
      it.node_off = (int64_t)base.size(), it.edge_off = (int64_t)pred.size(), it.seq_off = (int64_t)seqs.size();
      const int n = (int)(rng() % 90), len = rng() % 7 ? 1 + (int)(rng() % 300) : 0;
      std::vector<int> has_out((size_t)n, 0);
      const size_t e0 = pred.size();
      for (int r = 0; r < n; ++r) {
        base.push_back((uint8_t)al[rng() % 4]), id.push_back(n - 1 - r);
        if (r > 0 && rng() % 9) pred.push_back(r - 1), has_out[(size_t)r - 1] = 1;
        if (r > 3 && rng() % 3 == 0) {
          const int p = r - 2 - (int)(rng() % 2);
          pred.push_back(p), has_out[(size_t)p] = 1;
        }
        in_end.push_back((int32_t)(pred.size() - e0));
      }
      for (int r = 0; r < n; ++r) out.push_back((uint8_t)has_out[(size_t)r]);
      for (int i = 0; i < len; ++i) seqs.push_back(i < n && rng() % 6 ? base[(size_t)it.node_off + (size_t)i] : (uint8_t)al[rng() % 4]);
      it.n_nodes = n, it.n_edges = (int32_t)(pred.size() - e0), it.seq_len = len;
      if (n && len) need += n + len;
      items.push_back(it);
    }
    const gb_poa_graphs G{base.data(), id.data(), out.data(), in_end.data(), pred.data(), (int64_t)base.size(), (int64_t)pred.size()};
    std::vector<int32_t> scores((size_t)n_items, -7), pairs((size_t)need * 2 + 2, -9);
    std::vector<int64_t> off((size_t)n_items + 1, -5);
    int64_t used = -1;
    if (gb_poa_align(&P, &G, seqs.data(), (int64_t)seqs.size(), items.data(), n_items, scores.data(), pairs.data(), need,
                     off.data(), &used))
      return fail("gb_poa_align", trial);
    if (off[0] != 0 || off[(size_t)n_items] != used || used > need) return fail("offsets", trial);
    for (int k = 0; k < n_items; ++k) {
      int next = 0;
      for (int64_t i = off[(size_t)k]; i < off[(size_t)k + 1]; ++i) {
        const int32_t a = pairs[(size_t)(2 * i)], b = pairs[(size_t)(2 * i + 1)];
        if (a < -1 || a >= items[(size_t)k].n_nodes || (a == -1 && b == -1)) return fail("pair out of range", trial);
        if (b != -1 && b != next++) return fail("positions not ascending", trial);
      }
      if (off[(size_t)k + 1] > off[(size_t)k] && next != items[(size_t)k].seq_len) return fail("positions missing", trial);
    }
    if (need > 0) {
      used = -1;
      if (gb_poa_align(&P, &G, seqs.data(), (int64_t)seqs.size(), items.data(), n_items, scores.data(), pairs.data(), need - 1,
                       off.data(), &used) != GB_ERR_ARG ||
          used != need)
        return fail("a cap one short was not refused", trial);
    }
    items[0].seq_len = GB_POA_MAX_LEN + 1;
    if (gb_poa_align(&P, &G, seqs.data(), (int64_t)seqs.size(), items.data(), n_items, scores.data(), pairs.data(), need,
                     off.data(), &used) != GB_ERR_ARG)
      return fail("an over-long item was not refused", trial);
  }
  printf("ok\n");
  return 0;
}
