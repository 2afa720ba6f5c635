// chain_extd2_host_check.cpp -- stand-alone host program over the host path of gb_chain_extd2
// (csrc/chain_extd2.hip), meant to be built with the address and undefined-behaviour sanitizers on the host
// side (`make chain-extd2-sanitize` builds it together with the library's two source files and runs it). It
// touches no device: GB_CHAIN_EXTD2_HOST=1 is set before the first call. Random parameter sets (presets, a
// swapped pair, one that overflows 8 bits, one that returns early) and items: lengths 0 to a few hundred, with
// lengths at multiples of 16, every accepted flag, bands from none to 40 and 751, N bases; a CIGAR buffer of
// exactly the need, one of one word less, and a refused item. The outputs are checked for shape only (the
// fixture checks values). Prints "ok" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../include/gb_chain_extd2.h"

int main() {
  setenv("GB_CHAIN_EXTD2_HOST", "1", 1);
  setenv("GB_CHAIN_THREADS", "3", 1);
  std::mt19937_64 rng(29);
  const gb_chain_extd2_params sets[] = {{2, 4, 1, 4, 2, 24, 1, 0},  {1, 19, 1, 39, 3, 81, 1, 0}, {2, 4, 0, 24, 1, 4, 2, 0},
                                        {3, 5, 2, 60, 20, 100, 40, 0}, {1, 19, 1, 4, 2, 24, 1, 0}};
  const int flags[] = {0, 0x40, 0x08, 0xc2, 0x18, 0x02, 0x80, 0x58, 0xda};
  const int lens[] = {0, 1, 2, 15, 16, 17, 32, 33, 64, 100, 128, 129, 257, 400};
  for (int trial = 0; trial < 40; ++trial) {
    const gb_chain_extd2_params P = sets[trial % 5];
    const int n_items = 1 + (int)(rng() % 24);
    std::vector<uint8_t> seqs;
    std::vector<gb_chain_extd2_item> items;
    int64_t need = 0;
    for (int k = 0; k < n_items; ++k) {
      gb_chain_extd2_item it{};
      it.qlen = lens[rng() % 14], it.tlen = lens[rng() % 14];
      if (rng() % 3 == 0) it.qlen = (int)(rng() % 300), it.tlen = (int)(rng() % 300);
      it.t_off = (int64_t)seqs.size();
      for (int i = 0; i < it.tlen; ++i) seqs.push_back(rng() % 50 ? (uint8_t)(rng() % 4) : 4);
      it.q_off = (int64_t)seqs.size();
      for (int i = 0; i < it.qlen; ++i)  // the target with substitutions and slips, so that paths run long
        seqs.push_back(i < it.tlen && rng() % 8 ? seqs[(size_t)it.t_off + (size_t)i] : (uint8_t)(rng() % 5));
      it.w = rng() % 5 == 0 ? 751 : (int)(rng() % 42) - 1;
      it.zdrop = rng() % 4 == 0 ? -1 : (int)(rng() % 400);
      it.end_bonus = rng() % 2 ? -1 : 10;
      it.flag = flags[rng() % 9];
      items.push_back(it);
      need += it.qlen + it.tlen;
    }
    std::vector<gb_chain_extd2_result> res((size_t)n_items);
    std::vector<uint32_t> cigar((size_t)need);  // exactly the need: a word past it is the sanitizer's to find
    std::vector<int64_t> off((size_t)n_items + 1, -5);
    int64_t used = -1;
    int st = gb_chain_extd2(&P, seqs.data(), (int64_t)seqs.size(), items.data(), n_items, res.data(), cigar.data(), need,
                            off.data(), &used);
    if (st) {
      printf("trial %d: %s\n", trial, gb_last_error());
      return 1;
    }
    if (off[0] != 0 || off[(size_t)n_items] != used || used > need) {
      printf("trial %d: offsets\n", trial);
      return 1;
    }
    for (int k = 0; k < n_items; ++k) {
      const gb_chain_extd2_item &it = items[(size_t)k];
      const gb_chain_extd2_result &r = res[(size_t)k];
      const int64_t n = off[(size_t)k + 1] - off[(size_t)k];
      int64_t ql = 0, tl = 0;
      for (int64_t j = 0; j < n; ++j) {
        const uint32_t w = cigar[(size_t)(off[(size_t)k] + j)], op = w & 15, len = w >> 4;
        if (op != 1) tl += len;
        if (op != 2) ql += len;
      }
      // the walk starts at the corner, at (mqe_t, qlen - 1) or at (max_t, max_q), and ends before the matrix
      int i0 = -1, j0 = -1;
      if (!r.zdropped && !(it.flag & GB_EXTD2_EXTZ_ONLY)) i0 = it.tlen - 1, j0 = it.qlen - 1;
      else if (r.reach_end) i0 = r.mqe_t, j0 = it.qlen - 1;
      else if (r.max_t >= 0 && r.max_q >= 0) i0 = r.max_t, j0 = r.max_q;
      const bool walked = n > 0;
      if (n != r.n_cigar || n > it.qlen + it.tlen || (walked && (tl != i0 + 1 || ql != j0 + 1)) || r.pad != 0) {
        printf("trial %d: item %d: %lld words over %lld x %lld from (%d, %d)\n", trial, k, (long long)n, (long long)ql,
               (long long)tl, i0, j0);
        return 1;
      }
    }
    // one word short: refused with the need, nothing else written
    std::vector<int64_t> kept((size_t)n_items + 1, -5);
    int64_t short_used = -1;
    bool untouched = true;
    if (need > 0) {
      st = gb_chain_extd2(&P, seqs.data(), (int64_t)seqs.size(), items.data(), n_items, res.data(), cigar.data(), need - 1,
                          kept.data(), &short_used);
      for (int64_t v : kept) untouched = untouched && v == -5;
      if (st != GB_ERR_ARG || short_used != need || !untouched) {
        printf("trial %d: short buffer: status %d, need %lld of %lld\n", trial, st, (long long)short_used, (long long)need);
        return 1;
      }
    }
    // a sequence that ends one byte past seqs: refused, outputs untouched
    items.back().t_off = (int64_t)seqs.size() - items.back().tlen + 1;
    short_used = -1;
    st = gb_chain_extd2(&P, seqs.data(), (int64_t)seqs.size(), items.data(), n_items, res.data(), cigar.data(), need,
                        kept.data(), &short_used);
    for (int64_t v : kept) untouched = untouched && v == -5;
    if (st != GB_ERR_ARG || short_used != -1 || !untouched) {
      printf("trial %d: refusal: status %d, untouched %d\n", trial, st, (int)untouched);
      return 1;
    }
    if (trial % 8 == 0) printf("trial %d: %d items, %lld words of at most %lld\n", trial, n_items, (long long)used, (long long)need);
  }
  puts("ok");
  return 0;
}
