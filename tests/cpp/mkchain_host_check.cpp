// mkchain_host_check.cpp -- stand-alone host program over the host path of gb_bsw_seeds2chains
// (csrc/bsw_mkchain.hip), meant to be built with the address and undefined-behaviour sanitizers on the
// host side (`make mkchain-sanitize` builds it together with the library's two source files and runs it).
// It touches no device: GB_BSW_MKCHAIN_HOST=1 is set before the first call. Random SMEMs, options and
// coordinate ranges, narrow ones among them so that equal pos are common and the B-tree grows levels; the
// outputs are checked for shape only (the fixture checks values): offsets that rise, every chain with a
// seed, every seed inside its read. Prints "ok" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../include/gb_bsw.h"

int main() {
  setenv("GB_BSW_MKCHAIN_HOST", "1", 1);
  std::mt19937_64 rng(5);
  for (int trial = 0; trial < 60; ++trial) {
    const int64_t l_pac = 1000 + (int64_t)(rng() % 100000);
    const std::vector<int64_t> ce = {l_pac / 3, l_pac / 2, l_pac};
    const std::vector<uint8_t> alt = {0, 1, 0};
    gb_bsw_chain_opt o;
    gb_bsw_chain_default_opt(&o);
    o.max_occ = 1 + (int)(rng() % 600);
    o.w = (int)(rng() % 200);
    o.max_chain_gap = (int)(rng() % 300);
    o.min_chain_weight = rng() % 2 ? 0 : 15 + (int)(rng() % 30);  // 1.1f * it must pass 0.05f * l_query
    o.max_chain_extend = 1 + (int)(rng() % 50);
    const int n_reads = 1 + (int)(rng() % 40);
    std::vector<int32_t> lq;
    std::vector<gb_bsw_mem> mems;
    std::vector<int64_t> coords;
    for (int r = 0; r < n_reads; ++r) {
      const int l = 20 + (int)(rng() % 230);
      lq.push_back(l);
      const int nm = (int)(rng() % 12);
      for (int k = 0; k < nm; ++k) {
        gb_bsw_mem m{};
        m.read = r;
        m.m = (int)(rng() % (l - 1));
        m.n = m.m + (int)(rng() % (l - m.m));
        m.s = 1 + (int64_t)(rng() % 3 ? rng() % 40 : rng() % 3000);
        const int64_t step = m.s > o.max_occ ? m.s / o.max_occ : 1;
        int64_t c = (m.s + step - 1) / step;
        if (c > o.max_occ) c = o.max_occ;
        m.n_coord = (int)c;
        const int64_t span = trial % 3 ? 2 * l_pac : 400;  // a narrow span makes equal pos common
        for (int j = 0; j < c; ++j) coords.push_back((int64_t)(rng() % span) + (trial % 3 ? 0 : l_pac - 200));
        mems.push_back(m);
      }
    }
    const int64_t nc = (int64_t)coords.size();
    std::vector<int64_t> rco(n_reads + 1), cso(nc + 1);
    std::vector<gb_bsw_seed> seeds(nc ? nc : 1);
    std::vector<gb_bsw_chain_info> info(nc ? nc : 1);
    int64_t cu = 0, su = 0;
    for (int stage = 0; stage < 2; ++stage) {
      const int st = gb_bsw_seeds2chains(&o, stage, l_pac, ce.data(), alt.data(), 3, n_reads, lq.data(), mems.data(),
                                         (int64_t)mems.size(), coords.data(), nc, rco.data(), cso.data(), seeds.data(),
                                         info.data(), nc, nc, &cu, &su);
      if (st) {
        printf("trial %d stage %d: %s\n", trial, stage, gb_last_error());
        return 1;
      }
      bool good = rco[0] == 0 && rco[n_reads] == cu && cso[0] == 0 && cso[cu] == su && cu <= nc && su <= nc;
      for (int r = 0; r < n_reads && good; ++r)
        for (int64_t c = rco[r]; c < rco[r + 1] && good; ++c) {
          good = cso[c + 1] > cso[c] && info[c].pos == seeds[cso[c]].rbeg;
          for (int64_t k = cso[c]; k < cso[c + 1] && good; ++k)
            good = seeds[k].qbeg >= 0 && seeds[k].len >= 1 && seeds[k].qbeg + seeds[k].len <= lq[r] &&
                   seeds[k].score == seeds[k].len;
        }
      if (!good) {
        printf("trial %d stage %d: malformed output\n", trial, stage);
        return 1;
      }
    }
    if (trial % 10 == 0)
      printf("trial %d: %lld coordinates -> %lld chains, %lld seeds\n", trial, (long long)nc, (long long)cu, (long long)su);
  }
  puts("ok");
  return 0;
}
