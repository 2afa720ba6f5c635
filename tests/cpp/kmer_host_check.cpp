// kmer_host_check.cpp -- stand-alone host program over the host path of gb_kmer_count and gb_kmer_index
// (csrc/fmi_kmer.hip), meant to be built with the address and undefined-behaviour sanitizers on the host side
// (`make kmer-sanitize` builds it together with the library's two source files and runs it). It touches no device:
// GB_KMER_HOST=1 is set before the first call. A stored case with the live reference's counts, the edge lengths at
// every k of the fixture, random read sets through every export with buffers of exactly the need, a homopolymer,
// every refusal and the empty inputs. Values are checked on the stored case, shapes elsewhere (the fixture checks
// values). Prints "ok" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/gb_fmi_kmer.h"

static int fail(const char *what, int trial) {
  printf("trial %d: %s: %s\n", trial, what, gb_last_error());
  return 1;
}

struct Set {
  std::vector<uint8_t> bytes;
  std::vector<int64_t> off{0};
  void add(const std::string &s) {
    bytes.insert(bytes.end(), s.begin(), s.end());
    off.push_back((int64_t)bytes.size());
  }
};

static int run(const Set &S, int k, int trial, int32_t min_freq, float select, int32_t tandem, float repeat) {
  gb_kmer_counts *h = nullptr;
  if (gb_kmer_count(k, S.bytes.data(), (int64_t)S.bytes.size(), S.off.data(), (int64_t)S.off.size() - 1, &h))
    return fail("gb_kmer_count", trial);
  int64_t nd = 0, occ = 0, over = 0, mx = 0, used = -1;
  if (gb_kmer_counts_stats(h, &nd, &occ, &over, &mx)) return fail("stats", trial);
  std::vector<uint64_t> codes((size_t)nd);
  std::vector<uint32_t> counts((size_t)nd), freq((size_t)nd + 2);
  if (gb_kmer_counts_export(h, codes.data(), counts.data(), nd, &used) || used != nd) return fail("export", trial);
  int64_t sum = 0;
  for (int64_t i = 0; i < nd; ++i) {
    sum += counts[(size_t)i];
    if (i && codes[(size_t)i] <= codes[(size_t)i - 1]) return fail("codes not ascending", trial);
  }
  if (sum != occ) return fail("counts do not add up", trial);
  std::vector<uint64_t> q(codes);
  q.push_back(~0ull), q.push_back(nd ? codes[0] + 1 : 0);
  if (gb_kmer_counts_freq(h, q.data(), (int64_t)q.size(), freq.data())) return fail("freq", trial);
  for (int64_t i = 0; i < nd; ++i)
    if (freq[(size_t)i] != counts[(size_t)i]) return fail("freq differs from counts", trial);
  std::vector<int64_t> hist((size_t)(trial % 7) + 1);
  if (gb_kmer_counts_hist(h, hist.data(), (int64_t)hist.size())) return fail("hist", trial);
  gb_kmer_idx *x = nullptr;
  if (gb_kmer_index(h, min_freq, select, tandem, repeat, &x)) return fail("gb_kmer_index", trial);
  int64_t nc = 0, ne = 0, nr = 0, rf = 0;
  if (gb_kmer_idx_stats(x, &nc, &ne, &nr, &rf)) return fail("idx stats", trial);
  std::vector<uint64_t> ic((size_t)nc), rep((size_t)nr);
  std::vector<int64_t> off((size_t)nc + 1), pos((size_t)ne);
  if (gb_kmer_idx_export(x, nc ? ic.data() : q.data(), off.data(), nc, pos.data(), ne, rep.data(), nr))
    return fail("idx export", trial);
  if (off[0] != 0 || off[(size_t)nc] != ne) return fail("offsets", trial);
  for (int64_t c = 0; c < nc; ++c)
    for (int64_t i = off[(size_t)c]; i < off[(size_t)c + 1]; ++i)
      if (pos[(size_t)i] < 0 || pos[(size_t)i] >= 2 * (int64_t)S.bytes.size() ||
          (i > off[(size_t)c] && pos[(size_t)i] <= pos[(size_t)i - 1]))
        return fail("positions", trial);
  gb_kmer_idx_free(x);
  gb_kmer_free(h);
  return 0;
}

int main() {
  setenv("GB_KMER_HOST", "1", 1);
  setenv("GB_KMER_THREADS", "3", 1);
  std::mt19937_64 rng(17);
  const char al[] = "ACGTacgt";
  {  // the stored case: live Flye gives {1: 1, 6: 2, 16: 1, 21: 1, 36: 1} at k = 3
    Set S;
    for (const char *r : {"ACGTTGCA", "ACG", "", "GGGA"}) S.add(r);
    gb_kmer_counts *h = nullptr;
    if (gb_kmer_count(3, S.bytes.data(), (int64_t)S.bytes.size(), S.off.data(), 4, &h)) return fail("stored", 0);
    uint64_t codes[5];
    uint32_t counts[5];
    int64_t used = 0;
    const uint64_t want_codes[5] = {1, 6, 16, 21, 36};
    const uint32_t want_counts[5] = {1, 2, 1, 1, 1};
    if (gb_kmer_counts_export(h, codes, counts, 5, &used) || used != 5 || memcmp(codes, want_codes, sizeof codes) ||
        memcmp(counts, want_counts, sizeof counts))
      return fail("stored case differs", 0);
    gb_kmer_free(h);
  }
  int trial = 1;
  for (int k : {1, 4, 8, 11, 12, 13, 16, 17, 21, 31}) {
    for (int rep = 0; rep < 3; ++rep, ++trial) {
      Set S;
      for (int len : {0, k - 1, k, k + 1, k + 2, 33 + k, 64, 65, 200 + (int)(rng() % 300)}) {
        std::string s((size_t)len, 'A');
        for (auto &c : s) c = al[rng() % (rep == 2 ? 2 : 8)];
        S.add(s);
        if (rng() % 2) S.add(s.substr(0, s.size() / 2) + s);  // repeated content
      }
      if (rep == 1) S.add(std::string(5000, 'T'));
      const int32_t tandem = rep == 0 ? 0 : rep == 1 ? 3 : 100;
      if (run(S, k, trial, 1 + rep % 2, rep ? 0.7f : 0.4f, tandem, rep == 2 ? 100.0f : 2.0f)) return 1;
    }
  }
  {  // refusals leave the handle pointer alone
    Set S;
    S.add("ACGTNACGT");
    gb_kmer_counts *h = (gb_kmer_counts *)0x10;
    if (gb_kmer_count(3, S.bytes.data(), 9, S.off.data(), 1, &h) != GB_ERR_ARG || h != (gb_kmer_counts *)0x10)
      return fail("bad byte accepted", trial);
    if (gb_kmer_count(32, S.bytes.data(), 4, S.off.data(), 0, &h) != GB_ERR_ARG) return fail("k = 32 accepted", trial);
    const int64_t bad[3] = {0, 5, 3};
    if (gb_kmer_count(3, S.bytes.data(), 9, bad, 2, &h) != GB_ERR_ARG) return fail("offsets accepted", trial);
    if (gb_kmer_count(3, nullptr, 0, nullptr, 0, &h)) return fail("empty", trial);
    gb_kmer_idx *x = nullptr;
    if (gb_kmer_index(h, 1, 1.5f, 0, 2.0f, &x) != GB_ERR_ARG) return fail("select rate accepted", trial);
    if (gb_kmer_index(h, 1, 0.4f, 0, 2.0f, &x)) return fail("empty index", trial);
    gb_kmer_idx_free(x);
    gb_kmer_free(h);
  }
  printf("ok\n");
  return 0;
}
