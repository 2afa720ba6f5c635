// abea_host_check.cpp -- stand-alone host program over the host path of gb_abea_align (csrc/bsw_abea.hip),
// meant to be built with the address and undefined-behaviour sanitizers on the host side (`make
// abea-sanitize` builds it together with the library's two source files and runs it). It touches no
// device: GB_ABEA_HOST=1 is set before the first call. Random models and reads: tiny ones, ones with far
// more events than k-mers and the reverse, noisy ones and ones with bases other than ACGT; a call with a
// pair_cap that is too small; a lowered GB_ABEA_WS_BYTES so that calls are cut into chunks. The outputs are
// checked for shape only (the fixture checks values). Prints "ok" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../include/gb_bsw_abea.h"

int main() {
  setenv("GB_ABEA_HOST", "1", 1);
  setenv("GB_ABEA_THREADS", "3", 1);
  std::mt19937_64 rng(11);
  std::normal_distribution<float> gauss(0.f, 1.f);
  for (int trial = 0; trial < 40; ++trial) {
    setenv("GB_ABEA_WS_BYTES", trial % 2 ? "200000" : "1073741824", 1);
    std::vector<gb_abea_model> model(GB_ABEA_MODEL_SIZE);
    for (auto &m : model) {
      m.level_mean = 60.f + 60.f * (float)(rng() % 1000) / 1000.f;
      m.level_stdv = 1.f + (float)(rng() % 300) / 100.f;
      m.level_log_stdv = std::log(m.level_stdv);
    }
    const int n_reads = 1 + (int)(rng() % 12);
    std::string seqs;
    std::vector<float> events;
    std::vector<gb_abea_read> reads;
    int64_t cap = 0;
    for (int r = 0; r < n_reads; ++r) {
      const int kind = (int)(rng() % 4);
      const int len = kind == 0 ? 6 + (int)(rng() % 7) : 20 + (int)(rng() % 600);
      const double ratio = kind == 1 ? 0.4 : kind == 2 ? 6.0 : 1.6;
      const float noise = trial % 5 == 4 ? 4.f : 0.7f;
      gb_abea_read rd{};
      rd.seq_off = (int64_t)seqs.size(), rd.event_off = (int64_t)events.size(), rd.seq_len = len;
      for (int i = 0; i < len; ++i) seqs.push_back(rng() % 50 ? "ACGT"[rng() % 4] : 'N');
      const int n_kmers = len - GB_ABEA_K + 1;
      const int n_events = kind == 0 ? 1 + (int)(rng() % 8) : 1 + (int)(n_kmers * ratio);
      rd.n_events = n_events, rd.scale = 1.f + 0.05f * gauss(rng), rd.shift = 3.f * gauss(rng);
      for (int i = 0; i < n_events; ++i) {
        const int k = (int)((int64_t)i * n_kmers / n_events);
        int rank = 0;
        for (int j = 0; j < GB_ABEA_K; ++j) {
          const char b = seqs[(size_t)rd.seq_off + k + j];
          rank = rank * 4 + (b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 0);
        }
        events.push_back(rd.scale * model[(size_t)rank].level_mean + rd.shift +
                         noise * model[(size_t)rank].level_stdv * gauss(rng));
      }
      cap += n_events + n_kmers;
      reads.push_back(rd);
    }
    std::vector<gb_abea_pair> pairs((size_t)cap);
    std::vector<int64_t> off((size_t)n_reads + 1);
    std::vector<gb_abea_stat> stats((size_t)n_reads);
    int64_t used = -1;
    int st = gb_abea_align(model.data(), seqs.data(), (int64_t)seqs.size(), events.data(), (int64_t)events.size(),
                           reads.data(), n_reads, pairs.data(), cap, off.data(), stats.data(), &used);
    if (st) {
      printf("trial %d: %s\n", trial, gb_last_error());
      return 1;
    }
    bool good = off[0] == 0 && off[(size_t)n_reads] == used && used <= cap;
    for (int r = 0; r < n_reads && good; ++r) {
      const gb_abea_stat &s = stats[(size_t)r];
      const int n_kmers = reads[(size_t)r].seq_len - GB_ABEA_K + 1;
      good = off[(size_t)r + 1] - off[(size_t)r] == s.n_raw && (s.n_pairs == 0 || s.n_pairs == s.n_raw) &&
             (s.no_end_cell ? s.n_raw == 0 : s.n_raw >= 1);
      for (int64_t k = off[(size_t)r]; k < off[(size_t)r + 1] && good; ++k) {
        good = pairs[(size_t)k].ref_pos >= 0 && pairs[(size_t)k].ref_pos < n_kmers && pairs[(size_t)k].read_pos >= 0 &&
               pairs[(size_t)k].read_pos < reads[(size_t)r].n_events;
        if (k > off[(size_t)r])  // both coordinates rise, by at most one
          good = good && pairs[(size_t)k].ref_pos - pairs[(size_t)k - 1].ref_pos >= 0 &&
                 pairs[(size_t)k].ref_pos - pairs[(size_t)k - 1].ref_pos <= 1 &&
                 pairs[(size_t)k].read_pos - pairs[(size_t)k - 1].read_pos >= 0 &&
                 pairs[(size_t)k].read_pos - pairs[(size_t)k - 1].read_pos <= 1;
      }
    }
    if (!good) {
      printf("trial %d: malformed output\n", trial);
      return 1;
    }
    if (used > 0) {  // one pair short: refused, the need reported
      int64_t need = -1;
      st = gb_abea_align(model.data(), seqs.data(), (int64_t)seqs.size(), events.data(), (int64_t)events.size(),
                         reads.data(), n_reads, pairs.data(), used - 1, off.data(), stats.data(), &need);
      if (st != GB_ERR_ARG || need != used) {
        printf("trial %d: pair_cap protocol: status %d, need %lld of %lld\n", trial, st, (long long)need, (long long)used);
        return 1;
      }
    }
    if (trial % 8 == 0) printf("trial %d: %d reads -> %lld pairs\n", trial, n_reads, (long long)used);
  }
  puts("ok");
  return 0;
}
