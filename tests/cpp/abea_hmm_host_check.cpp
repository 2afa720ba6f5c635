// abea_hmm_host_check.cpp -- stand-alone host program over the host path of gb_abea_hmm_score
// (csrc/bsw_abea_hmm.hip), meant to be built with the address and undefined-behaviour sanitizers on the host
// side (`make abea-hmm-sanitize` builds it together with the library's two source files and runs it). It
// touches no device: GB_ABEA_HOST=1 is set before the first call. Random models, reads and items: one k-mer
// to 256, one row to a few hundred, both strands with the item at either end of its read, all four flag
// values, bytes other than ACGMT, events_per_base == 1; a refused call. The outputs are checked for shape
// only (the fixture checks values). Prints "ok" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../include/gb_bsw_abea_hmm.h"

int main() {
  setenv("GB_ABEA_HOST", "1", 1);
  setenv("GB_ABEA_THREADS", "3", 1);
  std::mt19937_64 rng(17);
  std::normal_distribution<float> gauss(0.f, 1.f);
  std::vector<float> table(GB_ABEA_HMM_LOGSUM_TBL);
  if (gb_abea_hmm_logsum_table(table.data()) || !(table[0] > 0.693f && table[0] < 0.694f)) {
    puts("log-sum table");
    return 1;
  }
  const int kmers[] = {1, 2, 16, 17, 40, 64, 65, 129, 256};
  for (int trial = 0; trial < 30; ++trial) {
    std::vector<gb_abea_model> model(GB_ABEA_HMM_MODEL_SIZE);
    for (auto &m : model) {
      m.level_mean = 60.f + 60.f * (float)(rng() % 1000) / 1000.f;
      m.level_stdv = 1.f + (float)(rng() % 300) / 100.f;
      m.level_log_stdv = std::log(m.level_stdv);
    }
    const int n_reads = 1 + (int)(rng() % 6);
    std::string seqs;
    std::vector<float> events;
    std::vector<gb_abea_hmm_read> reads;
    std::vector<gb_abea_hmm_item> items;
    for (int r = 0; r < n_reads; ++r) {
      const int nk = kmers[rng() % 9], rows = 1 + (int)(rng() % (trial % 3 ? 40 : 400));
      const int lead = (int)(rng() % 3), tail = (int)(rng() % 3);
      gb_abea_hmm_read rd{};
      rd.event_off = (int64_t)events.size(), rd.n_events = lead + rows + tail;
      rd.scale = 1.f + 0.05f * gauss(rng), rd.shift = 3.f * gauss(rng), rd.var = 1.f + (float)(rng() % 100) / 200.f;
      rd.log_var = std::log(rd.var), rd.events_per_base = r % 3 ? 1.0 + (double)(rng() % 300) / 100.0 : 1.0;
      for (int i = 0; i < rd.n_events; ++i) events.push_back(90.f + 20.f * gauss(rng));
      reads.push_back(rd);
      for (int copy = 0; copy < 2; ++copy) {
        gb_abea_hmm_item it{};
        it.seq_off = (int64_t)seqs.size(), it.seq_len = nk + GB_ABEA_K - 1, it.read = r;
        it.rc = (uint8_t)(r & 1), it.flags = (uint8_t)(rng() % 4);
        it.event_start = it.rc ? lead + rows - 1 : lead, it.event_stop = it.rc ? lead : lead + rows - 1;
        for (int i = 0; i < it.seq_len; ++i) seqs.push_back(rng() % 40 ? "ACGMT"[rng() % 5] : 'N');
        items.push_back(it);
      }
    }
    std::vector<float> scores(items.size(), 777.f);
    int st = gb_abea_hmm_score(model.data(), seqs.data(), (int64_t)seqs.size(), events.data(), (int64_t)events.size(),
                               reads.data(), n_reads, items.data(), (int64_t)items.size(), scores.data());
    if (st) {
      printf("trial %d: %s\n", trial, gb_last_error());
      return 1;
    }
    for (size_t i = 0; i < scores.size(); ++i)
      if (std::isnan(scores[i]) || scores[i] > 0.f) {
        printf("trial %d: item %zu scores %g\n", trial, i, (double)scores[i]);
        return 1;
      }
    // one row past the read: refused, scores untouched
    std::vector<float> kept(items.size(), 777.f);
    gb_abea_hmm_item &last = items.back();
    (last.rc ? last.event_start : last.event_stop) = reads[(size_t)last.read].n_events;
    st = gb_abea_hmm_score(model.data(), seqs.data(), (int64_t)seqs.size(), events.data(), (int64_t)events.size(),
                           reads.data(), n_reads, items.data(), (int64_t)items.size(), kept.data());
    bool untouched = true;
    for (float v : kept) untouched = untouched && v == 777.f;
    if (st != GB_ERR_ARG || !untouched) {
      printf("trial %d: refusal: status %d, untouched %d\n", trial, st, (int)untouched);
      return 1;
    }
    if (trial % 6 == 0) printf("trial %d: %zu items, first score %g\n", trial, scores.size(), (double)scores[0]);
  }
  puts("ok");
  return 0;
}
