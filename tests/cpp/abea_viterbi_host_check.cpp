// abea_viterbi_host_check.cpp -- stand-alone host program over the host path of gb_abea_hmm_align
// (csrc/bsw_abea_viterbi.hip), meant to be built with the address and undefined-behaviour sanitizers on the host
// side (`make abea-viterbi-sanitize` builds it together with the library's two source files and runs it). It
// touches no device: GB_ABEA_HOST=1 is set before the first call. Random models, reads and items: one k-mer
// to 256, two rows to a few hundred, both strands with the item at either end of its read, bytes other than
// ACGT, events_per_base == 1; a path buffer of exactly the need, one of one record less, and a refused item.
// The outputs are checked for shape only (the fixture checks values). Prints "ok" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../include/gb_bsw_abea_viterbi.h"

int main() {
  setenv("GB_ABEA_HOST", "1", 1);
  setenv("GB_ABEA_THREADS", "3", 1);
  std::mt19937_64 rng(23);
  std::normal_distribution<float> gauss(0.f, 1.f);
  const int kmers[] = {1, 2, 16, 17, 40, 64, 65, 129, 256};
  for (int trial = 0; trial < 30; ++trial) {
    std::vector<gb_abea_model> model(GB_ABEA_VITERBI_MODEL_SIZE);
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
    int64_t need = 0;
    for (int r = 0; r < n_reads; ++r) {
      const int nk = kmers[rng() % 9], rows = 3 + (int)(rng() % (trial % 3 ? 40 : 400));
      const int lead = (int)(rng() % 3), tail = (int)(rng() % 3);
      gb_abea_hmm_read rd{};
      rd.event_off = (int64_t)events.size(), rd.n_events = lead + rows + tail;
      rd.scale = 1.f + 0.05f * gauss(rng), rd.shift = 3.f * gauss(rng), rd.var = 1.f + (float)(rng() % 100) / 200.f;
      rd.log_var = std::log(rd.var), rd.events_per_base = r % 3 ? 1.0 + (double)(rng() % 300) / 100.0 : 1.0;
      for (int i = 0; i < rd.n_events; ++i) events.push_back(90.f + 20.f * gauss(rng));
      reads.push_back(rd);
      for (int copy = 0; copy < 2; ++copy) {  // the whole window, and its first two rows
        gb_abea_hmm_item it{};
        const int n = copy ? 2 : rows;
        it.seq_off = (int64_t)seqs.size(), it.seq_len = nk + GB_ABEA_K - 1 + copy, it.read = r, it.rc = (uint8_t)(r & 1);
        it.event_start = it.rc ? lead + rows - 1 : lead, it.event_stop = it.rc ? it.event_start - (n - 1) : lead + n - 1;
        for (int i = 0; i < it.seq_len; ++i) seqs.push_back(rng() % 40 ? "ACGT"[rng() % 4] : 'N');
        if (it.seq_len - GB_ABEA_K + 1 > GB_ABEA_HMM_MAX_KMERS) it.seq_len -= 1;
        items.push_back(it);
        need += n + (it.seq_len - GB_ABEA_K + 1) - 1;
      }
    }
    const int64_t n_items = (int64_t)items.size();
    std::vector<gb_abea_path_rec> path((size_t)need);  // exactly the need: a record past it is the sanitizer's to find
    std::vector<int64_t> off((size_t)n_items + 1, -5);
    int64_t used = -1;
    int st = gb_abea_hmm_align(model.data(), seqs.data(), (int64_t)seqs.size(), events.data(), (int64_t)events.size(),
                               reads.data(), n_reads, items.data(), n_items, path.data(), need, off.data(), &used);
    if (st) {
      printf("trial %d: %s\n", trial, gb_last_error());
      return 1;
    }
    if (off[0] != 0 || off[(size_t)n_items] != used || used > need) {
      printf("trial %d: offsets\n", trial);
      return 1;
    }
    for (int64_t i = 0; i < n_items; ++i) {
      const gb_abea_hmm_item &it = items[(size_t)i];
      const gb_abea_path_rec *p = path.data() + off[(size_t)i];
      const int64_t len = off[(size_t)i + 1] - off[(size_t)i], rows = std::abs(it.event_stop - it.event_start) + 1;
      int64_t skips = 0;
      for (int64_t j = 0; j < len; ++j) skips += p[j].state == 'K';
      if (len != rows + skips || p[0].event_idx != it.event_start || p[0].kmer_idx != 0 || p[0].state != 'M' ||
          p[len - 1].event_idx != it.event_stop || p[len - 1].kmer_idx != it.seq_len - GB_ABEA_K || p[len - 1].state != 'M' ||
          !std::isfinite(p[len - 1].l_fm)) {
        printf("trial %d: item %lld: %lld records for %lld rows and %lld skips\n", trial, (long long)i, (long long)len,
               (long long)rows, (long long)skips);
        return 1;
      }
    }
    // one record short: refused with the need, nothing else written
    std::vector<int64_t> kept((size_t)n_items + 1, -5);
    int64_t short_used = -1;
    st = gb_abea_hmm_align(model.data(), seqs.data(), (int64_t)seqs.size(), events.data(), (int64_t)events.size(),
                           reads.data(), n_reads, items.data(), n_items, path.data(), need - 1, kept.data(), &short_used);
    bool untouched = true;
    for (int64_t v : kept) untouched = untouched && v == -5;
    if (st != GB_ERR_ARG || short_used != need || !untouched) {
      printf("trial %d: short buffer: status %d, need %lld of %lld\n", trial, st, (long long)short_used, (long long)need);
      return 1;
    }
    // one row past the read: refused, outputs untouched
    gb_abea_hmm_item &last = items.front();
    (last.rc ? last.event_start : last.event_stop) = reads[(size_t)last.read].n_events;
    short_used = -1;
    st = gb_abea_hmm_align(model.data(), seqs.data(), (int64_t)seqs.size(), events.data(), (int64_t)events.size(),
                           reads.data(), n_reads, items.data(), n_items, path.data(), need, kept.data(), &short_used);
    for (int64_t v : kept) untouched = untouched && v == -5;
    if (st != GB_ERR_ARG || short_used != -1 || !untouched) {
      printf("trial %d: refusal: status %d, untouched %d\n", trial, st, (int)untouched);
      return 1;
    }
    if (trial % 6 == 0) printf("trial %d: %lld items, %lld records of at most %lld\n", trial, (long long)n_items,
                               (long long)used, (long long)need);
  }
  puts("ok");
  return 0;
}
