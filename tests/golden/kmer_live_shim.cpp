// kmer_live_shim.cpp -- a stand-alone program over the unmodified Flye sources (vertex_index.cpp,
// sequence_container.cpp, sequence.cpp), built by make_kmer_golden.py in a temporary directory and compiled with
// -fno-access-control so that it can read VertexIndex's counter and repetitive frequency. One process per set: the
// reference sizes its flat table once per process.
//
//   kmer_live_shim IN OUT
// IN:  int64 k, flat, n_reads, n_queries, n_index_queries (0: no index), min_freq, tandem_freq;
//      float select_rate, repeat_rate; per read int64 length and its bytes; n_queries uint64 codes.
// OUT: int64 getKmerNum; double seconds of the count itself; n_queries uint64 getFreq; then, with an index: int64
//      repetitive frequency and, for each of the first n_index_queries codes, uint8 isRepetitive, int64 kmerFreq
//      and that many int64 global positions in iterKmerPos order.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sequence/vertex_index.h"

static void rd(FILE *f, void *p, size_t n) {
  if (n && fread(p, 1, n, f) != n) {
    fprintf(stderr, "kmer_live_shim: short input\n");
    exit(2);
  }
}
template <typename T>
static void wr(FILE *f, T v) {
  fwrite(&v, sizeof v, 1, f);
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int64_t h[7];
  float rates[2];
  rd(in, h, sizeof h);
  rd(in, rates, sizeof rates);
  const int64_t k = h[0], flat = h[1], n_reads = h[2], n_queries = h[3], n_index = h[4];
  Parameters::get().kmerSize = (size_t)k;
  Parameters::get().numThreads = 1;
  Parameters::get().minimumOverlap = 0;
  Parameters::get().unevenCoverage = true;
  Config::addParameters("repeat_kmer_rate=" + std::to_string(rates[1]));
  if ((float)Config::get("repeat_kmer_rate") != rates[1]) {
    fprintf(stderr, "kmer_live_shim: repeat rate %.9g does not survive the text form\n", rates[1]);
    return 3;
  }
  SequenceContainer sc;
  for (int64_t i = 0; i < n_reads; ++i) {
    int64_t len;
    rd(in, &len, 8);
    std::string s((size_t)len, 'A');
    rd(in, &s[0], (size_t)len);
    if (len == 0)
      sc.addSequence(DnaSequence(), "r" + std::to_string(i));  // the string constructor underflows on ""
    else
      sc.addSequence(DnaSequence(s), "r" + std::to_string(i));
  }
  sc.buildPositionIndex();
  std::vector<uint64_t> q((size_t)n_queries);
  rd(in, q.data(), 8 * q.size());

  if (!n_index) {
    KmerCounter kc(sc);
    const auto t0 = std::chrono::steady_clock::now();
    kc.count(flat != 0);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    wr<int64_t>(out, (int64_t)kc.getKmerNum());
    wr<double>(out, secs);
    for (uint64_t c : q) wr<uint64_t>(out, (uint64_t)kc.getFreq(Kmer(c)));
  } else {
    VertexIndex vi(sc, 1);
    const auto t0 = std::chrono::steady_clock::now();
    vi.countKmers();
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    wr<int64_t>(out, (int64_t)vi._kmerCounter.getKmerNum());
    wr<double>(out, secs);
    for (uint64_t c : q) wr<uint64_t>(out, (uint64_t)vi._kmerCounter.getFreq(Kmer(c)));
    vi.buildIndexUnevenCoverage((int)h[5], rates[0], (int)h[6]);
    wr<int64_t>(out, (int64_t)vi._repetitiveFrequency);
    for (int64_t i = 0; i < n_index; ++i) {
      const Kmer km(q[(size_t)i]);
      const int64_t size = (int64_t)vi.kmerFreq(km);
      wr<uint8_t>(out, vi.isRepetitive(km) ? 1 : 0);
      wr<int64_t>(out, size);
      if (size)
        for (const auto &rp : vi.iterKmerPos(km)) wr<int64_t>(out, (int64_t)sc.globalPosition(rp.readId, rp.position));
    }
  }
  fclose(out);
  return 0;
}
