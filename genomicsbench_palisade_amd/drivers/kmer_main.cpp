// kmer_main.cpp -- CLI for the kmer-cnt benchmark (benchmarks/kmer-cnt/kmer_cnt.cpp, the counting step):
//   kmer-cnt --reads a.fasta[,b.fastq.gz] --kmer K [--min-read N] [--min-ovlp N]
// Reads FASTA or FASTQ, plain or gz, keeps the reads longer than max(min-read, min-ovlp) (kmer_cnt.cpp:219,
// sequence_container.cpp:106; defaults 0 and 5000), counts the canonical k-mers through gb_kmer_count and prints the
// two lines KmerCounter::count logs ("Hash size: N" is the number of codes counted 16 times or more, "Total k-mers N"
// the distinct codes) and the k-mer histogram the reference keeps, one "frequency<TAB>codes" line per frequency
// that occurs. Times go to stderr.
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gb_fmi_kmer.h"

static void check(int st, const char *what) {
  if (st) {
    fprintf(stderr, "[gb kmer-cnt] %s failed (%d): %s\n", what, st, gb_last_error());
    exit(EXIT_FAILURE);
  }
}

// minimal FASTA/FASTQ reader over zlib (plain files pass through gzread unchanged)
struct Reader {
  gzFile f;
  std::vector<char> buf = std::vector<char>(1 << 20);
  std::string pending;
  bool has_pending = false;
  bool line(std::string &s) {
    if (has_pending) {
      s.swap(pending);
      has_pending = false;
      return true;
    }
    s.clear();
    while (gzgets(f, buf.data(), (int)buf.size())) {
      s += buf.data();
      if (!s.empty() && s.back() == '\n') break;
    }
    if (s.empty()) return false;
    while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
    return true;
  }
  void unread(std::string &s) {
    pending.swap(s);
    has_pending = true;
  }
};

static int usage() {
  fprintf(stderr, "Usage: kmer-cnt --reads path[,path..] --kmer size [--min-read length] [--min-ovlp size]\n");
  return 1;
}

int main(int argc, char **argv) {
  std::string reads_arg;
  int k = 0, min_read = 0, min_ovlp = 5000;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (i + 1 >= argc) return usage();
    if (a == "--reads") reads_arg = argv[++i];
    else if (a == "--kmer") k = atoi(argv[++i]);
    else if (a == "--min-read") min_read = atoi(argv[++i]);
    else if (a == "--min-ovlp") min_ovlp = atoi(argv[++i]);
    else return usage();
  }
  if (reads_arg.empty() || k <= 0) return usage();
  const size_t min_len = (size_t)std::max(0, std::max(min_read, min_ovlp));

  const auto t_read = std::chrono::steady_clock::now();
  std::vector<uint8_t> bytes;
  std::vector<int64_t> off(1, 0);
  for (size_t b = 0; b <= reads_arg.size();) {
    const size_t e = std::min(reads_arg.find(',', b), reads_arg.size());
    const std::string path = reads_arg.substr(b, e - b);
    b = e + 1;
    if (path.empty()) continue;
    Reader rd;
    rd.f = gzopen(path.c_str(), "r");
    if (!rd.f) {
      fprintf(stderr, "[gb kmer-cnt] cannot open %s\n", path.c_str());
      return 1;
    }
    std::string l, s;
    while (rd.line(l)) {
      if (l.empty()) continue;
      const char tag = l[0];
      if (tag != '@' && tag != '>') {
        fprintf(stderr, "[gb kmer-cnt] unexpected line in %s: %.40s\n", path.c_str(), l.c_str());
        return 1;
      }
      s.clear();
      while (rd.line(l)) {
        if (l.empty()) continue;
        if (l[0] == '>' || (tag == '@' && l[0] == '+')) {
          if (l[0] == '>') rd.unread(l);
          break;
        }
        s += l;
      }
      if (tag == '@') {  // skip the quality lines (same length as the sequence)
        size_t q = 0;
        while (q < s.size() && rd.line(l)) q += l.size();
      }
      if (s.size() > min_len) {  // strictly longer, as the reference's loadFromFile
        bytes.insert(bytes.end(), s.begin(), s.end());
        off.push_back((int64_t)bytes.size());
      }
    }
    gzclose(rd.f);
  }
  const double read_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_read).count();

  const char *host = getenv("GB_KMER_HOST");
  if (!(host && *host == '1')) {
    const char *dev = getenv("GB_DEVICE");
    check(gb_set_device(dev ? atoi(dev) : 0), "gb_set_device");
  }
  const auto t0 = std::chrono::steady_clock::now();
  gb_kmer_counts *h = nullptr;
  check(gb_kmer_count(k, bytes.data(), (int64_t)bytes.size(), off.data(), (int64_t)off.size() - 1, &h), "gb_kmer_count");
  const double count_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  int64_t n_distinct = 0, n_occ = 0, n_over15 = 0, max_count = 0;
  check(gb_kmer_counts_stats(h, &n_distinct, &n_occ, &n_over15, &max_count), "gb_kmer_counts_stats");
  std::vector<int64_t> hist((size_t)max_count + 2);
  check(gb_kmer_counts_hist(h, hist.data(), (int64_t)hist.size()), "gb_kmer_counts_hist");
  printf("Hash size: %lld\n", (long long)n_over15);
  printf("Total k-mers %lld\n", (long long)n_distinct);
  for (int64_t f = 1; f <= max_count; ++f)
    if (hist[(size_t)f]) printf("%lld\t%lld\n", (long long)f, (long long)hist[(size_t)f]);
  fprintf(stderr, "[gb kmer-cnt] %lld reads, %lld k-mer occurrences; read %.3f s, count %.3f s\n",
          (long long)off.size() - 1, (long long)n_occ, read_s, count_s);
  gb_kmer_free(h);
  return 0;
}
