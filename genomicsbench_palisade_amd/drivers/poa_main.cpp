// poa_main.cpp -- bin/poa: the poa benchmark's command line (benchmarks/poa/msa_spoa_omp.cpp) on gb_poa_consensus.
//
//   poa -s input.fasta [-t threads] [-m match] [-x mismatch] [-o open1,open2] [-e ext1,ext2] [-n ignored]
//
// Input: a header line per read, whose second character is '0' for the first read of a window, then the read on
// one line. Output, in input order, is the reference's PRINT_OUTPUT form: ">Consensus_sequence" and the string
// per window. As in the reference, the engine's (g, e, q, c) are -(open1 + ext1), -ext1, -(open2 + ext2), -ext2.
// A single-value -o or -e is refused (the reference's switch falls through for them).
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/gb_bsw_poa.h"

static void help() {
  fprintf(stderr,
          "usage: poa -s input.fasta -t <num_threads> > cons.fasta\n"
          "    -m <int>      score for matching bases (default 2)\n"
          "    -x <int>      penalty for mismatching bases (default 4)\n"
          "    -o <int,int>  gap opening penalties (default 4,24)\n"
          "    -e <int,int>  gap extension penalties (default 2,1)\n"
          "    -s <file>     the input sequence set (default seq.fa)\n"
          "    -n <int>      ignored\n"
          "    -t <int>      host threads of the graph update (default 1)\n");
}

static bool two_values(const char *arg, long *a, long *b) {
  char *s = nullptr;
  *a = strtol(arg, &s, 10);
  if (s == arg || *s != ',') return false;
  const char *t = s + 1;
  *b = strtol(t, &s, 10);
  return s != t && *s == 0;
}

int main(int argc, char **argv) {
  std::string seq_file = "seq.fa";
  long m = 2, x = 4, o1 = 4, o2 = 24, e1 = 2, e2 = 1;
  int threads = 1;
  if (argc == 1) {
    help();
    return 1;
  }
  int opt;
  while ((opt = getopt(argc, argv, "m:x:o:n:e:s:t:h")) != -1) {
    switch (opt) {
      case 'm': m = atol(optarg); break;
      case 'x': x = atol(optarg); break;
      case 'o':
        if (!two_values(optarg, &o1, &o2)) {
          fprintf(stderr, "poa: -o takes two values, open1,open2 (got '%s')\n", optarg);
          return 1;
        }
        break;
      case 'e':
        if (!two_values(optarg, &e1, &e2)) {
          fprintf(stderr, "poa: -e takes two values, ext1,ext2 (got '%s')\n", optarg);
          return 1;
        }
        break;
      case 'n': break;
      case 's': seq_file = optarg; break;
      case 't': threads = atoi(optarg); break;
      case 'h': help(); return 0;
      default: help(); return 1;
    }
  }
  std::ifstream in(seq_file);
  if (!in.is_open()) {
    fprintf(stderr, "poa: cannot open %s\n", seq_file.c_str());
    return 1;
  }
  std::vector<int64_t> win_off, seq_off{0};
  std::vector<uint8_t> bytes;
  std::string header, seq;
  while (std::getline(in, header)) {
    if (header.empty()) continue;
    if (!std::getline(in, seq)) break;
    if (!seq.empty() && seq.back() == '\r') seq.pop_back();
    if ((header.size() > 1 && header[1] == '0') || win_off.empty()) win_off.push_back((int64_t)seq_off.size() - 1);
    bytes.insert(bytes.end(), seq.begin(), seq.end());
    seq_off.push_back((int64_t)bytes.size());
  }
  const int64_t n_seqs = (int64_t)seq_off.size() - 1, n_windows = (int64_t)win_off.size();
  win_off.push_back(n_seqs);
  auto i8 = [](long v) { return (int8_t)v; };
  const gb_poa_params P{i8(m), i8(-x), i8(-(o1 + e1)), i8(-e1), i8(-(o2 + e2)), i8(-e2), GB_POA_NW, 0};
  if (threads >= 1) setenv("GB_POA_THREADS", std::to_string(threads).c_str(), 1);
  std::vector<uint8_t> cons(bytes.size() + 1);
  std::vector<int64_t> cons_off((size_t)n_windows + 1);
  std::vector<int32_t> nodes((size_t)n_windows + 1);
  int64_t used = 0, done = 0;
  if (gb_poa_consensus(&P, win_off.data(), n_windows, seq_off.data(), n_seqs, bytes.data(), (int64_t)bytes.size(), nullptr,
                       cons.data(), (int64_t)bytes.size(), cons_off.data(), &used, nodes.data(), &done)) {
    fprintf(stderr, "poa: %s\n", gb_last_error());
    return 1;
  }
  for (int64_t w = 0; w < n_windows; ++w) {
    printf(">Consensus_sequence\n");
    fwrite(cons.data() + cons_off[(size_t)w], 1, (size_t)(cons_off[(size_t)w + 1] - cons_off[(size_t)w]), stdout);
    printf("\n");
  }
  float fill_ms = 0, walk_ms = 0, host_ms = 0;
  int64_t cells = 0;
  if (!gb_poa_timing(&fill_ms, &walk_ms, &host_ms, &cells))
    fprintf(stderr, "Number of windows: %lld, alignments: %lld, cells: %lld, fill %.2f ms, walk %.2f ms, host %.2f ms\n",
            (long long)n_windows, (long long)done, (long long)cells, fill_ms, walk_ms, host_ms);
  return 0;
}
