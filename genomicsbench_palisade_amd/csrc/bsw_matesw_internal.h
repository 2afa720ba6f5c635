// bsw_matesw_internal.h -- the seam between gb_bsw_mate_rescue's host bookkeeping and whatever answers its
// alignment requests: the device path of bsw_matesw.hip in the library, a table in
// tests/cpp/matesw_host_check.cpp.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/gb_bsw.h"

namespace gbms {

struct Req {  // one orientation of one anchor, 24 B: all the device needs besides the per-call tables
  int64_t rb;           // the anchor's rb
  int32_t rid, r, read; // the anchor's rid; orientation 0..3 (FF, FR, RF, RR); the mate's read index
  int32_t pad;
};

struct Out {  // 40 B
  int64_t rb, re;
  int32_t qb, qe, score, csub, seedcov;
  int32_t flags;  // bit 0: the alignment ran (mem_matesw's ++n); bit 1: it gave a region
};

struct Aligner {
  virtual ~Aligner() = default;
  // answers req[0 .. n) of one round into out[0 .. n); a non-zero gb_status ends the call
  virtual int run(const Req *req, int64_t n, Out *out) = 0;
};

struct Rescue {  // a validated call
  gb_bsw_pe_opt opt;
  struct gb_bsw_pestat pes[4];
  int64_t l_pac = 0, n_reads = 0;
  const int64_t *reg_off = nullptr;
  const gb_bsw_alnreg *regs = nullptr;
  std::vector<std::vector<gb_bsw_alnreg>> lists;  // per read, the result
  std::vector<int32_t> n_sw;                      // per read as the anchor side
  double host_ms = 0.;
  int32_t rounds = 0;
  int64_t requests = 0;
};

// The rounds: anchors, the skip test, the requests, and per answer the sorted insertion and the dedup.
int rescue_rounds(Rescue &C, Aligner &A);

}  // namespace gbms
