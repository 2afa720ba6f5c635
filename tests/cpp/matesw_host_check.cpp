// matesw_host_check.cpp -- stand-alone host program over the bookkeeping of gb_bsw_mate_rescue
// (csrc/bsw_matesw.hip: the anchors, the skip test, the sorted insertion and the dedup without mem_patch_reg),
// meant to be built with the address and undefined-behaviour sanitizers on the host side (`make
// matesw-sanitize` builds it together with the library's source files it needs and runs it). The alignment
// results come from a table: a hash of the request decides whether it ran and what region it gave, so no device
// is touched. One hand-made pair is checked for its values, random pairs for shape (the fixture checks
// values): regions inside their read, counts within the bound the header gives, n_sw equal to the answers
// that ran. gb_bsw_pestat and the public call with every orientation failed run too. Prints "ok", returns 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../genomicsbench_palisade_amd/csrc/bsw_matesw_internal.h"
#include "../../include/gb_bsw.h"

static gb_bsw_alnreg reg(int64_t rb, int len, int rid, int score) {
  gb_bsw_alnreg a;
  memset(&a, 0, sizeof(a));
  a.rb = rb, a.re = rb + len, a.qb = 0, a.qe = len, a.rid = rid;
  a.score = a.truesc = score, a.seedcov = len / 2 + 1, a.seedlen0 = 19, a.n_comp = 1;
  return a;
}

static uint64_t mix(uint64_t x) {
  x ^= x >> 33, x *= 0xff51afd7ed558ccdull, x ^= x >> 33, x *= 0xc4ceb9fe1a85ec53ull, x ^= x >> 33;
  return x;
}

struct Table : gbms::Aligner {
  int64_t l_pac = 0, ran = 0, asked = 0;
  const int32_t *l_query = nullptr;
  bool fixed = false;  // the hand-made pair: every request gives the same region
  int run(const gbms::Req *req, int64_t n, gbms::Out *out) override {
    for (int64_t k = 0; k < n; ++k) {
      const gbms::Req &q = req[k];
      gbms::Out o;
      memset(&o, 0, sizeof(o));
      const uint64_t h = mix((uint64_t)q.rb * 4 + (uint64_t)q.r + ((uint64_t)q.read << 40));
      const int lq = l_query[q.read];
      ++asked;
      if (fixed) {
        o.rb = 7000, o.re = 7100, o.qb = 0, o.qe = 100, o.score = 90, o.csub = 20, o.seedcov = 50, o.flags = 3;
      } else if (h % 4) {
        o.flags = 1;
        if (h % 3) {
          const int ql = 1 + (int)((h >> 8) % (uint64_t)lq), qb = (int)((h >> 20) % (uint64_t)(lq - ql + 1));
          const bool rev = (h >> 30) & 1;
          const int64_t rb = (int64_t)((h >> 32) % (uint64_t)(l_pac - 300)) + (rev ? l_pac : 0);
          o.rb = rb, o.re = rb + ql + (int64_t)((h >> 4) % 3), o.qb = qb, o.qe = qb + ql;
          o.score = 19 + (int)((h >> 12) % 5) * 10, o.csub = (int)((h >> 16) % 30), o.seedcov = ql >> 1, o.flags = 3;
        }
      }
      ran += o.flags & 1;
      out[k] = o;
    }
    return 0;
  }
};

int main() {
  std::mt19937_64 rng(11);
  const int64_t l_pac = 30000;
  for (int trial = 0; trial < 10; ++trial) {
    gbms::Rescue C;
    gb_bsw_pe_default_opt(&C.opt);
    if (trial % 3 == 1) C.opt.max_matesw = 2, C.opt.mask_level_redun = 0.5f;
    if (trial % 3 == 2) C.opt.pen_unpaired = 0;
    for (int r = 0; r < 4; ++r) {
      C.pes[r].low = 100, C.pes[r].high = 400, C.pes[r].failed = trial % 2 && r != 1, C.pes[r].pad = 0;
      C.pes[r].avg = 250., C.pes[r].std = 50.;
    }
    std::vector<int64_t> off(1, 0);
    std::vector<int32_t> lq;
    std::vector<gb_bsw_alnreg> regs;
    // pair 0: read 0 has two anchors at one place, read 1 no region. With FR alone the first anchor's rescue
    // makes the pair consistent and the second call is skipped.
    lq.push_back(100), lq.push_back(100);
    regs.push_back(reg(2 * l_pac - 7100 - 250, 100, 0, 100));
    regs.push_back(reg(2 * l_pac - 7100 - 249, 100, 0, 95));
    off.push_back(2), off.push_back(2);
    const int n_rand = 300 + (int)(rng() % 300);  // more than 256 tasks: several threads
    for (int p = 0; p < n_rand; ++p)
      for (int i = 0; i < 2; ++i) {
        const int l = 30 + (int)(rng() % 220);
        lq.push_back(l);
        const int nr = (int)(rng() % 5 ? rng() % 4 : 40 + rng() % 30);
        int score = l;
        for (int k = 0; k < nr; ++k) {
          const bool rev = rng() & 1;
          regs.push_back(reg((int64_t)(rng() % (uint64_t)(l_pac - 300)) + (rev ? l_pac : 0), l, 0, score));
          score -= (int)(rng() % 9);
          if (score < 1) score = 1;
        }
        off.push_back((int64_t)regs.size());
      }
    const int64_t n_reads = (int64_t)lq.size();
    C.l_pac = l_pac, C.n_reads = n_reads, C.reg_off = off.data(), C.regs = regs.data();
    Table T;
    T.l_pac = l_pac, T.l_query = lq.data();
    // the hand-made pair alone first
    {
      gbms::Rescue H = C;
      H.n_reads = 2;
      Table F;
      F.l_pac = l_pac, F.l_query = lq.data(), F.fixed = true;
      if (gbms::rescue_rounds(H, F)) {
        printf("trial %d: %s\n", trial, gb_last_error());
        return 1;
      }
      const int open = trial % 2 ? 1 : 4;
      // FR alone: the first anchor sends one request and gets the region, which lies at a proper FR distance
      // from the second anchor too, so that call is skipped. All four open: each call still asks for the
      // orientations in which the mate has no region, and only the first region's values are checked.
      if (H.lists[1].empty() || H.lists[1][0].score != 90 || H.lists[1][0].secondary != -1 || H.lists[0].size() != 2 ||
          (open == 1 && (F.asked != 1 || H.lists[1].size() != 1 || H.n_sw[0] != 1))) {
        printf("trial %d: the hand-made pair gave %zu regions after %lld requests\n", trial, H.lists[1].size(),
               (long long)F.asked);
        return 1;
      }
    }
    if (gbms::rescue_rounds(C, T)) {
      printf("trial %d: %s\n", trial, gb_last_error());
      return 1;
    }
    int64_t n_sw = 0, total = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
      const int64_t n = off[(size_t)r + 1] - off[(size_t)r], nm = off[(size_t)(r ^ 1) + 1] - off[(size_t)(r ^ 1)];
      const std::vector<gb_bsw_alnreg> &a = C.lists[(size_t)r];
      n_sw += C.n_sw[(size_t)r];
      total += (int64_t)a.size();
      bool good = (int64_t)a.size() <= n + 4 * std::min<int64_t>(nm, C.opt.max_matesw);
      for (const gb_bsw_alnreg &g : a) good = good && g.qb >= 0 && g.qb < g.qe && g.qe <= lq[(size_t)r] && g.rb < g.re;
      if (!good) {
        printf("trial %d read %lld: malformed list of %zu regions\n", trial, (long long)r, a.size());
        return 1;
      }
    }
    if (n_sw != T.ran || C.requests != T.asked) {
      printf("trial %d: n_sw %lld, ran %lld, requests %lld, asked %lld\n", trial, (long long)n_sw, (long long)T.ran,
             (long long)C.requests, (long long)T.asked);
      return 1;
    }
    // the public entries that touch no device: mem_pestat, and the rescue with every orientation failed, which
    // validates, builds the anchors and the lists, sends no request and returns the lists as they came
    struct gb_bsw_pestat pes[4];
    if (gb_bsw_pestat(&C.opt, l_pac, n_reads, off.data(), regs.data(), pes)) {
      printf("trial %d: %s\n", trial, gb_last_error());
      return 1;
    }
    for (int r = 0; r < 4; ++r) pes[r].failed = 1;
    std::vector<int64_t> idq((size_t)n_reads), out_off((size_t)n_reads);
    int64_t qbytes = 0, used = -1;
    for (int64_t r = 0; r < n_reads; ++r) idq[(size_t)r] = qbytes, qbytes += lq[(size_t)r];
    const std::vector<uint8_t> qer((size_t)qbytes, 0), pac((size_t)(l_pac + 3) / 4, 0x1b);
    std::vector<gb_bsw_alnreg> out(regs.size());
    std::vector<int32_t> n_out((size_t)n_reads), pair_sw((size_t)n_reads / 2, -1);
    gb_bsw_params gp;  // only mat is read: match 1, mismatch -4, ambiguous -1
    memset(&gp, 0, sizeof(gp));
    for (int i = 0; i < 5; ++i)
      for (int j = 0; j < 5; ++j) gp.mat[i * 5 + j] = (int8_t)(i == 4 || j == 4 ? -1 : i == j ? 1 : -4);
    gb_ref *ref = nullptr;
    int st = gb_ref_create(pac.data(), l_pac, &ref);
    if (!st)
      st = gb_bsw_mate_rescue(&gp, &C.opt, pes, ref, nullptr, 1, qer.data(), qbytes, n_reads / 2, idq.data(), lq.data(),
                              off.data(), regs.data(), out.data(), (int64_t)out.size(), out_off.data(), n_out.data(),
                              pair_sw.data(), &used);
    if (ref) gb_ref_destroy(ref);
    bool same = !st && used == (int64_t)regs.size() && !memcmp(out.data(), regs.data(), regs.size() * sizeof(gb_bsw_alnreg));
    for (int64_t r = 0; r < n_reads && same; ++r)
      same = out_off[(size_t)r] == off[(size_t)r] && n_out[(size_t)r] == off[(size_t)r + 1] - off[(size_t)r] &&
             pair_sw[(size_t)r / 2] == 0;
    if (!same) {
      printf("trial %d: the call with every orientation failed changed the lists (%d: %s)\n", trial, st, st ? gb_last_error() : "");
      return 1;
    }
    if (trial % 4 == 0)
      printf("trial %d: %lld reads, %zu regions in, %lld out, %lld requests in %d rounds, %lld ran\n", trial,
             (long long)n_reads, regs.size(), (long long)total, (long long)C.requests, C.rounds, (long long)T.ran);
  }
  puts("ok");
  return 0;
}
