// regs_host_check.cpp -- stand-alone host program over gb_bsw_finish_regs (csrc/bsw_regs.hip), meant to be
// built with the address and undefined-behaviour sanitizers on the host side (`make regs-sanitize` builds
// it together with the library's source files it needs and runs it). The call runs on the host and the
// program touches no device. A random reference with three
// contigs, the middle one ALT. Two hand-made reads come first: a read copied from the reference whose true
// alignment is cut into three pieces (two merges, n_comp 5), and a read with one hit on the ALT contig and
// two on the primary ones (n_pri = 2 of 3). Random region sets follow, up to 48 regions, on both strands.
// The two hand-made reads are checked for their values, the rest for shape (the fixture checks values):
// counts that do not grow, zeroed tails, regions inside their read. Prints "ok" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/gb_bsw.h"

static gb_bsw_alnreg reg(int64_t rb, int64_t re, int qb, int qe, int rid, int score) {
  gb_bsw_alnreg a;
  memset(&a, 0, sizeof(a));
  a.rb = rb, a.re = re, a.qb = qb, a.qe = qe, a.rid = rid;
  a.score = a.truesc = score, a.seedcov = (qe - qb) / 2 + 1, a.seedlen0 = 19, a.w = 3;
  return a;
}

int main() {
  std::mt19937_64 rng(9);
  const int64_t l_pac = 30000;
  const std::vector<int64_t> ce = {12000, 15000, l_pac};
  const std::vector<uint8_t> alt = {0, 1, 0};
  std::vector<uint8_t> codes((size_t)l_pac), pac((size_t)(l_pac + 3) / 4, 0);
  for (int64_t i = 0; i < l_pac; ++i) {
    codes[(size_t)i] = (uint8_t)(rng() & 3);
    pac[(size_t)(i >> 2)] |= (uint8_t)(codes[(size_t)i] << ((~i & 3) << 1));
  }
  auto rid_of = [&](int64_t rb) {
    const int64_t f = rb < l_pac ? rb : 2 * l_pac - 1 - rb;
    return f < ce[0] ? 0 : f < ce[1] ? 1 : 2;
  };
  gb_bsw_params gp;  // only mat is read: match 1, mismatch -4, ambiguous -1
  memset(&gp, 0, sizeof(gp));
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 5; ++j) gp.mat[i * 5 + j] = (int8_t)(i == 4 || j == 4 ? -1 : i == j ? 1 : -4);
  for (int trial = 0; trial < 12; ++trial) {
    gb_ref *ref = nullptr;
    if (gb_ref_create(pac.data(), l_pac, &ref)) {
      printf("gb_ref_create: %s\n", gb_last_error());
      return 1;
    }
    gb_bsw_reg_opt o;
    gb_bsw_reg_default_opt(&o);
    if (trial % 3 == 1) o.w = 4, o.mask_level_redun = 0.5f;
    if (trial % 3 == 2) o.max_chain_gap = 50, o.mapQ_coef_len = 0.f, o.primary5 = 1;
    std::vector<uint8_t> qer;
    std::vector<int64_t> idq, off(1, 0);
    std::vector<int32_t> lq;
    std::vector<gb_bsw_alnreg> regs;
    auto add_read = [&](int64_t s, int l, bool rev) {
      idq.push_back((int64_t)qer.size());
      lq.push_back(l);
      for (int k = 0; k < l; ++k) qer.push_back(rev ? (uint8_t)(3 - codes[(size_t)(s + l - 1 - k)]) : codes[(size_t)(s + k)]);
    };
    // read 0: 200 bases of contig 0 in three pieces with a gap and an overlap
    add_read(1000, 200, false);
    regs.push_back(reg(1000, 1070, 0, 70, 0, 70));
    regs.push_back(reg(1074, 1140, 74, 140, 0, 66));
    regs.push_back(reg(1135, 1200, 135, 200, 0, 65));
    off.push_back((int64_t)regs.size());
    // read 1: an ALT hit that shadows a primary one, and a second primary locus
    add_read(12500, 120, false);
    regs.push_back(reg(12500, 12620, 0, 120, 1, 120));
    regs.push_back(reg(3000, 3118, 0, 118, 0, 100));
    regs.push_back(reg(20000, 20060, 60, 120, 2, 55));
    off.push_back((int64_t)regs.size());
    const int n_rand = 1 + (int)(rng() % 60);
    for (int r = 0; r < n_rand; ++r) {
      const int l = 60 + (int)(rng() % 190);
      const bool rev = rng() & 1;
      const int c = (int)(rng() % 3);
      const int64_t c0 = c ? ce[(size_t)c - 1] : 0, base = c0 + 100 + (int64_t)(rng() % (uint64_t)(ce[(size_t)c] - c0 - 1200));
      add_read(base, l, rev);
      const int nr = (int)(rng() % 6 ? rng() % 7 : 16 + rng() % 33);
      for (int k = 0; k < nr; ++k) {
        const int qb = (int)(rng() % (uint64_t)(l - 25)), ql = 20 + (int)(rng() % (uint64_t)(l - qb - 19));
        int64_t rb = base + qb + (int64_t)(rng() % 9) - 4 + 150 * (int64_t)(rng() % 3), re = rb + ql + (int64_t)(rng() % 7) - 3;
        int q0 = qb, q1 = qb + ql;
        if (rev) {
          const int64_t t = rb;
          rb = 2 * l_pac - re, re = 2 * l_pac - t;
          q0 = l - (qb + ql), q1 = l - qb;
        }
        gb_bsw_alnreg a = reg(rb, re, q0, q1, rid_of(rb), 19 + (int)(rng() % 4) * 20);
        if (rng() % 8 == 0) a.csub = 1 + (int)(rng() % 60);
        if (rng() % 8 == 0) a.sub_n = 1 + (int)(rng() % 3);
        if (rng() % 8 == 0) a.frac_rep = 0.25f;
        regs.push_back(a);
      }
      off.push_back((int64_t)regs.size());
    }
    const int64_t n_reads = (int64_t)lq.size();
    for (int stage = 0; stage < 2; ++stage) {
      std::vector<gb_bsw_alnreg> work = regs;
      std::vector<int32_t> n_out((size_t)n_reads, -1);
      const int st = gb_bsw_finish_regs(&gp, &o, stage, ref, alt.data(), 3, qer.data(), (int64_t)qer.size(), n_reads,
                                        idq.data(), lq.data(), 1000 * trial, off.data(), work.data(), n_out.data());
      if (st) {
        printf("trial %d stage %d: %s\n", trial, stage, gb_last_error());
        return 1;
      }
      bool good = true;
      for (int64_t r = 0; r < n_reads && good; ++r) {
        const int64_t n = off[(size_t)r + 1] - off[(size_t)r];
        good = n_out[(size_t)r] >= (n ? 1 : 0) && n_out[(size_t)r] <= n;
        for (int64_t k = 0; k < n && good; ++k) {
          const gb_bsw_alnreg &a = work[(size_t)(off[(size_t)r] + k)];
          if (k < n_out[(size_t)r])
            good = a.qb >= 0 && a.qb < a.qe && a.qe <= lq[(size_t)r] && a.rb < a.re && a.mapq >= 0 && a.mapq <= 60 &&
                   (stage == 0 || a.secondary >= -1);
          else
            for (size_t b = 0; b < sizeof(a) && good; ++b) good = reinterpret_cast<const uint8_t *>(&a)[b] == 0;
        }
      }
      if (!good) {
        printf("trial %d stage %d: malformed output\n", trial, stage);
        return 1;
      }
      if (trial % 3 == 0) {  // the default options: the two hand-made reads
        const gb_bsw_alnreg &m = work[0];
        if (n_out[0] != 1 || m.n_comp != 5 || m.rb != 1000 || m.re != 1200 || m.qb != 0 || m.qe != 200 || m.score != 200 ||
            m.w != 9) {
          printf("trial %d stage %d: the three pieces gave %d regions, n_comp %d, score %d, w %d\n", trial, stage, n_out[0],
                 m.n_comp, m.score, m.w);
          return 1;
        }
        const gb_bsw_alnreg *a = &work[(size_t)off[1]];
        if (n_out[1] != 3 || (stage == 1 && !(a[0].rid == 0 && a[0].alt_sc == 120 && a[0].secondary == -1 && a[1].rid == 2 &&
                                              a[1].secondary == 0 && a[2].is_alt == 1 && a[2].secondary == -1))) {
          printf("trial %d stage %d: the ALT mix gave %d regions, first rid %d alt_sc %d\n", trial, stage, n_out[1], a[0].rid,
                 a[0].alt_sc);
          return 1;
        }
      }
      int32_t rounds = 0;
      int64_t reqs = 0, host_reads = 0;
      gb_bsw_finish_regs_timing(nullptr, nullptr, nullptr, &rounds, &reqs, &host_reads);
      if (host_reads != n_reads) {
        printf("trial %d: %lld of %lld reads on the host\n", trial, (long long)host_reads, (long long)n_reads);
        return 1;
      }
      if (stage == 1 && trial % 4 == 0)
        printf("trial %d: %lld reads, %zu regions, %lld alignments, at most %d per read\n", trial, (long long)n_reads,
               regs.size(), (long long)reqs, rounds);
    }
    gb_ref_destroy(ref);
  }
  puts("ok");
  return 0;
}
