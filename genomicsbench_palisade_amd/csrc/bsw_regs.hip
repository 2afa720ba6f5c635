// bsw_regs.hip -- from a read's regions to its primaries, bwa's mem_sort_dedup_patch with mem_patch_reg
// (tools/bwa/bwamem.c:406-489), mem_mark_primary_se (:493-558), mem_reorder_primary5 (:1019-1041) and
// mem_approx_mapq_se (:993-1017): per-read routines, host path and C ABI.
//
// Like the chains (bsw_mkchain.hip) this step is small arithmetic whose difficulty is order: three
// unstable sorts with different comparisons (bsw_ksort.h restates ks_introsort), a pairwise loop that
// changes the array it walks, and in the middle of that loop a banded global alignment.
//
// The per-read routines are written for one read per lane: dedup_read does not run the alignment itself.
// When mem_patch_reg's tests up to the DP have passed it fills a request {rb, re, query offset, len2, w},
// saves its place (i, j) in the pairwise loop and returns; called again with the alignment's score it goes
// on from that place and applies bwamem.c:429-434 and the merge. A read asks for its next alignment only
// after the previous answer, because a merge changes p. The call runs these routines on the host: a plain
// score-only banded DP over the reference's host copy answers a request at once, reads are spread over
// host threads. A device path (a dedup and a mark kernel around score-only gb_bsw_gen_cigar batches) is
// not part of this file: see DESIGN.md, "bsw (regions to primaries)".
//
// The MAPQ is computed in the output pass: mem_approx_mapq_se calls the C library's log() three times and
// one ulp can flip (int)(x + .499).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/gb_bsw.h"
#include "bsw_ksort.h"
#include "bsw_ref_internal.h"
#include "bsw_regs_internal.h"
#include "gb_common.h"

static_assert(sizeof(gb_bsw_alnreg) == 96, "gb_bsw_alnreg is 96 bytes (include/gb_bsw.h)");

namespace gbrg {

GBRG_HD uint64_t hash_64(uint64_t key) {
  key += ~(key << 32);
  key ^= (key >> 22);
  key += ~(key << 13);
  key ^= (key >> 8);
  key += (key << 3);
  key ^= (key >> 15);
  key += ~(key << 27);
  key ^= (key >> 31);
  return key;
}

// mem_mark_primary_se_core; z holds the indices of the hits that shadow
GBRG_HD void mark_core(const Opt &o, int n, Reg *a, int32_t *z) {
  int tmp = o.a + o.b;
  tmp = o.o_del + o.e_del > tmp ? o.o_del + o.e_del : tmp;
  tmp = o.o_ins + o.e_ins > tmp ? o.o_ins + o.e_ins : tmp;
  int zn = 0;
  z[zn++] = 0;
  for (int i = 1; i < n; ++i) {
    int k;
    for (k = 0; k < zn; ++k) {
      const int j = z[k];
      const int b_max = a[j].qb > a[i].qb ? a[j].qb : a[i].qb;
      const int e_min = a[j].qe < a[i].qe ? a[j].qe : a[i].qe;
      if (e_min > b_max) {
        const int min_l = a[i].qe - a[i].qb < a[j].qe - a[j].qb ? a[i].qe - a[i].qb : a[j].qe - a[j].qb;
        if ((float)(e_min - b_max) >= (float)min_l * o.mask_level) {
          if (a[j].sub == 0) a[j].sub = a[i].score;
          if (a[j].score - a[i].score <= tmp && (a[j].is_alt || !a[i].is_alt)) ++a[j].sub_n;
          break;
        }
      }
    }
    if (k == zn) z[zn++] = i;
    else a[i].secondary = z[k];
  }
}

// mem_mark_primary_se, then mem_reorder_primary5 when asked for
GBRG_HD void mark_read(const Opt &o, int n, Reg *a, int32_t *z, int64_t id) {
  if (n == 0) return;
  int n_pri = 0;
  for (int i = 0; i < n; ++i) {
    a[i].sub = a[i].alt_sc = 0, a[i].secondary = a[i].secondary_all = -1;
    a[i].hash = hash_64((uint64_t)id + (uint64_t)i);
    if (!a[i].is_alt) ++n_pri;
  }
  gbks::introsort(a, n, LtHash());
  mark_core(o, n, a, z);
  for (int i = 0; i < n; ++i) {
    Reg *p = &a[i];
    p->secondary_all = i;
    if (!p->is_alt && p->secondary >= 0 && a[p->secondary].is_alt) p->alt_sc = a[p->secondary].score;
  }
  if (n_pri < n) {
    if (n_pri > 0) gbks::introsort(a, n, LtHash2());
    for (int i = 0; i < n; ++i) z[a[i].secondary_all] = i;
    for (int i = 0; i < n; ++i) {
      if (a[i].secondary >= 0) {
        a[i].secondary_all = z[a[i].secondary];
        if (a[i].is_alt) a[i].secondary = INT_MAX;
      } else {
        a[i].secondary_all = -1;
      }
    }
    if (n_pri > 0) {
      for (int i = 0; i < n_pri; ++i) a[i].sub = 0, a[i].secondary = -1;
      mark_core(o, n_pri, a, z);
    }
  } else {
    for (int i = 0; i < n; ++i) a[i].secondary_all = a[i].secondary;
  }
  if (!o.primary5) return;
  int np = 0, left_st = INT_MAX, left_k = -1;
  for (int k = 0; k < n; ++k)
    if (a[k].secondary < 0 && !a[k].is_alt && a[k].score >= o.T) ++np;
  if (np <= 1) return;
  for (int k = 0; k < n; ++k) {
    const Reg *p = &a[k];
    if (p->secondary >= 0 || p->is_alt || p->score < o.T) continue;
    if (p->qb < left_st) left_st = p->qb, left_k = k;
  }
  if (left_k <= 0) return;
  gbks::swap2(a, 0, left_k);
  for (int k = 1; k < n; ++k) {
    Reg *p = &a[k];
    if (p->secondary == 0) p->secondary = left_k;
    else if (p->secondary == left_k) p->secondary = 0;
    if (p->secondary_all == 0) p->secondary_all = left_k;
    else if (p->secondary_all == left_k) p->secondary_all = 0;
  }
}

// ---- host side ---------------------------------------------------------------------------------

// ksw_global2's score (tools/bwa/ksw.c:504-606 without the direction matrix): rows are target bases, row i
// covers the query columns [max(i - w, 0), min(i + w + 1, qlen)), everything outside the band is -inf, and
// the cell behind a row's last column is closed with that row's last H.
int global_score(const uint8_t *q, int qlen, const uint8_t *t, int tlen, const int8_t *mat, int o_del, int e_del,
                 int o_ins, int e_ins, int w, std::vector<int32_t> &hbuf) {
  hbuf.assign(2 * ((size_t)qlen + 1), kMinusInf);
  int32_t *H = hbuf.data(), *E = H + qlen + 1;  // H[j]: H(i - 1, j - 1) while row i runs
  const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
  H[0] = 0;
  for (int j = 1; j <= qlen && j <= w; ++j) H[j] = -(o_ins + e_ins * j);
  for (int i = 0; i < tlen; ++i) {
    const int beg = i > w ? i - w : 0, end = i + w + 1 < qlen ? i + w + 1 : qlen;
    int32_t f = kMinusInf, h1 = beg == 0 ? -(o_del + e_del * (i + 1)) : kMinusInf;
    const int8_t *row = mat + 5 * t[i];
    for (int j = beg; j < end; ++j) {
      const int32_t m = H[j] + row[q[j]];
      int32_t e = E[j];
      H[j] = h1;
      int32_t h = m >= e ? m : e;
      h = h >= f ? h : f;
      h1 = h;
      int32_t x = m - oe_del;
      e -= e_del;
      E[j] = e > x ? e : x;
      x = m - oe_ins;
      f -= e_ins;
      f = f > x ? f : x;
    }
    H[end] = h1, E[end] = kMinusInf;
  }
  return H[qlen];
}

inline int pac_base(const uint8_t *pac, int64_t l) { return pac[l >> 2] >> ((~l & 3) << 1) & 3; }

struct HostDp {  // per thread
  std::vector<uint8_t> t, q;
  std::vector<int32_t> h;
};

// bwa_gen_cigar2's score (bwa.c:121-167) for one request, from the reference's host copy
int host_dp(const gb_bsw_params &P, const uint8_t *pac, int64_t l_pac, const uint8_t *qer, const Request &rq, HostDp &W) {
  const int len1 = (int)(rq.re - rq.rb), len2 = rq.len2;
  W.t.resize((size_t)len1), W.q.resize((size_t)len2);
  const bool rev = rq.rb >= l_pac;
  // the reverse strand's bases are the complement read backwards, and the reference then reverses target
  // and query (bwa.c:135-140): the complement in forward order against the reversed query
  const int64_t f0 = rev ? 2 * l_pac - rq.re : rq.rb;
  for (int k = 0; k < len1; ++k) W.t[(size_t)k] = (uint8_t)(rev ? 3 - pac_base(pac, f0 + k) : pac_base(pac, f0 + k));
  for (int k = 0; k < len2; ++k) W.q[(size_t)k] = std::min<uint8_t>(qer[rq.qoff + (rev ? len2 - 1 - k : k)], 4);
  if (len2 == len1 && rq.w == 0) {
    int s = 0;
    for (int k = 0; k < len2; ++k) s += P.mat[W.t[(size_t)k] * 5 + W.q[(size_t)k]];
    return s;
  }
  const int w = gb_bsw_global_band(&P, len2, len1, rq.w);
  return global_score(W.q.data(), len2, W.t.data(), len1, P.mat, P.o_del, P.e_del, P.o_ins, P.e_ins, w, W.h);
}

// mem_approx_mapq_se
int approx_mapq(const gb_bsw_reg_opt &o, const Reg &a) {
  int mapq, l, sub = a.sub ? a.sub : o.min_seed_len * o.a;
  double identity;
  sub = a.csub > sub ? a.csub : sub;
  if (sub >= a.score) return 0;
  l = a.qe - a.qb > a.re - a.rb ? a.qe - a.qb : (int)(a.re - a.rb);
  identity = 1. - (double)(l * o.a - a.score) / (o.a + o.b) / l;
  if (a.score == 0) {
    mapq = 0;
  } else if (o.mapQ_coef_len > 0) {
    double tmp;
    tmp = l < o.mapQ_coef_len ? 1. : o.mapQ_coef_fac / log(l);
    tmp *= identity * identity;
    mapq = (int)(6.02 * (a.score - sub) / o.a * tmp * tmp + .499);
  } else {
    mapq = (int)(30 * (1. - (double)sub / a.score) * log(a.seedcov) + .499);  // MEM_MAPQ_COEF 30.0
    mapq = identity < 0.95 ? (int)(mapq * identity * identity + .499) : mapq;
  }
  if (a.sub_n > 0) mapq -= (int)(4.343 * log(a.sub_n + 1) + .499);
  if (mapq > 60) mapq = 60;
  if (mapq < 0) mapq = 0;
  mapq = (int)(mapq * (1. - a.frac_rep) + .499);
  return mapq;
}

struct Timing {
  int32_t rounds;
  int64_t requests, host_reads;
  bool valid;
};
thread_local Timing g_timing = {0, 0, 0, false};

struct Call {
  const char *who = "gb_bsw_finish_regs";
  Opt opt;
  gb_bsw_params dp;  // mat from params, the gap penalties from opt
  int32_t stage = 0;
  int64_t n_reads = 0, n_regs = 0;
  const int64_t *reg_off = nullptr, *idq = nullptr;
  const uint8_t *qer = nullptr, *is_alt = nullptr;
  int64_t n_contigs = 0;
  std::vector<Reg> work;
  std::vector<State> state;
};

int run_host(Call &C, gb_ref *R) {
  bool any2 = false;
  for (int64_t r = 0; r < C.n_reads && !any2; ++r) any2 = C.reg_off[r + 1] - C.reg_off[r] >= 2;
  std::unique_lock<std::mutex> lock(R->mu);  // the host copy must stay while it is read
  GB_ARG(!any2 || !R->host.empty(),
         "%s: the call reads the reference's host copy, which was released at the reference's first device use",
         C.who);
  const uint8_t *pac = R->host.data();
  int nth = 1;
  if (const int st = gb::thread_count(C.who, "GB_BSW_REGS_THREADS", &nth)) return st;
  if (C.n_reads < 256) nth = 1;
  std::vector<int32_t> zall((size_t)std::max<int64_t>(C.n_regs, 1));
  std::atomic<int64_t> bad_read{-1};
  const int pst = gb::parallel(C.who, nth, [&](int t) {
    HostDp W;
    for (int64_t r = C.n_reads * t / nth; r < C.n_reads * (t + 1) / nth; ++r) {
      const int64_t off = C.reg_off[r];
      State &st = C.state[(size_t)r];
      std::memset(&st, 0, sizeof(st));
      st.n = st.n_out = (int32_t)(C.reg_off[r + 1] - off);
      Request rq{};
      bool have = false;
      int score = 0;
      for (;;) {
        dedup_read(C.opt, C.is_alt, C.work.data() + off, st, have, score, C.idq[r], &rq);
        if (!st.waiting) break;
        if (rq.re - rq.rb > GB_BSW_GLOBAL_MAX_TLEN) {
          int64_t none = -1;
          bad_read.compare_exchange_strong(none, r);
          return;
        }
        score = host_dp(C.dp, pac, R->l_pac, C.qer, rq, W);
        have = true;
      }
      if (C.stage) mark_read(C.opt, st.n_out, C.work.data() + off, zall.data() + off, C.opt.id0 + r);
    }
  });
  if (pst) return pst;
  GB_ARG(bad_read.load() < 0, "%s: read %lld needs a merge alignment over more than %d reference bases", C.who,
         (long long)bad_read.load(), GB_BSW_GLOBAL_MAX_TLEN);
  g_timing.host_reads = C.n_reads;
  return GB_OK;
}

int finish_impl(const gb_bsw_params *params, const gb_bsw_reg_opt *opt, int32_t stage, const gb_ref *ref,
                const uint8_t *contig_is_alt, int64_t n_contigs, const uint8_t *qer, int64_t qer_bytes, int64_t n_reads,
                const int64_t *idq, const int32_t *l_query, int64_t id0, const int64_t *reg_off, gb_bsw_alnreg *regs,
                int32_t *n_out) {
  Call C;
  const char *who = C.who;
  GB_ARG(params && opt && ref, "%s: null params, opt or ref", who);
  GB_ARG(stage == 0 || stage == 1, "%s: stage = %d (0: mem_sort_dedup_patch, 1: and mem_mark_primary_se, MAPQ)", who,
         stage);
  GB_ARG(n_reads >= 0 && n_reads < (1ll << 31), "%s: n_reads = %lld", who, (long long)n_reads);
  GB_ARG(n_contigs >= 1 && n_contigs < (1ll << 31), "%s: n_contigs = %lld", who, (long long)n_contigs);
  GB_ARG(qer_bytes >= 0 && (qer_bytes == 0 || qer), "%s: bad sequence buffer", who);
  GB_ARG(opt->w >= 0 && opt->w < (1 << 28), "%s: opt->w = %d must lie in [0, 2^28)", who, opt->w);
  GB_ARG(opt->max_chain_gap >= 0, "%s: max_chain_gap = %d", who, opt->max_chain_gap);
  GB_ARG((int64_t)opt->a + opt->b >= 1 && opt->a >= 1 && opt->a < kMaxPenalty && opt->b > -kMaxPenalty &&
             opt->b < kMaxPenalty,
         "%s: a = %d, b = %d (need a >= 1, a + b >= 1, both below %d)", who, opt->a, opt->b, kMaxPenalty);
  GB_ARG(std::isfinite(opt->mask_level), "%s: mask_level is not finite", who);
  GB_ARG(std::isfinite(opt->mask_level_redun), "%s: mask_level_redun is not finite", who);
  GB_ARG(std::isfinite(opt->mapQ_coef_len), "%s: mapQ_coef_len is not finite", who);
  GB_ARG(opt->min_seed_len < (1 << 15) && opt->min_seed_len > -(1 << 15), "%s: min_seed_len = %d", who, opt->min_seed_len);
  const int pen[4] = {opt->o_del, opt->e_del, opt->o_ins, opt->e_ins};
  for (int v : pen)
    GB_ARG(v >= 0 && v < kMaxPenalty, "%s: gap penalties (o_del %d, e_del %d, o_ins %d, e_ins %d) must lie in [0, %d)", who,
           pen[0], pen[1], pen[2], pen[3], kMaxPenalty);
  GB_ARG(opt->e_del > 0 && opt->e_ins > 0, "%s: gap extension penalties (e_del %d, e_ins %d) must be > 0", who, opt->e_del,
         opt->e_ins);
  g_timing = Timing{0, 0, 0, true};
  if (n_reads == 0) return GB_OK;
  GB_ARG(idq && l_query && reg_off && n_out, "%s: null idq, l_query, reg_off or n_out", who);
  GB_ARG(reg_off[0] == 0, "%s: reg_off[0] = %lld", who, (long long)reg_off[0]);
  const int64_t l_pac = ref->l_pac;
  for (int64_t r = 0; r < n_reads; ++r) {
    GB_ARG(reg_off[r + 1] >= reg_off[r], "%s: read %lld: reg_off decreases (%lld after %lld)", who, (long long)r,
           (long long)reg_off[r + 1], (long long)reg_off[r]);
    GB_ARG(reg_off[r + 1] < (1ll << 31), "%s: read %lld: %lld regions (the call takes fewer than 2^31)", who, (long long)r,
           (long long)reg_off[r + 1]);
  }
  const int64_t n_regs = reg_off[n_reads];
  GB_ARG(n_regs == 0 || regs, "%s: null regs", who);
  for (int64_t r = 0; r < n_reads; ++r) {
    if (reg_off[r + 1] == reg_off[r]) continue;
    const int lq = l_query[r];
    GB_ARG(lq >= 1 && lq <= GB_BSW_MAX_QLEN, "%s: read %lld: l_query = %d (need [1, %d])", who, (long long)r, lq,
           GB_BSW_MAX_QLEN);
    GB_ARG(idq[r] >= 0 && idq[r] <= qer_bytes - lq, "%s: read %lld has its query outside the sequence buffer", who,
           (long long)r);
    for (int64_t k = reg_off[r]; k < reg_off[r + 1]; ++k) {
      const Reg &g = regs[k];
      const long long rr = (long long)r, kk = (long long)(k - reg_off[r]);
      GB_ARG(g.qb >= 0 && g.qb < g.qe && g.qe <= lq, "%s: read %lld region %lld: [qb, qe) = [%d, %d), l_query = %d", who, rr,
             kk, g.qb, g.qe, lq);
      GB_ARG(g.rb >= 0 && g.rb < g.re && g.re <= 2 * l_pac && !(g.rb < l_pac && g.re > l_pac),
             "%s: read %lld region %lld: [rb, re) = [%lld, %lld) with l_pac = %lld", who, rr, kk, (long long)g.rb,
             (long long)g.re, (long long)l_pac);
      GB_ARG(g.rid >= 0 && g.rid < n_contigs, "%s: read %lld region %lld: rid = %d outside [0, %lld)", who, rr, kk, g.rid,
             (long long)n_contigs);
      GB_ARG(g.score >= 1, "%s: read %lld region %lld: score = %d", who, rr, kk, g.score);
      GB_ARG(g.seedcov >= 1, "%s: read %lld region %lld: seedcov = %d", who, rr, kk, g.seedcov);
      GB_ARG(g.sub >= 0 && g.csub >= 0 && g.sub_n >= 0, "%s: read %lld region %lld: sub = %d, csub = %d, sub_n = %d", who, rr,
             kk, g.sub, g.csub, g.sub_n);
      GB_ARG(g.w >= 0 && g.w < (1 << 28), "%s: read %lld region %lld: w = %d outside [0, 2^28)", who, rr, kk, g.w);
    }
  }
  Opt &o = C.opt;
  o.a = opt->a, o.b = opt->b, o.o_del = opt->o_del, o.e_del = opt->e_del, o.o_ins = opt->o_ins, o.e_ins = opt->e_ins;
  o.w = opt->w, o.max_chain_gap = opt->max_chain_gap, o.T = opt->T, o.primary5 = opt->primary5 != 0;
  o.mask_level = opt->mask_level, o.mask_level_redun = opt->mask_level_redun;
  o.l_pac = l_pac, o.id0 = id0;
  o.no_patch = 0, o.pad = 0;
  C.dp = *params;
  C.dp.o_del = opt->o_del, C.dp.e_del = opt->e_del, C.dp.o_ins = opt->o_ins, C.dp.e_ins = opt->e_ins;
  C.stage = stage, C.n_reads = n_reads, C.n_regs = n_regs;
  C.reg_off = reg_off, C.idq = idq, C.qer = qer, C.is_alt = contig_is_alt, C.n_contigs = n_contigs;
  C.work.assign(regs, regs + n_regs);
  C.state.resize((size_t)n_reads);

  int st;
  if ((st = run_host(C, const_cast<gb_ref *>(ref)))) return st;
  for (const State &s : C.state) {
    g_timing.rounds = std::max(g_timing.rounds, s.n_dp);
    g_timing.requests += s.n_dp;
  }
  // the output pass: the MAPQ, the zeroed tails, and only now the caller's arrays
  for (int64_t r = 0; r < n_reads; ++r) {
    const int64_t off = reg_off[r], n = reg_off[r + 1] - off;
    const int m = C.state[(size_t)r].n_out;
    if (m < 0 || m > n) {
      gb::set_error("%s: read %lld: %d regions left of %lld", who, (long long)r, m, (long long)n);
      return GB_ERR_STATE;
    }
    for (int k = 0; k < m; ++k) {
      Reg &g = C.work[(size_t)(off + k)];
      g.mapq = stage && g.secondary < 0 ? approx_mapq(*opt, g) : 0;
    }
    if (m < n) std::memset(static_cast<void *>(C.work.data() + off + m), 0, (size_t)(n - m) * sizeof(Reg));
  }
  if (n_regs) std::memcpy(static_cast<void *>(regs), C.work.data(), (size_t)n_regs * sizeof(Reg));
  for (int64_t r = 0; r < n_reads; ++r) n_out[r] = C.state[(size_t)r].n_out;
  return GB_OK;
}

}  // namespace gbrg

extern "C" {

void gb_bsw_reg_default_opt(gb_bsw_reg_opt *o) {
  if (!o) return;
  o->a = 1, o->b = 4, o->o_del = o->o_ins = 6, o->e_del = o->e_ins = 1;
  o->w = 100, o->max_chain_gap = 10000, o->min_seed_len = 19;
  o->mask_level = 0.50f, o->mask_level_redun = 0.95f, o->mapQ_coef_len = 50.f;
  o->mapQ_coef_fac = (int)std::log(50.);
  o->T = 30, o->primary5 = 0;
}

// The C ABI lets no exception out: the copy, the host path and the request batches allocate.
int gb_bsw_finish_regs(const gb_bsw_params *params, const gb_bsw_reg_opt *opt, int32_t stage, const gb_ref *ref,
                       const uint8_t *contig_is_alt, int64_t n_contigs, const uint8_t *seq_buf_qer, int64_t qer_bytes,
                       int64_t n_reads, const int64_t *idq, const int32_t *l_query, int64_t id0, const int64_t *reg_off,
                       gb_bsw_alnreg *regs, int32_t *n_out) {
  gb::Range range_("gb.bsw.finish_regs");
  try {
    return gbrg::finish_impl(params, opt, stage, ref, contig_is_alt, n_contigs, seq_buf_qer, qer_bytes, n_reads, idq,
                             l_query, id0, reg_off, regs, n_out);
  } catch (const std::bad_alloc &) {
    gb::set_error("gb_bsw_finish_regs: out of host memory");
    return GB_ERR_NOMEM;
  } catch (const std::exception &e) {
    gb::set_error("gb_bsw_finish_regs: %s", e.what());
    return GB_ERR_STATE;
  }
}

int gb_bsw_alnreg_from_regions(const gb_bsw_region *regions, int64_t n, const gb_bsw_chain_info *chain_info,
                               int64_t n_chains, gb_bsw_alnreg *out) {
  const char *who = "gb_bsw_alnreg_from_regions";
  GB_ARG(n >= 0 && n_chains >= 0 && (n == 0 || (regions && chain_info && out)), "%s: bad arguments", who);
  for (int64_t k = 0; k < n; ++k)
    GB_ARG(regions[k].chain >= 0 && regions[k].chain < n_chains, "%s: region %lld: chain = %d outside [0, %lld)", who,
           (long long)k, regions[k].chain, (long long)n_chains);
  for (int64_t k = 0; k < n; ++k) {
    const gb_bsw_region &g = regions[k];
    gb_bsw_alnreg &a = out[k];
    std::memset(&a, 0, sizeof(a));
    a.rb = g.rb, a.re = g.re, a.qb = g.qb, a.qe = g.qe;
    a.score = g.score, a.truesc = g.truesc, a.w = g.w, a.seedcov = g.seedcov, a.seedlen0 = g.seedlen0;
    a.rid = chain_info[g.chain].rid, a.frac_rep = chain_info[g.chain].frac_rep;
  }
  return GB_OK;
}

int gb_bsw_finish_regs_timing(float *dedup_ms, float *dp_ms, float *mark_ms, int32_t *dp_rounds, int64_t *dp_requests,
                              int64_t *host_reads) {
  using namespace gbrg;
  if (!g_timing.valid) {
    gb::set_error("gb_bsw_finish_regs_timing: no gb_bsw_finish_regs call on this thread");
    return GB_ERR_STATE;
  }
  if (dedup_ms) *dedup_ms = 0.f;  // device times: the call runs on the host
  if (dp_ms) *dp_ms = 0.f;
  if (mark_ms) *mark_ms = 0.f;
  if (dp_rounds) *dp_rounds = g_timing.rounds;
  if (dp_requests) *dp_requests = g_timing.requests;
  if (host_reads) *host_reads = g_timing.host_reads;
  return GB_OK;
}

}  // extern "C"
