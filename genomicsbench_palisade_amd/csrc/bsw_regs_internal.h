// bsw_regs_internal.h -- what bsw_regs.hip shares with bsw_matesw.hip: the per-read routines of
// mem_sort_dedup_patch (tools/bwa/bwamem.c:406-489), written for one read per lane and run on the host,
// and the comparisons of its sorts. Opt::no_patch turns mem_patch_reg off: that is the call mem_matesw
// makes, with a null bns (bwamem_pair.c:175), after which the routine never asks for an alignment.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gb_bsw.h"
#include "bsw_ksort.h"

namespace gbrg {

typedef gb_bsw_alnreg Reg;

constexpr int kMaxPenalty = 32768;
constexpr int kMinusInf = -0x40000000;  // ksw.c's MINUS_INF

struct Opt {
  int32_t a, b, o_del, e_del, o_ins, e_ins, w, max_chain_gap, T, primary5;
  float mask_level, mask_level_redun;
  int64_t l_pac, id0;
  int32_t no_patch, pad;  // no_patch: mem_patch_reg returns 0 at once (a null bns)
};

struct State {  // per read, 32 B
  int32_t n, n_out;  // regions given; regions left once the read is done
  int32_t i, j, w;   // where the pairwise loop waits, and the band it asked for
  int32_t n_dp;      // alignments asked for so far
  int32_t waiting;   // the read has a request out
  int32_t pad;
};

struct Request {  // 40 B
  int64_t rb, re, qoff;
  int32_t len2, w, read, pad;
};

#define GBRG_HD __host__ __device__ inline  // one read per lane, should a kernel call them

struct LtRe {  // mem_ars2
  GBRG_HD bool operator()(const Reg &x, const Reg &y) const { return x.re < y.re; }
};
struct LtArs {  // mem_ars
  GBRG_HD bool operator()(const Reg &x, const Reg &y) const {
    return x.score > y.score || (x.score == y.score && (x.rb < y.rb || (x.rb == y.rb && x.qb < y.qb)));
  }
};
struct LtHash {  // mem_ars_hash
  GBRG_HD bool operator()(const Reg &x, const Reg &y) const {
    return x.score > y.score ||
           (x.score == y.score && (x.is_alt < y.is_alt || (x.is_alt == y.is_alt && x.hash < y.hash)));
  }
};
struct LtHash2 {  // mem_ars_hash2
  GBRG_HD bool operator()(const Reg &x, const Reg &y) const {
    return x.is_alt < y.is_alt ||
           (x.is_alt == y.is_alt && (x.score > y.score || (x.score == y.score && x.hash < y.hash)));
  }
};

// mem_patch_reg up to the alignment (bwamem.c:412-426): true when a (left) and b need one, with its w.
// The two quotients are IEEE double divisions; the limits are floats widened, as the reference's are.
GBRG_HD bool patch_pre(const Opt &o, const Reg &a, const Reg &b, int *w_out) {
  if (a.rb < o.l_pac && b.rb >= o.l_pac) return false;
  if (a.qb >= b.qb || a.qe >= b.qe || a.re >= b.re) return false;
  int w = (int)((a.re - b.rb) - (a.qe - b.qb));
  w = w > 0 ? w : -w;
  double r = (double)(a.re - b.rb) / (double)(b.re - a.rb) - (double)(a.qe - b.qb) / (double)(b.qe - a.qb);
  r = r > 0. ? r : -r;
  if (a.re < b.rb || a.qe < b.qb) {
    if (w > o.w << 1 || r >= (double)0.05f) return false;
  } else if (w > o.w << 2 || r >= (double)(0.05f * 2)) {
    return false;
  }
  w += a.w + b.w;
  *w_out = w < o.w << 2 ? w : o.w << 2;
  return true;
}

// bwamem.c:429-434: the alignment's score, or 0 when it lies below 0.90 of the predicted one
GBRG_HD int patch_post(const Reg &a, const Reg &b, int score) {
  const int q_s = (int)((double)(b.qe - a.qb) / ((b.qe - b.qb) + (a.qe - a.qb)) * (b.score + a.score) + .499);
  const int r_s = (int)((double)(b.re - a.rb) / (double)((b.re - b.rb) + (a.re - a.rb)) * (b.score + a.score) + .499);
  if ((double)score / (q_s > r_s ? q_s : r_s) < (double)0.90f) return 0;
  return score;
}

// mem_sort_dedup_patch for one read, in steps: a first call (have == false) sorts and walks the pairwise
// loop; it leaves st.waiting set and *req filled when the loop waits for an alignment, and a later call
// with have == true and that alignment's score goes on from there. With st.waiting clear the read is done:
// st.n_out regions are left, in the reference's order, with is_alt set. The routine has one exit and its
// loops carry their stop conditions in their heads (`waiting`, `dropped`).
GBRG_HD void dedup_read(const Opt &o, const uint8_t *contig_is_alt, Reg *a, State &st, bool have, int score_in,
                        int64_t qbase, Request *req) {
  const int n = st.n;
  int i = 1, j = 0;
  bool waiting = false;
  if (!have) {
    st.n_out = n;
    if (n > 1) {
      gbks::introsort(a, n, LtRe());
      for (int k = 0; k < n; ++k) a[k].n_comp = 1;
    }
  } else {
    i = st.i, j = st.j;
  }
  if (n > 1) {
    while (i < n && !waiting) {
      Reg *p = &a[i];
      bool row = have;  // a row that waited for its alignment goes on where it stopped
      if (!have) {
        row = !(p->rid != a[i - 1].rid || p->rb >= a[i - 1].re + o.max_chain_gap);
        j = i - 1;
      }
      bool dropped = false;  // p lost against a better redundant hit (the reference's break)
      while (row && !waiting && !dropped && (have || (j >= 0 && p->rid == a[j].rid && p->rb < a[j].re + o.max_chain_gap))) {
        Reg *q = &a[j];
        int score = 0, w = 0;
        if (have) {
          have = false;
          score = patch_post(*q, *p, score_in);
          w = st.w;
        } else if (q->qe != q->qb) {  // else a[j] has been excluded
          const int64_t orr = q->re - p->rb;
          const int64_t oq = q->qb < p->qb ? q->qe - p->qb : p->qe - q->qb;
          const int64_t mr = q->re - q->rb < p->re - p->rb ? q->re - q->rb : p->re - p->rb;
          const int64_t mq = q->qe - q->qb < p->qe - p->qb ? q->qe - q->qb : p->qe - p->qb;
          if ((float)orr > o.mask_level_redun * (float)mr && (float)oq > o.mask_level_redun * (float)mq) {
            if (p->score < q->score) p->qe = p->qb, dropped = true;
            else q->qe = q->qb;
          } else if (q->rb < p->rb && !o.no_patch && patch_pre(o, *q, *p, &w)) {
            req->rb = q->rb, req->re = p->re, req->qoff = qbase + q->qb;
            req->len2 = p->qe - q->qb, req->w = w;
            st.i = i, st.j = j, st.w = w;
            ++st.n_dp;
            waiting = true;
          }
        }
        if (score > 0) {  // merge q into p
          p->n_comp += q->n_comp + 1;
          p->seedcov = p->seedcov > q->seedcov ? p->seedcov : q->seedcov;
          p->sub = p->sub > q->sub ? p->sub : q->sub;
          p->csub = p->csub > q->csub ? p->csub : q->csub;
          p->qb = q->qb, p->rb = q->rb;
          p->truesc = p->score = score;
          p->w = w;
          q->qb = q->qe;
        }
        if (!waiting) --j;
      }
      if (!waiting) ++i;
    }
    if (!waiting) {
      int m = 0;
      for (i = 0; i < n; ++i)
        if (a[i].qe > a[i].qb) {
          if (m != i) a[m] = a[i];
          ++m;
        }
      const int n2 = m;
      gbks::introsort(a, n2, LtArs());
      for (i = 1; i < n2; ++i)
        if (a[i].score == a[i - 1].score && a[i].rb == a[i - 1].rb && a[i].qb == a[i - 1].qb) a[i].qe = a[i].qb;
      m = n2 < 1 ? n2 : 1;
      for (i = 1; i < n2; ++i)
        if (a[i].qe > a[i].qb) {
          if (m != i) a[m] = a[i];
          ++m;
        }
      st.n_out = m;
    }
  }
  if (!waiting && contig_is_alt)
    for (i = 0; i < st.n_out; ++i)
      if (contig_is_alt[a[i].rid]) a[i].is_alt = 1;
  st.waiting = waiting;
}

}  // namespace gbrg
