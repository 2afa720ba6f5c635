// bsw_mkchain.hip -- MI355X (gfx950): chains from seeds, bwa's mem_chain after mem_collect_intv
// (tools/bwa/bwamem.c:265-310) and mem_chain_flt (:327-385): kernels, host path and C ABI.
//
// The step is small arithmetic whose difficulty is order, so the per-read routines below restate the
// reference's containers exactly, on chain ids instead of chain structs:
//   the B-tree (kbtree.h, t = 5 for mem_chain_t: nodes of up to 9 keys, the root splits on the 10th chain):
//     kb_intervalp's descent with __kb_getp_aux's lower bound, so that of several equal pos the leftmost
//     one of the first node that holds one is returned; kb_putp's top-down splits and its insertion
//     behind the leftmost equal key of a leaf; __kb_traverse's in-order walk.
//   ks_introsort (ksort.h:176-226) by decreasing weight: the n == 2 case, the depth counter with its
//     comb-sort fallback, the median-of-three partition that swaps, the push only of sides longer than
//     16, the closing insertion sort. It is not stable and equal weights are the normal case.
// A chain's state is 72 bytes: pos, the first seed's qbeg, the last seed's rbeg / qbeg / len, rid, the
// number of seeds and the two running coverages of mem_chain_weight (the weight is a left-to-right
// fold over the seeds in insertion order, so it is kept while the chain grows). Seeds do not move while
// the chains are built: per coordinate the kernel records the id of the chain it joined, or -1 for a
// seed that bns_intv2rid skips or that is contained.
//
// Device path, one read per lane (the work per read is a serial pointer walk; a wave per read would idle
// 63 lanes), every loop bounded by the read's coordinate count:
//   build   the loop of mem_chain; the traversal writes the chain order
//   filter  weights, the drop by min_chain_weight, the introsort on a permutation of chain ids, the
//           pairwise pass, first -> kept = 1, the max_chain_extend cut, the compaction (stage 1)
//   emit    count of chains per read, scan, seeds per chain, scan, and a stable scatter of the seeds by
//           chain id into the CSR, with the info records
// The per-read workspace is a slice sized by the read's coordinate count n: n chain states, n / 4 + 2
// nodes (every node but the root keeps at least 4 keys), n ids for the order, n 8-byte sort keys and n 16-byte
// records of the kept list. The host path runs the same per-read routines over std::vector slices.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <stdexcept>
#include <vector>

#include "../../include/gb_bsw.h"
#include "gb_common.h"

static_assert(sizeof(gb_bsw_mem) == 24, "gb_bsw_mem is 24 bytes (include/gb_bsw.h)");
static_assert(sizeof(gb_bsw_chain_info) == 32, "gb_bsw_chain_info is 32 bytes (include/gb_bsw.h)");
static_assert(sizeof(gb_bsw_seed) == 24, "gb_bsw_seed is 24 bytes (include/gb_bsw.h)");

namespace gbmk {

constexpr int kT = 5;               // kb_init(chn, 512) with sizeof(mem_chain_t) == 40
constexpr int kKeys = 2 * kT - 1;   // keys per node
constexpr int kTreeDepth = 24;      // > log_5 of 2^31 + 2
constexpr int kSortStack = 64;      // the pushed depths decrease strictly and start below 2 * 31
constexpr int kScanThreads = 1024;

struct Opt {
  int32_t w, max_chain_gap, max_occ, min_seed_len, min_chain_weight, max_chain_extend;
  float mask_level, drop_ratio;
  int64_t l_pac;
  int32_t n_contigs, stage;
};

struct SMem {  // one SMEM in mem_chain's order, 24 B
  int64_t coord_off;  // of its first coordinate in the caller's array
  int32_t qbeg, len, n_coord, rep;  // rep: s > max_occ; qend = qbeg + len
};

struct ReadItem {  // 40 B
  int64_t mem_off, coord_base, node_base;  // slices of the sorted SMEMs, the workspace and its nodes
  int32_t n_mems, n_coords, l_query, host;  // host: the read takes the host path
};

struct Chain {  // 72 B
  int64_t pos, last_rbeg, end_r;
  int32_t first_qbeg, last_qbeg, last_len, rid, n, wq, wr, end_q;
  int32_t w, kept, cursor, out;  // out: the chain's index in the call's output, or -1; cursor: where the emit
                                 // step writes the chain's next seed (fewer than 2^31 seeds in a call)
};

struct Node {  // 160 B
  int64_t pos[kKeys];
  int32_t id[kKeys];
  int32_t child[kKeys + 1];
  int32_t n, internal;
};

struct Kept {  // 16 B: what the pairwise pass reads of a kept chain
  int32_t beg, end;  // chn_beg, chn_end
  int32_t w_alt;     // the weight (29 bits) | is_alt << 30
  int32_t first;     // the first chain it shadowed (an index into the sorted list), or -1
};

struct ReadWs {  // a read's workspace slice
  Chain *ch;
  Node *nodes;
  int32_t *cc;     // per coordinate in sorted order: the chain joined, or -1
  int32_t *order;  // the output order of chain ids (traversal, then what the filter leaves)
  int64_t *perm;   // the filter's permutation: weight << 32 | chain id, so that the sort reads one array
  Kept *kept;      // the filter's list of kept chains, packed so that the pairwise pass streams through it
};

struct ReadOut {  // per read
  int32_t n_chains, n_out, l_rep, pad;
};

#define GBMK_HD __host__ __device__ inline

// bns_pos2rid: the contig that holds forward position pos_f < l_pac (anns[i].offset is contig_end[i - 1])
GBMK_HD int pos2rid(const Opt &o, const int64_t *contig_end, int64_t pos_f) {
  int left = 0, right = o.n_contigs;  // the first contig whose end lies beyond pos_f
  while (left < right) {
    const int mid = (left + right) >> 1;
    if (contig_end[mid] > pos_f) right = mid;
    else left = mid + 1;
  }
  return left;
}

// bns_intv2rid (bntseq.c:371-379) with bns_depos
GBMK_HD int intv2rid(const Opt &o, const int64_t *contig_end, int64_t rb, int64_t re) {
  if (rb < o.l_pac && re > o.l_pac) return -2;
  const int64_t b = rb >= o.l_pac ? (o.l_pac << 1) - 1 - rb : rb;
  const int64_t e1 = re - 1 >= o.l_pac ? (o.l_pac << 1) - 1 - (re - 1) : re - 1;
  const int rid_b = pos2rid(o, contig_end, b);
  const int rid_e = rb < re ? pos2rid(o, contig_end, e1) : rid_b;
  return rid_b == rid_e ? rid_b : -1;
}

// __kb_getp_aux: the position of the last key <= k after a lower-bound search, so that among equal keys
// the leftmost is found; *r is 0 on equality
GBMK_HD int getp_aux(const Node &x, int64_t k, int *r) {
  int begin = 0, end = x.n;
  if (x.n == 0) return -1;
  while (begin < end) {
    const int mid = (begin + end) >> 1;
    if (x.pos[mid] < k) begin = mid + 1;
    else end = mid;
  }
  if (begin == x.n) {
    *r = 1;
    return x.n - 1;
  }
  *r = (x.pos[begin] < k) - (k < x.pos[begin]);
  if (*r < 0) --begin;
  return begin;
}

// kb_intervalp's lower: the id of the chain found, or -1
GBMK_HD int tree_lower(const Node *nodes, int root, int64_t k) {
  int lower = -1, x = root;
  for (int lvl = 0; lvl < kTreeDepth; ++lvl) {
    const Node &nd = nodes[x];
    int r = 0;
    const int i = getp_aux(nd, k, &r);
    if (i >= 0 && r == 0) return nd.id[i];
    if (i >= 0) lower = nd.id[i];
    if (!nd.internal) break;
    x = nd.child[i + 1];
  }
  return lower;
}

// __kb_split: y = x.child[i] is full; its upper t - 1 keys move to a new node z behind it
GBMK_HD void tree_split(Node *nodes, int *n_nodes, int xi, int i, int yi) {
  const int zi = (*n_nodes)++;
  Node &x = nodes[xi], &y = nodes[yi], &z = nodes[zi];
  z.internal = y.internal;
  z.n = kT - 1;
  for (int j = 0; j < kT - 1; ++j) z.pos[j] = y.pos[kT + j], z.id[j] = y.id[kT + j];
  if (y.internal)
    for (int j = 0; j < kT; ++j) z.child[j] = y.child[kT + j];
  y.n = kT - 1;
  for (int j = x.n; j > i; --j) x.child[j + 1] = x.child[j];
  x.child[i + 1] = zi;
  for (int j = x.n; j > i; --j) x.pos[j] = x.pos[j - 1], x.id[j] = x.id[j - 1];
  x.pos[i] = y.pos[kT - 1], x.id[i] = y.id[kT - 1];
  ++x.n;
}

// kb_putp
GBMK_HD void tree_put(Node *nodes, int *n_nodes, int *root, int64_t k, int id) {
  if (nodes[*root].n == kKeys) {
    const int s = (*n_nodes)++;
    nodes[s].internal = 1, nodes[s].n = 0;
    nodes[s].child[0] = *root;
    tree_split(nodes, n_nodes, s, 0, *root);
    *root = s;
  }
  int xi = *root;
  for (int lvl = 0; lvl < kTreeDepth; ++lvl) {
    Node &x = nodes[xi];
    int r = 0;
    if (!x.internal) {
      const int i = getp_aux(x, k, &r);
      for (int j = x.n - 1; j > i; --j) x.pos[j + 1] = x.pos[j], x.id[j + 1] = x.id[j];
      x.pos[i + 1] = k, x.id[i + 1] = id;
      ++x.n;
      return;
    }
    int i = getp_aux(x, k, &r) + 1;
    if (nodes[x.child[i]].n == kKeys) {
      tree_split(nodes, n_nodes, xi, i, x.child[i]);
      if (k > x.pos[i]) ++i;
    }
    xi = x.child[i];
  }
}

// __kb_traverse: in order. A level's state is 2 * i + phase: phase 0 descends into child i, phase 1 emits key i.
GBMK_HD int tree_traverse(const Node *nodes, int root, int32_t *order) {
  int sx[kTreeDepth], si[kTreeDepth], top = 0, n = 0;
  sx[0] = root, si[0] = 0;
  while (top >= 0) {
    const Node &x = nodes[sx[top]];
    const int i = si[top] >> 1;
    if (i > x.n) {
      --top;
      continue;
    }
    if (!(si[top] & 1)) {
      si[top] |= 1;
      if (x.internal && top + 1 < kTreeDepth) {
        ++top;
        sx[top] = x.child[i], si[top] = 0;
      }
      continue;
    }
    if (i < x.n) order[n++] = x.id[i];
    si[top] = 2 * (i + 1);
  }
  return n;
}

// mem_chain's loop over the sorted SMEMs of one read (bwamem.c:265-309). The nodes of the slice start
// zeroed or not: every field read was written before.
GBMK_HD void build_read(const Opt &o, const int64_t *contig_end, const ReadItem &rd, const SMem *mems,
                        const int64_t *coords, const ReadWs &ws, ReadOut *out) {
  out->n_chains = out->n_out = out->l_rep = out->pad = 0;
  if (rd.l_query < o.min_seed_len) {
    for (int p = 0; p < rd.n_coords; ++p) ws.cc[p] = -1;
    return;
  }
  int b = 0, e = 0, l_rep = 0;
  for (int i = 0; i < rd.n_mems; ++i) {
    const SMem &m = mems[i];
    if (!m.rep) continue;
    const int sb = m.qbeg, se = m.qbeg + m.len;
    if (sb > e) l_rep += e - b, b = sb, e = se;
    else e = e > se ? e : se;
  }
  l_rep += e - b;
  out->l_rep = l_rep;
  int n_keys = 0, n_nodes = 1, root = 0, p = 0;
  ws.nodes[0].n = 0, ws.nodes[0].internal = 0;
  for (int i = 0; i < rd.n_mems; ++i) {
    const SMem &m = mems[i];
    for (int j = 0; j < m.n_coord; ++j, ++p) {
      const int64_t rbeg = coords[m.coord_off + j];
      ws.cc[p] = -1;
      const int rid = intv2rid(o, contig_end, rbeg, rbeg + m.len);
      if (rid < 0) continue;
      bool to_add = true;
      if (n_keys) {
        const int lo = tree_lower(ws.nodes, root, rbeg);
        if (lo >= 0) {  // test_and_merge (bwamem.c:190-211)
          Chain &c = ws.ch[lo];
          const int64_t qend = c.last_qbeg + c.last_len, rend = c.last_rbeg + c.last_len;
          if (rid == c.rid) {
            if (m.qbeg >= c.first_qbeg && m.qbeg + m.len <= qend && rbeg >= c.pos && rbeg + m.len <= rend) {
              to_add = false;  // contained
            } else if (!((c.last_rbeg < o.l_pac || c.pos < o.l_pac) && rbeg >= o.l_pac)) {
              const int64_t x = m.qbeg - c.last_qbeg, y = rbeg - c.last_rbeg;
              if (y >= 0 && x - y <= o.w && y - x <= o.w && x - c.last_len < o.max_chain_gap &&
                  y - c.last_len < o.max_chain_gap) {
                to_add = false;
                ws.cc[p] = lo;
              }
            }
          }
        }
      }
      int id = ws.cc[p];
      if (to_add) {
        id = n_keys++;
        Chain &c = ws.ch[id];
        c.pos = rbeg, c.first_qbeg = m.qbeg, c.rid = rid, c.n = 0;
        c.wq = c.wr = c.end_q = 0, c.end_r = 0;
        c.w = c.kept = c.cursor = 0, c.out = -1;
        ws.cc[p] = id;
        tree_put(ws.nodes, &n_nodes, &root, rbeg, id);
      }
      if (id >= 0) {  // the seed is appended: mem_chain_weight's two folds (bwamem.c:217-229) advance
        Chain &c = ws.ch[id];
        const int qe = m.qbeg + m.len;
        const int64_t re = rbeg + m.len;
        if (m.qbeg >= c.end_q) c.wq += m.len;
        else if (qe > c.end_q) c.wq += qe - c.end_q;
        c.end_q = c.end_q > qe ? c.end_q : qe;
        if (rbeg >= c.end_r) c.wr += m.len;
        else if (re > c.end_r) c.wr += (int)(re - c.end_r);
        c.end_r = c.end_r > re ? c.end_r : re;
        c.last_rbeg = rbeg, c.last_qbeg = m.qbeg, c.last_len = m.len;
        ++c.n;
      }
    }
  }
  out->n_chains = n_keys;
  if (n_keys) out->n_out = tree_traverse(ws.nodes, root, ws.order);
}

GBMK_HD void sort_swap(int64_t *a, int i, int j) {
  const int64_t t = a[i];
  a[i] = a[j], a[j] = t;
}

// flt_lt on weight << 32 | id
#define GBMK_LT(x, y) (((x) >> 32) > ((y) >> 32))

GBMK_HD void insertsort(int64_t *a, int n) {
  for (int i = 1; i < n; ++i)
    for (int j = i; j > 0 && GBMK_LT(a[j], a[j - 1]); --j) sort_swap(a, j, j - 1);
}

// ks_combsort (ksort.h:154-175)
GBMK_HD void combsort(int64_t *a, int n) {
  const double shrink_factor = 1.2473309501039786540366528676643;
  int do_swap, gap = n;
  do {
    if (gap > 2) {
      gap = (int)(gap / shrink_factor);
      if (gap == 9 || gap == 10) gap = 11;
    }
    do_swap = 0;
    for (int i = 0; i < n - gap; ++i) {
      const int j = i + gap;
      if (GBMK_LT(a[j], a[i])) {
        sort_swap(a, i, j);
        do_swap = 1;
      }
    }
  } while (do_swap || gap > 2);
  if (gap != 1) insertsort(a, n);
}

// ks_introsort (ksort.h:176-226)
GBMK_HD void introsort(int64_t *a, int n) {
  if (n < 1) return;
  if (n == 2) {
    if (GBMK_LT(a[1], a[0])) sort_swap(a, 0, 1);
    return;
  }
  int d;
  for (d = 2; (1ll << d) < n; ++d) {
  }
  int sl[kSortStack], sr[kSortStack], sd[kSortStack], top = 0;
  int s = 0, t = n - 1;
  d <<= 1;
  for (;;) {
    if (s < t) {
      if (--d == 0) {
        combsort(a + s, t - s + 1);
        t = s;
        continue;
      }
      int i = s, j = t, k = i + ((j - i) >> 1) + 1;
      if (GBMK_LT(a[k], a[i])) {
        if (GBMK_LT(a[k], a[j])) k = j;
      } else {
        k = GBMK_LT(a[j], a[i]) ? i : j;
      }
      const int64_t rp = a[k];
      if (k != t) sort_swap(a, k, t);
      for (;;) {
        do ++i;
        while (GBMK_LT(a[i], rp));
        do --j;
        while (i <= j && GBMK_LT(rp, a[j]));
        if (j <= i) break;
        sort_swap(a, i, j);
      }
      sort_swap(a, i, t);
      if (i - s > t - i) {
        if (i - s > 16 && top < kSortStack) sl[top] = s, sr[top] = i - 1, sd[top] = d, ++top;
        s = t - i > 16 ? i + 1 : t;
      } else {
        if (t - i > 16 && top < kSortStack) sl[top] = i + 1, sr[top] = t, sd[top] = d, ++top;
        t = i - s > 16 ? i - 1 : s;
      }
    } else {
      if (top == 0) {
        insertsort(a, n);
        return;
      }
      --top;
      s = sl[top], t = sr[top], d = sd[top];
    }
  }
}

// mem_chain_flt (bwamem.c:327-385) on the chains of one read: in ws.order the traversal, out the chains
// the filter leaves, in its order
GBMK_HD void filter_read(const Opt &o, const ReadWs &ws, ReadOut *out) {
  Chain *ch = ws.ch;
  const int n0 = out->n_chains;
  if (n0 == 0) return;
  int n = 0;
  for (int i = 0; i < n0; ++i) {
    const int id = ws.order[i];
    Chain &c = ch[id];
    c.kept = 0;
    int w = c.wr < c.wq ? c.wr : c.wq;
    w = w < 1 << 30 ? w : (1 << 30) - 1;
    c.w = w & ((1 << 29) - 1);  // uint32_t w:29
    if (c.w >= o.min_chain_weight) ws.perm[n++] = ((int64_t)c.w << 32) | (uint32_t)id;
  }
  introsort(ws.perm, n);
  const int64_t *a = ws.perm;
#define GBMK_ID(x) ((int)((x) & 0xffffffff))
  if (n == 0) {  // a[0].kept = 3 lands on a chain that was dropped: nothing is left
    out->n_out = 0;
    return;
  }
  constexpr int kAlt = 1 << 30;
  int nk = 0;
  {
    Chain &c = ch[GBMK_ID(a[0])];  // is_alt is carried in the sign of rid while the read is filtered
    c.kept = 3;
    ws.kept[nk++] = Kept{c.first_qbeg, c.last_qbeg + c.last_len, c.w | (c.rid < 0 ? kAlt : 0), -1};
  }
  for (int i = 1; i < n; ++i) {
    Chain &ci = ch[GBMK_ID(a[i])];
    const int bi = ci.first_qbeg, ei = ci.last_qbeg + ci.last_len, wi = ci.w;
    const bool alt_i = ci.rid < 0;
    int large_ovlp = 0, k;
    for (k = 0; k < nk; ++k) {
      Kept cj = ws.kept[k];
      const int b_max = cj.beg > bi ? cj.beg : bi, e_min = cj.end < ei ? cj.end : ei;
      if (e_min > b_max && (!(cj.w_alt & kAlt) || alt_i)) {
        const int li = ei - bi, lj = cj.end - cj.beg, wj = cj.w_alt & ~kAlt;
        const int min_l = li < lj ? li : lj;
        if ((float)(e_min - b_max) >= (float)min_l * o.mask_level && min_l < o.max_chain_gap) {
          large_ovlp = 1;
          if (cj.first < 0) ws.kept[k].first = i;
          if ((float)wi < (float)wj * o.drop_ratio && wj - wi >= o.min_seed_len << 1) break;
        }
      }
    }
    if (k == nk) {
      ws.kept[nk++] = Kept{bi, ei, wi | (alt_i ? kAlt : 0), -1};
      ci.kept = large_ovlp ? 2 : 3;
    }
  }
  for (int i = 0; i < nk; ++i) {
    const int first = ws.kept[i].first;
    if (first >= 0) ch[GBMK_ID(a[first])].kept = 1;
  }
  int i = 0;
  for (int k = 0; i < n; ++i) {
    const int kept = ch[GBMK_ID(a[i])].kept;
    if (kept == 0 || kept == 3) continue;
    if (++k >= o.max_chain_extend) break;
  }
  for (; i < n; ++i)
    if (ch[GBMK_ID(a[i])].kept < 3) ch[GBMK_ID(a[i])].kept = 0;
  int m = 0;
  for (i = 0; i < n; ++i)
    if (ch[GBMK_ID(a[i])].kept != 0) ws.order[m++] = GBMK_ID(a[i]);
  out->n_out = m;
#undef GBMK_ID
}

// the read's info records and seed counts at its chains' places in the output
GBMK_HD void count_read(const Opt &o, const ReadWs &ws, const ReadOut &ro, int64_t chain_base, int32_t *chain_cnt) {
  for (int j = 0; j < ro.n_out; ++j) chain_cnt[chain_base + j] = ws.ch[ws.order[j]].n;
}

// stable scatter of the read's seeds by chain into the CSR, and the info records
GBMK_HD void emit_read(const Opt &o, const ReadItem &rd, const SMem *mems, const int64_t *coords, const ReadWs &ws,
                       const ReadOut &ro, int64_t chain_base, const int64_t *chain_seed_off, gb_bsw_seed *seeds,
                       gb_bsw_chain_info *info) {
  for (int j = 0; j < ro.n_out; ++j) {
    Chain &c = ws.ch[ws.order[j]];
    c.out = j;
    c.cursor = (int32_t)chain_seed_off[chain_base + j];
    gb_bsw_chain_info &f = info[chain_base + j];
    f.pos = c.pos;
    f.rid = c.rid < 0 ? ~c.rid : c.rid;
    f.is_alt = c.rid < 0;
    f.w = o.stage ? c.w : 0;
    f.kept = o.stage ? c.kept : 0;
    f.l_rep = ro.l_rep;
    f.frac_rep = 0.f;  // divided on the host
  }
  int p = 0;
  for (int i = 0; i < rd.n_mems; ++i) {
    const SMem &m = mems[i];
    for (int j = 0; j < m.n_coord; ++j, ++p) {
      const int id = ws.cc[p];
      if (id < 0 || ws.ch[id].out < 0) continue;
      gb_bsw_seed &s = seeds[ws.ch[id].cursor++];
      s.rbeg = coords[m.coord_off + j];
      s.qbeg = m.qbeg, s.len = m.len, s.score = m.len, s.pad = 0;
    }
  }
}

struct DevArgs {
  Opt opt;
  const int64_t *contig_end;
  const uint8_t *contig_is_alt;
  const ReadItem *reads;
  const SMem *mems;
  const int64_t *coords;
  int64_t n_reads;
  Chain *ch;
  Node *nodes;
  int32_t *cc, *order;
  int64_t *perm;
  Kept *kept;
  const int32_t *lane_read;  // the read of each lane of the filter kernel: by decreasing coordinate count
  ReadOut *rout;
  int32_t *read_cnt;       // chains per read
  int64_t *read_chain_off;  // n_reads + 1
  int32_t *chain_cnt;      // seeds per chain
  int64_t *chain_seed_off;
  gb_bsw_seed *seeds;
  gb_bsw_chain_info *info;
};

__device__ inline ReadWs slice(const DevArgs &A, const ReadItem &rd) {
  ReadWs ws;
  ws.ch = A.ch + rd.coord_base, ws.nodes = A.nodes + rd.node_base;
  ws.cc = A.cc + rd.coord_base, ws.order = A.order + rd.coord_base;
  ws.perm = A.perm + rd.coord_base, ws.kept = A.kept + rd.coord_base;
  return ws;
}

// is_alt rides in the sign of rid (~rid) from the build to the emit: the filter's only use of it is the
// ALT rule, and test_and_merge compares rids of one table, so the mapping keeps both
__host__ __device__ inline void mark_alt(const uint8_t *is_alt, const ReadWs &ws, int n) {
  if (!is_alt) return;
  for (int i = 0; i < n; ++i)
    if (is_alt[ws.ch[i].rid]) ws.ch[i].rid = ~ws.ch[i].rid;
}

__global__ void __launch_bounds__(64) bsw_mkchain_build_kernel(DevArgs A) {
  const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= A.n_reads) return;
  const ReadItem rd = A.reads[r];
  ReadOut ro;
  ro.n_chains = ro.n_out = ro.l_rep = ro.pad = 0;
  if (!rd.host) {
    const ReadWs ws = slice(A, rd);
    build_read(A.opt, A.contig_end, rd, A.mems + rd.mem_off, A.coords, ws, &ro);
    mark_alt(A.contig_is_alt, ws, ro.n_chains);
  }
  A.rout[r] = ro;
}

__global__ void __launch_bounds__(64) bsw_mkchain_filter_kernel(DevArgs A) {
  const int64_t lane = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (lane >= A.n_reads) return;
  const int64_t r = A.lane_read[lane];
  const ReadItem rd = A.reads[r];
  ReadOut ro = A.rout[r];
  if (!rd.host && A.opt.stage) {
    filter_read(A.opt, slice(A, rd), &ro);
    A.rout[r] = ro;
  }
  A.read_cnt[r] = ro.n_out;
}

// out[0] = 0, out[i + 1] = cnt[0] + ... + cnt[i]. One block walks the counts in tiles of its width, so
// that neighbouring lanes load and store neighbouring words; a tile is scanned in LDS and the running
// total carried on.
__global__ void __launch_bounds__(kScanThreads) bsw_mkchain_scan_kernel(const int32_t *cnt, int64_t n, int64_t *out) {
  __shared__ int64_t part[kScanThreads];
  const int t = threadIdx.x;
  int64_t carry = 0;
  if (t == 0) out[0] = 0;
  for (int64_t base = 0; base < n; base += kScanThreads) {
    const int64_t i = base + t;
    part[t] = i < n ? cnt[i] : 0;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
      const int64_t v = t >= d ? part[t - d] : 0;
      __syncthreads();
      part[t] += v;
      __syncthreads();
    }
    if (i < n) out[i + 1] = carry + part[t];
    carry += part[kScanThreads - 1];
    __syncthreads();  // the next tile overwrites part[]
  }
}

__global__ void __launch_bounds__(64) bsw_mkchain_count_kernel(DevArgs A) {
  const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= A.n_reads) return;
  const ReadItem rd = A.reads[r];
  if (rd.host) return;
  count_read(A.opt, slice(A, rd), A.rout[r], A.read_chain_off[r], A.chain_cnt);
}

__global__ void __launch_bounds__(64) bsw_mkchain_emit_kernel(DevArgs A) {
  const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= A.n_reads) return;
  const ReadItem rd = A.reads[r];
  if (rd.host) return;
  emit_read(A.opt, rd, A.mems + rd.mem_off, A.coords, slice(A, rd), A.rout[r], A.read_chain_off[r], A.chain_seed_off,
            A.seeds, A.info);
}

// ---- host side ---------------------------------------------------------------------------------

struct Plan {
  Opt opt;
  std::vector<int64_t> contig_end;
  std::vector<SMem> mems;  // per read in mem_chain's order
  std::vector<ReadItem> reads;
  int64_t n_nodes = 0, host_reads = 0;
};

inline int expected_coords(int64_t s, int32_t max_occ) {
  const int64_t step = s > max_occ ? s / max_occ : 1;
  const int64_t cnt = (s + step - 1) / step;
  return (int)(cnt < max_occ ? cnt : max_occ);
}

int make_plan(const gb_bsw_chain_opt *opt, int32_t stage, int64_t l_pac, const int64_t *contig_end, int64_t n_contigs,
              int64_t n_reads, const int32_t *l_query, const gb_bsw_mem *mems, int64_t n_mems, const int64_t *coords,
              int64_t n_coords, bool all_host, int64_t dev_coords, Plan *P) {
  const char *who = "gb_bsw_seeds2chains";
  GB_ARG(opt, "%s: null opt", who);
  GB_ARG(stage == 0 || stage == 1, "%s: stage = %d (0: mem_chain, 1: and mem_chain_flt)", who, stage);
  GB_ARG(opt->max_occ >= 1, "%s: max_occ = %d", who, opt->max_occ);
  GB_ARG(opt->w >= 0, "%s: w = %d", who, opt->w);
  GB_ARG(opt->max_chain_gap >= 0, "%s: max_chain_gap = %d", who, opt->max_chain_gap);
  GB_ARG(opt->max_chain_extend >= 1, "%s: max_chain_extend = %d", who, opt->max_chain_extend);
  GB_ARG(std::isfinite(opt->mask_level), "%s: mask_level is not finite", who);
  GB_ARG(std::isfinite(opt->drop_ratio), "%s: drop_ratio is not finite", who);
  GB_ARG(opt->min_seed_len < (1 << 30) && opt->min_seed_len > -(1 << 30), "%s: min_seed_len = %d", who,
         opt->min_seed_len);
  GB_ARG(l_pac >= 1 && l_pac < (1ll << 61), "%s: l_pac = %lld", who, (long long)l_pac);
  GB_ARG(n_reads >= 0 && n_mems >= 0 && n_coords >= 0, "%s: negative count", who);
  GB_ARG(n_reads < (1ll << 31), "%s: %lld reads (the call takes fewer than 2^31)", who, (long long)n_reads);
  GB_ARG(n_coords < (1ll << 31), "%s: %lld coordinates (the call takes fewer than 2^31)", who, (long long)n_coords);
  GB_ARG(n_reads == 0 || l_query, "%s: null l_query", who);
  GB_ARG(n_mems == 0 || mems, "%s: null mems", who);
  GB_ARG(n_coords == 0 || coords, "%s: null coords", who);
  if (contig_end) {
    GB_ARG(n_contigs >= 1 && n_contigs < (1ll << 31), "%s: n_contigs = %lld", who, (long long)n_contigs);
    for (int64_t i = 0; i < n_contigs; ++i)
      GB_ARG(contig_end[i] > (i ? contig_end[i - 1] : 0), "%s: contig_end[%lld] = %lld does not increase", who,
             (long long)i, (long long)contig_end[i]);
    GB_ARG(contig_end[n_contigs - 1] == l_pac, "%s: contig_end ends at %lld, l_pac is %lld", who,
           (long long)contig_end[n_contigs - 1], (long long)l_pac);
    P->contig_end.assign(contig_end, contig_end + n_contigs);
  } else {
    P->contig_end.assign(1, l_pac);
  }
  Opt &o = P->opt;
  o.w = opt->w, o.max_chain_gap = opt->max_chain_gap, o.max_occ = opt->max_occ, o.min_seed_len = opt->min_seed_len;
  o.min_chain_weight = opt->min_chain_weight, o.max_chain_extend = opt->max_chain_extend;
  o.mask_level = opt->mask_level, o.drop_ratio = opt->drop_ratio;
  o.l_pac = l_pac, o.n_contigs = (int32_t)P->contig_end.size(), o.stage = stage;

  P->mems.resize((size_t)n_mems);
  P->reads.resize((size_t)n_reads);
  int64_t i = 0, cbase = 0;
  for (int64_t r = 0; r < n_reads; ++r) {
    ReadItem &rd = P->reads[(size_t)r];
    rd.mem_off = i, rd.coord_base = cbase, rd.node_base = P->n_nodes, rd.l_query = l_query[r];
    GB_ARG(l_query[r] >= 0, "%s: read %lld: l_query = %d", who, (long long)r, l_query[r]);
    int64_t nc = 0;
    for (; i < n_mems && mems[i].read == r; ++i) {
      const gb_bsw_mem &m = mems[i];
      GB_ARG(m.m >= 0 && m.n >= m.m && m.n < l_query[r], "%s: SMEM %lld of read %lld: [m, n] = [%d, %d], l_query = %d",
             who, (long long)i, (long long)r, m.m, m.n, l_query[r]);
      GB_ARG(m.s >= 1, "%s: SMEM %lld of read %lld: s = %lld", who, (long long)i, (long long)r, (long long)m.s);
      const int want = expected_coords(m.s, o.max_occ);
      GB_ARG(m.n_coord == want, "%s: SMEM %lld of read %lld: n_coord = %d, s = %lld at max_occ = %d gives %d", who,
             (long long)i, (long long)r, m.n_coord, (long long)m.s, o.max_occ, want);
      GB_ARG(cbase + nc + want <= n_coords, "%s: SMEM %lld of read %lld: the n_coord sum passes n_coords = %lld", who,
             (long long)i, (long long)r, (long long)n_coords);
      for (int j = 0; j < want; ++j) {
        const int64_t c = coords[cbase + nc + j];
        GB_ARG(c >= 0 && c < (l_pac << 1), "%s: SMEM %lld of read %lld: coordinate %lld = %lld outside [0, %lld)", who,
               (long long)i, (long long)r, (long long)(cbase + nc + j), (long long)c, (long long)(l_pac << 1));
      }
      SMem &s = P->mems[(size_t)i];
      s.coord_off = cbase + nc, s.qbeg = m.m, s.len = m.n + 1 - m.m, s.n_coord = want, s.rep = m.s > o.max_occ;
      nc += want;
    }
    GB_ARG(i == n_mems || (mems[i].read > r && mems[i].read < n_reads),
           "%s: SMEM %lld: read = %d after read %lld (reads must not decrease and lie in [0, %lld))", who, (long long)i,
           mems[i].read, (long long)r, (long long)n_reads);
    rd.n_mems = (int32_t)(i - rd.mem_off), rd.n_coords = (int32_t)nc;
    if (rd.n_mems && rd.l_query >= o.min_seed_len) {
      // mem_flt_chained_seeds (bwamem.c:600-602) must be the identity
      const double min_l = o.min_chain_weight ? 1.1f * o.min_chain_weight : 5.5f * std::log((double)rd.l_query);
      GB_ARG(min_l > 0.05f * rd.l_query,
             "%s: read %lld: l_query = %d is long enough for mem_flt_chained_seeds to re-score seeds (min_l = %g)", who,
             (long long)r, rd.l_query, min_l);
    }
    // mem_chain's order; equal keys are the same substring
    std::stable_sort(P->mems.begin() + rd.mem_off, P->mems.begin() + i, [](const SMem &a, const SMem &b) {
      return a.qbeg != b.qbeg ? a.qbeg < b.qbeg : a.len < b.len;
    });
    rd.host = all_host || nc > dev_coords;
    P->host_reads += rd.host;
    cbase += nc;
    P->n_nodes += nc / 4 + 2;
  }
  GB_ARG(i == n_mems, "%s: SMEM %lld: read = %d outside [0, %lld)", who, (long long)i, mems[i].read, (long long)n_reads);
  GB_ARG(cbase == n_coords, "%s: the SMEMs own %lld coordinates, n_coords = %lld", who, (long long)cbase,
         (long long)n_coords);
  return GB_OK;
}

// What the host path leaves for a range of reads, packed in read order
struct HostOut {
  std::vector<int32_t> n_out;  // per host read of the range
  std::vector<int32_t> chain_n;
  std::vector<gb_bsw_chain_info> info;
  std::vector<gb_bsw_seed> seeds;
};

void host_range(const Plan &P, const uint8_t *is_alt, const int64_t *coords, int64_t lo, int64_t hi, HostOut *H) {
  std::vector<Chain> ch;
  std::vector<Node> nodes;
  std::vector<int32_t> ids;
  std::vector<int64_t> cso, perm;
  std::vector<Kept> kept;
  for (int64_t r = lo; r < hi; ++r) {
    const ReadItem &rd = P.reads[(size_t)r];
    if (!rd.host) continue;
    const size_t n = (size_t)rd.n_coords;
    if (ch.size() < n + 1) ch.resize(n + 1), ids.resize(2 * (n + 1)), perm.resize(n + 1), kept.resize(n + 1);
    if (nodes.size() < n / 4 + 2) nodes.resize(n / 4 + 2);
    ReadWs ws;
    ws.ch = ch.data(), ws.nodes = nodes.data();
    ws.cc = ids.data(), ws.order = ids.data() + n, ws.perm = perm.data(), ws.kept = kept.data();
    ReadOut ro;
    const SMem *mems = P.mems.data() + rd.mem_off;
    build_read(P.opt, P.contig_end.data(), rd, mems, coords, ws, &ro);
    mark_alt(is_alt, ws, ro.n_chains);
    if (P.opt.stage) filter_read(P.opt, ws, &ro);
    H->n_out.push_back(ro.n_out);
    const size_t c0 = H->info.size(), s0 = H->seeds.size();
    cso.assign((size_t)ro.n_out + 1, 0);
    for (int j = 0; j < ro.n_out; ++j) {
      const int cn = ch[(size_t)ws.order[j]].n;
      H->chain_n.push_back(cn);
      cso[(size_t)j + 1] = cso[(size_t)j] + cn;
    }
    H->info.resize(c0 + (size_t)ro.n_out);
    H->seeds.resize(s0 + (size_t)cso[(size_t)ro.n_out]);
    emit_read(P.opt, rd, mems, coords, ws, ro, 0, cso.data(), H->seeds.data() + s0, H->info.data() + c0);
  }
}

struct MWs {  // the calling thread's, through gb::thread_ws
  int device = -1;
  gb::Stream stream;
  gb::Event ev[4];
  gb::PinnedBuf<uint8_t> h_in;
  gb::DevBuf<uint8_t> d_in;
  gb::DevBuf<Chain> d_ch;
  gb::DevBuf<Node> d_nodes;
  gb::DevBuf<int32_t> d_ids, d_read_cnt, d_chain_cnt;
  gb::DevBuf<int64_t> d_perm;
  gb::DevBuf<Kept> d_kept;
  std::vector<int32_t> lane_read;
  gb::DevBuf<ReadOut> d_rout;
  gb::DevBuf<int64_t> d_rco, d_cso;
  gb::DevBuf<gb_bsw_seed> d_seeds;
  gb::DevBuf<gb_bsw_chain_info> d_info;
};

struct Timing {
  float build_ms, filter_ms, emit_ms;
  int64_t host_reads;
  bool valid;
};
thread_local Timing g_timing = {0.f, 0.f, 0.f, 0, false};

int get_ws(int dev, MWs **out) {
  return gb::thread_ws(dev, out, [](int dev, MWs **out) {
    auto *W = new MWs();
    W->device = dev;
    hipError_t e = W->stream.create();
    for (auto &ev : W->ev)
      if (e == hipSuccess) e = ev.create();
    if (e != hipSuccess) {
      gb::set_error("gb_bsw_seeds2chains workspace: %s", hipGetErrorString(e));
      delete W;
      return GB_ERR_HIP;
    }
    *out = W;
    return GB_OK;
  });
}

// The device reads of the call: CSR over all reads (a host read owns no chain here) into the given host
// arrays, which hold n_reads + 1, n_coords + 1, n_coords and n_coords entries.
int run_device(const Plan &P, const uint8_t *is_alt, const int64_t *coords, int64_t n_coords, int64_t *rco, int64_t *cso,
               gb_bsw_seed *seeds, gb_bsw_chain_info *info, int64_t chain_cap, int64_t seed_cap, int64_t *n_chains,
               int64_t *n_seeds) {
  int dev = 0, st;
  GB_HIP(hipGetDevice(&dev));
  MWs *W = nullptr;
  if ((st = get_ws(dev, &W))) return st;
  const int64_t nr = (int64_t)P.reads.size(), nm = (int64_t)P.mems.size(), nct = (int64_t)P.contig_end.size();
  const int64_t ncz = std::max<int64_t>(n_coords, 1);
  int64_t size = 0;
  auto take = [&](int64_t bytes) {
    const int64_t at = size;
    size += gb::round_up<int64_t>(std::max<int64_t>(bytes, 1), 16);
    return at;
  };
  const int64_t o_reads = take(nr * (int64_t)sizeof(ReadItem)), o_mems = take(nm * (int64_t)sizeof(SMem)),
                o_coords = take(n_coords * 8), o_ce = take(nct * 8), o_alt = take(nct), o_lane = take(nr * 4);
  if ((st = W->h_in.reserve((size_t)size, (size_t)size * 2))) return st;
  if ((st = W->d_in.reserve((size_t)size, (size_t)size * 2))) return st;
  if ((st = W->d_ch.reserve((size_t)ncz))) return st;
  if ((st = W->d_nodes.reserve((size_t)std::max<int64_t>(P.n_nodes, 1)))) return st;
  if ((st = W->d_ids.reserve((size_t)(2 * ncz)))) return st;
  if ((st = W->d_perm.reserve((size_t)ncz))) return st;
  if ((st = W->d_kept.reserve((size_t)ncz))) return st;
  if ((st = W->d_read_cnt.reserve((size_t)nr))) return st;
  if ((st = W->d_chain_cnt.reserve((size_t)ncz))) return st;
  if ((st = W->d_rout.reserve((size_t)nr))) return st;
  if ((st = W->d_rco.reserve((size_t)nr + 1))) return st;
  if ((st = W->d_cso.reserve((size_t)ncz + 1))) return st;
  if ((st = W->d_seeds.reserve((size_t)ncz))) return st;
  if ((st = W->d_info.reserve((size_t)ncz))) return st;
  uint8_t *h = W->h_in, *d = W->d_in;
  std::memcpy(h + o_reads, P.reads.data(), (size_t)nr * sizeof(ReadItem));
  if (nm) std::memcpy(h + o_mems, P.mems.data(), (size_t)nm * sizeof(SMem));
  if (n_coords) std::memcpy(h + o_coords, coords, (size_t)n_coords * 8);
  std::memcpy(h + o_ce, P.contig_end.data(), (size_t)nct * 8);
  if (is_alt) std::memcpy(h + o_alt, is_alt, (size_t)nct);
  // The filter's time per read grows faster than linearly (the pairwise pass) and a wave takes as long as
  // its longest read, so there the reads go to the lanes by decreasing coordinate count: heavy reads
  // share waves (and start first), light waves retire quickly. The build and emit kernels keep the reads
  // in order: they are bound by memory locality, and neighbouring lanes then work on neighbouring slices
  // (ordered lanes took the build kernel from 48 to 137 ms on the probe's set).
  W->lane_read.resize((size_t)nr);
  for (int64_t r = 0; r < nr; ++r) W->lane_read[(size_t)r] = (int32_t)r;
  if (nr > 64)
    std::stable_sort(W->lane_read.begin(), W->lane_read.end(), [&P](int32_t x, int32_t y) {
      return P.reads[(size_t)x].n_coords > P.reads[(size_t)y].n_coords;
    });
  std::memcpy(h + o_lane, W->lane_read.data(), (size_t)nr * 4);
  GB_HIP(hipMemcpyAsync(d, h, (size_t)size, hipMemcpyHostToDevice, W->stream));
  DevArgs A;
  A.opt = P.opt;
  A.contig_end = reinterpret_cast<const int64_t *>(d + o_ce);
  A.contig_is_alt = is_alt ? d + o_alt : nullptr;
  A.reads = reinterpret_cast<const ReadItem *>(d + o_reads);
  A.mems = reinterpret_cast<const SMem *>(d + o_mems);
  A.coords = reinterpret_cast<const int64_t *>(d + o_coords);
  A.n_reads = nr;
  A.ch = W->d_ch, A.nodes = W->d_nodes;
  int32_t *ids = W->d_ids.get();
  A.cc = ids, A.order = ids + ncz, A.perm = W->d_perm, A.kept = W->d_kept;
  A.lane_read = reinterpret_cast<const int32_t *>(d + o_lane);
  A.rout = W->d_rout;
  A.read_cnt = W->d_read_cnt, A.read_chain_off = W->d_rco;
  A.chain_cnt = W->d_chain_cnt, A.chain_seed_off = W->d_cso;
  A.seeds = W->d_seeds, A.info = W->d_info;
  const dim3 grid((unsigned)((nr + 63) / 64)), block(64);
  GB_HIP(hipEventRecord(W->ev[0], W->stream));
  hipLaunchKernelGGL(bsw_mkchain_build_kernel, grid, block, 0, W->stream, A);
  GB_HIP(hipGetLastError());
  GB_HIP(hipEventRecord(W->ev[1], W->stream));
  hipLaunchKernelGGL(bsw_mkchain_filter_kernel, grid, block, 0, W->stream, A);
  GB_HIP(hipGetLastError());
  GB_HIP(hipEventRecord(W->ev[2], W->stream));
  hipLaunchKernelGGL(bsw_mkchain_scan_kernel, dim3(1), dim3(kScanThreads), 0, W->stream, A.read_cnt, nr, A.read_chain_off);
  GB_HIP(hipGetLastError());
  // the chain count sizes the second scan
  int64_t nc = 0;
  GB_HIP(hipMemcpyAsync(&nc, W->d_rco.get() + nr, 8, hipMemcpyDeviceToHost, W->stream));
  GB_HIP(hipStreamSynchronize(W->stream));
  hipLaunchKernelGGL(bsw_mkchain_count_kernel, grid, block, 0, W->stream, A);
  GB_HIP(hipGetLastError());
  hipLaunchKernelGGL(bsw_mkchain_scan_kernel, dim3(1), dim3(kScanThreads), 0, W->stream, A.chain_cnt, nc, A.chain_seed_off);
  GB_HIP(hipGetLastError());
  hipLaunchKernelGGL(bsw_mkchain_emit_kernel, grid, block, 0, W->stream, A);
  GB_HIP(hipGetLastError());
  GB_HIP(hipEventRecord(W->ev[3], W->stream));
  int64_t ns = 0;
  GB_HIP(hipMemcpyAsync(&ns, W->d_cso.get() + nc, 8, hipMemcpyDeviceToHost, W->stream));
  GB_HIP(hipMemcpyAsync(rco, W->d_rco, (size_t)(nr + 1) * 8, hipMemcpyDeviceToHost, W->stream));
  GB_HIP(hipStreamSynchronize(W->stream));
  GB_HIP(hipEventElapsedTime(&g_timing.build_ms, W->ev[0], W->ev[1]));
  GB_HIP(hipEventElapsedTime(&g_timing.filter_ms, W->ev[1], W->ev[2]));
  GB_HIP(hipEventElapsedTime(&g_timing.emit_ms, W->ev[2], W->ev[3]));
  *n_chains = nc, *n_seeds = ns;
  if (nc <= chain_cap) GB_HIP(hipMemcpy(cso, W->d_cso, (size_t)(nc + 1) * 8, hipMemcpyDeviceToHost));
  if (nc <= chain_cap && ns <= seed_cap) {
    if (nc) GB_HIP(hipMemcpy(info, W->d_info, (size_t)nc * sizeof(gb_bsw_chain_info), hipMemcpyDeviceToHost));
    if (ns) GB_HIP(hipMemcpy(seeds, W->d_seeds, (size_t)ns * sizeof(gb_bsw_seed), hipMemcpyDeviceToHost));
  }
  return GB_OK;
}

}  // namespace gbmk

extern "C" {

void gb_bsw_chain_default_opt(gb_bsw_chain_opt *o) {
  if (!o) return;
  o->w = 100, o->max_chain_gap = 10000, o->max_occ = 500, o->min_seed_len = 19;
  o->min_chain_weight = 0, o->max_chain_extend = 1 << 30;
  o->mask_level = 0.50f, o->drop_ratio = 0.50f;
}

static int seeds2chains_impl(const gb_bsw_chain_opt *opt, int32_t stage, int64_t l_pac, const int64_t *contig_end,
                             const uint8_t *contig_is_alt, int64_t n_contigs, int64_t n_reads, const int32_t *l_query,
                             const gb_bsw_mem *mems, int64_t n_mems, const int64_t *coords, int64_t n_coords,
                             int64_t *read_chain_off, int64_t *chain_seed_off, gb_bsw_seed *seeds,
                             gb_bsw_chain_info *info, int64_t chain_cap, int64_t seed_cap, int64_t *chains_used,
                             int64_t *seeds_used) {
  using namespace gbmk;
  const char *who = "gb_bsw_seeds2chains";
  const bool all_host = gb::env_flag("GB_BSW_MKCHAIN_HOST");
  // GB_BSW_MKCHAIN_DEV_COORDS lowers (or raises) the bound above which a read takes the host path: the
  // tests reach the mixed call with it
  int64_t dev_coords = GB_BSW_MKCHAIN_DEV_COORDS;
  if (const char *de = getenv("GB_BSW_MKCHAIN_DEV_COORDS")) {
    char *end = nullptr;
    const long long v = strtoll(de, &end, 10);
    GB_ARG(end != de && *end == 0 && v >= 0, "%s: GB_BSW_MKCHAIN_DEV_COORDS = \"%s\" is not a count", who, de);
    dev_coords = v;
  }
  Plan P;
  int st = make_plan(opt, stage, l_pac, contig_end, n_contigs, n_reads, l_query, mems, n_mems, coords, n_coords,
                     all_host, dev_coords, &P);
  if (st) return st;
  GB_ARG(read_chain_off && chain_seed_off, "%s: null offsets", who);
  GB_ARG(chain_cap >= 0 && seed_cap >= 0 && (chain_cap == 0 || info) && (seed_cap == 0 || seeds),
         "%s: bad chain or seed buffer", who);
  g_timing = Timing{0.f, 0.f, 0.f, P.host_reads, true};
  if (chains_used) *chains_used = 0;
  if (seeds_used) *seeds_used = 0;
  read_chain_off[0] = 0;
  if (n_reads == 0) {
    chain_seed_off[0] = 0;
    return GB_OK;
  }
  const uint8_t *is_alt = contig_is_alt;

  // the host reads, on threads over contiguous ranges
  std::vector<HostOut> H;
  std::vector<int64_t> cut;
  if (P.host_reads) {
    int nth = 1;
    if ((st = gb::thread_count(who, "GB_BSW_MKCHAIN_THREADS", &nth))) return st;
    if (P.host_reads < 256) nth = 1;
    H.resize((size_t)nth);
    for (int t = 0; t <= nth; ++t) cut.push_back(n_reads * t / nth);
    if ((st = gb::parallel(who, nth, [&](int t) {
           host_range(P, is_alt, coords, cut[(size_t)t], cut[(size_t)t + 1], &H[(size_t)t]);
         })))
      return st;
  }
  const bool any_dev = P.host_reads < n_reads;
  // with both paths in one call the device's CSR is spliced with the host reads' afterwards
  const bool splice = any_dev && P.host_reads;
  std::vector<int64_t> d_rco, d_cso;
  std::vector<gb_bsw_seed> d_seeds;
  std::vector<gb_bsw_chain_info> d_info;
  int64_t dnc = 0, dns = 0;
  if (any_dev) {
    if (splice) {
      d_rco.resize((size_t)n_reads + 1), d_cso.resize((size_t)n_coords + 1);
      d_seeds.resize((size_t)n_coords), d_info.resize((size_t)n_coords);
      st = run_device(P, is_alt, coords, n_coords, d_rco.data(), d_cso.data(), d_seeds.data(), d_info.data(), n_coords,
                      n_coords, &dnc, &dns);
    } else {
      st = run_device(P, is_alt, coords, n_coords, read_chain_off, chain_seed_off, seeds, info, chain_cap, seed_cap,
                      &dnc, &dns);
    }
    if (st) return st;
  }
  int64_t nc = dnc, ns = dns;
  if (P.host_reads) {
    // totals and read_chain_off first, the rest only when the caps suffice
    for (auto &h : H) nc += (int64_t)h.info.size(), ns += (int64_t)h.seeds.size();
    int64_t c = 0;
    {
      size_t t = 0, k = 0;
      for (int64_t r = 0; r < n_reads; ++r) {
        while (r >= cut[t + 1]) ++t, k = 0;
        read_chain_off[r] = c;
        c += P.reads[(size_t)r].host ? H[t].n_out[k++] : d_rco[(size_t)r + 1] - d_rco[(size_t)r];
      }
      read_chain_off[n_reads] = c;
    }
    if (nc <= chain_cap) {
      const bool full = ns <= seed_cap;
      size_t t = 0, k = 0, hc = 0, hs = 0;  // cursors into H[t]
      int64_t oc = 0, os = 0;
      chain_seed_off[0] = 0;
      for (int64_t r = 0; r < n_reads; ++r) {
        while (r >= cut[t + 1]) ++t, k = 0, hc = 0, hs = 0;
        if (P.reads[(size_t)r].host) {
          const int n = H[t].n_out[k++];
          for (int j = 0; j < n; ++j) {
            const int cn = H[t].chain_n[hc];
            if (full) {
              info[oc] = H[t].info[hc];
              std::memcpy(seeds + os, H[t].seeds.data() + hs, (size_t)cn * sizeof(gb_bsw_seed));
            }
            ++hc, hs += (size_t)cn, os += cn;
            chain_seed_off[++oc] = os;
          }
        } else {
          for (int64_t c2 = d_rco[(size_t)r]; c2 < d_rco[(size_t)r + 1]; ++c2) {
            const int64_t s0 = d_cso[(size_t)c2], cn = d_cso[(size_t)c2 + 1] - s0;
            if (full) {
              info[oc] = d_info[(size_t)c2];
              std::memcpy(seeds + os, d_seeds.data() + s0, (size_t)cn * sizeof(gb_bsw_seed));
            }
            os += cn;
            chain_seed_off[++oc] = os;
          }
        }
      }
    }
  }
  if (chains_used) *chains_used = nc;
  if (seeds_used) *seeds_used = ns;
  GB_ARG(nc <= chain_cap && ns <= seed_cap, "%s: chain_cap = %lld, seed_cap = %lld, the call needs %lld and %lld", who,
         (long long)chain_cap, (long long)seed_cap, (long long)nc, (long long)ns);
  // frac_rep, divided on the host as the reference does (bwamem.c:310)
  for (int64_t r = 0; r < n_reads; ++r)
    for (int64_t c = read_chain_off[r]; c < read_chain_off[r + 1]; ++c)
      info[c].frac_rep = (float)info[c].l_rep / l_query[r];
  return GB_OK;
}

// The C ABI lets no exception out: the plan, the host path and the splice allocate and start threads.
int gb_bsw_seeds2chains(const gb_bsw_chain_opt *opt, int32_t stage, int64_t l_pac, const int64_t *contig_end,
                        const uint8_t *contig_is_alt, int64_t n_contigs, int64_t n_reads, const int32_t *l_query,
                        const gb_bsw_mem *mems, int64_t n_mems, const int64_t *coords, int64_t n_coords,
                        int64_t *read_chain_off, int64_t *chain_seed_off, gb_bsw_seed *seeds, gb_bsw_chain_info *info,
                        int64_t chain_cap, int64_t seed_cap, int64_t *chains_used, int64_t *seeds_used) {
  gb::Range range_("gb.bsw.seeds2chains");
  try {
    return seeds2chains_impl(opt, stage, l_pac, contig_end, contig_is_alt, n_contigs, n_reads, l_query, mems, n_mems,
                             coords, n_coords, read_chain_off, chain_seed_off, seeds, info, chain_cap, seed_cap,
                             chains_used, seeds_used);
  } catch (const std::bad_alloc &) {
    gb::set_error("gb_bsw_seeds2chains: out of host memory");
    return GB_ERR_NOMEM;
  } catch (const std::exception &e) {
    gb::set_error("gb_bsw_seeds2chains: %s", e.what());
    return GB_ERR_STATE;
  }
}

int gb_bsw_seeds2chains_timing(float *build_ms, float *filter_ms, float *emit_ms, int64_t *host_reads) {
  using namespace gbmk;
  if (!g_timing.valid) {
    gb::set_error("gb_bsw_seeds2chains_timing: no gb_bsw_seeds2chains call on this thread");
    return GB_ERR_STATE;
  }
  if (build_ms) *build_ms = g_timing.build_ms;
  if (filter_ms) *filter_ms = g_timing.filter_ms;
  if (emit_ms) *emit_ms = g_timing.emit_ms;
  if (host_reads) *host_reads = g_timing.host_reads;
  return GB_OK;
}

}  // extern "C"
