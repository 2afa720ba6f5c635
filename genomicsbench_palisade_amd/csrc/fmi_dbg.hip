// fmi_dbg.hip -- de Bruijn graph assembly of regions (include/gb_fmi_dbg.h; Platypus' assembleReadsAndDetectVariants
// with its k loop). DESIGN.md, "dbg", has the contract and the reasoning.
//
// Device: one workgroup per (region, k), seven short kernels a round. A region's walk positions ("edges") are numbered
// text by text (the reference, then the reads in pool order), so visit 2e is edge e's start k-mer and visit 2e + 1 its
// end k-mer, and the reference's insertion order is the order of the smallest visit of each k-mer.
//   clear   the region's node table, edge table and node arrays
//   build   every valid edge's two k-mers into an open-addressing table keyed by a 64-bit rolled fingerprint: first
//           visit by atomicMin, weight by integer add, colours by atomicOr; the slot of every visit is kept
//   rank    every visit's k bytes against the bytes of its slot's first visit (a mismatch is a fingerprint collision
//           and marks the region), then node ids as the ranks of the first visits (a scan over the visits)
//   edges   A: (start id, end id) into a second table with first edge and weight sum; B: each distinct edge appends
//           itself to its start node's list (8 entries; more marks the region); C: a lane per node sorts its list by
//           first edge, keeps 4, writes the node's record and counts the filtered in-degrees
//   cycle   Kahn peeling: a lane that removes a node goes on with a successor whose in-degree it emptied, so a chain
//           is one walk and not one barrier a node; the graph is cyclic exactly when nodes remain
// Only integer atomics are used and every value they leave is order-independent. Every loop has a bound (table
// capacity, node count, list length); a bound overrun marks the region and does not spin. A marked region is built
// again by the host path inside the same call. After a round the host gathers the regions that are cyclic with
// k <= k_max and launches them again at k + k_step.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "../../include/gb_fmi_dbg.h"
#include "fmi_dbg_internal.h"
#include "gb_common.h"
#include "gb_common_wave.h"

namespace {

using gb::dbg::fingerprint;
using gb::dbg::mix64;
using gb::dbg::poly;
using gb::dbg::roll;
using gb::dbg::Texts;
using gb::dbg::walk_edges;

constexpr int kThreads = 256, kRun = 8, kScanItems = 8, kList = 8;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int64_t kDefaultBudget = int64_t(8) << 30;
constexpr int64_t kSlotBytes = 48, kEdgeBytes = 12, kNodeBytes = 116;
enum { cNodes, cEdges, cNodeW, cEdgeW, cBoth, cCyclic, cRedo, cValid, cCount };
typedef unsigned long long ull;

struct Reg {  // one region of a round
  int64_t ref_beg, read_first, ebase_off, tab_off, edge_off, node_off;
  int32_t ref_len, n_texts, n_edges, node_cap;
  uint32_t cap;
  int32_t reserved;
};

struct Scratch {
  uint64_t *t_fp, *t_w, *e_key, *e_w;
  uint32_t *t_first, *t_col, *t_nid, *e_first;
  uint32_t *v_slot, *e_slot;
  uint32_t *n_first, *n_slot, *n_cnt, *n_lst, *n_indeg, *n_removed;
  int32_t *o_col, *o_ne, *o_to;
  int64_t *o_w, *o_ew;
  const int32_t *ebase;
  ull *counters;
};

struct Round {
  int k, min_qual, min_weight;
  uint64_t top, fp_mask;
};

// ------------------------------------------------------------------------------------------------------- device

// the text that holds edge e: the t with eb[t] <= e < eb[t + 1] (texts without an edge are passed over)
__device__ __forceinline__ int text_of(const int32_t *eb, int n_texts, int e) {
  int lo = 0, hi = n_texts - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (eb[mid + 1] > e)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ const uint8_t *text_ptr(const Texts &T, const Reg &R, int t, const uint8_t **qual) {
  if (t == 0) {
    *qual = nullptr;
    return T.ref_bytes + R.ref_beg;
  }
  const int64_t o = T.read_off[R.read_first + t - 1];
  *qual = T.qual + o;
  return T.seq + o;
}

// the slot of key in a table of mask + 1 slots, claimed if it was empty; kNone after mask + 1 probes
__device__ __forceinline__ uint32_t find_or_claim(uint64_t *keys, uint32_t mask, uint64_t key, uint64_t hash) {
  uint32_t h = (uint32_t)(hash ^ (hash >> 32)) & mask;
  for (uint32_t n = 0; n <= mask; ++n) {
    const ull cur = atomicCAS((ull *)&keys[h], 0ull, (ull)key);
    if (cur == 0 || cur == key) return h;
    h = (h + 1) & mask;
  }
  return kNone;
}

__global__ __launch_bounds__(kThreads) void k_dbg_clear(const Reg *regs, Scratch S) {
  const Reg R = regs[blockIdx.x];
  for (uint32_t i = threadIdx.x; i < R.cap; i += kThreads) {
    const int64_t o = R.tab_off + i;
    S.t_fp[o] = 0, S.t_w[o] = 0, S.t_first[o] = kNone, S.t_col[o] = 0, S.t_nid[o] = 0;
    S.e_key[o] = 0, S.e_w[o] = 0, S.e_first[o] = kNone;
  }
  for (int i = threadIdx.x; i < R.node_cap; i += kThreads) {
    const int64_t o = R.node_off + i;
    S.n_cnt[o] = 0, S.n_indeg[o] = 0, S.n_removed[o] = 0;
  }
  if (threadIdx.x < cCount) S.counters[(int64_t)blockIdx.x * cCount + threadIdx.x] = 0;
}

__global__ __launch_bounds__(kThreads) void k_dbg_build(const Reg *regs, Scratch S, Texts T, Round P) {
  const Reg R = regs[blockIdx.x];
  const int32_t *eb = S.ebase + R.ebase_off;
  const uint32_t mask = R.cap - 1;
  const int k = P.k, E = R.n_edges;
  uint64_t *fp = S.t_fp + R.tab_off;
  uint32_t *first = S.t_first + R.tab_off, *col = S.t_col + R.tab_off;
  uint64_t *wsum = S.t_w + R.tab_off;
  uint32_t *v_slot = S.v_slot + 2 * R.edge_off, *e_wt = S.e_slot + R.edge_off;
  ull *ctr = S.counters + (int64_t)blockIdx.x * cCount;
  int n_valid = 0;
  bool overrun = false;
  for (int e0 = threadIdx.x * kRun; e0 < E; e0 += kThreads * kRun) {
    const int e1 = min(E, e0 + kRun);
    int t = text_of(eb, R.n_texts, e0);
    const uint8_t *q, *s = text_ptr(T, R, t, &q);
    bool fresh = true;
    uint64_t p = 0;
    int cur_min = 0, n_n = 0;
    for (int e = e0; e < e1; ++e) {
      if (e >= eb[t + 1]) {
        do ++t;
        while (e >= eb[t + 1]);  // eb[n_texts] = E > e
        s = text_ptr(T, R, t, &q);
        fresh = true;
      }
      const int i = e - eb[t];
      if (fresh) p = poly(s + i, k);
      const uint64_t pn = roll(p, s[i], s[i + k], P.top);
      bool valid = true;
      uint32_t w = 1, colour = 1;
      if (q) {  // the smallest quality and the 'N's of the k + 1 bases i .. i + k
        if (fresh) {
          n_n = 0;
          for (int j = i; j <= i + k; ++j) n_n += s[j] == 'N';
        } else {
          n_n += (s[i + k] == 'N') - (s[i - 1] == 'N');
        }
        if (fresh || q[i - 1] == cur_min) {
          cur_min = 255;
          for (int j = i; j <= i + k; ++j) cur_min = min(cur_min, (int)q[j]);
        } else {
          cur_min = min(cur_min, (int)q[i + k]);
        }
        valid = cur_min >= P.min_qual && n_n == 0;
        w = (uint32_t)cur_min, colour = 2;
      }
      fresh = false;
      uint32_t sa = kNone, sb = kNone;
      if (valid) {
        const uint64_t fa = fingerprint(p, P.fp_mask), fb = fingerprint(pn, P.fp_mask);
        sa = find_or_claim(fp, mask, fa, fa);
        sb = find_or_claim(fp, mask, fb, fb);
        if (sa == kNone || sb == kNone) {
          overrun = true;
          sa = sb = kNone;
        } else {
          atomicMin(&first[sa], (uint32_t)(2 * e));
          atomicMin(&first[sb], (uint32_t)(2 * e + 1));
          atomicAdd((ull *)&wsum[sa], (ull)w);
          atomicAdd((ull *)&wsum[sb], (ull)w);
          atomicOr(&col[sa], colour);
          atomicOr(&col[sb], colour);
          ++n_valid;
        }
      }
      v_slot[2 * e] = sa, v_slot[2 * e + 1] = sb;
      e_wt[e] = w;
      p = pn;
    }
  }
  if (n_valid) atomicAdd(&ctr[cValid], (ull)n_valid);
  if (overrun) atomicOr((uint32_t *)&ctr[cRedo], 1u);
}

__device__ __forceinline__ const uint8_t *visit_bytes(const Texts &T, const Reg &R, const int32_t *eb, uint32_t v) {
  const int e = (int)(v >> 1), t = text_of(eb, R.n_texts, e);
  const uint8_t *q;
  return text_ptr(T, R, t, &q) + (e - eb[t]) + (int)(v & 1);
}

__global__ __launch_bounds__(kThreads) void k_dbg_rank(const Reg *regs, Scratch S, Texts T, Round P) {
  __shared__ int lds[4];
  const Reg R = regs[blockIdx.x];
  const int32_t *eb = S.ebase + R.ebase_off;
  const uint32_t *first = S.t_first + R.tab_off, *v_slot = S.v_slot + 2 * R.edge_off;
  uint32_t *nid = S.t_nid + R.tab_off, *n_first = S.n_first + R.node_off, *n_slot = S.n_slot + R.node_off;
  ull *ctr = S.counters + (int64_t)blockIdx.x * cCount;
  const int V = 2 * R.n_edges;
  bool differ = false;
  for (int v = threadIdx.x; v < V; v += kThreads) {
    const uint32_t h = v_slot[v];
    if (h == kNone) continue;
    const uint32_t fv = first[h];
    if (fv == (uint32_t)v) continue;
    const uint8_t *a = visit_bytes(T, R, eb, (uint32_t)v), *b = visit_bytes(T, R, eb, fv);
    for (int j = 0; j < P.k; ++j) differ |= a[j] != b[j];
  }
  if (differ) atomicOr((uint32_t *)&ctr[cRedo], 1u);
  int carry = 0;
  for (int c = 0; c < V; c += kThreads * kScanItems) {
    const int base = c + threadIdx.x * kScanItems;
    uint32_t slot[kScanItems];
    int n = 0;
    for (int j = 0; j < kScanItems; ++j) {
      const int v = base + j;
      const uint32_t h = v < V ? v_slot[v] : kNone;
      slot[j] = h != kNone && first[h] == (uint32_t)v ? h : kNone;
      n += slot[j] != kNone;
    }
    int total;
    int id = carry + gb::block_scan_excl<kThreads>(n, &total, lds);
    for (int j = 0; j < kScanItems; ++j)
      if (slot[j] != kNone) {
        if (id < R.node_cap) nid[slot[j]] = (uint32_t)id, n_first[id] = (uint32_t)(base + j), n_slot[id] = slot[j];
        ++id;
      }
    carry += total;
  }
  if (threadIdx.x == 0) {
    ctr[cNodes] = (ull)min(carry, R.node_cap);
    if (carry > R.node_cap) atomicOr((uint32_t *)&ctr[cRedo], 1u);
  }
}

__global__ __launch_bounds__(kThreads) void k_dbg_edges_a(const Reg *regs, Scratch S) {
  const Reg R = regs[blockIdx.x];
  const uint32_t mask = R.cap - 1;
  const uint32_t *v_slot = S.v_slot + 2 * R.edge_off, *nid = S.t_nid + R.tab_off;
  uint32_t *e_slot = S.e_slot + R.edge_off, *e_first = S.e_first + R.tab_off;
  uint64_t *e_key = S.e_key + R.tab_off, *e_w = S.e_w + R.tab_off;
  bool overrun = false;
  for (int e = threadIdx.x; e < R.n_edges; e += kThreads) {
    const uint32_t a = v_slot[2 * e], b = v_slot[2 * e + 1], w = e_slot[e];
    uint32_t h = kNone;
    if (a != kNone && b != kNone) {
      const uint64_t key = (((uint64_t)nid[a] << 32) | nid[b]) + 1;
      h = find_or_claim(e_key, mask, key, mix64(key));
      if (h == kNone) {
        overrun = true;
      } else {
        atomicMin(&e_first[h], (uint32_t)e);
        atomicAdd((ull *)&e_w[h], (ull)w);
      }
    }
    e_slot[e] = h;
  }
  if (overrun) atomicOr((uint32_t *)&S.counters[(int64_t)blockIdx.x * cCount + cRedo], 1u);
}

__global__ __launch_bounds__(kThreads) void k_dbg_edges_b(const Reg *regs, Scratch S) {
  const Reg R = regs[blockIdx.x];
  const uint32_t *e_slot = S.e_slot + R.edge_off, *e_first = S.e_first + R.tab_off;
  const uint64_t *e_key = S.e_key + R.tab_off;
  uint32_t *n_cnt = S.n_cnt + R.node_off, *n_lst = S.n_lst + kList * R.node_off;
  bool overrun = false;
  for (int e = threadIdx.x; e < R.n_edges; e += kThreads) {
    const uint32_t h = e_slot[e];
    if (h == kNone || e_first[h] != (uint32_t)e) continue;
    const uint32_t s = (uint32_t)((e_key[h] - 1) >> 32);
    if (s >= (uint32_t)R.node_cap) {
      overrun = true;
      continue;
    }
    const uint32_t at = atomicAdd(&n_cnt[s], 1u);
    if (at < (uint32_t)kList)
      n_lst[(int64_t)kList * s + at] = h;
    else
      overrun = true;
  }
  if (overrun) atomicOr((uint32_t *)&S.counters[(int64_t)blockIdx.x * cCount + cRedo], 1u);
}

__global__ __launch_bounds__(kThreads) void k_dbg_edges_c(const Reg *regs, Scratch S, Round P) {
  const Reg R = regs[blockIdx.x];
  ull *ctr = S.counters + (int64_t)blockIdx.x * cCount;
  const int N = (int)ctr[cNodes];
  const uint32_t *e_first = S.e_first + R.tab_off, *t_col = S.t_col + R.tab_off;
  const uint64_t *e_key = S.e_key + R.tab_off, *e_w = S.e_w + R.tab_off, *t_w = S.t_w + R.tab_off;
  const uint32_t *n_cnt = S.n_cnt + R.node_off, *n_lst = S.n_lst + kList * R.node_off, *n_slot = S.n_slot + R.node_off;
  uint32_t *n_indeg = S.n_indeg + R.node_off;
  int32_t *o_col = S.o_col + R.node_off, *o_ne = S.o_ne + R.node_off, *o_to = S.o_to + 4 * R.node_off;
  int64_t *o_w = S.o_w + R.node_off, *o_ew = S.o_ew + 4 * R.node_off;
  ull node_w = 0, edge_w = 0;
  uint32_t n_edges = 0, n_both = 0;
  for (int n = threadIdx.x; n < N; n += kThreads) {
    const int cnt = (int)min(n_cnt[n], (uint32_t)kList);
    uint32_t fst[kList], slot[kList];
    for (int j = 0; j < cnt; ++j) {  // insertion sort by first edge
      const uint32_t h = n_lst[(int64_t)kList * n + j], f = e_first[h];
      int at = j;
      for (; at > 0 && fst[at - 1] > f; --at) fst[at] = fst[at - 1], slot[at] = slot[at - 1];
      fst[at] = f, slot[at] = h;
    }
    const int ne = min(cnt, 4);
    const uint32_t colour = t_col[n_slot[n]];
    o_col[n] = (int32_t)colour, o_ne[n] = ne, o_w[n] = (int64_t)t_w[n_slot[n]];
    node_w += t_w[n_slot[n]], n_both += colour == 3, n_edges += (uint32_t)ne;
    for (int j = 0; j < 4; ++j) {
      int32_t to = -1;
      int64_t w = 0;
      if (j < ne) {
        to = (int32_t)(uint32_t)(e_key[slot[j]] - 1), w = (int64_t)e_w[slot[j]];
        if (to < 0 || to >= N) to = 0;  // only in a region that is already marked
        edge_w += (ull)w;
        if (!(t_col[n_slot[to]] == 2 && w < P.min_weight)) atomicAdd(&n_indeg[to], 1u);
      }
      o_to[4 * (int64_t)n + j] = to, o_ew[4 * (int64_t)n + j] = w;
    }
  }
  if (node_w) atomicAdd(&ctr[cNodeW], node_w);
  if (edge_w) atomicAdd(&ctr[cEdgeW], edge_w);
  if (n_edges) atomicAdd(&ctr[cEdges], (ull)n_edges);
  if (n_both) atomicAdd(&ctr[cBoth], (ull)n_both);
}

__device__ __forceinline__ uint32_t load_now(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kThreads) void k_dbg_cycle(const Reg *regs, Scratch S, Round P) {
  __shared__ int s_progress;
  __shared__ uint32_t s_total;
  const Reg R = regs[blockIdx.x];
  ull *ctr = S.counters + (int64_t)blockIdx.x * cCount;
  const int N = (int)ctr[cNodes];
  uint32_t *indeg = S.n_indeg + R.node_off, *removed = S.n_removed + R.node_off;
  const int32_t *o_col = S.o_col + R.node_off, *o_ne = S.o_ne + R.node_off, *o_to = S.o_to + 4 * R.node_off;
  const int64_t *o_ew = S.o_ew + 4 * R.node_off;
  if (threadIdx.x == 0) s_total = 0;
  bool overrun = false;
  int round = 0;
  for (; round <= N; ++round) {  // a round with progress removes a node, so round N finds none
    if (threadIdx.x == 0) s_progress = 0;
    __syncthreads();
    uint32_t cnt = 0;
    for (int n = threadIdx.x; n < N; n += kThreads) {
      if (load_now(&indeg[n]) != 0 || load_now(&removed[n]) != 0 || atomicExch(&removed[n], 1u) != 0) continue;
      int cur = n, step = 0;
      for (; cur >= 0 && step < N; ++step) {  // every step removes another node
        ++cnt;
        int next = -1;
        const int ne = o_ne[cur];
        for (int j = 0; j < ne; ++j) {
          const int to = o_to[4 * (int64_t)cur + j];
          if (o_col[to] == 2 && o_ew[4 * (int64_t)cur + j] < P.min_weight) continue;
          if (atomicSub(&indeg[to], 1u) == 1u && next < 0 && atomicExch(&removed[to], 1u) == 0) next = to;
        }
        cur = next;
      }
      overrun |= cur >= 0;
    }
    if (cnt) atomicAdd(&s_total, cnt), s_progress = 1;
    __syncthreads();
    const int progress = s_progress;
    __syncthreads();
    if (!progress) break;
  }
  if (overrun || round > N) atomicOr((uint32_t *)&ctr[cRedo], 1u);
  if (threadIdx.x == 0) ctr[cCyclic] = s_total < (uint32_t)N;
}

// ------------------------------------------------------------------------------------------------- host side

struct Stats {  // of the calling thread's last call
  float pack_ms, build_ms, rank_ms, edges_ms, cycle_ms, redo_ms;
  int64_t positions, valid, max_slots, ws_bytes, chunks, rounds, calls;
};
Stats &stats() {
  thread_local Stats s{};
  return s;
}

struct Ws : gb::WsBase<6> {};  // the calling thread's, through gb::get_ws

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct Graph {
  std::vector<int32_t> src, off, col, pos, ne, to;
  std::vector<int64_t> w, ew;
  bool cyclic = false;
  int64_t valid = 0;
  void resize(size_t n) {
    src.resize(n), off.resize(n), col.resize(n), pos.resize(n), ne.resize(n), w.resize(n);
    to.resize(4 * n), ew.resize(4 * n);
  }
};

struct Input {
  Texts T;
  const int32_t *ref_start;
  const int64_t *read_first, *read_last;
  const uint32_t *flag;
  gb_dbg_params P;
};

inline int64_t text_edges(const Input &in, int64_t r, int64_t t, int k) {
  if (t == 0) return walk_edges(in.T.ref_off[r + 1] - in.T.ref_off[r], k);
  const int64_t j = in.read_first[r] + t - 1;
  return in.flag[j] & 512u ? 0 : walk_edges(in.T.read_off[j + 1] - in.T.read_off[j], k);
}

// The graph of region r at k on the host: the reference's walk over a dictionary of k-byte views.
void build_host(const Input &in, int64_t r, int k, Graph *g) {
  *g = Graph();
  std::unordered_map<std::string_view, int32_t> ids;
  auto visit = [&](const uint8_t *p, int32_t src, int32_t off, int32_t colour, int32_t pos, int64_t w) {
    const auto ins = ids.try_emplace(std::string_view((const char *)p, (size_t)k), (int32_t)g->src.size());
    const int32_t id = ins.first->second;
    if (ins.second) {
      g->src.push_back(src), g->off.push_back(off), g->col.push_back(colour), g->pos.push_back(pos);
      g->w.push_back(w), g->ne.push_back(0);
      g->to.insert(g->to.end(), 4, -1), g->ew.insert(g->ew.end(), 4, 0);
    } else {
      g->col[(size_t)id] |= colour, g->w[(size_t)id] += w;
    }
    return id;
  };
  auto add_edge = [&](const uint8_t *s, int32_t src, int32_t i, int32_t colour, int64_t pos, int64_t w) {
    // a reference position is summed in 64 bits and cut to int32, as the device path's is; a read's is -1
    const int32_t a = visit(s + i, src, i, colour, (int32_t)pos, w);
    const int32_t b = visit(s + i + 1, src, i + 1, colour, src < 0 ? (int32_t)(pos + 1) : -1, w);
    for (int j = 0; j < 4; ++j) {
      if (j == g->ne[(size_t)a]) {
        g->to[4 * (size_t)a + j] = b, g->ew[4 * (size_t)a + j] = w, ++g->ne[(size_t)a];
        break;
      }
      if (g->to[4 * (size_t)a + j] == b) {
        g->ew[4 * (size_t)a + j] += w;
        break;
      }
    }
  };
  {
    const uint8_t *s = in.T.ref_bytes + in.T.ref_off[r];
    const int64_t n = walk_edges(in.T.ref_off[r + 1] - in.T.ref_off[r], k);
    ids.reserve((size_t)n + 16);
    for (int64_t i = 0; i < n; ++i) add_edge(s, -1, (int32_t)i, 1, (int64_t)in.ref_start[r] + i, 1);
  }
  for (int64_t j = in.read_first[r]; j < in.read_last[r]; ++j) {
    if (in.flag[j] & 512u) continue;
    const uint8_t *s = in.T.seq + in.T.read_off[j], *q = in.T.qual + in.T.read_off[j];
    const int64_t n = walk_edges(in.T.read_off[j + 1] - in.T.read_off[j], k);
    for (int64_t i = 0; i < n; ++i) {
      int mn = 100000000;
      bool has_n = false;
      for (int64_t x = i; x <= i + k; ++x) mn = std::min(mn, (int)q[x]), has_n |= s[x] == 'N';
      if (mn >= in.P.min_qual && !has_n) add_edge(s, (int32_t)j, (int32_t)i, 2, -1, mn), ++g->valid;
    }
  }
  g->valid += walk_edges(in.T.ref_off[r + 1] - in.T.ref_off[r], k);
  // Kahn peeling over the filtered edges: cyclic exactly when nodes remain
  const size_t N = g->src.size();
  std::vector<int32_t> indeg(N, 0), work;
  auto kept = [&](size_t n, int j) {
    return !(g->col[(size_t)g->to[4 * n + j]] == 2 && g->ew[4 * n + j] < in.P.min_weight);
  };
  for (size_t n = 0; n < N; ++n)
    for (int j = 0; j < g->ne[n]; ++j)
      if (kept(n, j)) ++indeg[(size_t)g->to[4 * n + j]];
  for (size_t n = 0; n < N; ++n)
    if (!indeg[n]) work.push_back((int32_t)n);
  size_t removed = 0;
  while (!work.empty()) {
    const size_t n = (size_t)work.back();
    work.pop_back(), ++removed;
    for (int j = 0; j < g->ne[n]; ++j)
      if (kept(n, j) && --indeg[(size_t)g->to[4 * n + j]] == 0) work.push_back(g->to[4 * n + j]);
  }
  g->cyclic = removed < N;
}

void summarize(const Graph &g, int k, gb_dbg_region_summary *s) {
  s->k = k, s->cyclic = g.cyclic, s->n_nodes = (int32_t)g.src.size();
  s->n_edges = s->n_ref_and_read = 0, s->node_weight_sum = s->edge_weight_sum = 0;
  for (size_t n = 0; n < g.src.size(); ++n) {
    s->n_edges += g.ne[n], s->n_ref_and_read += g.col[n] == 3, s->node_weight_sum += g.w[n];
    for (int j = 0; j < 4; ++j) s->edge_weight_sum += g.ew[4 * n + (size_t)j];
  }
}

}  // namespace

struct gb_dbg {
  bool keep = false;
  std::vector<gb_dbg_region_summary> sum;
  std::vector<Graph> graphs;  // keep only
};

namespace {

// true while the k loop goes on after a graph at k that was cyclic or not
inline bool goes_on(const gb_dbg_params &P, bool cyclic, int k) { return cyclic && k <= P.k_max; }

int assemble_host(const char *who, const Input &in, int64_t n_regions, gb_dbg *h) {
  int nth = 1, st;
  if ((st = gb::thread_count(who, "GB_DBG_THREADS", &nth))) return st;
  std::atomic<int64_t> next{0}, positions{0}, valid{0};
  st = gb::parallel(who, (int)std::max<int64_t>(1, std::min<int64_t>(nth, n_regions)), [&](int) {
    Graph g;
    for (int64_t r; (r = next.fetch_add(1)) < n_regions;) {
      gb_dbg_region_summary &s = h->sum[(size_t)r];
      for (int k = in.P.k0;; k += in.P.k_step) {
        build_host(in, r, k, &g);
        ++s.n_graphs;
        valid += g.valid;
        for (int64_t t = 0; t <= in.read_last[r] - in.read_first[r]; ++t) positions += text_edges(in, r, t, k);
        if (!goes_on(in.P, g.cyclic, k)) {
          summarize(g, k, &s);
          break;
        }
      }
      if (h->keep) h->graphs[(size_t)r] = std::move(g);
    }
  });
  Stats &S = stats();
  S.positions = positions.load(), S.valid = valid.load();
  return st;
}

struct Plan {  // of one region, at k0
  int64_t edges, n_texts, cap, node_cap, bytes;
};

int assemble_device(const char *who, const Input &in, int64_t n_regions, int64_t n_ref_bytes, int64_t n_read_bytes,
                    int64_t n_reads, const std::vector<Plan> &plan, int64_t budget, uint64_t fp_mask, gb_dbg *h) {
  int st, dev = -1;
  GB_HIP(hipGetDevice(&dev));
  Ws *W = nullptr;
  if ((st = gb::get_ws("gb_dbg", dev, &W))) return st;
  hipStream_t s = W->stream;
  Stats &S = stats();

  double t0 = now_ms();
  gb::DevBuf<uint8_t> d_ref, d_seq, d_qual;
  gb::DevBuf<int64_t> d_ref_off, d_read_off;
  if ((st = d_ref.reserve((size_t)n_ref_bytes + 1)) || (st = d_seq.reserve((size_t)n_read_bytes + 1)) ||
      (st = d_qual.reserve((size_t)n_read_bytes + 1)) || (st = d_ref_off.reserve((size_t)n_regions + 1)) ||
      (st = d_read_off.reserve((size_t)n_reads + 1)))
    return st;
  if (n_ref_bytes) GB_HIP(gb::memcpy_big(d_ref, in.T.ref_bytes, (size_t)n_ref_bytes, hipMemcpyHostToDevice));
  if (n_read_bytes) {
    GB_HIP(gb::memcpy_big(d_seq, in.T.seq, (size_t)n_read_bytes, hipMemcpyHostToDevice));
    GB_HIP(gb::memcpy_big(d_qual, in.T.qual, (size_t)n_read_bytes, hipMemcpyHostToDevice));
  }
  GB_HIP(hipMemcpy(d_ref_off, in.T.ref_off, 8 * (size_t)(n_regions + 1), hipMemcpyHostToDevice));
  if (n_reads)  // a call without a pool may pass no offsets, and no kernel reads them then
    GB_HIP(hipMemcpy(d_read_off, in.T.read_off, 8 * (size_t)(n_reads + 1), hipMemcpyHostToDevice));
  const Texts DT{d_ref, d_ref_off, d_seq, d_qual, d_read_off};
  S.pack_ms += (float)(now_ms() - t0);

  gb::DevBuf<uint64_t> t_fp, t_w, e_key, e_w;
  gb::DevBuf<uint32_t> t_first, t_col, t_nid, e_first, v_slot, e_slot, n_first, n_slot, n_cnt, n_lst, n_indeg, n_removed;
  gb::DevBuf<int32_t> o_col, o_ne, o_to, d_ebase;
  gb::DevBuf<int64_t> o_w, o_ew;
  gb::DevBuf<ull> d_ctr;
  gb::DevBuf<Reg> d_regs;
  std::vector<Reg> regs;
  std::vector<int32_t> ebase;
  std::vector<ull> ctr;
  std::vector<int64_t> active, still;
  std::vector<uint32_t> first;
  Graph g;

  for (int64_t r0 = 0; r0 < n_regions;) {
    int64_t r1 = r0, bytes = 0, slots = 0, edges = 0, nodes = 0, texts = 0;
    while (r1 < n_regions && (r1 == r0 || bytes + plan[(size_t)r1].bytes <= budget)) {
      const Plan &p = plan[(size_t)r1];
      bytes += p.bytes, slots += p.cap, edges += p.edges, nodes += p.node_cap, texts += p.n_texts + 1;
      ++r1;
    }
    ++S.chunks;
    S.ws_bytes = std::max(S.ws_bytes, bytes);
    const size_t ns = (size_t)slots + 1, ne = (size_t)edges + 1, nn = (size_t)nodes + 1, nr = (size_t)(r1 - r0);
    if ((st = t_fp.reserve(ns)) || (st = t_w.reserve(ns)) || (st = e_key.reserve(ns)) || (st = e_w.reserve(ns)) ||
        (st = t_first.reserve(ns)) || (st = t_col.reserve(ns)) || (st = t_nid.reserve(ns)) ||
        (st = e_first.reserve(ns)) || (st = v_slot.reserve(2 * ne)) || (st = e_slot.reserve(ne)) ||
        (st = n_first.reserve(nn)) || (st = n_slot.reserve(nn)) || (st = n_cnt.reserve(nn)) ||
        (st = n_lst.reserve(kList * nn)) || (st = n_indeg.reserve(nn)) || (st = n_removed.reserve(nn)) ||
        (st = o_col.reserve(nn)) || (st = o_ne.reserve(nn)) || (st = o_to.reserve(4 * nn)) || (st = o_w.reserve(nn)) ||
        (st = o_ew.reserve(4 * nn)) || (st = d_ebase.reserve((size_t)texts + 1)) ||
        (st = d_ctr.reserve(cCount * nr)) || (st = d_regs.reserve(nr)))
      return st;
    // the segments of the chunk's regions, sized at k0: a later round's walk is shorter
    std::vector<Reg> seg(nr);
    {
      int64_t so = 0, eo = 0, no = 0;
      for (int64_t r = r0; r < r1; ++r) {
        const Plan &p = plan[(size_t)r];
        Reg &R = seg[(size_t)(r - r0)];
        R = Reg{};
        R.ref_beg = in.T.ref_off[r], R.ref_len = (int32_t)(in.T.ref_off[r + 1] - in.T.ref_off[r]);
        R.read_first = in.read_first[r], R.n_texts = (int32_t)p.n_texts;
        R.tab_off = so, R.edge_off = eo, R.node_off = no, R.cap = (uint32_t)p.cap, R.node_cap = (int32_t)p.node_cap;
        so += p.cap, eo += p.edges, no += p.node_cap;
      }
    }
    active.clear();
    for (int64_t r = r0; r < r1; ++r) active.push_back(r);
    for (int k = in.P.k0; !active.empty(); k += in.P.k_step) {
      t0 = now_ms();
      regs.clear(), ebase.clear();
      for (const int64_t r : active) {
        Reg R = seg[(size_t)(r - r0)];
        R.ebase_off = (int64_t)ebase.size();
        int64_t e = 0;
        for (int t = 0; t < R.n_texts; ++t) ebase.push_back((int32_t)e), e += text_edges(in, r, t, k);
        ebase.push_back((int32_t)e);
        R.n_edges = (int32_t)e;
        S.positions += e;
        regs.push_back(R);
      }
      const int na = (int)active.size();
      GB_HIP(hipMemcpyAsync(d_regs, regs.data(), sizeof(Reg) * regs.size(), hipMemcpyHostToDevice, s));
      GB_HIP(hipMemcpyAsync(d_ebase, ebase.data(), 4 * ebase.size(), hipMemcpyHostToDevice, s));
      const Scratch SC{t_fp,   t_w,    e_key, e_w,     t_first,   t_col, t_nid, e_first, v_slot, e_slot, n_first, n_slot,
                       n_cnt,  n_lst,  n_indeg, n_removed, o_col, o_ne,  o_to,  o_w,     o_ew,   d_ebase, d_ctr};
      Round P{k, in.P.min_qual, in.P.min_weight, 1, fp_mask};
      for (int j = 1; j < k; ++j) P.top *= gb::dbg::kBase;
      S.pack_ms += (float)(now_ms() - t0);
      GB_HIP(hipEventRecord(W->ev[0], s));
      k_dbg_clear<<<na, kThreads, 0, s>>>(d_regs, SC);
      k_dbg_build<<<na, kThreads, 0, s>>>(d_regs, SC, DT, P);
      GB_HIP(hipEventRecord(W->ev[1], s));
      k_dbg_rank<<<na, kThreads, 0, s>>>(d_regs, SC, DT, P);
      GB_HIP(hipEventRecord(W->ev[2], s));
      k_dbg_edges_a<<<na, kThreads, 0, s>>>(d_regs, SC);
      k_dbg_edges_b<<<na, kThreads, 0, s>>>(d_regs, SC);
      k_dbg_edges_c<<<na, kThreads, 0, s>>>(d_regs, SC, P);
      GB_HIP(hipEventRecord(W->ev[3], s));
      k_dbg_cycle<<<na, kThreads, 0, s>>>(d_regs, SC, P);
      GB_HIP(hipEventRecord(W->ev[4], s));
      GB_HIP(hipGetLastError());
      ctr.resize((size_t)cCount * (size_t)na);
      GB_HIP(hipMemcpyAsync(ctr.data(), d_ctr, 8 * ctr.size(), hipMemcpyDeviceToHost, s));
      GB_HIP(hipStreamSynchronize(s));
      ++S.rounds;
      float ms[4];
      for (int i = 0; i < 4; ++i) GB_HIP(hipEventElapsedTime(&ms[i], W->ev[i], W->ev[i + 1]));
      S.build_ms += ms[0], S.rank_ms += ms[1], S.edges_ms += ms[2], S.cycle_ms += ms[3];

      still.clear();
      for (int a = 0; a < na; ++a) {
        const int64_t r = active[(size_t)a];
        const ull *c = ctr.data() + (size_t)cCount * (size_t)a;
        const Reg &R = regs[(size_t)a];
        gb_dbg_region_summary &sm = h->sum[(size_t)r];
        ++sm.n_graphs;
        bool cyclic, have_graph = false;
        if (c[cRedo]) {  // a fingerprint collision or a bound overrun: this graph again, on the host
          t0 = now_ms();
          build_host(in, r, k, &g);
          cyclic = g.cyclic, have_graph = true, sm.redone = 1;
          S.valid += g.valid;
          S.redo_ms += (float)(now_ms() - t0);
        } else {
          cyclic = c[cCyclic] != 0;
          S.valid += (int64_t)c[cValid];
        }
        if (goes_on(in.P, cyclic, k)) {
          still.push_back(r);
          continue;
        }
        if (have_graph) {
          summarize(g, k, &sm);
        } else {
          sm.k = k, sm.cyclic = cyclic, sm.n_nodes = (int32_t)c[cNodes], sm.n_edges = (int32_t)c[cEdges];
          sm.n_ref_and_read = (int32_t)c[cBoth], sm.node_weight_sum = (int64_t)c[cNodeW];
          sm.edge_weight_sum = (int64_t)c[cEdgeW];
        }
        if (!h->keep) continue;
        if (!have_graph) {  // the node records, and src / off / position from the first visits
          const size_t N = (size_t)c[cNodes];
          g = Graph();
          g.resize(N), first.resize(N);
          g.cyclic = cyclic;
          if (N) {
            GB_HIP(hipMemcpy(first.data(), n_first + R.node_off, 4 * N, hipMemcpyDeviceToHost));
            GB_HIP(hipMemcpy(g.col.data(), o_col + R.node_off, 4 * N, hipMemcpyDeviceToHost));
            GB_HIP(hipMemcpy(g.ne.data(), o_ne + R.node_off, 4 * N, hipMemcpyDeviceToHost));
            GB_HIP(hipMemcpy(g.w.data(), o_w + R.node_off, 8 * N, hipMemcpyDeviceToHost));
            GB_HIP(hipMemcpy(g.to.data(), o_to + 4 * R.node_off, 16 * N, hipMemcpyDeviceToHost));
            GB_HIP(hipMemcpy(g.ew.data(), o_ew + 4 * R.node_off, 32 * N, hipMemcpyDeviceToHost));
          }
          const int32_t *eb = ebase.data() + R.ebase_off;
          for (size_t n = 0; n < N; ++n) {
            const int32_t e = (int32_t)(first[n] >> 1);
            const int t = (int)(std::upper_bound(eb, eb + R.n_texts + 1, e) - eb) - 1;
            g.off[n] = e - eb[t] + (int32_t)(first[n] & 1);
            g.src[n] = t == 0 ? -1 : (int32_t)(R.read_first + t - 1);
            g.pos[n] = t == 0 ? (int32_t)((int64_t)in.ref_start[r] + g.off[n]) : -1;
          }
        }
        h->graphs[(size_t)r] = std::move(g);
        g = Graph();
      }
      active.swap(still);
    }
    r0 = r1;
  }
  return GB_OK;
}

}  // namespace

extern "C" {

int gb_dbg_assemble(const uint8_t *ref_bytes, int64_t n_ref_bytes, const int64_t *ref_off, const int32_t *ref_start,
                    const int64_t *read_first, const int64_t *read_last, int64_t n_regions, const uint8_t *seq,
                    const uint8_t *qual, int64_t n_read_bytes, const int64_t *read_off, const uint32_t *flag,
                    int64_t n_reads, const gb_dbg_params *params, int keep, gb_dbg **out) {
  const char *who = "gb_dbg_assemble";
  gb::Range range(who);
  GB_ARG(out, "%s: null out", who);
  GB_ARG(keep == 0 || keep == 1, "%s: keep = %d (need 0 or 1)", who, keep);
  Input in{};
  in.P = params ? *params : gb_dbg_params{15, 5, 50, 20, 40};
  GB_ARG(in.P.k0 >= 1, "%s: k0 = %d (need >= 1)", who, in.P.k0);
  GB_ARG(in.P.k_step >= 1, "%s: k_step = %d (need >= 1)", who, in.P.k_step);
  {
    int64_t top = in.P.k0;
    if (top <= in.P.k_max) top += ((int64_t)in.P.k_max - top) / in.P.k_step * in.P.k_step + in.P.k_step;
    GB_ARG(top <= GB_DBG_MAX_K, "%s: k0 = %d, k_step = %d, k_max = %d can reach k = %lld, above GB_DBG_MAX_K = %d", who,
           in.P.k0, in.P.k_step, in.P.k_max, (long long)top, GB_DBG_MAX_K);
  }
  GB_ARG(n_regions >= 0 && n_reads >= 0 && n_ref_bytes >= 0 && n_read_bytes >= 0,
         "%s: negative count (n_regions %lld, n_reads %lld, n_ref_bytes %lld, n_read_bytes %lld)", who,
         (long long)n_regions, (long long)n_reads, (long long)n_ref_bytes, (long long)n_read_bytes);
  GB_ARG(n_regions == 0 || (ref_off && ref_start && read_first && read_last && (ref_bytes || n_ref_bytes == 0)),
         "%s: null region array", who);
  GB_ARG(n_reads == 0 || (read_off && flag && ((seq && qual) || n_read_bytes == 0)), "%s: null read array", who);
  for (int64_t j = 0; j < n_reads; ++j)
    GB_ARG(read_off[j] >= 0 && read_off[j] <= read_off[j + 1] && read_off[j + 1] <= n_read_bytes,
           "%s: read %lld has offsets %lld..%lld in an array of %lld bytes", who, (long long)j, (long long)read_off[j],
           (long long)read_off[j + 1], (long long)n_read_bytes);
  for (int64_t r = 0; r < n_regions; ++r) {
    GB_ARG(ref_off[r] >= 0 && ref_off[r] <= ref_off[r + 1] && ref_off[r + 1] <= n_ref_bytes,
           "%s: region %lld has reference offsets %lld..%lld in an array of %lld bytes", who, (long long)r,
           (long long)ref_off[r], (long long)ref_off[r + 1], (long long)n_ref_bytes);
    GB_ARG(read_first[r] >= 0 && read_first[r] <= read_last[r] && read_last[r] <= n_reads,
           "%s: region %lld has reads %lld..%lld of a pool of %lld", who, (long long)r, (long long)read_first[r],
           (long long)read_last[r], (long long)n_reads);
  }
  in.T = Texts{ref_bytes, ref_off, seq, qual, read_off};
  in.ref_start = ref_start, in.read_first = read_first, in.read_last = read_last, in.flag = flag;
  int64_t budget = 0, fp_bits = 64;
  int st;
  if ((st = gb::env_number(who, "GB_DBG_WS", 1, INT64_MAX, kDefaultBudget, &budget))) return st;
  if ((st = gb::env_number(who, "GB_DBG_FP_BITS", 1, 64, 64, &fp_bits))) return st;
  const bool on_host = gb::env_flag("GB_DBG_HOST");
  std::vector<Plan> plan;
  gb_dbg *h = nullptr;
  try {
    plan.resize((size_t)n_regions);
    for (int64_t r = 0; r < n_regions; ++r) {
      Plan &p = plan[(size_t)r];
      p.n_texts = 1 + read_last[r] - read_first[r];
      p.edges = 0;
      for (int64_t t = 0; t < p.n_texts && p.edges <= GB_DBG_MAX_EDGES; ++t) p.edges += text_edges(in, r, t, in.P.k0);
      GB_ARG(p.edges + p.n_texts <= GB_DBG_MAX_EDGES,
             "%s: region %lld has %lld walk positions and texts, above %lld: its visits cannot be indexed in 32 bits",
             who, (long long)r, (long long)(p.edges + p.n_texts), (long long)GB_DBG_MAX_EDGES);
      p.node_cap = std::min(p.edges + p.n_texts, 2 * p.edges);
      p.cap = 16;
      while (p.cap < 2 * (p.edges + p.n_texts + 1)) p.cap *= 2;
      p.bytes = kSlotBytes * p.cap + kEdgeBytes * (p.edges + 1) + kNodeBytes * (p.node_cap + 1) + 4 * (p.n_texts + 1) +
                (int64_t)sizeof(Reg) + 8 * cCount;
      GB_ARG(on_host || p.bytes <= budget,
             "%s: region %lld needs %lld bytes of device workspace, above the budget of %lld (GB_DBG_WS)", who,
             (long long)r, (long long)p.bytes, (long long)budget);
    }
    // a NUL byte: in a reference, or in a read that some region takes
    for (int64_t r = 0; r < n_regions; ++r) {
      const int64_t len = ref_off[r + 1] - ref_off[r];
      const void *z = len ? memchr(ref_bytes + ref_off[r], 0, (size_t)len) : nullptr;
      GB_ARG(!z, "%s: the reference of region %lld has a NUL byte at position %lld", who, (long long)r,
             (long long)((const uint8_t *)z - (ref_bytes + ref_off[r])));
    }
    {
      std::vector<int32_t> cover((size_t)n_reads + 1, 0);
      for (int64_t r = 0; r < n_regions; ++r) ++cover[(size_t)read_first[r]], --cover[(size_t)read_last[r]];
      int32_t depth = 0;
      for (int64_t j = 0; j < n_reads; ++j) {
        depth += cover[(size_t)j];
        const int64_t len = read_off[j + 1] - read_off[j];
        if (!depth || !len) continue;
        const void *z = memchr(seq + read_off[j], 0, (size_t)len);
        GB_ARG(!z, "%s: read %lld has a NUL byte at position %lld", who, (long long)j,
               (long long)((const uint8_t *)z - (seq + read_off[j])));
      }
    }
    h = new gb_dbg();
    h->keep = keep != 0;
    h->sum.assign((size_t)n_regions, gb_dbg_region_summary{});
    if (h->keep) h->graphs.resize((size_t)n_regions);
    Stats &S = stats();
    const int64_t calls = S.calls;
    S = Stats{};
    if (n_regions == 0) {
      st = GB_OK;
    } else if (on_host) {
      st = assemble_host(who, in, n_regions, h);
    } else {
      for (const Plan &p : plan) S.max_slots = std::max(S.max_slots, p.cap);
      const uint64_t fp_mask = fp_bits >= 64 ? ~uint64_t(0) : (uint64_t(1) << fp_bits) - 1;
      st = assemble_device(who, in, n_regions, n_ref_bytes, n_read_bytes, n_reads, plan, budget, fp_mask, h);
    }
    S.calls = calls + 1;
  } catch (...) {
    gb::set_error("%s: out of host memory", who);
    st = GB_ERR_NOMEM;
  }
  if (st) {
    delete h;
    return st;
  }
  *out = h;
  return GB_OK;
}

void gb_dbg_free(gb_dbg *h) { delete h; }

int gb_dbg_summary(const gb_dbg *h, gb_dbg_region_summary *out, int64_t cap) {
  const char *who = "gb_dbg_summary";
  GB_ARG(h, "%s: null handle", who);
  const int64_t n = (int64_t)h->sum.size();
  GB_ARG(cap >= n, "%s: room for %lld regions, %lld needed", who, (long long)cap, (long long)n);
  GB_ARG(n == 0 || out, "%s: null array", who);
  if (n) memcpy(out, h->sum.data(), sizeof(gb_dbg_region_summary) * (size_t)n);
  return GB_OK;
}

int gb_dbg_export(const gb_dbg *h, int64_t region, int64_t node_cap, int32_t *src, int32_t *off, int32_t *colours,
                  int32_t *position, int64_t *weight, int32_t *n_edges, int32_t *edge_to, int64_t *edge_weight,
                  int64_t *n_nodes) {
  const char *who = "gb_dbg_export";
  GB_ARG(h && n_nodes, "%s: null argument", who);
  GB_ARG(region >= 0 && region < (int64_t)h->sum.size(), "%s: region %lld of %lld", who, (long long)region,
         (long long)h->sum.size());
  *n_nodes = h->sum[(size_t)region].n_nodes;
  GB_ARG(h->keep, "%s: the handle was made with keep = 0 and holds no graph", who);
  const Graph &g = h->graphs[(size_t)region];
  const size_t n = g.src.size();
  GB_ARG(node_cap >= (int64_t)n, "%s: room for %lld nodes, %lld needed", who, (long long)node_cap, (long long)n);
  if (!n) return GB_OK;
  if (src) memcpy(src, g.src.data(), 4 * n);
  if (off) memcpy(off, g.off.data(), 4 * n);
  if (colours) memcpy(colours, g.col.data(), 4 * n);
  if (position) memcpy(position, g.pos.data(), 4 * n);
  if (weight) memcpy(weight, g.w.data(), 8 * n);
  if (n_edges) memcpy(n_edges, g.ne.data(), 4 * n);
  if (edge_to) memcpy(edge_to, g.to.data(), 16 * n);
  if (edge_weight) memcpy(edge_weight, g.ew.data(), 32 * n);
  return GB_OK;
}

int gb_dbg_timing(float *pack_ms, float *build_ms, float *rank_ms, float *edges_ms, float *cycle_ms, float *redo_ms,
                  int64_t *positions, int64_t *valid_positions) {
  const Stats &S = stats();
  if (!S.calls) {
    gb::set_error("gb_dbg_timing: no gb_dbg_assemble on this thread yet");
    return GB_ERR_STATE;
  }
  if (pack_ms) *pack_ms = S.pack_ms;
  if (build_ms) *build_ms = S.build_ms;
  if (rank_ms) *rank_ms = S.rank_ms;
  if (edges_ms) *edges_ms = S.edges_ms;
  if (cycle_ms) *cycle_ms = S.cycle_ms;
  if (redo_ms) *redo_ms = S.redo_ms;
  if (positions) *positions = S.positions;
  if (valid_positions) *valid_positions = S.valid;
  return GB_OK;
}

int gb_dbg_plan(int64_t *max_table_slots, int64_t *workspace_bytes, int64_t *chunks, int64_t *rounds) {
  const Stats &S = stats();
  if (max_table_slots) *max_table_slots = S.max_slots;
  if (workspace_bytes) *workspace_bytes = S.ws_bytes;
  if (chunks) *chunks = S.chunks;
  if (rounds) *rounds = S.rounds;
  return GB_OK;
}

}  // extern "C"
