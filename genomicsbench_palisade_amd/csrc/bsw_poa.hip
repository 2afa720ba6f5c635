// bsw_poa.hip -- gb_poa_align / gb_poa_consensus (include/gb_bsw_poa.h): spoa's global sequence-to-graph alignment on
// the device, and the window consensus built on it in rounds.
//
// Layout. An item keeps the reference's matrices as they are: (n_nodes + 1) rows of (seq_len + 1) int32, H and,
// by subtype, F, E and O, Q, one after the other, 4, 12 or 20 bytes per cell. Row 0 and column 0 hold the
// reference's initial values, kNegativeInfinity included, so the walk reads what the reference's walk reads.
//
// Fill. One workgroup per item (one wave up to GB_POA_WAVE_MAX_LEN bases, four above), rows in rank order, a
// thread owning a run of consecutive columns (at most four, kept in registers between the sweeps, up to
// GB_POA_GROUP_MAX_LEN bases; any number, read back from the item's own rows, above). A row is three sweeps of
// the thread's own columns with a workgroup-wide exclusive prefix maximum between them:
//   1. hp[j] = max over the in-edges of the diagonal, F and O terms: predecessor rows only, fully parallel;
//   2. H[j] = max(hp[j], max over k < j of hp[k] + gap(j - k)) with gap(l) = max(g + (l-1) e, q + (l-1) c), as
//      prefix maxima of hp[k] - k e and hp[k] - k c (column 0 counts as hp[0]). This is the reference's H: its
//      E[j] and Q[j] open from H[j-1], which may itself end a gap, but two gaps in a row never beat the one gap
//      of their summed length, because gap(a) + gap(b) <= gap(a + b) whenever g <= e, q <= c, g <= c and q <= e,
//      which the subtype rule guarantees (affine: q = g < e = c; convex: q < g < e < c).
//   3. E[j] = max over k < j of H[k] + g + (j-1-k) e over the final H, and Q[j] likewise: the reference's
//      recurrences E[j] = max(H[j-1] + g, E[j-1] + e) unrolled. Its one more term, E[i][0] + j e with E[i][0] =
//      kNegativeInfinity, never wins in the reference either (every score is above -2^28), so E and Q hold the
//      reference's values, not just values that give the same H.
// The scans run on biased values (v - k e) that stay within +-2^29; kNegativeInfinity never enters one.
//
// Walk. One thread per item restates the reference's walk of the subtype over the stored matrices. Every pair it
// writes is counted against n_nodes + seq_len, and it stops with a status when the count is reached or when a
// cell matches none of the moves (where the reference would go on with stale indices).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/gb_bsw_poa.h"
#include "gb_common.h"
#include "gb_common_wave.h"

namespace gbpoa {

constexpr int32_t kNegInf = INT32_MIN + 1024;  // the reference's kNegativeInfinity
constexpr int kNone = -(1 << 30);              // "no column yet" in the prefix maxima
constexpr int64_t kDefaultBudget = int64_t(4) << 30;

enum { kWalkOk = 0, kWalkBound = 1, kWalkGuard = 2, kWalkNoSink = 3 };

struct Par { int32_t m, n, g, e, q, c, sub; };

static int make_par(const char *who, const gb_poa_params *p, Par *P) {
  GB_ARG(p->type == GB_POA_SW || p->type == GB_POA_NW || p->type == GB_POA_OV, "%s: invalid alignment type %d", who,
         (int)p->type);
  GB_ARG(p->type != GB_POA_SW, "%s: alignment type kSW is not supported (kNW only)", who);
  GB_ARG(p->type != GB_POA_OV, "%s: alignment type kOV is not supported (kNW only)", who);
  GB_ARG(p->g <= 0 && p->q <= 0, "%s: gap opening penalty must be non-positive! (g = %d, q = %d)", who, (int)p->g,
         (int)p->q);
  GB_ARG(p->e <= 0 && p->c <= 0, "%s: gap extension penalty must be non-positive! (e = %d, c = %d)", who, (int)p->e,
         (int)p->c);
  P->m = p->m, P->n = p->n, P->g = p->g, P->e = p->e, P->q = p->q, P->c = p->c;
  P->sub = p->g >= p->e ? GB_POA_LINEAR : (p->g <= p->q || p->e >= p->c ? GB_POA_AFFINE : GB_POA_CONVEX);
  if (P->sub == GB_POA_LINEAR) P->e = P->g;
  if (P->sub != GB_POA_CONVEX) P->q = P->g, P->c = P->e;
  return GB_OK;
}

static inline int n_mats(int sub) { return sub == GB_POA_LINEAR ? 1 : sub == GB_POA_AFFINE ? 3 : 5; }
static inline int64_t n_cells(int n, int len) { return ((int64_t)n + 1) * ((int64_t)len + 1); }
static inline int64_t mat_words(int sub, int n, int len) {  // int32 words, a multiple of 4
  return gb::round_up(n_cells(n, len) * n_mats(sub), 4);
}
static inline int64_t item_bytes(int sub, int n, int len) {
  if (n == 0 || len == 0) return 0;
  return mat_words(sub, n, len) * 4 + ((int64_t)n + len) * 8;
}
static inline int size_class(int len) {
  return len <= GB_POA_WAVE_MAX_LEN ? GB_POA_CLASS_WAVE : len <= GB_POA_GROUP_MAX_LEN ? GB_POA_CLASS_GROUP : GB_POA_CLASS_LONG;
}

// one item's view, the pointers already at its first node and edge
struct View {
  const uint8_t *base;
  const int32_t *id;
  const uint8_t *out;
  const int32_t *in_end;
  const int32_t *pred;
  const uint8_t *seq;
  int32_t n, len;
};
struct Mats {
  int32_t *H, *F, *E, *O, *Q;
  int64_t w;
};
__host__ __device__ inline Mats mats_at(int32_t *p, int sub, int n, int len) {
  const int64_t cells = ((int64_t)n + 1) * ((int64_t)len + 1);
  Mats M;
  M.w = (int64_t)len + 1;
  M.H = p;
  M.F = sub >= GB_POA_AFFINE ? p + cells : nullptr;
  M.E = sub >= GB_POA_AFFINE ? p + 2 * cells : nullptr;
  M.O = sub == GB_POA_CONVEX ? p + 3 * cells : nullptr;
  M.Q = sub == GB_POA_CONVEX ? p + 4 * cells : nullptr;
  return M;
}
__host__ __device__ inline int imax(int a, int b) { return a > b ? a : b; }

// Row 0's cell j and column 0's cell of row i (SisdAlignmentEngine::initialize, kNW). Column 0 of row i needs
// column 0 of its predecessor rows.
__host__ __device__ inline void init_row0(const Par &P, const Mats &M, int64_t j) {
  if (P.sub == GB_POA_LINEAR) {
    M.H[j] = (int32_t)j * P.g;
    return;
  }
  const int32_t ev = j ? P.g + ((int32_t)j - 1) * P.e : 0;
  M.F[j] = j ? kNegInf : 0, M.E[j] = ev;
  if (P.sub == GB_POA_CONVEX) {
    const int32_t qv = j ? P.q + ((int32_t)j - 1) * P.c : 0;
    M.O[j] = j ? kNegInf : 0, M.Q[j] = qv;
    M.H[j] = j ? imax(qv, ev) : 0;
  } else {
    M.H[j] = ev;
  }
}
// returns H[i][0]; store is false for the threads that only need the value
__host__ __device__ inline int32_t init_col0(const Par &P, const Mats &M, const View &G, int r, bool store) {
  const int64_t i = (int64_t)r + 1;
  const int b = r ? G.in_end[r - 1] : 0, e = G.in_end[r];
  int32_t h;
  if (P.sub == GB_POA_LINEAR) {
    int32_t pen = b == e ? 0 : kNegInf;
    for (int k = b; k < e; ++k) pen = imax(pen, M.H[((int64_t)G.pred[k] + 1) * M.w]);
    h = pen + P.g;
  } else {
    int32_t pen = b == e ? P.g - P.e : kNegInf;
    for (int k = b; k < e; ++k) pen = imax(pen, M.F[((int64_t)G.pred[k] + 1) * M.w]);
    const int32_t f = pen + P.e;
    h = f;
    int32_t o = 0;
    if (P.sub == GB_POA_CONVEX) {
      int32_t pq = b == e ? P.q - P.c : kNegInf;
      for (int k = b; k < e; ++k) pq = imax(pq, M.O[((int64_t)G.pred[k] + 1) * M.w]);
      o = pq + P.c;
      h = imax(o, f);
    }
    if (store) {
      M.F[i * M.w] = f, M.E[i * M.w] = kNegInf;
      if (P.sub == GB_POA_CONVEX) M.O[i * M.w] = o, M.Q[i * M.w] = kNegInf;
    }
  }
  if (store) M.H[i * M.w] = h;
  return h;
}

// The terms of cell (r + 1, j), j >= 1, that come from predecessor rows: *f and *o by subtype, and the return
// value max(diagonal, F, O), or for the linear subtype max(diagonal, up).
__host__ __device__ inline int32_t pred_terms(const Par &P, const Mats &M, const View &G, int r, int64_t j, int32_t *f,
                                              int32_t *o) {
  const int b = r ? G.in_end[r - 1] : 0, e = G.in_end[r];
  const int32_t mc = G.base[r] == G.seq[j - 1] ? P.m : P.n;
  int32_t d = INT32_MIN, fv = INT32_MIN, ov = INT32_MIN;
  for (int k = b; k < e || k == b; ++k) {  // a node without in-edges has row 0 as its one predecessor
    const int64_t row = (k < e ? (int64_t)G.pred[k] + 1 : 0) * M.w;
    const int32_t hu = M.H[row + j];
    d = imax(d, M.H[row + j - 1] + mc);
    if (P.sub == GB_POA_LINEAR) {
      d = imax(d, hu + P.g);
    } else {
      fv = imax(fv, imax(hu + P.g, M.F[row + j] + P.e));
      if (P.sub == GB_POA_CONVEX) ov = imax(ov, imax(hu + P.q, M.O[row + j] + P.c));
    }
    if (k >= e) break;
  }
  if (P.sub == GB_POA_LINEAR) return d;
  *f = fv;
  if (P.sub == GB_POA_CONVEX) {
    *o = ov;
    return imax(d, imax(fv, ov));
  }
  return imax(d, fv);
}

// The reference's walk of the subtype from (max_i, len). The pairs go to end[-2], end[-4], ... in walk order, so
// that they stand in the reference's (reversed) order at end - 2 * count. Returns the count, or -status.
__host__ __device__ inline int walk(const Par &P, const Mats &M, const View &G, int max_i, int32_t *end) {
  const int cap = G.n + G.len;
  const int64_t w = M.w;
  int cnt = 0;
  int64_t i = max_i, j = G.len, prev_i = 0, prev_j = 0;
#define GB_POA_EMIT(a, b)                \
  do {                                   \
    if (cnt >= cap) return -kWalkBound;  \
    ++cnt;                               \
    end[-2 * cnt] = (a), end[-2 * cnt + 1] = (b); \
  } while (0)
  while (!(i == 0 && j == 0)) {
    const int32_t h = M.H[i * w + j];
    bool found = false, ext_left = false, ext_up = false;
    const int r = (int)i - 1;
    const int b = i ? (r ? G.in_end[r - 1] : 0) : 0, e = i ? G.in_end[r] : 0;
    if (i != 0 && j != 0) {
      const int32_t mc = G.base[r] == G.seq[j - 1] ? P.m : P.n;
      for (int k = b; k < e || k == b; ++k) {
        const int64_t pi = k < e ? (int64_t)G.pred[k] + 1 : 0;
        if (h == M.H[pi * w + j - 1] + mc) {
          prev_i = pi, prev_j = j - 1, found = true;
          break;
        }
        if (k >= e) break;
      }
    }
    if (!found && i != 0) {
      for (int k = b; k < e || k == b; ++k) {
        const int64_t pi = k < e ? (int64_t)G.pred[k] + 1 : 0;
        bool hit;
        if (P.sub == GB_POA_LINEAR) {
          hit = h == M.H[pi * w + j] + P.g;
        } else if (P.sub == GB_POA_AFFINE) {
          hit = (ext_up = h == M.F[pi * w + j] + P.e) || h == M.H[pi * w + j] + P.g;
        } else {
          hit = (ext_up = h == M.F[pi * w + j] + P.e) || h == M.H[pi * w + j] + P.g ||
                (ext_up = h == M.O[pi * w + j] + P.c) || h == M.H[pi * w + j] + P.q;
        }
        if (hit) {
          prev_i = pi, prev_j = j, found = true;
          break;
        }
        if (k >= e) break;
      }
    }
    if (!found && j != 0) {
      bool hit;
      if (P.sub == GB_POA_LINEAR) {
        hit = h == M.H[i * w + j - 1] + P.g;
      } else if (P.sub == GB_POA_AFFINE) {
        hit = (ext_left = h == M.E[i * w + j - 1] + P.e) || h == M.H[i * w + j - 1] + P.g;
      } else {
        hit = (ext_left = h == M.E[i * w + j - 1] + P.e) || h == M.H[i * w + j - 1] + P.g ||
              (ext_left = h == M.Q[i * w + j - 1] + P.c) || h == M.H[i * w + j - 1] + P.q;
      }
      if (hit) prev_i = i, prev_j = j - 1, found = true;
    }
    if (!found) return -kWalkGuard;
    GB_POA_EMIT(i == prev_i ? -1 : G.id[i - 1], j == prev_j ? -1 : (int32_t)j - 1);
    i = prev_i, j = prev_j;
    if (ext_left) {
      while (true) {
        if (j == 0) return -kWalkGuard;  // the reference would read column -1
        GB_POA_EMIT(-1, (int32_t)j - 1);
        --j;
        const bool e_ends = M.E[i * w + j] + P.e != M.E[i * w + j + 1];
        if (P.sub == GB_POA_AFFINE ? e_ends : (e_ends && M.Q[i * w + j] + P.c != M.Q[i * w + j + 1])) break;
      }
    } else if (ext_up) {
      while (true) {
        if (i == 0) return -kWalkGuard;  // the reference would read node -1
        const int rr = (int)i - 1;
        const int bb = rr ? G.in_end[rr - 1] : 0, ee = G.in_end[rr];
        const int32_t fv = M.F[i * w + j];
        bool stop;
        prev_i = 0;
        if (P.sub == GB_POA_AFFINE) {
          stop = false;
          for (int k = bb; k < ee; ++k) {
            const int64_t pi = (int64_t)G.pred[k] + 1;
            if ((stop = fv == M.H[pi * w + j] + P.g) || fv == M.F[pi * w + j] + P.e) {
              prev_i = pi;
              break;
            }
          }
        } else {
          const int32_t ov = M.O[i * w + j];
          stop = true;
          for (int k = bb; k < ee; ++k) {
            const int64_t pi = (int64_t)G.pred[k] + 1;
            if (fv == M.F[pi * w + j] + P.e || ov == M.O[pi * w + j] + P.c) {
              prev_i = pi, stop = false;
              break;
            }
          }
          if (stop) {
            for (int k = bb; k < ee; ++k) {
              const int64_t pi = (int64_t)G.pred[k] + 1;
              if (fv == M.H[pi * w + j] + P.g || ov == M.H[pi * w + j] + P.q) {
                prev_i = pi;
                break;
              }
            }
          }
        }
        GB_POA_EMIT(G.id[i - 1], -1);
        i = prev_i;
        if (stop || i == 0) break;
      }
    }
  }
#undef GB_POA_EMIT
  return cnt;
}

// ---- device ----

struct DItem {
  int64_t node_off, edge_off, seq_off, mat_off /* int32 words */, pair_off /* pairs */;
  int32_t n, len, out, pad;
};
struct DRes { int32_t score, max_i, n_pairs, status; };
struct Args {
  Par P;
  const uint8_t *base, *out, *seqs;
  const int32_t *id, *in_end, *pred;
  int32_t *mats, *walked;
  DRes *res;
  const DItem *items;
  int64_t n;
};

__device__ inline View view_of(const Args &A, const DItem &I) {
  return View{A.base + I.node_off, A.id + I.node_off,     A.out + I.node_off, A.in_end + I.node_off,
              A.pred + I.edge_off, A.seqs + I.seq_off, I.n,                I.len};
}

// Exclusive prefix maximum over the workgroup's threads, of a and of b at once. s holds 2 * NT / 64 words that no
// thread reads again before the next barrier but one.
template <int NT>
__device__ __forceinline__ void excl_scan2(int &a, int &b, int *s, int lane, int wv) {
  const int ia = gb::scan_max<kNone>(a), ib = gb::scan_max<kNone>(b);
  a = gb::wave_shr1(ia, kNone), b = gb::wave_shr1(ib, kNone);
  if (NT > 64) {
    if (lane == 63) s[wv] = ia, s[NT / 64 + wv] = ib;
    __syncthreads();
    for (int k = 0; k < wv; ++k) a = max(a, s[k]), b = max(b, s[NT / 64 + k]);
  }
}

// REG: a thread owns at most four columns and keeps their values in registers from one sweep to the next; without
// it the sweeps read back what the thread itself stored.
template <int NT, bool REG>
__global__ __launch_bounds__(NT) void poa_fill_kernel(Args A) {
  __shared__ int s_tot[2][2 * (NT / 64)];
  const DItem I = A.items[blockIdx.x];
  const Par P = A.P;
  const View G = view_of(A, I);
  const Mats M = mats_at(A.mats + I.mat_off, P.sub, I.n, I.len);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int len = I.len, n = I.n;
  const int cpt = (len + NT - 1) / NT;  // columns per thread; len >= 1, and cpt <= 4 with REG
  const int j0 = min(1 + t * cpt, len + 1), j1 = min(j0 + cpt, len + 1);
  const bool owner = j0 <= len && j1 == len + 1;  // the thread of the last column
  for (int j = t; j <= len; j += NT) init_row0(P, M, j);
  __syncthreads();
  int32_t best = kNegInf, best_i = -1;
  int32_t hv[4] = {0, 0, 0, 0};
  // body(j, k) for the thread's columns j = j0 + k
  auto cols = [&](auto &&body) {
    if (REG) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j0 + k < j1) body(j0 + k, k);
    } else {
      for (int j = j0; j < j1; ++j) body(j, 0);
    }
  };
  for (int r = 0; r < n; ++r) {
    const int64_t row = ((int64_t)r + 1) * M.w;
    const int32_t h0 = init_col0(P, M, G, r, t == 0);
    // 1: the predecessor rows' terms
    int a = kNone, b = kNone;
    if (t == 0) a = h0, b = h0;
    cols([&](int j, int k) {
      int32_t f = 0, o = 0;
      const int32_t hp = pred_terms(P, M, G, r, j, &f, &o);
      if (REG) hv[k] = hp;
      else M.H[row + j] = hp;
      if (P.sub != GB_POA_LINEAR) M.F[row + j] = f;
      if (P.sub == GB_POA_CONVEX) M.O[row + j] = o;
      a = max(a, hp - j * P.e), b = max(b, hp - j * P.c);
    });
    excl_scan2<NT>(a, b, s_tot[0], lane, wv);
    // 2: H, from the prefix maxima of hp
    int a2 = kNone, b2 = kNone;
    if (t == 0) a = h0, b = h0, a2 = h0, b2 = h0;
    cols([&](int j, int k) {
      const int32_t hp = REG ? hv[k] : M.H[row + j];
      int32_t h = max(hp, a + (j - 1) * P.e + P.g);
      if (P.sub == GB_POA_CONVEX) h = max(h, b + (j - 1) * P.c + P.q);
      a = max(a, hp - j * P.e), b = max(b, hp - j * P.c);
      M.H[row + j] = h;
      if (REG) hv[k] = h;
      a2 = max(a2, h - j * P.e), b2 = max(b2, h - j * P.c);
      if (j == len && !G.out[r] && best < h) best = h, best_i = r + 1;
    });
    if (P.sub != GB_POA_LINEAR) {
      excl_scan2<NT>(a2, b2, s_tot[1], lane, wv);
      // 3: E and Q, from the prefix maxima of the final H
      if (t == 0) a2 = h0, b2 = h0;
      cols([&](int j, int k) {
        const int32_t h = REG ? hv[k] : M.H[row + j];
        M.E[row + j] = a2 + (j - 1) * P.e + P.g;
        if (P.sub == GB_POA_CONVEX) M.Q[row + j] = b2 + (j - 1) * P.c + P.q;
        a2 = max(a2, h - j * P.e), b2 = max(b2, h - j * P.c);
      });
    }
    __syncthreads();  // the row is in memory for the rows that follow
  }
  if (owner) A.res[I.out] = DRes{best, best_i, 0, best_i < 0 ? kWalkNoSink : kWalkOk};
}

__global__ __launch_bounds__(64) void poa_walk_kernel(Args A) {
  const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (k >= A.n) return;
  const DItem I = A.items[k];
  DRes R = A.res[I.out];
  if (R.status != kWalkOk) return;
  const Mats M = mats_at(A.mats + I.mat_off, A.P.sub, I.n, I.len);
  const int c = walk(A.P, M, view_of(A, I), R.max_i, A.walked + 2 * (I.pair_off + I.n + I.len));
  R.n_pairs = c < 0 ? 0 : c, R.status = c < 0 ? -c : kWalkOk;
  A.res[I.out] = R;
}

// ---- host path ----

// SisdAlignmentEngine::{linear, affine, convex}'s fill as the reference writes it, row by row and column by
// column; returns max_i and sets *score
static int host_fill(const Par &P, const Mats &M, const View &G, int32_t *score) {
  for (int64_t j = 0; j <= G.len; ++j) init_row0(P, M, j);
  int32_t best = kNegInf, best_i = -1;
  for (int r = 0; r < G.n; ++r) {
    const int64_t row = ((int64_t)r + 1) * M.w;
    init_col0(P, M, G, r, true);
    for (int64_t j = 1; j <= G.len; ++j) {
      int32_t f = 0, o = 0;
      M.H[row + j] = pred_terms(P, M, G, r, j, &f, &o);
      if (P.sub != GB_POA_LINEAR) M.F[row + j] = f;
      if (P.sub == GB_POA_CONVEX) M.O[row + j] = o;
    }
    for (int64_t j = 1; j <= G.len; ++j) {
      if (P.sub == GB_POA_LINEAR) {
        M.H[row + j] = imax(M.H[row + j - 1] + P.g, M.H[row + j]);
      } else {
        M.E[row + j] = imax(M.H[row + j - 1] + P.g, M.E[row + j - 1] + P.e);
        int32_t h = imax(M.H[row + j], M.E[row + j]);
        if (P.sub == GB_POA_CONVEX) {
          M.Q[row + j] = imax(M.H[row + j - 1] + P.q, M.Q[row + j - 1] + P.c);
          h = imax(h, M.Q[row + j]);
        }
        M.H[row + j] = h;
      }
    }
    if (!G.out[r] && best < M.H[row + G.len]) best = M.H[row + G.len], best_i = r + 1;
  }
  *score = best;
  return best_i;
}

// ---- a pass over a batch of items ----

struct Batch {
  gb_poa_graphs g;
  const uint8_t *seqs;
  int64_t seq_bytes;
  const gb_poa_item *items;
  int64_t n_items;
};

struct Stats {  // of the calling thread's last call; plain data, so thread storage is fine
  float fill_ms, walk_ms, host_ms;
  int64_t cells, chunks, ws_bytes, calls;
};
static Stats &stats() {
  thread_local Stats s{};
  return s;
}

struct Ws : gb::WsBase<3> {  // the calling thread's, through gb::get_ws
  gb::DevBuf<uint8_t> d_base, d_out, d_seqs;
  gb::DevBuf<int32_t> d_id, d_in_end, d_pred, d_mats, d_walked;
  gb::DevBuf<DItem> d_items;
  gb::DevBuf<DRes> d_res;
  gb::PinnedBuf<DItem> h_items;
  gb::PinnedBuf<DRes> h_res;
  gb::PinnedBuf<int32_t> h_walked;
};

static inline bool live_item(const gb_poa_item &it) { return it.n_nodes > 0 && it.seq_len > 0; }

static int validate(const char *who, const char *what, const Batch &B) {
  const gb_poa_graphs &g = B.g;
  for (int64_t i = 0; i < B.n_items; ++i) {
    const gb_poa_item &it = B.items[i];
    const long long li = (long long)i;
    GB_ARG(it.n_nodes >= 0 && it.n_nodes <= GB_POA_MAX_NODES, "%s: %s %lld has %d nodes (0 .. %d)", who, what, li,
           it.n_nodes, GB_POA_MAX_NODES);
    GB_ARG(it.seq_len >= 0 && it.seq_len <= GB_POA_MAX_LEN, "%s: %s %lld has a sequence of %d bases (0 .. %d)", who,
           what, li, it.seq_len, GB_POA_MAX_LEN);
    GB_ARG(it.n_edges >= 0, "%s: %s %lld has %d edges", who, what, li, it.n_edges);
    GB_ARG(it.seq_off >= 0 && it.seq_off <= B.seq_bytes - it.seq_len,
           "%s: %s %lld has a sequence outside the %lld bytes of seqs", who, what, li, (long long)B.seq_bytes);
    GB_ARG(it.node_off >= 0 && it.node_off <= g.n_nodes - it.n_nodes,
           "%s: %s %lld has a view outside the %lld nodes of the graphs", who, what, li, (long long)g.n_nodes);
    GB_ARG(it.edge_off >= 0 && it.edge_off <= g.n_edges - it.n_edges,
           "%s: %s %lld has in-edges outside the %lld of the graphs", who, what, li, (long long)g.n_edges);
    GB_ARG(it.n_nodes > 0 || it.n_edges == 0, "%s: %s %lld has no node but %d in-edges", who, what, li, it.n_edges);
    int32_t prev = 0;
    for (int r = 0; r < it.n_nodes; ++r) {
      const int32_t e = g.in_end[it.node_off + r];
      GB_ARG(e >= prev && e <= it.n_edges, "%s: %s %lld has the in-edge range [%d, %d) at rank %d, outside its %d edges",
             who, what, li, prev, e, r, it.n_edges);
      for (int32_t k = prev; k < e; ++k) {
        const int32_t p = g.pred_rank[it.edge_off + k];
        GB_ARG(p >= 0 && p < r, "%s: %s %lld is not topologically sorted: rank %d has predecessor rank %d", who, what,
               li, r, p);
      }
      prev = e;
    }
    GB_ARG(prev == it.n_edges, "%s: %s %lld has in-edge ranges that end at %d, not at its %d edges", who, what, li,
           prev, it.n_edges);
  }
  return GB_OK;
}

struct Need {
  int64_t words /* of matrices */, pairs;
  int64_t bytes() const { return words * 4 + pairs * 8; }
  void operator+=(const Need &o) { words += o.words, pairs += o.pairs; }
  void max_with(const Need &o) { words = std::max(words, o.words), pairs = std::max(pairs, o.pairs); }
};
using Chunk = gb::Chunk<Need>;  // of the live items

// The chunks of a batch: the live items in order, as many as fit the budget. Refuses the item that alone does not.
static int make_chunks(const char *who, const char *what, const int64_t *names, const Par &P, const Batch &B,
                       const std::vector<int64_t> &live, int64_t budget, std::vector<Chunk> *chunks) {
  auto need_of = [&](int64_t k) {
    const gb_poa_item &it = B.items[live[(size_t)k]];
    return Need{mat_words(P.sub, it.n_nodes, it.seq_len), (int64_t)it.n_nodes + it.seq_len};
  };
  const int64_t k = gb::cut_chunks((int64_t)live.size(), budget, need_of, chunks);
  GB_ARG(k < 0, "%s: %s %lld needs %lld bytes of workspace, more than the budget of %lld (GB_POA_WS)", who, what,
         (long long)(names ? names[live[(size_t)k]] : live[(size_t)k]), (long long)need_of(k).bytes(), (long long)budget);
  return GB_OK;
}

static View host_view(const Batch &B, const gb_poa_item &it) {
  return View{B.g.node_base + it.node_off, B.g.node_id + it.node_off,     B.g.node_out + it.node_off,
              B.g.in_end + it.node_off,    B.g.pred_rank + it.edge_off, B.seqs + it.seq_off,
              it.n_nodes,                  it.seq_len};
}

static int walk_failed(const char *who, const char *what, long long name, int status) {
  gb::set_error(status == kWalkNoSink  ? "%s: %s %lld has no node without out-edges to end the alignment at"
                : status == kWalkBound ? "%s: the walk of %s %lld passed its bound of nodes + bases"
                                       : "%s: the walk of %s %lld met a cell that no move explains",
                who, what, name);
  return GB_ERR_STATE;
}

// The alignments of a validated batch whose chunks are made: slot[i] (n_nodes + seq_len pairs at begin[i]) takes
// item i's pairs, count[i] their number, scores[i] the score. `names` maps an item to the index a message uses.
static int run_batch(const char *who, const char *what, const int64_t *names, const Par &P, const Batch &B,
                     const std::vector<int64_t> &live, const std::vector<Chunk> &chunks, bool host, int32_t *scores,
                     int32_t *slots, const int64_t *begin, int32_t *count) {
  Stats &S = stats();
  for (int64_t i = 0; i < B.n_items; ++i) scores[i] = 0, count[i] = 0;
  for (int64_t i : live) S.cells += (int64_t)B.items[i].n_nodes * B.items[i].seq_len;
  if (live.empty()) return GB_OK;
  int st;
  if (host) {
    int nth = 1;
    if ((st = gb::thread_count(who, "GB_POA_THREADS", &nth))) return st;
    std::atomic<int64_t> next{0};
    std::atomic<int64_t> bad{-1};
    std::atomic<int> bad_status{0};
    if ((st = gb::parallel(who, (int)std::min<int64_t>(nth, (int64_t)live.size()), [&](int) {
           std::vector<int32_t> mem;
           for (int64_t k; (k = next.fetch_add(1)) < (int64_t)live.size();) {
             const int64_t i = live[(size_t)k];
             const gb_poa_item &it = B.items[i];
             mem.resize((size_t)mat_words(P.sub, it.n_nodes, it.seq_len));
             const Mats M = mats_at(mem.data(), P.sub, it.n_nodes, it.seq_len);
             const View G = host_view(B, it);
             const int mi = host_fill(P, M, G, &scores[i]);
             int32_t *slot = slots + 2 * begin[i];
             const int c = mi < 0 ? -kWalkNoSink : walk(P, M, G, mi, slot + 2 * ((int64_t)it.n_nodes + it.seq_len));
             if (c < 0) {
               int64_t none = -1;
               if (bad.compare_exchange_strong(none, i)) bad_status.store(-c);
               continue;
             }
             count[i] = c;
             std::memmove(slot, slot + 2 * ((int64_t)it.n_nodes + it.seq_len - c), (size_t)c * 8);
           }
         })))
      return st;
    if (bad.load() >= 0) return walk_failed(who, what, (long long)(names ? names[bad.load()] : bad.load()), bad_status.load());
    return GB_OK;
  }
  int dev = 0;
  GB_HIP(hipGetDevice(&dev));
  Ws *W = nullptr;
  if ((st = gb::get_ws("gb_poa", dev, &W))) return st;
  const auto big = gb::largest(chunks);
  const int64_t big_words = big.need.words, big_pairs = big.need.pairs, big_n = big.count;
  const gb_poa_graphs &g = B.g;
  if ((st = W->d_base.reserve((size_t)g.n_nodes)) || (st = W->d_out.reserve((size_t)g.n_nodes)) ||
      (st = W->d_id.reserve((size_t)g.n_nodes)) || (st = W->d_in_end.reserve((size_t)g.n_nodes)) ||
      (st = W->d_pred.reserve((size_t)std::max<int64_t>(g.n_edges, 1))) || (st = W->d_seqs.reserve((size_t)B.seq_bytes)) ||
      (st = W->d_mats.reserve((size_t)big_words)) || (st = W->d_walked.reserve((size_t)big_pairs * 2)) ||
      (st = W->h_walked.reserve((size_t)big_pairs * 2)) || (st = W->d_items.reserve((size_t)big_n)) ||
      (st = W->h_items.reserve((size_t)big_n)) || (st = W->d_res.reserve((size_t)big_n)) ||
      (st = W->h_res.reserve((size_t)big_n)))
    return st;
  hipStream_t s = W->stream;
  GB_HIP(hipMemcpyAsync(W->d_base, g.node_base, (size_t)g.n_nodes, hipMemcpyHostToDevice, s));
  GB_HIP(hipMemcpyAsync(W->d_out, g.node_out, (size_t)g.n_nodes, hipMemcpyHostToDevice, s));
  GB_HIP(hipMemcpyAsync(W->d_id, g.node_id, (size_t)g.n_nodes * 4, hipMemcpyHostToDevice, s));
  GB_HIP(hipMemcpyAsync(W->d_in_end, g.in_end, (size_t)g.n_nodes * 4, hipMemcpyHostToDevice, s));
  if (g.n_edges) GB_HIP(hipMemcpyAsync(W->d_pred, g.pred_rank, (size_t)g.n_edges * 4, hipMemcpyHostToDevice, s));
  GB_HIP(hipMemcpyAsync(W->d_seqs, B.seqs, (size_t)B.seq_bytes, hipMemcpyHostToDevice, s));
  GB_HIP(hipStreamSynchronize(s));  // the sources are the caller's pageable arrays
  for (const Chunk &ch : chunks) {
    const int64_t n = ch.last - ch.first;
    // the items by size class, one launch each
    int64_t cnt[3] = {0, 0, 0}, mo = 0, po = 0;
    for (int64_t k = 0; k < n; ++k) cnt[size_class(B.items[live[(size_t)(ch.first + k)]].seq_len)] += 1;
    const int64_t first[3] = {0, cnt[0], cnt[0] + cnt[1]};
    int64_t at[3] = {first[0], first[1], first[2]};
    DItem *hi = W->h_items;
    for (int64_t k = 0; k < n; ++k) {
      const gb_poa_item &it = B.items[live[(size_t)(ch.first + k)]];
      hi[at[size_class(it.seq_len)]++] = DItem{it.node_off, it.edge_off, it.seq_off, mo, po, it.n_nodes, it.seq_len, (int32_t)k, 0};
      mo += mat_words(P.sub, it.n_nodes, it.seq_len), po += (int64_t)it.n_nodes + it.seq_len;
    }
    GB_HIP(hipMemcpyAsync(W->d_items, hi, (size_t)n * sizeof(DItem), hipMemcpyHostToDevice, s));
    Args A;
    A.P = P, A.base = W->d_base, A.out = W->d_out, A.seqs = W->d_seqs, A.id = W->d_id, A.in_end = W->d_in_end;
    A.pred = W->d_pred, A.mats = W->d_mats, A.walked = W->d_walked, A.res = W->d_res, A.items = W->d_items, A.n = n;
    GB_HIP(hipEventRecord(W->ev[0], s));
    for (int c = 0; c < 3; ++c) {
      if (!cnt[c]) continue;
      Args Ac = A;
      Ac.items = W->d_items.get() + first[c];
      const dim3 grid((unsigned)cnt[c]);
      if (c == GB_POA_CLASS_WAVE)
        hipLaunchKernelGGL((poa_fill_kernel<64, true>), grid, dim3(64), 0, s, Ac);
      else if (c == GB_POA_CLASS_GROUP)
        hipLaunchKernelGGL((poa_fill_kernel<256, true>), grid, dim3(256), 0, s, Ac);
      else
        hipLaunchKernelGGL((poa_fill_kernel<256, false>), grid, dim3(256), 0, s, Ac);
      GB_HIP(hipGetLastError());
    }
    GB_HIP(hipEventRecord(W->ev[1], s));
    hipLaunchKernelGGL(poa_walk_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, A);
    GB_HIP(hipGetLastError());
    GB_HIP(hipEventRecord(W->ev[2], s));
    GB_HIP(hipMemcpyAsync(W->h_res, W->d_res, (size_t)n * sizeof(DRes), hipMemcpyDeviceToHost, s));
    GB_HIP(hipMemcpyAsync(W->h_walked, W->d_walked, (size_t)ch.need.pairs * 8, hipMemcpyDeviceToHost, s));
    GB_HIP(hipStreamSynchronize(s));
    float fill_ms = 0.f, walk_ms = 0.f;
    GB_HIP(hipEventElapsedTime(&fill_ms, W->ev[0], W->ev[1]));
    GB_HIP(hipEventElapsedTime(&walk_ms, W->ev[1], W->ev[2]));
    S.fill_ms += fill_ms, S.walk_ms += walk_ms;
    po = 0;
    for (int64_t k = 0; k < n; ++k) {
      const int64_t i = live[(size_t)(ch.first + k)];
      const gb_poa_item &it = B.items[i];
      const DRes R = W->h_res[k];
      if (R.status != kWalkOk) return walk_failed(who, what, (long long)(names ? names[i] : i), R.status);
      const int64_t cap = (int64_t)it.n_nodes + it.seq_len;
      scores[i] = R.score, count[i] = R.n_pairs;
      std::memcpy(slots + 2 * begin[i], W->h_walked.get() + 2 * (po + cap - R.n_pairs), (size_t)R.n_pairs * 8);
      po += cap;
    }
  }
  S.chunks += (int64_t)chunks.size(), S.ws_bytes = std::max(S.ws_bytes, big.bytes);
  return GB_OK;
}

// ---- the host graph (Graph::add_alignment, topological_sort, traverse_heaviest_bundle) ----

struct Edge { int32_t begin, end; int64_t weight; };
struct Node {
  uint8_t base;
  std::vector<int32_t> in, out;  // edge indices, in the order the edges were made
  std::vector<int32_t> aligned;
};
struct Graph {
  std::vector<Node> nodes;
  std::vector<Edge> edges;
  std::vector<int32_t> rank_to_node;

  int32_t add_node(uint8_t base) {
    nodes.emplace_back();
    nodes.back().base = base;
    return (int32_t)nodes.size() - 1;
  }
  void add_edge(int32_t b, int32_t e, uint32_t weight) {
    for (int32_t k : nodes[(size_t)b].out)
      if (edges[(size_t)k].end == e) {
        edges[(size_t)k].weight += weight;
        return;
      }
    edges.push_back(Edge{b, e, (int64_t)weight});
    nodes[(size_t)b].out.push_back((int32_t)edges.size() - 1);
    nodes[(size_t)e].in.push_back((int32_t)edges.size() - 1);
  }
  int32_t add_sequence(const uint8_t *seq, const uint32_t *wt, uint32_t begin, uint32_t end) {
    if (begin == end) return -1;
    const int32_t first = add_node(seq[begin]);
    for (uint32_t i = begin + 1; i < end; ++i) {
      const int32_t id = add_node(seq[i]);
      add_edge(id - 1, id, wt[i - 1] + wt[i]);  // both nodes contribute to the edge weight
    }
    return first;
  }
  // the float sum of the reference's add_edge(head, node, prev_weight + weights[..]) calls
  static uint32_t fsum(float prev, uint32_t w) { return (uint32_t)(prev + (float)w); }

  void add_alignment(const int32_t *pairs, int64_t n_pairs, const uint8_t *seq, uint32_t len, const uint32_t *wt) {
    if (len == 0) return;
    if (n_pairs == 0) {
      add_sequence(seq, wt, 0, len);
      topological_sort();
      return;
    }
    int64_t first_valid = -1, last_valid = -1;
    for (int64_t k = 0; k < n_pairs; ++k)
      if (pairs[2 * k + 1] != -1) {
        if (first_valid < 0) first_valid = pairs[2 * k + 1];
        last_valid = pairs[2 * k + 1];
      }
    const size_t before = nodes.size();
    add_sequence(seq, wt, 0, (uint32_t)first_valid);
    int32_t head = before == nodes.size() ? -1 : (int32_t)nodes.size() - 1;
    const int32_t tail = add_sequence(seq, wt, (uint32_t)last_valid + 1, len);
    int32_t node = -1;
    float prev_weight = head == -1 ? 0.f : (float)wt[first_valid - 1];
    for (int64_t k = 0; k < n_pairs; ++k) {
      const int32_t at = pairs[2 * k], pos = pairs[2 * k + 1];
      if (pos == -1) continue;
      const uint8_t letter = seq[pos];
      if (at == -1) {
        node = add_node(letter);
      } else if (nodes[(size_t)at].base == letter) {
        node = at;
      } else {
        int32_t to = -1;
        for (int32_t aid : nodes[(size_t)at].aligned)
          if (nodes[(size_t)aid].base == letter) {
            to = aid;
            break;
          }
        if (to == -1) {
          node = add_node(letter);
          const std::vector<int32_t> others = nodes[(size_t)at].aligned;
          for (int32_t aid : others) {
            nodes[(size_t)node].aligned.push_back(aid);
            nodes[(size_t)aid].aligned.push_back(node);
          }
          nodes[(size_t)node].aligned.push_back(at);
          nodes[(size_t)at].aligned.push_back(node);
        } else {
          node = to;
        }
      }
      if (head != -1) add_edge(head, node, fsum(prev_weight, wt[pos]));
      head = node;
      prev_weight = (float)wt[pos];
    }
    if (tail != -1) add_edge(head, tail, fsum(prev_weight, wt[last_valid + 1]));
    topological_sort();
  }

  void topological_sort() {
    rank_to_node.clear();
    const size_t n = nodes.size();
    std::vector<uint8_t> mark(n, 0), check(n, 1);  // 0 unmarked, 1 temporarily, 2 permanently marked
    std::vector<int32_t> stack;
    for (size_t i = 0; i < n; ++i) {
      if (mark[i] != 0) continue;
      stack.push_back((int32_t)i);
      while (!stack.empty()) {
        const int32_t id = stack.back();
        bool valid = true;
        if (mark[(size_t)id] != 2) {
          for (int32_t k : nodes[(size_t)id].in)
            if (mark[(size_t)edges[(size_t)k].begin] != 2) stack.push_back(edges[(size_t)k].begin), valid = false;
          if (check[(size_t)id])
            for (int32_t aid : nodes[(size_t)id].aligned)
              if (mark[(size_t)aid] != 2) stack.push_back(aid), check[(size_t)aid] = 0, valid = false;
          if (valid) {
            mark[(size_t)id] = 2;
            if (check[(size_t)id]) {
              rank_to_node.push_back(id);
              for (int32_t aid : nodes[(size_t)id].aligned) rank_to_node.push_back(aid);
            }
          } else {
            mark[(size_t)id] = 1;
          }
        }
        if (valid) stack.pop_back();
      }
    }
  }

  int32_t branch_completion(std::vector<int64_t> &scores, std::vector<int32_t> &preds, uint32_t rank) const {
    const int32_t node_id = rank_to_node[rank];
    for (int32_t k : nodes[(size_t)node_id].out)
      for (int32_t o : nodes[(size_t)edges[(size_t)k].end].in)
        if (edges[(size_t)o].begin != node_id) scores[(size_t)edges[(size_t)o].begin] = -1;
    int64_t max_score = 0;
    int32_t max_id = 0;
    for (size_t i = rank + 1; i < rank_to_node.size(); ++i) {
      const int32_t id = rank_to_node[i];
      scores[(size_t)id] = -1, preds[(size_t)id] = -1;
      for (int32_t k : nodes[(size_t)id].in) {
        const Edge &ed = edges[(size_t)k];
        if (scores[(size_t)ed.begin] == -1) continue;
        if (scores[(size_t)id] < ed.weight ||
            (scores[(size_t)id] == ed.weight && scores[(size_t)preds[(size_t)id]] <= scores[(size_t)ed.begin]))
          scores[(size_t)id] = ed.weight, preds[(size_t)id] = ed.begin;
      }
      if (preds[(size_t)id] != -1) scores[(size_t)id] += scores[(size_t)preds[(size_t)id]];
      if (max_score < scores[(size_t)id]) max_score = scores[(size_t)id], max_id = id;
    }
    return max_id;
  }

  void consensus(std::vector<uint8_t> *dst) const {  // generate_consensus()
    const size_t n = nodes.size();
    std::vector<int32_t> preds(n, -1);
    std::vector<int64_t> scores(n, -1);
    int32_t best = 0;
    for (int32_t id : rank_to_node) {
      for (int32_t k : nodes[(size_t)id].in) {
        const Edge &ed = edges[(size_t)k];
        if (scores[(size_t)id] < ed.weight ||
            (scores[(size_t)id] == ed.weight && scores[(size_t)preds[(size_t)id]] <= scores[(size_t)ed.begin]))
          scores[(size_t)id] = ed.weight, preds[(size_t)id] = ed.begin;
      }
      if (preds[(size_t)id] != -1) scores[(size_t)id] += scores[(size_t)preds[(size_t)id]];
      if (scores[(size_t)best] < scores[(size_t)id]) best = id;
    }
    if (!nodes[(size_t)best].out.empty()) {
      std::vector<uint32_t> rank_of(n, 0);
      for (size_t i = 0; i < n; ++i) rank_of[(size_t)rank_to_node[i]] = (uint32_t)i;
      while (!nodes[(size_t)best].out.empty()) best = branch_completion(scores, preds, rank_of[(size_t)best]);
    }
    std::vector<uint8_t> rev;
    while (preds[(size_t)best] != -1) rev.push_back(nodes[(size_t)best].base), best = preds[(size_t)best];
    rev.push_back(nodes[(size_t)best].base);
    dst->assign(rev.rbegin(), rev.rend());
  }

  // the view gb_poa_align takes, appended to the arrays
  void flatten(std::vector<uint8_t> *base, std::vector<int32_t> *id, std::vector<uint8_t> *out, std::vector<int32_t> *in_end,
               std::vector<int32_t> *pred, std::vector<int32_t> *rank_of) const {
    rank_of->resize(nodes.size());
    for (size_t r = 0; r < rank_to_node.size(); ++r) (*rank_of)[(size_t)rank_to_node[r]] = (int32_t)r;
    const size_t e0 = pred->size();
    for (int32_t nid : rank_to_node) {
      const Node &nd = nodes[(size_t)nid];
      base->push_back(nd.base), id->push_back(nid), out->push_back(!nd.out.empty());
      for (int32_t k : nd.in) pred->push_back((*rank_of)[(size_t)edges[(size_t)k].begin]);
      in_end->push_back((int32_t)(pred->size() - e0));
    }
  }
};

}  // namespace gbpoa

extern "C" {

int gb_poa_subtype(const gb_poa_params *p, int32_t *subtype) {
  GB_ARG(p && subtype, "gb_poa_subtype: null argument");
  gbpoa::Par P;
  gb_poa_params q = *p;
  q.type = GB_POA_NW;
  if (const int st = gbpoa::make_par("gb_poa_subtype", &q, &P)) return st;
  *subtype = P.sub;
  return GB_OK;
}

int64_t gb_poa_item_bytes(int32_t subtype, int32_t n_nodes, int32_t seq_len) {
  if (subtype < GB_POA_LINEAR || subtype > GB_POA_CONVEX || n_nodes < 0 || seq_len < 0) return 0;
  return gbpoa::item_bytes(subtype, n_nodes, seq_len);
}

int gb_poa_timing(float *fill_ms, float *walk_ms, float *host_ms, int64_t *cells) {
  GB_ARG(fill_ms && walk_ms && host_ms && cells, "gb_poa_timing: null argument");
  const gbpoa::Stats &S = gbpoa::stats();
  if (!S.calls) {
    gb::set_error("gb_poa_timing: neither gb_poa_align nor gb_poa_consensus has run on this thread");
    return GB_ERR_STATE;
  }
  *fill_ms = S.fill_ms, *walk_ms = S.walk_ms, *host_ms = S.host_ms, *cells = S.cells;
  return GB_OK;
}

int gb_poa_plan(int64_t *chunks, int64_t *workspace_bytes) {
  GB_ARG(chunks && workspace_bytes, "gb_poa_plan: null argument");
  const gbpoa::Stats &S = gbpoa::stats();
  if (!S.calls) {
    gb::set_error("gb_poa_plan: neither gb_poa_align nor gb_poa_consensus has run on this thread");
    return GB_ERR_STATE;
  }
  *chunks = S.chunks, *workspace_bytes = S.ws_bytes;
  return GB_OK;
}

int gb_poa_align(const gb_poa_params *p, const gb_poa_graphs *g, const uint8_t *seqs, int64_t seq_bytes,
                 const gb_poa_item *items, int64_t n_items, int32_t *scores, int32_t *pairs, int64_t pair_cap,
                 int64_t *pair_off, int64_t *pair_used) {
  using namespace gbpoa;
  const char *who = "gb_poa_align";
  gb::Range range_("gb.poa.align");
  try {
    GB_ARG(p && g && pair_off && pair_used && n_items >= 0 && seq_bytes >= 0 && (seq_bytes == 0 || seqs),
           "%s: null or negative argument", who);
    GB_ARG(g->n_nodes >= 0 && g->n_edges >= 0 &&
               (g->n_nodes == 0 || (g->node_base && g->node_id && g->node_out && g->in_end)) &&
               (g->n_edges == 0 || g->pred_rank),
           "%s: null or negative graph arrays", who);
    GB_ARG(n_items == 0 || (items && scores), "%s: null items or scores", who);
    GB_ARG(pair_cap >= 0 && (pair_cap == 0 || pairs), "%s: bad pair arguments", who);
    Par P;
    int st;
    if ((st = make_par(who, p, &P))) return st;
    const Batch B{*g, seqs, seq_bytes, items, n_items};
    if ((st = validate(who, "item", B))) return st;
    if (n_items == 0) {
      pair_off[0] = 0, *pair_used = 0;
      return GB_OK;
    }
    std::vector<int64_t> live, begin((size_t)n_items);
    int64_t need = 0;
    for (int64_t i = 0; i < n_items; ++i) {
      begin[(size_t)i] = need;
      if (live_item(items[i])) live.push_back(i), need += (int64_t)items[i].n_nodes + items[i].seq_len;
    }
    const bool host = gb::env_flag("GB_POA_HOST");
    std::vector<Chunk> chunks;
    int64_t budget = 0;
    if (!host && ((st = gb::env_number(who, "GB_POA_WS", 1, INT64_MAX, kDefaultBudget, &budget)) ||
                  (st = make_chunks(who, "item", nullptr, P, B, live, budget, &chunks))))
      return st;
    if (pair_cap < need) {
      *pair_used = need;
      gb::set_error("%s: pair_cap is %lld, the items need %lld (n_nodes + seq_len each)", who, (long long)pair_cap,
                    (long long)need);
      return GB_ERR_ARG;
    }
    Stats &S = stats();
    S = Stats{};
    std::vector<int32_t> slots((size_t)need * 2), count((size_t)n_items), sc((size_t)n_items);
    if ((st = run_batch(who, "item", nullptr, P, B, live, chunks, host, sc.data(), slots.data(), begin.data(), count.data())))
      return st;
    int64_t used = 0;
    for (int64_t i = 0; i < n_items; ++i) {
      pair_off[i] = used, scores[i] = sc[(size_t)i];
      if (count[(size_t)i])
        std::memcpy(pairs + 2 * used, slots.data() + 2 * begin[(size_t)i], (size_t)count[(size_t)i] * 8);
      used += count[(size_t)i];
    }
    pair_off[n_items] = *pair_used = used;
    S.calls = 1;
    return GB_OK;
  } catch (const std::bad_alloc &) {
    gb::set_error("%s: out of host memory", who);
    return GB_ERR_NOMEM;
  }
}

int gb_poa_consensus(const gb_poa_params *p, const int64_t *win_off, int64_t n_windows, const int64_t *seq_off,
                     int64_t n_seqs, const uint8_t *bytes, int64_t n_bytes, const uint32_t *weights, uint8_t *cons,
                     int64_t cons_cap, int64_t *cons_off, int64_t *cons_used, int32_t *node_count,
                     int64_t *n_alignments) {
  using namespace gbpoa;
  using clk = std::chrono::steady_clock;
  const char *who = "gb_poa_consensus";
  gb::Range range_("gb.poa.consensus");
  try {
    GB_ARG(p && win_off && seq_off && cons_off && cons_used && n_alignments && n_windows >= 0 && n_seqs >= 0 &&
               n_bytes >= 0 && (n_bytes == 0 || bytes),
           "%s: null or negative argument", who);
    GB_ARG(n_windows == 0 || node_count, "%s: null node_count", who);
    GB_ARG(cons_cap >= 0 && (cons_cap == 0 || cons), "%s: bad consensus arguments", who);
    Par P;
    int st;
    if ((st = make_par(who, p, &P))) return st;
    for (int64_t s = 0; s < n_seqs; ++s) {
      GB_ARG(seq_off[s] >= 0 && seq_off[s] <= seq_off[s + 1] && seq_off[s + 1] <= n_bytes,
             "%s: sequence %lld lies at [%lld, %lld), outside the %lld bytes", who, (long long)s, (long long)seq_off[s],
             (long long)seq_off[s + 1], (long long)n_bytes);
      GB_ARG(seq_off[s + 1] - seq_off[s] <= GB_POA_MAX_LEN, "%s: sequence %lld has %lld bases (0 .. %d)", who,
             (long long)s, (long long)(seq_off[s + 1] - seq_off[s]), GB_POA_MAX_LEN);
    }
    int64_t max_round = 0;
    for (int64_t w = 0; w < n_windows; ++w) {
      GB_ARG(win_off[w] >= 0 && win_off[w] <= win_off[w + 1] && win_off[w + 1] <= n_seqs,
             "%s: window %lld holds the sequences [%lld, %lld), outside the %lld", who, (long long)w, (long long)win_off[w],
             (long long)win_off[w + 1], (long long)n_seqs);
      GB_ARG(seq_off[win_off[w + 1]] - seq_off[win_off[w]] <= GB_POA_MAX_NODES,
             "%s: window %lld holds %lld bases, more than a graph's %d nodes", who, (long long)w,
             (long long)(seq_off[win_off[w + 1]] - seq_off[win_off[w]]), GB_POA_MAX_NODES);
      max_round = std::max(max_round, win_off[w + 1] - win_off[w]);
    }
    const bool host = gb::env_flag("GB_POA_HOST");
    int64_t budget = 0;
    if (!host && (st = gb::env_number(who, "GB_POA_WS", 1, INT64_MAX, kDefaultBudget, &budget))) return st;
    const int64_t need = n_seqs ? seq_off[n_seqs] - seq_off[0] : 0;
    if (cons_cap < need) {
      *cons_used = need;
      gb::set_error("%s: cons_cap is %lld, the windows need %lld (their bytes)", who, (long long)cons_cap, (long long)need);
      return GB_ERR_ARG;
    }
    int nth = 1;
    if ((st = gb::thread_count(who, "GB_POA_THREADS", &nth))) return st;
    Stats &S = stats();
    S = Stats{};
    std::vector<uint32_t> ones;
    if (!weights) ones.assign((size_t)n_bytes, 1u), weights = ones.data();
    std::vector<Graph> graphs((size_t)n_windows);
    int64_t done = 0;
    std::vector<uint8_t> v_base, v_out;
    std::vector<int32_t> v_id, v_in_end, v_pred, rank_of, sc, count, slots;
    std::vector<gb_poa_item> items;
    std::vector<int64_t> names, begin, live;
    double host_s = 0.0;
    for (int64_t j = 0; j < max_round; ++j) {
      const auto t0 = clk::now();
      v_base.clear(), v_out.clear(), v_id.clear(), v_in_end.clear(), v_pred.clear(), items.clear(), names.clear();
      begin.clear(), live.clear();
      int64_t pairs_need = 0;
      for (int64_t w = 0; w < n_windows; ++w) {
        if (win_off[w + 1] - win_off[w] <= j) continue;
        const int64_t s = win_off[w] + j;
        const Graph &G = graphs[(size_t)w];
        gb_poa_item it{};
        it.node_off = (int64_t)v_base.size(), it.edge_off = (int64_t)v_pred.size(), it.seq_off = seq_off[s];
        it.seq_len = (int32_t)(seq_off[s + 1] - seq_off[s]), it.n_nodes = (int32_t)G.nodes.size();
        if (it.seq_len && it.n_nodes) G.flatten(&v_base, &v_id, &v_out, &v_in_end, &v_pred, &rank_of);
        else it.n_nodes = 0;  // nothing to align: the sequence opens the graph, or is empty
        it.n_edges = (int32_t)((int64_t)v_pred.size() - it.edge_off);
        begin.push_back(pairs_need);
        if (live_item(it)) live.push_back((int64_t)items.size()), pairs_need += (int64_t)it.n_nodes + it.seq_len;
        items.push_back(it), names.push_back(w);
      }
      host_s += std::chrono::duration<double>(clk::now() - t0).count();
      const int64_t n_items = (int64_t)items.size();
      sc.assign((size_t)n_items, 0), count.assign((size_t)n_items, 0), slots.resize((size_t)pairs_need * 2);
      const Batch B{gb_poa_graphs{v_base.data(), v_id.data(), v_out.data(), v_in_end.data(), v_pred.data(),
                                  (int64_t)v_base.size(), (int64_t)v_pred.size()},
                    bytes, n_bytes, items.data(), n_items};
      std::vector<Chunk> chunks;
      if (!host && (st = make_chunks(who, "window", names.data(), P, B, live, budget, &chunks))) return st;
      if ((st = run_batch(who, "window", names.data(), P, B, live, chunks, host, sc.data(), slots.data(), begin.data(),
                          count.data())))
        return st;
      done += (int64_t)live.size();
      const auto t1 = clk::now();
      std::atomic<int64_t> next{0};
      if ((st = gb::parallel(who, (int)std::max<int64_t>(1, std::min<int64_t>(nth, n_items)), [&](int) {
             for (int64_t k; (k = next.fetch_add(1)) < n_items;) {
               const gb_poa_item &it = items[(size_t)k];
               graphs[(size_t)names[(size_t)k]].add_alignment(slots.data() + 2 * begin[(size_t)k], count[(size_t)k],
                                                             bytes + it.seq_off, (uint32_t)it.seq_len,
                                                             weights + it.seq_off);
             }
           })))
        return st;
      host_s += std::chrono::duration<double>(clk::now() - t1).count();
    }
    const auto t2 = clk::now();
    std::vector<std::vector<uint8_t>> out((size_t)n_windows);
    std::atomic<int64_t> next{0};
    if ((st = gb::parallel(who, (int)std::max<int64_t>(1, std::min<int64_t>(nth, n_windows)), [&](int) {
           for (int64_t w; (w = next.fetch_add(1)) < n_windows;)
             if (!graphs[(size_t)w].nodes.empty()) graphs[(size_t)w].consensus(&out[(size_t)w]);
         })))
      return st;
    int64_t used = 0;
    for (int64_t w = 0; w < n_windows; ++w) {
      cons_off[w] = used, node_count[w] = (int32_t)graphs[(size_t)w].nodes.size();
      if (!out[(size_t)w].empty()) std::memcpy(cons + used, out[(size_t)w].data(), out[(size_t)w].size());
      used += (int64_t)out[(size_t)w].size();
    }
    cons_off[n_windows] = *cons_used = used, *n_alignments = done;
    host_s += std::chrono::duration<double>(clk::now() - t2).count();
    S.host_ms = (float)(host_s * 1e3), S.calls = 1;
    return GB_OK;
  } catch (const std::bad_alloc &) {
    gb::set_error("%s: out of host memory", who);
    return GB_ERR_NOMEM;
  }
}

}  // extern "C"
