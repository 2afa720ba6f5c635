// chain_extd2.hip -- gb_chain_extd2: minimap2's ksw_extd2_sse (dual affine gaps, band, z-drop, CIGAR) for a
// batch of (query, target) items, bit for bit (chain_extd2_internal.h has the arithmetic and says what is kept
// of the reference's memory).
//
// Fill: one wave per item sweeps the item's anti-diagonals in order. The reference's block of row arrays and
// its 32-bit H[] live in the workgroup's LDS (dynamic, sized by the launch's largest item), or, for an item
// whose state passes 64 KiB, in the chunk's device workspace. A row is the reference's: the edge bytes, the
// scores in runs of 16 from st0, then the aligned range [st, en] with B bytes per lane (4 or 16: a quarter of
// the reference's __m128i block, or one), then H and the row maximum with the reference's tie rule, then the
// record's bookkeeping, which every lane carries. A row wider than 64 * B bytes is taken in pieces from the
// right: a piece's first cell reads the old x, v, x2 of the piece to its left, which is then still untouched,
// and inside a piece every lane has loaded before any lane stores. A cell leaves one byte of backtrack code
// at the reference's place, p[r * n_col_ * 16 + t - st].
//
// Size classes, by the blocks of a row (n_col_) and the state's size:
//   0  n_col_ <= 16            B = 4,  one piece          state in LDS
//   1  n_col_ <= 64            B = 16, one piece          state in LDS
//   2  n_col_ >  64            B = 16, pieces of 64 lanes state in LDS
//   3  state above 64 KiB      B = 16, pieces of 64 lanes state in the workspace
// A chunk's items of classes 0 to 2 are launched by class and by the LDS they need (up to 8, 16, 32, 64 KiB:
// a launch asks every workgroup for its largest item's), the launches side by side on four streams.
// Walk: one lane per item runs ksw_backtrack over the codes into the item's part of a word buffer. Pack: the
// host scans the lengths, a wave per item copies the words to their place, reversed unless REV_CIGAR is set.
// No kernel waits on another workgroup; every loop is bounded by the item's qlen + tlen - 1 rows.
//
// GB_CHAIN_EXTD2_HOST=1 runs host_item below instead, on GB_CHAIN_THREADS threads.
#include "chain_extd2_internal.h"
#include "gb_common_wave.h"

namespace gbx2 {

constexpr int64_t kDefaultBudget = int64_t(4) << 30;
constexpr int kLdsMax = 64 * 1024;
constexpr int kClasses = 4;
constexpr int kBuckets = 4;                        // of the LDS a workgroup asks for: up to 8, 16, 32, 64 KiB
constexpr int kGroups = (kClasses - 1) * kBuckets + 1;  // launches of a chunk: class x bucket, and class 3
constexpr int kStreams = 4;

GB_HD bool early_item(const Par &P, const gb_chain_extd2_item &it) { return it.qlen <= 0 || it.tlen <= 0 || P.early; }
static inline int size_class(const gb_chain_extd2_item &it) {
  if (state_bytes(it.qlen, it.tlen) > kLdsMax) return 3;
  const int nc = n_col(it.qlen, it.tlen, eff_w(it.qlen, it.tlen, it.w));
  return nc <= 16 ? 0 : nc <= 64 ? 1 : 2;
}
// the launch an item goes to: the largest states first, so that the longest sweeps start first
static inline int launch_group(const gb_chain_extd2_item &it) {
  const int c = size_class(it);
  if (c == 3) return 0;
  const int64_t sb = state_bytes(it.qlen, it.tlen);
  const int b = sb <= 8 * 1024 ? 0 : sb <= 16 * 1024 ? 1 : sb <= 32 * 1024 ? 2 : 3;
  return 1 + (kBuckets - 1 - b) * (kClasses - 1) + (kClasses - 2 - c);
}
static inline int64_t item_codes(const gb_chain_extd2_item &it) {  // bytes, a multiple of 16
  return (int64_t)(it.qlen + it.tlen - 1) * n_col(it.qlen, it.tlen, eff_w(it.qlen, it.tlen, it.w)) * 16;
}

// ---- host path ----

struct HostScratch {
  std::vector<uint8_t> mem, codes;
  std::vector<int32_t> H;
  std::vector<uint32_t> cigar;
};

template <bool RIGHT>
static void host_core(const Par &P, const Lay &L, uint8_t *mem, const Row &R, int x1, int x21, int v1, uint8_t *pr) {
  int8_t *m8 = reinterpret_cast<int8_t *>(mem);
  int8_t *u = m8 + L.u(), *v = m8 + L.v(), *x = m8 + L.x(), *y = m8 + L.y(), *x2 = m8 + L.x2(), *y2 = m8 + L.y2();
  const int8_t *s = m8 + L.s();
  int xl = x1, x2l = x21, vl = v1;
  for (int t = R.st; t <= R.en; ++t) {
    const int xo = x[t], vo = v[t], x2o = x2[t];
    int nu, nv, nx, ny, nx2, ny2;
    pr[t - R.st] = (uint8_t)cell<RIGHT>(P, s[t], xl, vl, x2l, u[t], y[t], y2[t], &nu, &nv, &nx, &ny, &nx2, &ny2);
    u[t] = (int8_t)nu, v[t] = (int8_t)nv, x[t] = (int8_t)nx, y[t] = (int8_t)ny, x2[t] = (int8_t)nx2, y2[t] = (int8_t)ny2;
    xl = xo, vl = vo, x2l = x2o;
  }
}

// One item: the record, and its CIGAR words in the reference's order at cigar[0 ..). Returns the cells swept.
static int64_t host_item(const Par &P, const uint8_t *seqs, const gb_chain_extd2_item &it, HostScratch *hs,
                         gb_chain_extd2_result *ez, uint32_t *cigar) {
  reset_result(ez);
  if (early_item(P, it)) return 0;
  const int qlen = it.qlen, tlen = it.tlen, w = eff_w(qlen, tlen, it.w), flag = it.flag;
  const Lay L = make_lay(qlen, tlen);
  const int64_t ncol16 = (int64_t)n_col(qlen, tlen, w) * 16;
  const bool approx = flag & GB_EXTD2_APPROX_MAX;
  hs->mem.assign((size_t)L.bytes(), 0);
  uint8_t *mem = hs->mem.data();
  std::memset(mem + L.u(), P.nqe, (size_t)4 * L.T16);
  std::memset(mem + L.x2(), P.nqe2, (size_t)2 * L.T16);
  hs->H.assign((size_t)L.T16, kNegInf);
  hs->codes.resize((size_t)((qlen + tlen - 1) * ncol16));
  const uint8_t *query = seqs + it.q_off, *target = seqs + it.t_off;
  for (int t = 0; t < qlen; ++t) mem[L.qr() + t] = query[qlen - 1 - t];
  std::memcpy(mem + L.sf(), target, (size_t)tlen);
  int8_t *m8 = reinterpret_cast<int8_t *>(mem);
  int8_t *u8 = m8 + L.u(), *v8 = m8 + L.v();
  int32_t *H = hs->H.data(), H0 = 0;
  int last_st = -1, last_en = -1, last_H0_t = 0;
  int64_t cells = 0;
  for (int r = 0; r < qlen + tlen - 1; ++r) {
    Row R;
    if (!row_bounds(r, qlen, tlen, w, &R)) {
      ez->zdropped = 1;
      break;
    }
    cells += R.en0 - R.st0 + 1;
    int x1 = P.nqe, x21 = P.nqe2, v1 = P.nqe;
    if (R.st > 0) {
      if (R.st - 1 >= last_st && R.st - 1 <= last_en)
        x1 = m8[L.x() + R.st - 1], x21 = m8[L.x2() + R.st - 1], v1 = v8[R.st - 1];
    } else {
      v1 = edge_gap(P, r);
    }
    if (R.en >= r) m8[L.y() + r] = P.nqe, m8[L.y2() + r] = P.nqe2, u8[r] = (int8_t)edge_gap(P, r);
    const int qoff = L.qr() + qlen - 1 - r;
    for (int t = R.st0; t <= R.en0; t += 16)
      for (int k = t; k < t + 16; ++k) m8[L.s() + k] = (int8_t)score_of(P, mem[L.sf() + k], mem[qoff + k]);
    uint8_t *pr = hs->codes.data() + (int64_t)r * ncol16;
    if (flag & GB_EXTD2_RIGHT)
      host_core<true>(P, L, mem, R, x1, x21, v1, pr);
    else
      host_core<false>(P, L, mem, R, x1, x21, v1, pr);
    bool stop;
    if (!approx) {
      int32_t max_H;
      int max_t;
      if (r > 0) {
        max_H = H[R.en0] = R.en0 > 0 ? H[R.en0 - 1] + u8[R.en0] : H[R.en0] + v8[R.en0];
        int best = 0;
        for (int t = R.st0; t < R.en0; ++t) {
          H[t] += v8[t];
          const int rank = tie_rank(t, R.st0, R.en0);
          if (H[t] > max_H || (H[t] == max_H && rank < best)) max_H = H[t], best = rank;
        }
        max_t = best ? best & 0xffff : R.en0;
      } else {
        H[0] = v8[0] - P.qe_pre, max_H = H[0], max_t = 0;
      }
      stop = after_row_exact(P, ez, r, R, qlen, tlen, it.zdrop, max_H, max_t, H[R.en0], H[R.st0]);
    } else {
      stop = after_row_approx(P, ez, r, R, qlen, tlen, it.zdrop, flag, u8, v8, &H0, &last_H0_t);
    }
    if (stop) break;
    last_st = R.st, last_en = R.en;
  }
  int i0, j0;
  if (walk_start(ez, qlen, tlen, it.end_bonus, flag, &i0, &j0)) {
    hs->cigar.resize((size_t)(qlen + tlen));
    const int n = walk(hs->codes.data(), ncol16, qlen, tlen, w, i0, j0, hs->cigar.data());
    const bool rev = flag & GB_EXTD2_REV_CIGAR;
    for (int k = 0; k < n; ++k) cigar[k] = hs->cigar[(size_t)(rev ? k : n - 1 - k)];
    ez->n_cigar = n;
  }
  return cells;
}

// ---- device path ----

struct DItem {
  int64_t q_off, t_off;
  int64_t code_off;   // bytes into the chunk's codes, a multiple of 16
  int64_t state_off;  // bytes into the chunk's state, a multiple of 16 (class 3 only)
  int64_t cig_off;    // words into the chunk's walk buffer
  int32_t qlen, tlen, w, zdrop, end_bonus, flag;
  int32_t out, pad;   // index in the chunk
};
static_assert(sizeof(DItem) == 72, "DItem is packed");

struct Args {
  Par P;
  const uint8_t *seqs;
  const DItem *items;
  int64_t n;  // the walk and the pack: the chunk's items
  uint8_t *codes, *state;
  gb_chain_extd2_result *res;
  int64_t *cells;
  uint32_t *walked, *packed;
  const int64_t *offs;
};

__device__ __forceinline__ uint32_t splat(int8_t b) { return 0x01010101u * (uint8_t)b; }
__device__ __forceinline__ int byte_of(uint32_t w, int k) { return (int)(int8_t)(w >> (8 * k)); }

template <int B, bool LDS>
__global__ __launch_bounds__(64) void extd2_fill_kernel(Args A) {
  extern __shared__ __align__(16) uint8_t lds[];
  constexpr int W = B / 4;  // words per lane
  const DItem I = A.items[blockIdx.x];
  const Par P = A.P;
  const int lane = threadIdx.x;
  const int qlen = I.qlen, tlen = I.tlen, w = I.w, flag = I.flag;
  const Lay L = make_lay(qlen, tlen);
  const int64_t ncol16 = (int64_t)n_col(qlen, tlen, w) * 16;
  uint8_t *mem = LDS ? lds : A.state + I.state_off;
  int32_t *H = reinterpret_cast<int32_t *>(mem + L.bytes());  // L.bytes() is a multiple of 16
  uint32_t *mw = reinterpret_cast<uint32_t *>(mem);
  const bool approx = flag & GB_EXTD2_APPROX_MAX, right = flag & GB_EXTD2_RIGHT;

  // the reference's memsets, calloc, the reversed query and the target
  for (int i = lane; i < L.T16; i += 64) mw[i] = splat(P.nqe);                             // u v x y
  for (int i = L.T16 + lane; i < L.T16 * 3 / 2; i += 64) mw[i] = splat(P.nqe2);            // x2 y2
  for (int i = L.T16 * 3 / 2 + lane; i < L.bytes() / 4; i += 64) mw[i] = 0;                 // s, the padding
  for (int i = lane; i < L.T16; i += 64) H[i] = kNegInf;
  __syncthreads();
  const uint8_t *query = A.seqs + I.q_off, *target = A.seqs + I.t_off;
  for (int t = lane; t < qlen; t += 64) mem[L.qr() + t] = query[qlen - 1 - t];
  for (int t = lane; t < tlen; t += 64) mem[L.sf() + t] = target[t];
  __syncthreads();

  int8_t *m8 = reinterpret_cast<int8_t *>(mem);
  uint8_t *codes = A.codes + I.code_off;
  gb_chain_extd2_result ez;
  reset_result(&ez);
  int32_t H0 = 0;
  int last_st = -1, last_en = -1, last_H0_t = 0;
  int64_t cells = 0;
  const int rows = qlen + tlen - 1;
  for (int r = 0; r < rows; ++r) {
    Row R;
    if (!row_bounds(r, qlen, tlen, w, &R)) {
      ez.zdropped = 1;
      break;
    }
    cells += R.en0 - R.st0 + 1;
    // the edges: every lane reads the three bytes left of st before anything of this row is stored
    int x1 = P.nqe, x21 = P.nqe2, v1 = P.nqe;
    if (R.st > 0) {
      if (R.st - 1 >= last_st && R.st - 1 <= last_en)
        x1 = m8[L.x() + R.st - 1], x21 = m8[L.x2() + R.st - 1], v1 = m8[L.v() + R.st - 1];
    } else {
      v1 = edge_gap(P, r);
    }
    if (R.en >= r && lane == 0) m8[L.y() + r] = P.nqe, m8[L.y2() + r] = P.nqe2, m8[L.u() + r] = (int8_t)edge_gap(P, r);
    // the scores: 16-byte runs from st0, whatever bytes lie there
    {
      const int n = ((R.en0 - R.st0) / 16 + 1) * 16, qoff = L.qr() + qlen - 1 - r;
      for (int k = R.st0 + lane; k < R.st0 + n; k += 64) m8[L.s() + k] = (int8_t)score_of(P, mem[L.sf() + k], mem[qoff + k]);
    }
    __syncthreads();
    // the aligned range, in pieces of 64 lanes from the right
    const int span = R.en - R.st + 1;
    for (int piece = (span - 1) / (64 * B); piece >= 0; --piece) {
      const int t = R.st + (piece * 64 + lane) * B;
      const bool on = t <= R.en;
      uint32_t zs[W], uo[W], vo[W], xo[W], yo[W], x2o[W], y2o[W];
      int xl = x1, vl = v1, x2l = x21;
      if (on) {
#pragma unroll
        for (int k = 0; k < W; ++k) {
          const int o = t / 4 + k;
          zs[k] = mw[L.s() / 4 + o], uo[k] = mw[L.u() / 4 + o], vo[k] = mw[L.v() / 4 + o], xo[k] = mw[L.x() / 4 + o];
          yo[k] = mw[L.y() / 4 + o], x2o[k] = mw[L.x2() / 4 + o], y2o[k] = mw[L.y2() / 4 + o];
        }
        if (t > R.st) xl = m8[L.x() + t - 1], vl = m8[L.v() + t - 1], x2l = m8[L.x2() + t - 1];
      }
      __syncthreads();  // every lane has loaded; the stores of this piece follow
      if (on) {
        uint32_t un[W], vn[W], xn[W], yn[W], x2n[W], y2n[W], dn[W];
#pragma unroll
        for (int k = 0; k < W; ++k) {
          un[k] = vn[k] = xn[k] = yn[k] = x2n[k] = y2n[k] = dn[k] = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            int nu, nv, nx, ny, nx2, ny2;
            const int z = byte_of(zs[k], b), ut = byte_of(uo[k], b), yt = byte_of(yo[k], b), y2t = byte_of(y2o[k], b);
            const unsigned d = right ? cell<true>(P, z, xl, vl, x2l, ut, yt, y2t, &nu, &nv, &nx, &ny, &nx2, &ny2)
                                     : cell<false>(P, z, xl, vl, x2l, ut, yt, y2t, &nu, &nv, &nx, &ny, &nx2, &ny2);
            xl = byte_of(xo[k], b), vl = byte_of(vo[k], b), x2l = byte_of(x2o[k], b);
            un[k] |= (uint32_t)(uint8_t)nu << (8 * b), vn[k] |= (uint32_t)(uint8_t)nv << (8 * b);
            xn[k] |= (uint32_t)(uint8_t)nx << (8 * b), yn[k] |= (uint32_t)(uint8_t)ny << (8 * b);
            x2n[k] |= (uint32_t)(uint8_t)nx2 << (8 * b), y2n[k] |= (uint32_t)(uint8_t)ny2 << (8 * b);
            dn[k] |= d << (8 * b);
          }
        }
        uint32_t *pr = reinterpret_cast<uint32_t *>(codes + (int64_t)r * ncol16 + (t - R.st));
#pragma unroll
        for (int k = 0; k < W; ++k) {
          const int o = t / 4 + k;
          mw[L.u() / 4 + o] = un[k], mw[L.v() / 4 + o] = vn[k], mw[L.x() / 4 + o] = xn[k], mw[L.y() / 4 + o] = yn[k];
          mw[L.x2() / 4 + o] = x2n[k], mw[L.y2() / 4 + o] = y2n[k];
          pr[k] = dn[k];
        }
      }
    }
    __syncthreads();
    bool stop;
    if (!approx) {
      int32_t max_H;
      int max_t;
      if (r > 0) {
        const int32_t H_en0 = R.en0 > 0 ? H[R.en0 - 1] + m8[L.u() + R.en0] : H[R.en0] + m8[L.v() + R.en0];
        __syncthreads();  // H[en0 - 1] is read by every lane before its owner adds to it
        int32_t best = H_en0;
        int rank = 0;
        for (int t = R.st0 + lane; t < R.en0; t += 64) {
          const int32_t h = H[t] + m8[L.v() + t];
          H[t] = h;
          const int rk = tie_rank(t, R.st0, R.en0);
          if (h > best || (h == best && rk < rank)) best = h, rank = rk;
        }
        if (lane == 0) H[R.en0] = H_en0;
        max_H = gb::wave_max<INT32_MIN>(best);
        rank = best == max_H ? rank : INT32_MAX;
        rank = __builtin_amdgcn_readlane(gb::scan_min<INT32_MAX>(rank), 63);
        max_t = rank ? rank & 0xffff : R.en0;
      } else {
        max_H = m8[L.v()] - P.qe_pre, max_t = 0;
        if (lane == 0) H[0] = max_H;
      }
      __syncthreads();
      stop = after_row_exact(P, &ez, r, R, qlen, tlen, I.zdrop, max_H, max_t, H[R.en0], H[R.st0]);
    } else {
      stop = after_row_approx(P, &ez, r, R, qlen, tlen, I.zdrop, flag, m8 + L.u(), m8 + L.v(), &H0, &last_H0_t);
    }
    if (stop) break;
    last_st = R.st, last_en = R.en;
  }
  if (lane == 0) A.res[I.out] = ez, A.cells[I.out] = cells;
}

// one lane per item of the chunk: where the walk starts, the walk, n_cigar and reach_end
__global__ __launch_bounds__(64) void extd2_walk_kernel(Args A) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= A.n) return;
  const DItem I = A.items[i];
  gb_chain_extd2_result ez = A.res[I.out];
  int i0, j0;
  if (!walk_start(&ez, I.qlen, I.tlen, I.end_bonus, I.flag, &i0, &j0)) return;
  const int64_t ncol16 = (int64_t)n_col(I.qlen, I.tlen, I.w) * 16;
  ez.n_cigar = walk(A.codes + I.code_off, ncol16, I.qlen, I.tlen, I.w, i0, j0, A.walked + I.cig_off);
  A.res[I.out] = ez;
}

// a wave per item: the walked words to packed[offs ..], reversed unless REV_CIGAR keeps the walk's order
__global__ __launch_bounds__(256) void extd2_pack_kernel(Args A) {
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < A.n; i += (int64_t)gridDim.x * 4) {
    const DItem I = A.items[i];
    const int n = A.res[I.out].n_cigar;
    const bool rev = I.flag & GB_EXTD2_REV_CIGAR;
    const uint32_t *src = A.walked + I.cig_off;
    uint32_t *dst = A.packed + A.offs[I.out];
    for (int j = lane; j < n; j += 64) dst[j] = src[rev ? j : n - 1 - j];
  }
}

struct Ws : gb::WsBase<5> {  // the calling thread's, through gb::get_ws
  gb::Stream side[kStreams - 1];  // the fill's launches are spread over `stream` and these
  gb::Event fork, join[kStreams - 1];
  gb::DevBuf<uint8_t> d_seqs, d_codes, d_state;
  gb::DevBuf<DItem> d_items;
  gb::DevBuf<gb_chain_extd2_result> d_res;
  gb::DevBuf<int64_t> d_cells, d_offs;
  gb::DevBuf<uint32_t> d_walked, d_packed;
  gb::PinnedBuf<DItem> h_items;
  gb::PinnedBuf<gb_chain_extd2_result> h_res;
  gb::PinnedBuf<int64_t> h_cells, h_offs;
  gb::PinnedBuf<uint32_t> h_packed;
  float fill_ms = 0.f, walk_ms = 0.f;
  int64_t cells = 0, calls = 0, chunks = 0, ws_bytes = 0;
};

static hipError_t make_sides(Ws *W) {  // the workspace's own part of gb::get_ws, which words the error
  hipError_t e = hipSuccess;
  for (auto &st : W->side)
    if (e == hipSuccess) e = st.create();
  for (auto &ev : W->join)
    if (e == hipSuccess) e = ev.create();
  return e == hipSuccess ? W->fork.create() : e;
}

struct Need {
  int64_t codes, state, words;
  int64_t bytes() const { return codes + state + 2 * words * (int64_t)sizeof(uint32_t); }
  void operator+=(const Need &o) { codes += o.codes, state += o.state, words += o.words; }
  void max_with(const Need &o) {
    codes = std::max(codes, o.codes), state = std::max(state, o.state), words = std::max(words, o.words);
  }
};
using Chunk = gb::Chunk<Need>;  // of the call's list of live items

static inline Need item_need(const gb_chain_extd2_item &it) {
  const int64_t st = size_class(it) == 3 ? gb::round_up(state_bytes(it.qlen, it.tlen), 16) : 0;
  return Need{item_codes(it), st, (int64_t)it.qlen + it.tlen};
}

// The chunks of a call: the live items in order, as many as fit GB_CHAIN_EXTD2_WS or the default. Refuses the item
// that alone does not.
static int make_chunks(const char *who, const gb_chain_extd2_item *items, const std::vector<int64_t> &live,
                       std::vector<Chunk> *chunks) {
  int64_t budget = 0;
  if (const int st = gb::env_number(who, "GB_CHAIN_EXTD2_WS", 1, INT64_MAX, kDefaultBudget, &budget)) return st;
  auto need_of = [&](int64_t k) { return item_need(items[live[(size_t)k]]); };
  const int64_t k = gb::cut_chunks((int64_t)live.size(), budget, need_of, chunks);
  GB_ARG(k < 0, "%s: item %lld needs %lld bytes of workspace, more than the budget of %lld (GB_CHAIN_EXTD2_WS)", who,
         (long long)live[(size_t)k], (long long)need_of(k).bytes(), (long long)budget);
  return GB_OK;
}

// One chunk: fill by class, walk, pack, copy back. The records go to res, the words to cigar[*used ..] in item
// order, and cigar_off of the chunk's items is set.
static int run_chunk(Ws *W, const Par &P, const Chunk &ch, const gb_chain_extd2_item *items,
                     const std::vector<int64_t> &live, gb_chain_extd2_result *res, uint32_t *cigar, int64_t *cigar_off,
                     int64_t *used) {
  const int64_t n = ch.last - ch.first;
  std::vector<int32_t> order((size_t)n);
  int64_t count[kGroups] = {}, first[kGroups];
  int lds[kGroups] = {}, cls[kGroups] = {};
  for (int64_t i = 0; i < n; ++i) {
    const gb_chain_extd2_item &it = items[live[(size_t)(ch.first + i)]];
    order[(size_t)i] = (int32_t)i;
    const int g = launch_group(it), c = size_class(it);
    count[g] += 1, cls[g] = c;
    if (c < 3) lds[g] = std::max(lds[g], (int)state_bytes(it.qlen, it.tlen));
  }
  // by launch, the items of most rows first, so that the long ones do not start last
  auto key = [&](int32_t i) {
    const gb_chain_extd2_item &it = items[live[(size_t)(ch.first + i)]];
    return ((int64_t)launch_group(it) << 32) | (int64_t)(2 * GB_EXTD2_MAX_LEN - (it.qlen + it.tlen));
  };
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key(a) < key(b); });
  std::vector<int64_t> code_off((size_t)n), state_off((size_t)n), cig_off((size_t)n);
  int64_t co = 0, so = 0, wo = 0;
  for (int64_t i = 0; i < n; ++i) {  // the buffers in item order
    const Need one = item_need(items[live[(size_t)(ch.first + i)]]);
    code_off[(size_t)i] = co, state_off[(size_t)i] = so, cig_off[(size_t)i] = wo;
    co += one.codes, so += one.state, wo += one.words;
  }
  DItem *hi = W->h_items;
  int64_t pos = 0;
  for (int c = 0; c < kGroups; ++c) {
    first[c] = pos;
    for (int64_t j = 0; j < count[c]; ++j, ++pos) {
      const int32_t i = order[(size_t)pos];
      const gb_chain_extd2_item &it = items[live[(size_t)(ch.first + i)]];
      hi[pos] = DItem{it.q_off,  it.t_off, code_off[(size_t)i],           state_off[(size_t)i], cig_off[(size_t)i],
                      it.qlen,   it.tlen,  eff_w(it.qlen, it.tlen, it.w), it.zdrop,             it.end_bonus,
                      it.flag,   i,        0};
    }
  }
  GB_HIP(hipMemcpyAsync(W->d_items, hi, (size_t)n * sizeof(DItem), hipMemcpyHostToDevice, W->stream));
  Args A;
  A.P = P, A.seqs = W->d_seqs, A.codes = W->d_codes, A.state = W->d_state, A.res = W->d_res, A.cells = W->d_cells;
  A.walked = W->d_walked, A.packed = W->d_packed, A.offs = W->d_offs, A.n = n;
  GB_HIP(hipEventRecord(W->ev[0], W->stream));
  // Fork: a launch asks every workgroup for the LDS of its largest item, and a sweep is as long as its item's
  // rows, so the launches run side by side on four streams instead of each waiting for the one before it.
  GB_HIP(hipEventRecord(W->fork, W->stream));
  for (auto &st : W->side) GB_HIP(hipStreamWaitEvent(st, W->fork, 0));
  int launches = 0;
  for (int g = 0; g < kGroups; ++g) {
    if (!count[g]) continue;
    A.items = W->d_items.get() + first[g];
    const dim3 grid((unsigned)count[g]), block(64);
    const size_t shm = (size_t)gb::round_up(lds[g], 256);
    const int k = launches++ % kStreams;
    hipStream_t st = k == 0 ? (hipStream_t)W->stream : (hipStream_t)W->side[k - 1];
    if (cls[g] == 0)
      hipLaunchKernelGGL((extd2_fill_kernel<4, true>), grid, block, shm, st, A);
    else if (cls[g] < 3)
      hipLaunchKernelGGL((extd2_fill_kernel<16, true>), grid, block, shm, st, A);
    else
      hipLaunchKernelGGL((extd2_fill_kernel<16, false>), grid, block, 0, st, A);
    GB_HIP(hipGetLastError());
  }
  for (int k = 0; k < kStreams - 1; ++k) {  // join
    GB_HIP(hipEventRecord(W->join[k], W->side[k]));
    GB_HIP(hipStreamWaitEvent(W->stream, W->join[k], 0));
  }
  GB_HIP(hipEventRecord(W->ev[1], W->stream));
  A.items = W->d_items;
  hipLaunchKernelGGL(extd2_walk_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, W->stream, A);
  GB_HIP(hipGetLastError());
  GB_HIP(hipEventRecord(W->ev[2], W->stream));
  GB_HIP(hipMemcpyAsync(W->h_res, W->d_res, (size_t)n * sizeof(gb_chain_extd2_result), hipMemcpyDeviceToHost, W->stream));
  GB_HIP(hipMemcpyAsync(W->h_cells, W->d_cells, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, W->stream));
  GB_HIP(hipStreamSynchronize(W->stream));
  int64_t got = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t g = live[(size_t)(ch.first + i)];
    W->h_offs[i] = got;
    cigar_off[g] = *used + got;
    res[g] = W->h_res[i];
    got += W->h_res[i].n_cigar;
    W->cells += W->h_cells[i];
  }
  GB_HIP(hipMemcpyAsync(W->d_offs, W->h_offs, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, W->stream));
  GB_HIP(hipEventRecord(W->ev[3], W->stream));
  const int64_t pack_blocks = std::min<int64_t>((n + 3) / 4, (int64_t)W->num_cus * 8);
  hipLaunchKernelGGL(extd2_pack_kernel, dim3((unsigned)pack_blocks), dim3(256), 0, W->stream, A);
  GB_HIP(hipGetLastError());
  GB_HIP(hipEventRecord(W->ev[4], W->stream));
  if (got) GB_HIP(hipMemcpyAsync(W->h_packed, W->d_packed, (size_t)got * sizeof(uint32_t), hipMemcpyDeviceToHost, W->stream));
  GB_HIP(hipStreamSynchronize(W->stream));
  float fill_ms = 0.f, walk_ms = 0.f, pack_ms = 0.f;
  GB_HIP(hipEventElapsedTime(&fill_ms, W->ev[0], W->ev[1]));
  GB_HIP(hipEventElapsedTime(&walk_ms, W->ev[1], W->ev[2]));
  GB_HIP(hipEventElapsedTime(&pack_ms, W->ev[3], W->ev[4]));
  W->fill_ms += fill_ms, W->walk_ms += walk_ms + pack_ms;
  if (got) std::memcpy(cigar + *used, W->h_packed.get(), (size_t)got * sizeof(uint32_t));
  *used += got;
  return GB_OK;
}

}  // namespace gbx2

extern "C" {

int gb_chain_extd2_timing(float *fill_ms, float *walk_ms, int64_t *cells) {
  GB_ARG(fill_ms && walk_ms && cells, "gb_chain_extd2_timing: null argument");
  const gbx2::Ws *W = nullptr;
  if (const int st = gb::ran_ws("gb_chain_extd2_timing", "gb_chain_extd2", &W, &gbx2::Ws::calls)) return st;
  *fill_ms = W->fill_ms, *walk_ms = W->walk_ms, *cells = W->cells;
  return GB_OK;
}

int gb_chain_extd2_plan(int64_t *chunks, int64_t *workspace_bytes) {
  GB_ARG(chunks && workspace_bytes, "gb_chain_extd2_plan: null argument");
  const gbx2::Ws *W = nullptr;
  if (const int st = gb::ran_ws("gb_chain_extd2_plan", "gb_chain_extd2", &W, &gbx2::Ws::calls)) return st;
  *chunks = W->chunks, *workspace_bytes = W->ws_bytes;
  return GB_OK;
}

int gb_chain_extd2(const gb_chain_extd2_params *p, const uint8_t *seqs, int64_t seq_bytes,
                   const gb_chain_extd2_item *items, int64_t n_items, gb_chain_extd2_result *res, uint32_t *cigar,
                   int64_t cigar_cap, int64_t *cigar_off, int64_t *cigar_used) {
  using namespace gbx2;
  const char *who = "gb_chain_extd2";
  gb::Range range_("gb.chain.extd2");
  try {
    GB_ARG(p && cigar_off && cigar_used && n_items >= 0 && seq_bytes >= 0 && (seq_bytes == 0 || seqs),
           "%s: null or negative argument", who);
    GB_ARG(n_items == 0 || (items && res), "%s: null items or results", who);
    GB_ARG(cigar_cap >= 0 && (cigar_cap == 0 || cigar), "%s: bad cigar arguments", who);
    const Par P = make_par(*p);
    int64_t need = 0;
    std::vector<int64_t> live;  // the items that reach the sweep
    for (int64_t i = 0; i < n_items; ++i) {
      const gb_chain_extd2_item &it = items[i];
      GB_ARG(!(it.flag & ~GB_EXTD2_FLAGS), "%s: item %lld has flag 0x%x (accepted bits: 0x%x)", who, (long long)i,
             (unsigned)it.flag, GB_EXTD2_FLAGS);
      GB_ARG(it.qlen >= 0 && it.tlen >= 0 && it.qlen <= GB_EXTD2_MAX_LEN && it.tlen <= GB_EXTD2_MAX_LEN,
             "%s: item %lld has lengths %d and %d (0 .. %d)", who, (long long)i, it.qlen, it.tlen, GB_EXTD2_MAX_LEN);
      GB_ARG(it.q_off >= 0 && it.t_off >= 0 && it.q_off <= seq_bytes - it.qlen && it.t_off <= seq_bytes - it.tlen,
             "%s: item %lld lies outside the %lld bytes of seqs", who, (long long)i, (long long)seq_bytes);
      need += (int64_t)it.qlen + it.tlen;
      if (!early_item(P, it)) live.push_back(i);
    }
    for (int64_t i = 0; i < n_items; ++i) {
      const gb_chain_extd2_item &it = items[i];
      for (int side = 0; side < 2; ++side) {
        const uint8_t *s = seqs + (side ? it.t_off : it.q_off);
        const int len = side ? it.tlen : it.qlen;
        for (int k = 0; k < len; ++k)
          GB_ARG(s[k] <= 4, "%s: item %lld has base code %d at %d of its %s", who, (long long)i, (int)s[k], k,
                 side ? "target" : "query");
      }
    }
    if (n_items == 0) {
      cigar_off[0] = 0, *cigar_used = 0;
      return GB_OK;
    }
    const bool host = gb::env_flag("GB_CHAIN_EXTD2_HOST");
    std::vector<Chunk> chunks;
    int st;
    if (!host && (st = make_chunks(who, items, live, &chunks))) return st;
    if (cigar_cap < need) {
      *cigar_used = need;
      gb::set_error("%s: cigar_cap is %lld, the items need %lld (qlen + tlen each)", who, (long long)cigar_cap,
                    (long long)need);
      return GB_ERR_ARG;
    }
    if (host) {
      int nth = 1;
      if ((st = gb::thread_count(who, "GB_CHAIN_THREADS", &nth))) return st;
      std::vector<uint32_t> words((size_t)need);
      std::vector<int64_t> begin((size_t)n_items);
      int64_t acc = 0;
      for (int64_t i = 0; i < n_items; ++i) begin[(size_t)i] = acc, acc += (int64_t)items[i].qlen + items[i].tlen;
      std::atomic<int64_t> next{0};
      if ((st = gb::parallel(who, (int)std::min<int64_t>(nth, n_items), [&](int) {
             HostScratch hs;
             for (int64_t i; (i = next.fetch_add(1)) < n_items;)
               host_item(P, seqs, items[i], &hs, &res[i], words.data() + begin[(size_t)i]);
           })))
        return st;
      int64_t used = 0;
      for (int64_t i = 0; i < n_items; ++i) {
        cigar_off[i] = used;
        if (res[i].n_cigar)
          std::memcpy(cigar + used, words.data() + begin[(size_t)i], (size_t)res[i].n_cigar * sizeof(uint32_t));
        used += res[i].n_cigar;
      }
      cigar_off[n_items] = *cigar_used = used;
      return GB_OK;
    }
    int64_t used = 0;
    if (!live.empty()) {
      int dev = 0;
      GB_HIP(hipGetDevice(&dev));
      Ws *W = nullptr;
      if ((st = gb::get_ws(who, dev, &W, make_sides))) return st;
      W->calls = 0, W->cells = 0, W->fill_ms = W->walk_ms = 0.f;
      const auto big = gb::largest(chunks);  // every buffer at the largest any chunk asks of it
      const int64_t big_n = big.count;
      if ((st = W->d_seqs.reserve((size_t)seq_bytes)) || (st = W->d_codes.reserve((size_t)big.need.codes)) ||
          (st = W->d_state.reserve((size_t)big.need.state)) || (st = W->d_items.reserve((size_t)big_n)) ||
          (st = W->h_items.reserve((size_t)big_n)) || (st = W->d_res.reserve((size_t)big_n)) ||
          (st = W->h_res.reserve((size_t)big_n)) || (st = W->d_cells.reserve((size_t)big_n)) ||
          (st = W->h_cells.reserve((size_t)big_n)) || (st = W->d_offs.reserve((size_t)big_n)) ||
          (st = W->h_offs.reserve((size_t)big_n)) || (st = W->d_walked.reserve((size_t)big.need.words)) ||
          (st = W->d_packed.reserve((size_t)big.need.words)) || (st = W->h_packed.reserve((size_t)big.need.words)))
        return st;
      GB_HIP(hipMemcpyAsync(W->d_seqs, seqs, (size_t)seq_bytes, hipMemcpyHostToDevice, W->stream));
      // an item that returns early keeps the offset of the next live one (it owns no words)
      for (int64_t i = 0; i < n_items; ++i) cigar_off[i] = -1;
      for (const Chunk &c : chunks)
        if ((st = run_chunk(W, P, c, items, live, res, cigar, cigar_off, &used))) return st;
      W->chunks = (int64_t)chunks.size(), W->ws_bytes = big.bytes;
      W->calls = 1;
    }
    cigar_off[n_items] = *cigar_used = used;
    for (int64_t i = n_items - 1; i >= 0; --i)
      if (early_item(P, items[i])) reset_result(&res[i]), cigar_off[i] = cigar_off[i + 1];
    return GB_OK;
  } catch (const std::bad_alloc &) {
    gb::set_error("%s: out of host memory", who);
    return GB_ERR_NOMEM;
  }
}

}  // extern "C"
