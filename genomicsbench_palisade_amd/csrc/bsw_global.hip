// bsw_global.hip -- MI355X (gfx950) banded global alignment with CIGAR traceback: kernels and C ABI.
//
// Semantics: bwa's ksw_global2 (tools/bwa/ksw.c:504-606), the step bwa_gen_cigar2 (tools/bwa/bwa.c:
// 121-208) runs on a region the banded extension chose; NM as bwa.c:169-200 counts it. Integer
// arithmetic throughout, so results are bit-exact by construction.
//
// Two kernels per chunk of pairs:
//   fill: one pair per wave64 (persistent grid, pairs pulled from an atomic counter), lanes across
//     the query, lane l owning the K = ceil((qlen+1)/64) consecutive columns j = l*K .. l*K+K-1 of
//     the reference's eh[0..qlen] in registers, exactly the shape of extend<K> in bsw.hip. Within a
//     row only F is sequential, F(i,j) = max_{beg<=k<j} (M_k - oe_ins - e_ins (j-1-k)), one max-plus
//     prefix scan (in-lane over K, then DPP across lanes); direction and extension bits are then
//     local comparisons per column. Each lane packs its K cells' 4-bit records (bits 0-1: H's
//     source, bit 2: E extends, bit 3: F extends) into one 16-bit word; row i of the pair's
//     direction matrix is the nl = ceil(qlen/K) words of the lanes that own a query column, stored
//     by the lanes whose columns meet the band.
//   walk: one pair per lane. Every step reads one word of the direction matrix; 64 independent walks
//     per wave and many waves hide the load latency. The walk runs twice: the first pass counts runs
//     and NM, then one atomic add reserves the pair's slice of the chunk's operation pool, and the
//     second pass writes the merged runs there in forward order. The kernel boundary orders the
//     fill's vector stores before the walk's vector loads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/gb_bsw.h"
#include "bsw_global_internal.h"
#include "gb_common.h"
#include "gb_common_wave.h"

static_assert(sizeof(gb_bsw_gpair) == 48, "gb_bsw_gpair is 48 bytes (include/gb_bsw.h)");

namespace gbbswg {

constexpr int kNegInf = -0x40000000;  // MINUS_INF (ksw.c:490)
constexpr int kWavesPerBlock = 4;
constexpr int kBlocksPerCU = 8;
constexpr int kMaxPenalty = 32768;  // gap penalties lie in [0, kMaxPenalty)

struct FillArgs {
  const Pair *pairs;
  int64_t n;
  const uint8_t *tgt, *qry;
  int32_t *out4;  // per pair: score, n_cigar, nm, pool offset
  uint16_t *dir;  // null: scores only
  unsigned int *next;
  int o_del, e_del, o_ins, e_ins;
  int8_t mat[28];
};

struct WalkArgs {
  const Pair *pairs;
  int64_t n;
  const uint8_t *tgt, *qry;
  int32_t *out4;
  const uint16_t *dir;
  uint32_t *pool;
  unsigned int *pool_used;  // operations reserved so far
  unsigned int *bad;        // lowest pair index whose walk hit the step clamp
};

template <int K, bool DIR>
__device__ __forceinline__ void fill(const FillArgs &A, const Pair &P, const int8_t *smat, int lane, int32_t *o4) {
  const int qlen = P.qlen, tlen = P.tlen, w = P.w;
  const int o_del = A.o_del, e_del = A.e_del, o_ins = A.o_ins, e_ins = A.e_ins;
  const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
  const uint8_t *qry = A.qry + P.q_off;
  const uint8_t *tgt = A.tgt + P.t_off;
  const int nl = (qlen + K - 1) / K;

  // Borders (ksw.c:522-525,532,585). Minus infinity is -2^30 as in the reference, but only its
  // order matters here, not the reference's exact out-of-band values. Inside the accepted domain
  // (w >= |tlen - qlen|, tlen <= 2047, qlen <= 255, penalties < 32768, |score| <= 128) the band
  // moves right by at most one column per row, so every in-band cell's diagonal predecessor is an
  // in-band cell of the row above or a finite border, and m = H(i-1,j-1) + S is always a real value,
  // of magnitude below 32768 * 2304 + 255 * 128 < 2^27. E is minus infinity at the band's upper-right
  // edge (eh[end].e) and F at its left edge; each then only loses penalties, at most 2047 * 32767 <
  // 2^26 for E down a column and 255 * 32767 < 2^23 for F along a row, so such an e or f stays
  // between -2^31 and every real value: it neither wins nor ties h, nor sets an extension bit (both
  // tests are against m minus a penalty). The traceback therefore never leaves the band, and no
  // int32 sum overflows.
  int H[K], E[K], plo[K], phi[K], ej[K];
#pragma unroll
  for (int c = 0; c < K; ++c) {
    const int j = lane * K + c;
    int qb = 4;
    if (j < qlen) qb = min((int)qry[j], 4);
    plo[c] = (smat[qb] & 0xFF) | (smat[5 + qb] & 0xFF) << 8 | (smat[10 + qb] & 0xFF) << 16 |
             (smat[15 + qb] & 0xFF) << 24;
    phi[c] = smat[20 + qb];
    H[c] = j == 0 ? 0 : (j <= qlen && j <= w ? -(o_ins + e_ins * j) : kNegInf);
    E[c] = kNegInf;
    ej[c] = e_ins * j;
  }
  uint16_t *drow = nullptr;
  if (DIR) drow = A.dir + P.dir_off + lane;

  int tword = 0;
  for (int i = 0; i < tlen; ++i) {
    const int ir = i & 255;
    if (ir == 0) {  // 256 target bases per VGPR: lane l holds bases i+4l .. i+4l+3
      tword = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int t = i + 4 * lane + b;
        if (t < tlen) tword |= (int)tgt[t] << (8 * b);
      }
    }
    const int tb = min((__builtin_amdgcn_readlane(tword, ir >> 2) >> (8 * (ir & 3))) & 0xFF, 4);
    const int sh = 8 * (tb & 3);
    const bool hi = tb >= 4;
    const int beg = max(i - w, 0), end = min(i + w + 1, qlen);  // ksw.c:530-531
    const int h1init = beg == 0 ? -(o_del + e_del * (i + 1)) : kNegInf;

    // F of the whole row: f(beg) is minus infinity (the scan's identity, kept below every real
    // value by the bounds above), f(j) for j > beg the exact maximum over its real terms
    int M[K], lpx[K];
    int lp = kNegInf;
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const int j = lane * K + c;
      const bool inb = j >= beg && j < end;
      const int s = __builtin_amdgcn_sbfe(hi ? phi[c] : plo[c], sh, 8);
      M[c] = H[c] + s;  // M = H(i-1,j-1) + S
      lpx[c] = lp;
      lp = max(lp, inb ? M[c] - oe_ins + ej[c] : kNegInf);
    }
    const int lex = gb::wave_shr1(gb::scan_max<kNegInf>(lp), kNegInf);
    int h[K], En[K];
    uint32_t word = 0;
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const int m = M[c], e = E[c];
      const int f = max(lex, lpx[c]) - ej[c] + e_ins;  // F(i,j)
      // ksw.c:551-564: M wins ties over E, both over F; the extension tests are strict
      uint32_t d = m >= e ? 0u : 1u;
      int hh = m >= e ? m : e;
      d = hh >= f ? d : 2u;
      hh = hh >= f ? hh : f;
      h[c] = hh;
      const int te = m - oe_del, e2 = e - e_del;
      d |= e2 > te ? 4u : 0u;
      En[c] = e2 > te ? e2 : te;  // E(i+1,j)
      d |= f - e_ins > m - oe_ins ? 8u : 0u;
      word |= d << (4 * c);
    }
    if (DIR) {
      // lanes whose columns meet the band; cells outside it are never read back
      if (lane < nl && lane * K < end && lane * K + K > beg) drow[(int64_t)i * nl] = (uint16_t)word;
    }
    // eh[j].h <- H(i,j-1) for j in (beg, end], eh[beg].h <- first column, eh[j].e <- E(i+1,j),
    // eh[end].e <- minus infinity (ksw.c:549,560,585)
    const int hprev = gb::wave_shr1(h[K - 1], 0);
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const int j = lane * K + c;
      const int hs = c ? h[c - 1] : hprev;
      if (j >= beg && j <= end) {
        H[c] = j == beg ? h1init : hs;
        E[c] = j == end ? kNegInf : En[c];
      }
    }
  }
  // score = eh[qlen].h (ksw.c:587)
  const int ce = qlen % K;
  int hsel = H[0];
#pragma unroll
  for (int c = 1; c < K; ++c)
    if (ce == c) hsel = H[c];
  // stored by the lane that owns column qlen (never lane 0: a store under `lane == 0` here was merged
  // with the work counter's `lane == 0` branch of the next iteration, see the kernel's loop)
  if (lane == qlen / K) {
    o4[0] = hsel;
    o4[1] = 0;
    o4[2] = -1;
    o4[3] = 0;
  }
}

template <bool DIR>
__global__ __launch_bounds__(64 * kWavesPerBlock) void bsw_global_fill_kernel(FillArgs A) {
  __shared__ int8_t smat[32];
  if (threadIdx.x < 25) smat[threadIdx.x] = A.mat[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (;;) {
    unsigned int p = 0;
    if (lane == 0) p = atomicAdd(A.next, 1u);
    p = __builtin_amdgcn_readfirstlane(p);
    if ((int64_t)p >= A.n) break;
    const Pair P = A.pairs[p];
    int32_t *o4 = A.out4 + 4 * (int64_t)p;
    const int K = cols_per_lane(P.qlen);
    if (K <= 1)
      fill<1, DIR>(A, P, smat, lane, o4);
    else if (K == 2)
      fill<2, DIR>(A, P, smat, lane, o4);
    else if (K == 3)
      fill<3, DIR>(A, P, smat, lane, o4);
    else
      fill<4, DIR>(A, P, smat, lane, o4);
    // The whole wave meets here before any lane fetches the next pair. Without a convergent
    // operation between a pair's last divergent branch and the loop's head, the compiler threaded
    // lane 0's path straight into the next atomicAdd and sent the other lanes round the loop alone,
    // where readfirstlane handed them pair 0 for ever.
    __builtin_amdgcn_wave_barrier();
  }
}

// The traceback of ksw.c:588-602 with push_cigar's run merging and bwa.c:169-200's NM count. Runs
// are closed in walk order, that is from the alignment's last operation to its first; run r of n
// goes to dst[n - 1 - r]. Every step lowers i, k or both, and the loop also stops after tlen + qlen
// steps, so a wrong direction record can give a wrong CIGAR but no endless walk, and i and k stay
// inside the pair's own direction matrix and sequences. Returns the number of runs.
template <bool WRITE>
__device__ __forceinline__ int walk(const Pair &P, const uint16_t *dir, const uint8_t *tgt, const uint8_t *qry,
                                    uint32_t *dst, int n_total, int &nm, bool &clamped) {
  const int K = cols_per_lane(P.qlen), nl = row_words(P.qlen);
  const int limit = P.tlen + P.qlen;
  int i = P.tlen - 1, k = min(P.tlen + P.w, P.qlen) - 1;
  int state = 0, steps = 0;
  int op_cur = -1, len_cur = 0, r = 0, mm = 0, gaps = 0, last_d = 0;
  auto close = [&]() {
    if (len_cur == 0) return;
    if (WRITE && r < n_total) dst[n_total - 1 - r] = (uint32_t)len_cur << 4 | (uint32_t)op_cur;
    // a D run counts unless it is the alignment's last operation (r == 0) or its first (undone below)
    last_d = 0;
    if (op_cur == 1) gaps += len_cur;
    if (op_cur == 2 && r > 0) gaps += len_cur, last_d = len_cur;
    ++r;
  };
  auto push = [&](int op, int len) {
    if (op != op_cur) {
      close();
      op_cur = op;
      len_cur = 0;
    }
    len_cur += len;
  };
  clamped = false;
  while (i >= 0 && k >= 0) {
    if (steps++ >= limit) {
      clamped = true;
      break;
    }
    const int lane = k / K, c = k - lane * K;
    const uint32_t rec = ((uint32_t)dir[(int64_t)i * nl + lane] >> (4 * c)) & 15u;
    // next state = the current cell's field selected by the current state (ksw.c:593)
    state = state == 0 ? min((int)(rec & 3u), 2) : state == 1 ? (int)((rec >> 2) & 1u) : (int)((rec >> 3) & 1u) * 2;
    if (state == 0) {
      mm += qry[k] != tgt[i] ? 1 : 0;
      push(0, 1), --i, --k;
    } else if (state == 1) {
      push(2, 1), --i;
    } else {
      push(1, 1), --k;
    }
  }
  if (i >= 0) push(2, i + 1);
  if (k >= 0) push(1, k + 1);
  close();
  nm = mm + gaps - last_d;
  return r;
}

__global__ __launch_bounds__(64) void bsw_global_walk_kernel(WalkArgs A) {
  const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (p >= A.n) return;
  const Pair P = A.pairs[p];
  const uint16_t *dir = A.dir + P.dir_off;
  const uint8_t *tgt = A.tgt + P.t_off, *qry = A.qry + P.q_off;
  int nm = 0, nm2 = 0;
  bool clamped = false, clamped2 = false;
  const int n = walk<false>(P, dir, tgt, qry, nullptr, 0, nm, clamped);
  // n <= tlen + qlen, and the pool holds the chunk's sum of tlen + qlen
  const unsigned int base = atomicAdd(A.pool_used, (unsigned int)n);
  walk<true>(P, dir, tgt, qry, A.pool + base, n, nm2, clamped2);
  if (clamped) atomicMin(A.bad, (unsigned int)p);
  int32_t *o4 = A.out4 + 4 * p;
  o4[1] = n;
  o4[2] = nm;
  o4[3] = (int32_t)base;
}

// Chunk bounds: a chunk's direction matrices take at most kDirWords 16-bit words (1 GiB) and its
// operation pool, sized for the worst case sum of tlen + qlen, at most kPoolOps entries (256 MiB).
// One pair needs at most 64 * 2047 words and 2302 operations, so a chunk always holds a pair.
constexpr int64_t kDirWords = int64_t(1) << 29;
constexpr int64_t kPoolOps = int64_t(1) << 26;
constexpr int64_t kChunkPairs = int64_t(1) << 22;

int64_t dir_words_limit() {  // GB_BSW_GLOBAL_DIR_WORDS (tests: many chunks from a small set), read per call
  const char *e = getenv("GB_BSW_GLOBAL_DIR_WORDS");
  return e ? std::max<int64_t>(1, std::min<int64_t>(atoll(e), kDirWords)) : kDirWords;
}

int get_ws(int dev, Ws **out) {
  return gb::get_ws("gb_bsw_global", dev, out, [](Ws *W) { return W->d_ctl.reserve(4); });
}

// Every refusal of include/gb_bsw.h, before any device work.
int validate(const gb_bsw_params *params, const gb_bsw_gpair *pairs, int64_t n, const uint8_t *ref, int64_t ref_bytes,
             const uint8_t *qer, int64_t qer_bytes, const uint32_t *cigar, int64_t cigar_cap) {
  GB_ARG(params && n >= 0 && (n == 0 || pairs), "gb_bsw_global: bad arguments");
  GB_ARG(ref_bytes >= 0 && qer_bytes >= 0 && (ref_bytes == 0 || ref) && (qer_bytes == 0 || qer),
         "gb_bsw_global: bad sequence buffers");
  GB_ARG(!cigar || cigar_cap >= 0, "gb_bsw_global: negative cigar_cap");
  const int pen[4] = {params->o_del, params->e_del, params->o_ins, params->e_ins};
  for (int v : pen)
    GB_ARG(v >= 0 && v < kMaxPenalty, "gb_bsw_global: gap penalties (o_del %d, e_del %d, o_ins %d, e_ins %d) must lie in [0, %d)",
           pen[0], pen[1], pen[2], pen[3], kMaxPenalty);
  for (int64_t p = 0; p < n; ++p) {
    const gb_bsw_gpair &s = pairs[p];
    GB_ARG(s.len2 >= 1 && s.len2 <= GB_BSW_MAX_QLEN && s.len1 >= 1 && s.len1 <= GB_BSW_GLOBAL_MAX_TLEN,
           "gb_bsw_global: pair %lld has len1=%d len2=%d (need len1 in [1,%d], len2 in [1,%d])", (long long)p, s.len1,
           s.len2, GB_BSW_GLOBAL_MAX_TLEN, GB_BSW_MAX_QLEN);
    GB_ARG(s.w >= std::abs(s.len1 - s.len2), "gb_bsw_global: pair %lld has w=%d below |len1 - len2| = %d", (long long)p,
           s.w, std::abs(s.len1 - s.len2));
    GB_ARG(s.idr >= 0 && s.idr <= ref_bytes - s.len1 && s.idq >= 0 && s.idq <= qer_bytes - s.len2,
           "gb_bsw_global: pair %lld lies outside the sequence buffers", (long long)p);
  }
  return GB_OK;
}

}  // namespace gbbswg

extern "C" {

int gb_bsw_global_band(const gb_bsw_params *params, int32_t len2, int32_t len1, int32_t w_cap) {
  GB_ARG(params && params->e_ins > 0 && params->e_del > 0, "gb_bsw_global_band: gap extension must be > 0");
  // bwa.c:153-160, in the reference's double arithmetic
  const int a = params->mat[0];
  const int max_ins = (int)((double)(((len2 + 1) >> 1) * a - params->o_ins) / params->e_ins + 1.);
  const int max_del = (int)((double)(((len2 + 1) >> 1) * a - params->o_del) / params->e_del + 1.);
  int max_gap = max_ins > max_del ? max_ins : max_del;
  max_gap = max_gap > 1 ? max_gap : 1;
  int w = (max_gap + std::abs(len1 - len2) + 1) >> 1;
  w = w < w_cap ? w : w_cap;
  const int min_w = std::abs(len1 - len2) + 3;
  return w > min_w ? w : min_w;
}

int gb_bsw_global_timing(float *fill_ms, float *walk_ms) {
  GB_ARG(fill_ms && walk_ms, "gb_bsw_global_timing: null argument");
  const gbbswg::Ws *W = nullptr;
  if (const int st = gb::ran_ws("gb_bsw_global_timing", "gb_bsw_global", &W)) return st;
  *fill_ms = W->fill_ms;
  *walk_ms = W->walk_ms;
  return GB_OK;
}

int gb_bsw_global(const gb_bsw_params *params, gb_bsw_gpair *pairs, int64_t n, const uint8_t *ref, int64_t ref_bytes,
                  const uint8_t *qer, int64_t qer_bytes, uint32_t *cigar, int64_t cigar_cap, int64_t *cigar_used) {
  using namespace gbbswg;
  gb::Range range_("gb.bsw.global");
  int st = validate(params, pairs, n, ref, ref_bytes, qer, qer_bytes, cigar, cigar_cap);
  if (st) return st;
  if (cigar_used) *cigar_used = 0;
  if (n == 0) return GB_OK;

  int dev = 0;
  GB_HIP(hipGetDevice(&dev));
  Ws *W = nullptr;
  if ((st = get_ws(dev, &W))) return st;
  W->fill_ms = W->walk_ms = 0.f;
  if ((st = W->d_tgt.reserve((size_t)ref_bytes))) return st;
  if ((st = W->d_qry.reserve((size_t)qer_bytes))) return st;
  GB_HIP(hipMemcpyAsync(W->d_tgt, ref, (size_t)ref_bytes, hipMemcpyHostToDevice, W->stream));
  GB_HIP(hipMemcpyAsync(W->d_qry, qer, (size_t)qer_bytes, hipMemcpyHostToDevice, W->stream));
  return run_resident(W, "gb_bsw_global", params, pairs, n, W->d_tgt, W->d_qry, cigar, cigar_cap, cigar_used,
                      &W->fill_ms, &W->walk_ms, nullptr);
}

}  // extern "C"

namespace gbbswg {

int run_resident(Ws *W, const char *who, const gb_bsw_params *params, gb_bsw_gpair *pairs, int64_t n,
                 const uint8_t *d_tgt, const uint8_t *d_qry, uint32_t *cigar, int64_t cigar_cap, int64_t *cigar_used,
                 float *fill_ms, float *walk_ms, ChunkHook *hook) {
  int st = GB_OK;
  if (cigar_used) *cigar_used = 0;
  const bool want = cigar != nullptr;
  // Operations go straight into cigar[] when it holds the worst case; otherwise they are staged so
  // that cigar[] stays untouched should the total exceed cigar_cap.
  int64_t worst = 0;
  for (int64_t p = 0; p < n; ++p) worst += pairs[p].len1 + pairs[p].len2;
  const bool direct = want && cigar_cap >= worst;
  std::vector<uint32_t> staged;
  std::vector<Pair> P;
  std::vector<int32_t> o4;
  std::vector<uint32_t> pool;
  int64_t total = 0, bad_pair = -1;
  const int64_t dir_limit = dir_words_limit();

  for (int64_t lo = 0; lo < n;) {
    // plan one chunk [lo, hi)
    int64_t hi = lo, words = 0, ops = 0;
    P.clear();
    while (hi < n && hi - lo < kChunkPairs) {
      const gb_bsw_gpair &s = pairs[hi];
      const int64_t wd = want ? (int64_t)row_words(s.len2) * s.len1 : 0, op = (int64_t)s.len1 + s.len2;
      if (hi > lo && (words + wd > dir_limit || ops + op > kPoolOps)) break;
      P.push_back(Pair{s.idr, s.idq, words, s.len1, s.len2, s.w, 0});
      words += wd;
      ops += op;
      ++hi;
    }
    const int64_t m = hi - lo;
    if ((st = W->d_pairs.reserve((size_t)m))) return st;
    if ((st = W->d_out4.reserve((size_t)m * 4))) return st;
    if (want) {
      if ((st = W->d_dir.reserve((size_t)words))) return st;
      if ((st = W->d_pool.reserve((size_t)ops))) return st;
    }
    const unsigned int ctl0[4] = {0u, 0u, 0xFFFFFFFFu, 0u};
    GB_HIP(hipMemcpyAsync(W->d_ctl, ctl0, sizeof(ctl0), hipMemcpyHostToDevice, W->stream));
    GB_HIP(hipMemcpyAsync(W->d_pairs, P.data(), (size_t)m * sizeof(Pair), hipMemcpyHostToDevice, W->stream));
    FillArgs F;
    F.pairs = W->d_pairs;
    F.n = m;
    F.tgt = d_tgt;
    F.qry = d_qry;
    F.out4 = W->d_out4;
    F.dir = want ? W->d_dir.get() : nullptr;
    F.next = W->d_ctl;
    F.o_del = params->o_del;
    F.e_del = params->e_del;
    F.o_ins = params->o_ins;
    F.e_ins = params->e_ins;
    std::memset(F.mat, 0, sizeof(F.mat));
    std::memcpy(F.mat, params->mat, 25);
    const int64_t blocks = std::max<int64_t>(
        1, std::min<int64_t>((int64_t)W->num_cus * kBlocksPerCU, (m + kWavesPerBlock - 1) / kWavesPerBlock));
    GB_HIP(hipEventRecord(W->ev[0], W->stream));
    if (want)
      hipLaunchKernelGGL(bsw_global_fill_kernel<true>, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0, W->stream, F);
    else
      hipLaunchKernelGGL(bsw_global_fill_kernel<false>, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0, W->stream, F);
    GB_HIP(hipGetLastError());
    GB_HIP(hipEventRecord(W->ev[1], W->stream));
    if (want) {
      WalkArgs A;
      A.pairs = W->d_pairs;
      A.n = m;
      A.tgt = d_tgt;
      A.qry = d_qry;
      A.out4 = W->d_out4;
      A.dir = W->d_dir;
      A.pool = W->d_pool;
      A.pool_used = W->d_ctl + 1;
      A.bad = W->d_ctl + 2;
      hipLaunchKernelGGL(bsw_global_walk_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, W->stream, A);
      GB_HIP(hipGetLastError());
    }
    GB_HIP(hipEventRecord(W->ev[2], W->stream));
    if (want && hook && (st = hook->enqueue(W->stream, lo, m, W->d_pairs, W->d_out4, W->d_pool))) return st;
    o4.resize((size_t)m * 4);
    unsigned int ctl[4] = {0, 0, 0, 0};
    GB_HIP(hipMemcpyAsync(o4.data(), W->d_out4, (size_t)m * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, W->stream));
    GB_HIP(hipMemcpyAsync(ctl, W->d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, W->stream));
    GB_HIP(hipStreamSynchronize(W->stream));
    float ms = 0.f;
    GB_HIP(hipEventElapsedTime(&ms, W->ev[0], W->ev[1]));
    *fill_ms += ms;
    GB_HIP(hipEventElapsedTime(&ms, W->ev[1], W->ev[2]));
    *walk_ms += ms;
    const int64_t used = want ? (int64_t)ctl[1] : 0;
    if (used > ops) {
      gb::set_error("%s: the device reserved %lld operations for a chunk that can need at most %lld",
                    who, (long long)used, (long long)ops);
      return GB_ERR_STATE;
    }
    if (want && ctl[2] != 0xFFFFFFFFu && bad_pair < 0) bad_pair = lo + (int64_t)ctl[2];
    if (used) {
      pool.resize((size_t)used);
      GB_HIP(hipMemcpy(pool.data(), W->d_pool, (size_t)used * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (want && !direct) staged.resize((size_t)(total + used));
    uint32_t *dst = direct ? cigar : staged.data();
    for (int64_t k = 0; k < m; ++k) {
      gb_bsw_gpair &s = pairs[lo + k];
      const int32_t *o = o4.data() + 4 * k;
      s.score = o[0];
      s.n_cigar = want ? o[1] : 0;
      s.nm = want ? o[2] : -1;
      s.cigar_off = want ? total : 0;
      if (want) {
        const int64_t nc = o[1], off = (int64_t)(uint32_t)o[3];
        if (nc < 0 || off + nc > used) {
          gb::set_error("%s: pair %lld reports %lld operations at pool offset %lld of %lld",
                        who, (long long)(lo + k), (long long)nc, (long long)off, (long long)used);
          return GB_ERR_STATE;
        }
        std::memcpy(dst + total, pool.data() + off, (size_t)nc * sizeof(uint32_t));
        total += nc;
      }
    }
    if (want && hook && (st = hook->collect(lo, m))) return st;
    lo = hi;
  }
  if (cigar_used) *cigar_used = total;
  if (bad_pair >= 0) {
    gb::set_error("%s: the traceback of pair %lld did not end within len1 + len2 steps", who, (long long)bad_pair);
    return GB_ERR_STATE;
  }
  if (want && !direct) {
    GB_ARG(total <= cigar_cap, "%s: cigar_cap %lld is below the %lld operations of this call", who,
           (long long)cigar_cap, (long long)total);
    if (total) std::memcpy(cigar, staged.data(), (size_t)total * sizeof(uint32_t));
  }
  return GB_OK;
}

}  // namespace gbbswg
