// bsw_local.hip -- MI355X (gfx950) unbanded local alignment with sub-optimal score and start
// positions: kernel and C ABI.
//
// Semantics: bwa's ksw_align2 (tools/bwa/ksw.c:63-365: ksw_qinit, ksw_u8, ksw_i16, ksw_align2), the
// call mem_matesw makes for mate rescue (tools/bwa/bwamem_pair.c:150-151). The reference is a striped
// SSE kernel with a lazy-F loop; what it computes is the ordinary affine-gap local DP
//   m = H(i-1,j-1) + S(t[i],j)      H(i,j) = max(m, E(i,j), F(i,j), 0)
//   F(i,j+1) = max(H(i,j) - oe_ins, F(i,j) - e_ins, 0)
//   E(i+1,j) = max(H(i,j) - oe_del, E(i,j) - e_del, 0)
// with five properties of its own that this kernel reproduces:
//   1. the query is padded to L = a multiple of p columns (p = 16 with KSW_XBYTE, else 8); the pad
//      columns score 0 against every base (ksw.c:96,105) and take part in the row maximum;
//   2. one pass over the rows, H and E zero before row 0, imax = the row's maximum over all L columns;
//   3. per row (ksw.c:192-206): with imax >= minsc a list of (imax, row) entries grows, merging a run
//      of adjacent rows into its best; with imax > gmax the row becomes the kept row, and the pass
//      stops once gmax >= endsc;
//   4. after the pass qe = the smallest column holding the kept row's maximum, and score2 / te2 = the
//      first best list entry more than ceil(score / max(mat)) rows away from te.
//   5. with o_ins == 0 the lazy-F loop (ksw.c:177-188,285-295) ends after its first step, because an
//      H that was just raised to F always "dominates" that F when opening a gap costs nothing. F then
//      runs only inside each of the reference's p stripes of slen = L/p consecutive columns; the F
//      that leaves a stripe reaches the first column of the next one and goes no further, and that
//      column's E still comes from its H before the F arrived. With o_ins > 0 the loop is exact, and
//      so is taking E from the final H.
// The start positions come from a second pass of the same function over the reversed prefixes
// (ksw.c:356-364): query[qe..0], target[te - i] for rows i <= te and target[i] beyond (the reference
// reverses only the prefix and still passes the full length), stopping at the first pass's score.
// Integer arithmetic throughout, 32-bit here: inside the accepted domain (include/gb_bsw.h) neither
// of the reference's saturating 8- or 16-bit lanes saturates, so the two "precisions" differ only
// in p.
//
// One pair per wave64 on a persistent grid, pairs pulled from an atomic counter. Lanes lie across
// the L <= 256 padded columns, lane l owning the K = ceil(L/64) <= 4 consecutive columns l*K ..
// l*K+K-1 with H, E and the kept row in registers. Within a row only F is sequential:
// F(i,j) = max(0, max_{k<j} (A_k - oe_ins - e_ins (j-1-k))) with A = max(m, E, 0) (a cell whose H is
// its F never opens a better gap than that F extended), one max-plus prefix scan, in-lane over K and
// then DPP across lanes, as in bsw_global.hip. The row maximum needs a wave reduction only on the
// rows where some lane's maximum reaches minsc or beats gmax, which a ballot decides first. The entry
// list lives in a per-wave slice of a scratch buffer, one packed word (score << 14 | row) per entry.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/gb_bsw.h"
#include "bsw_local_internal.h"
#include "gb_common.h"
#include "gb_common_wave.h"

static_assert(sizeof(gb_bsw_lpair) == 56, "gb_bsw_lpair is 56 bytes (include/gb_bsw.h)");
static_assert(GB_BSW_LOCAL_MAX_TLEN < (1 << 14), "a list entry keeps its row in 14 bits");
static_assert(GB_BSW_MAX_QLEN * 127 < (1 << 15), "a list entry keeps its score in 15 bits");

namespace gbbswl {

constexpr int kNegInf = -0x40000000;  // identity of the max scans; every real term stays far above it
constexpr int kWavesPerBlock = 4;
constexpr int kBlocksPerCU = 8;
constexpr int kMaxPenalty = 32768;    // o + e < kMaxPenalty
constexpr int kNoThreshold = 0x10000; // minsc / endsc without their flag (ksw.c:128-129)
constexpr int kRowBits = 14;
constexpr uint32_t kRowMask = (1u << kRowBits) - 1u;
constexpr int kStripeBias = 1 << 24;  // above the spread of F's scan terms (< 2^15 + 2^23 + 2^15), times p <= 16 below 2^30
constexpr int kFlags = GB_KSW_XBYTE | GB_KSW_XSTOP | GB_KSW_XSUBO | GB_KSW_XSTART;

struct Args {
  const Pair *pairs;
  int64_t n;
  const uint8_t *tgt, *qry;
  int32_t *out8;     // per pair: score, te, qe, score2, te2, tb, qb, 0
  uint32_t *list;    // list_cap entries per wave of the grid
  int64_t list_cap;
  unsigned int *next;
  int oe_del, e_del, oe_ins, e_ins, max_mat;
  int8_t mat[28];
};

struct Res {
  int gmax, te, qe, score2, te2;
};

// One pass of ksw_u8 / ksw_i16 over tlen rows and L = a multiple of p columns, of which the first
// qlen carry the query. Forward: column j is qry[j], row i is tgt[i] (te0 = -1). Reverse (the start
// pass): column j is qry[qlen-1-j], row i is tgt[te0-i] up to te0 and tgt[i] beyond. Every argument
// but lane is wave-uniform. list has room for list_cap entries; it is only touched with minsc <
// kNoThreshold. ZO is o_ins == 0, property 5 above: the scan's terms carry kStripeBias times their
// stripe's number, so that in a column's exclusive maximum the terms of its own stripe beat all
// others, and where there are none (the stripe's first column) the previous stripe's do.
template <int K, bool ZO>
__device__ __forceinline__ void pass(const Args &A, const int8_t *smat, const uint8_t *tgt, const uint8_t *qry,
                                     int tlen, int qlen, int L, int pw, int te0, bool rev, int minsc, int endsc,
                                     uint32_t *list, int list_cap, int lane, Res &R) {
  const int oe_del = A.oe_del, e_del = A.e_del, oe_ins = A.oe_ins, e_ins = A.e_ins;
  int H[K], E[K], Hk[K], plo[K], phi[K], ej[K], live[K], first[K];
  const int slen = L / pw;
#pragma unroll
  for (int c = 0; c < K; ++c) {
    const int j = lane * K + c;
    plo[c] = phi[c] = 0;  // the pad columns qlen .. L-1 score 0 against every base
    if (j < qlen) {
      const int qb = min((int)qry[rev ? qlen - 1 - j : j], 4);
      plo[c] = (smat[qb] & 0xFF) | (smat[5 + qb] & 0xFF) << 8 | (smat[10 + qb] & 0xFF) << 16 |
               (smat[15 + qb] & 0xFF) << 24;
      phi[c] = smat[20 + qb];
    }
    live[c] = j < L ? -1 : 0;  // columns L .. 64K-1 do not exist: their H is held at 0
    H[c] = E[c] = Hk[c] = 0;
    ej[c] = e_ins * j;
    first[c] = 0;
    if (ZO) {
      ej[c] += min(j / slen, pw - 1) * kStripeBias;
      first[c] = j > 0 && j < L && j % slen == 0 ? kStripeBias : 0;
    }
  }
  int gmax = 0, te = -1, n_b = 0, last_s = 0, last_r = -2;

  int tword = 0;
  for (int i = 0; i < tlen; ++i) {
    const int ir = i & 255;
    if (ir == 0) {  // 256 target bases per VGPR: lane l holds the bases of rows i+4l .. i+4l+3
      tword = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int r = i + 4 * lane + b;
        if (r < tlen) tword |= (int)tgt[r <= te0 ? te0 - r : r] << (8 * b);
      }
    }
    const int tb = min((__builtin_amdgcn_readlane(tword, ir >> 2) >> (8 * (ir & 3))) & 0xFF, 4);
    const int sh = 8 * (tb & 3);
    const bool hi = tb >= 4;

    // A = max(m, E, 0) per column, and the terms of F's scan: F(i,j) = max(0, max_{k<j} (A_k - oe_ins
    // + e_ins k) - e_ins (j-1)). All terms are at least -32768 and at most 2^15 + 2^23.
    const int hleft = gb::wave_shr1(H[K - 1], 0);  // H(i-1, lane*K - 1); H(i-1,-1) = 0 (ksw.c:149)
    int a[K], lpx[K];
    int lp = kNegInf;
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const int s = __builtin_amdgcn_sbfe(hi ? phi[c] : plo[c], sh, 8);
      const int m = (c ? H[c - 1] : hleft) + s;
      a[c] = max(max(m, E[c]), 0);
      lpx[c] = lp;
      lp = max(lp, a[c] - oe_ins + ej[c]);
    }
    const int lex = gb::wave_shr1(gb::scan_max<kNegInf>(lp), kNegInf);
    int hmax = 0;
#pragma unroll
    for (int c = 0; c < K; ++c) {
      // F(i,j) before its clamp at 0 (a >= 0 clamps H). ZO: at a stripe's first column, the F that
      // left the previous stripe
      const int f = max(lex, lpx[c]) - ej[c] + e_ins + (ZO ? first[c] : 0);
      const int h = max(a[c], f) & live[c];
      const int he = ZO && first[c] ? a[c] : h;
      E[c] = max(max(he - oe_del, E[c] - e_del), 0);  // E(i+1,j)
      H[c] = h;
      hmax = max(hmax, h);
    }

    // ksw.c:191-206. Only a row whose maximum reaches minsc or beats gmax does anything, and some
    // lane's own maximum then passes the same test.
    const int thr = min(minsc, gmax + 1);
    if (__builtin_amdgcn_ballot_w64(hmax >= thr) != 0) {
      const int imax = gb::wave_max<kNegInf>(hmax);
      if (imax >= minsc) {
        bool changed = false;
        if (n_b == 0 || last_r + 1 != i) {
          ++n_b;
          changed = true;
        } else if (last_s < imax) {
          changed = true;
        }
        if (changed) {
          last_s = imax;
          last_r = i;
          if (lane == 63 && n_b <= list_cap) list[n_b - 1] = (uint32_t)imax << kRowBits | (uint32_t)i;
        }
      }
      if (imax > gmax) {
        gmax = imax;
        te = i;
#pragma unroll
        for (int c = 0; c < K; ++c) Hk[c] = H[c];
        if (gmax >= endsc) break;
      }
    }
  }

  // qe: the smallest column holding the kept row's maximum (ksw.c:214-216,319-321); the kept row is
  // all zero when no row scored, and column 0 then wins
  int cand = 1 << 20;
#pragma unroll
  for (int c = K - 1; c >= 0; --c)
    if (Hk[c] == gmax && live[c]) cand = lane * K + c;
  R.gmax = gmax;
  R.te = te;
  R.qe = -gb::wave_max<kNegInf>(-cand);

  // score2, te2 (ksw.c:218-226): the first entry with the largest score among those outside te +- w.
  // Rows rise along the list, so "first" is "smallest row", and one max over score << 14 | ~row finds it.
  int best = -1;
  if (n_b > 0) {
    __threadfence_block();  // lane 63's stores before every lane's loads
    const int w = (gmax + A.max_mat - 1) / A.max_mat;
    const int low = te - w, high = te + w;
    const int nn = min(n_b, list_cap);
    for (int k = lane; k < nn; k += 64) {
      const uint32_t u = list[k];
      const int row = (int)(u & kRowMask);
      if (row < low || row > high) best = max(best, (int)((u & ~kRowMask) | (kRowMask - (uint32_t)row)));
    }
    best = gb::wave_max<kNegInf>(best);
  }
  R.score2 = best < 0 ? -1 : best >> kRowBits;
  R.te2 = best < 0 ? -1 : (int)kRowMask - (best & (int)kRowMask);
}

template <bool ZO>
__global__ __launch_bounds__(64 * kWavesPerBlock) void bsw_local_kernel(Args A) {
  __shared__ int8_t smat[32];
  if (threadIdx.x < 25) smat[threadIdx.x] = A.mat[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  uint32_t *list = A.list + wave * A.list_cap;
  const int list_cap = (int)A.list_cap;
  for (;;) {
    unsigned int p = 0;
    if (lane == 0) p = atomicAdd(A.next, 1u);
    p = __builtin_amdgcn_readfirstlane(p);
    if ((int64_t)p >= A.n) break;
    const Pair P = A.pairs[p];
    const uint8_t *tgt = A.tgt + P.t_off, *qry = A.qry + P.q_off;
    const int xtra = P.xtra, thresh = xtra & 0xffff;
    const int pw = (xtra & GB_KSW_XBYTE) ? 16 : 8;  // values per SSE register in the reference
    int score = 0, te = -1, qe = 0, score2 = -1, te2 = -1, tb = -1, qb = -1;
    int qlen = P.qlen, te0 = -1;
    int minsc = (xtra & GB_KSW_XSUBO) ? thresh : kNoThreshold;
    int endsc = (xtra & GB_KSW_XSTOP) ? thresh : kNoThreshold;
    for (int ps = 0; ps < 2; ++ps) {
      const int L = (qlen + pw - 1) / pw * pw;
      const int K = (L + 63) >> 6;
      Res R;
      if (K <= 1)
        pass<1, ZO>(A, smat, tgt, qry, P.tlen, qlen, L, pw, te0, ps != 0, minsc, endsc, list, list_cap, lane, R);
      else if (K == 2)
        pass<2, ZO>(A, smat, tgt, qry, P.tlen, qlen, L, pw, te0, ps != 0, minsc, endsc, list, list_cap, lane, R);
      else if (K == 3)
        pass<3, ZO>(A, smat, tgt, qry, P.tlen, qlen, L, pw, te0, ps != 0, minsc, endsc, list, list_cap, lane, R);
      else
        pass<4, ZO>(A, smat, tgt, qry, P.tlen, qlen, L, pw, te0, ps != 0, minsc, endsc, list, list_cap, lane, R);
      if (ps == 0) {
        score = R.gmax, te = R.te, qe = min(R.qe, P.qlen - 1), score2 = R.score2, te2 = R.te2;
        // ksw.c:356; the no-hit result (score 0, te -1, qe 0) goes through the start pass like any other
        if (!(xtra & GB_KSW_XSTART) || ((xtra & GB_KSW_XSUBO) && score < thresh)) break;
        qlen = qe + 1;
        te0 = te;
        minsc = kNoThreshold;  // xtra = KSW_XSTOP | score (ksw.c:359)
        endsc = score;
      } else if (R.gmax == score) {
        tb = te - R.te;
        qb = qe - R.qe;
      }
    }
    // one field per lane (no store under `lane == 0` next to the work counter's branch, see
    // bsw_global.hip)
    int v = score;
    v = lane == 1 ? te : v;
    v = lane == 2 ? qe : v;
    v = lane == 3 ? score2 : v;
    v = lane == 4 ? te2 : v;
    v = lane == 5 ? tb : v;
    v = lane == 6 ? qb : v;
    v = lane == 7 ? 0 : v;
    if (lane < 8) A.out8[8 * (int64_t)p + lane] = v;
    // the whole wave meets here before any lane fetches the next pair (see bsw_global.hip)
    __builtin_amdgcn_wave_barrier();
  }
}

constexpr int64_t kChunkPairs = int64_t(1) << 20;

int64_t chunk_pairs() {  // GB_BSW_LOCAL_CHUNK (tests: many chunks from a small set), read per call
  const char *e = getenv("GB_BSW_LOCAL_CHUNK");
  return e ? std::max<int64_t>(1, std::min<int64_t>(atoll(e), kChunkPairs)) : kChunkPairs;
}

int get_ws(int dev, Ws **out) {
  return gb::get_ws("gb_bsw_local", dev, out, [](Ws *W) { return W->d_ctl.reserve(4); });
}

int run_resident(Ws *W, const gb_bsw_params *params, int max_mat, const Pair *d_pairs, int64_t m, const uint8_t *d_tgt,
                 const uint8_t *d_qry, int32_t *d_out8, int64_t list_cap, hipEvent_t e0, hipEvent_t e1) {
  int st;
  const int64_t blocks = std::max<int64_t>(
      1, std::min<int64_t>((int64_t)W->num_cus * kBlocksPerCU, (m + kWavesPerBlock - 1) / kWavesPerBlock));
  if ((st = W->d_list.reserve((size_t)(blocks * kWavesPerBlock * list_cap)))) return st;
  GB_HIP(hipMemsetAsync(W->d_ctl, 0, 4 * sizeof(unsigned int), W->stream));
  Args A;
  A.pairs = d_pairs;
  A.n = m;
  A.tgt = d_tgt;
  A.qry = d_qry;
  A.out8 = d_out8;
  A.list = W->d_list;
  A.list_cap = list_cap;
  A.next = W->d_ctl;
  A.oe_del = params->o_del + params->e_del;
  A.e_del = params->e_del;
  A.oe_ins = params->o_ins + params->e_ins;
  A.e_ins = params->e_ins;
  A.max_mat = max_mat;
  std::memset(A.mat, 0, sizeof(A.mat));
  std::memcpy(A.mat, params->mat, 25);
  if (e0) GB_HIP(hipEventRecord(e0, W->stream));
  if (params->o_ins == 0)
    hipLaunchKernelGGL(bsw_local_kernel<true>, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0, W->stream, A);
  else
    hipLaunchKernelGGL(bsw_local_kernel<false>, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0, W->stream, A);
  GB_HIP(hipGetLastError());
  if (e1) GB_HIP(hipEventRecord(e1, W->stream));
  return GB_OK;
}

// Every refusal of include/gb_bsw.h, before any device work.
int validate(const gb_bsw_params *params, const gb_bsw_lpair *pairs, int64_t n, const uint8_t *ref, int64_t ref_bytes,
             const uint8_t *qer, int64_t qer_bytes, int *max_mat) {
  GB_ARG(params && n >= 0 && (n == 0 || pairs), "gb_bsw_local: bad arguments");
  GB_ARG(ref_bytes >= 0 && qer_bytes >= 0 && (ref_bytes == 0 || ref) && (qer_bytes == 0 || qer),
         "gb_bsw_local: bad sequence buffers");
  const int pen[4] = {params->o_del, params->e_del, params->o_ins, params->e_ins};
  GB_ARG(pen[0] >= 0 && pen[1] >= 0 && pen[2] >= 0 && pen[3] >= 0 && (int64_t)pen[0] + pen[1] < kMaxPenalty &&
             (int64_t)pen[2] + pen[3] < kMaxPenalty,
         "gb_bsw_local: gap penalties (o_del %d, e_del %d, o_ins %d, e_ins %d) must be >= 0 with o + e < %d", pen[0],
         pen[1], pen[2], pen[3], kMaxPenalty);
  int mx = params->mat[0], mn = params->mat[0];
  for (int k = 1; k < 25; ++k) mx = std::max<int>(mx, params->mat[k]), mn = std::min<int>(mn, params->mat[k]);
  GB_ARG(mx >= 1 && mn <= 0, "gb_bsw_local: the scoring matrix has max %d, min %d (need max >= 1, min <= 0)", mx, mn);
  *max_mat = mx;
  for (int64_t p = 0; p < n; ++p) {
    const gb_bsw_lpair &s = pairs[p];
    GB_ARG(s.len2 >= 1 && s.len2 <= GB_BSW_MAX_QLEN && s.len1 >= 1 && s.len1 <= GB_BSW_LOCAL_MAX_TLEN,
           "gb_bsw_local: pair %lld has len1=%d len2=%d (need len1 in [1,%d], len2 in [1,%d])", (long long)p, s.len1,
           s.len2, GB_BSW_LOCAL_MAX_TLEN, GB_BSW_MAX_QLEN);
    GB_ARG(s.idr >= 0 && s.idr <= ref_bytes - s.len1 && s.idq >= 0 && s.idq <= qer_bytes - s.len2,
           "gb_bsw_local: pair %lld lies outside the sequence buffers", (long long)p);
    GB_ARG((s.xtra & ~(kFlags | 0xffff)) == 0, "gb_bsw_local: pair %lld has xtra=0x%x with bits that are no KSW_X* flag",
           (long long)p, (unsigned)s.xtra);
    if (s.xtra & GB_KSW_XBYTE) {
      GB_ARG(pen[0] + pen[1] <= 255 && pen[2] + pen[3] <= 255,
             "gb_bsw_local: pair %lld asks for KSW_XBYTE with gap penalties o + e above 255", (long long)p);
      GB_ARG(s.len2 * mx - mn < 255,
             "gb_bsw_local: pair %lld asks for KSW_XBYTE with len2 * max(mat) - min(mat) = %d (need < 255)", (long long)p,
             s.len2 * mx - mn);
    }
  }
  return GB_OK;
}

}  // namespace gbbswl

extern "C" {

int gb_bsw_local_xtra(const gb_bsw_params *params, int32_t len2, int32_t min_seed_len) {
  GB_ARG(params && len2 >= 0, "gb_bsw_local_xtra: bad arguments");
  const int a = params->mat[0];
  const int64_t t = (int64_t)min_seed_len * a;
  GB_ARG(t >= 0 && t <= 0xffff, "gb_bsw_local_xtra: min_seed_len * a = %lld does not fit 16 bits", (long long)t);
  return GB_KSW_XSUBO | GB_KSW_XSTART | ((int64_t)len2 * a < 250 ? GB_KSW_XBYTE : 0) | (int)t;  // bwamem_pair.c:150
}

int gb_bsw_local_timing(float *kernel_ms) {
  GB_ARG(kernel_ms, "gb_bsw_local_timing: null argument");
  const gbbswl::Ws *W = nullptr;
  if (const int st = gb::ran_ws("gb_bsw_local_timing", "gb_bsw_local", &W)) return st;
  *kernel_ms = W->kernel_ms;
  return GB_OK;
}

int gb_bsw_local(const gb_bsw_params *params, gb_bsw_lpair *pairs, int64_t n, const uint8_t *ref, int64_t ref_bytes,
                 const uint8_t *qer, int64_t qer_bytes) {
  using namespace gbbswl;
  gb::Range range_("gb.bsw.local");
  int max_mat = 1;
  int st = validate(params, pairs, n, ref, ref_bytes, qer, qer_bytes, &max_mat);
  if (st) return st;
  if (n == 0) return GB_OK;

  int dev = 0;
  GB_HIP(hipGetDevice(&dev));
  Ws *W = nullptr;
  if ((st = get_ws(dev, &W))) return st;
  W->kernel_ms = 0.f;
  if ((st = W->d_tgt.reserve((size_t)ref_bytes))) return st;
  if ((st = W->d_qry.reserve((size_t)qer_bytes))) return st;
  GB_HIP(hipMemcpyAsync(W->d_tgt, ref, (size_t)ref_bytes, hipMemcpyHostToDevice, W->stream));
  GB_HIP(hipMemcpyAsync(W->d_qry, qer, (size_t)qer_bytes, hipMemcpyHostToDevice, W->stream));

  const int64_t chunk = chunk_pairs();
  for (int64_t lo = 0; lo < n; lo += chunk) {
    const int64_t m = std::min(chunk, n - lo);
    if ((st = W->h_pairs.reserve((size_t)m))) return st;
    if ((st = W->h_out8.reserve((size_t)m * 8))) return st;
    if ((st = W->d_pairs.reserve((size_t)m))) return st;
    if ((st = W->d_out8.reserve((size_t)m * 8))) return st;
    // the entry list of a wave holds the longest list any pair of this chunk can write
    int64_t list_cap = 1;
    Pair *hp = W->h_pairs;
    for (int64_t k = 0; k < m; ++k) {
      const gb_bsw_lpair &s = pairs[lo + k];
      hp[k] = Pair{s.idr, s.idq, s.len1, s.len2, s.xtra, 0};
      if (s.xtra & GB_KSW_XSUBO) list_cap = std::max(list_cap, list_entries(s.len1));
    }
    GB_HIP(hipMemcpyAsync(W->d_pairs, hp, (size_t)m * sizeof(Pair), hipMemcpyHostToDevice, W->stream));
    if ((st = run_resident(W, params, max_mat, W->d_pairs, m, W->d_tgt, W->d_qry, W->d_out8, list_cap, W->ev[0], W->ev[1])))
      return st;
    int32_t *ho = W->h_out8;
    GB_HIP(hipMemcpyAsync(ho, W->d_out8, (size_t)m * 8 * sizeof(int32_t), hipMemcpyDeviceToHost, W->stream));
    GB_HIP(hipStreamSynchronize(W->stream));
    float ms = 0.f;
    GB_HIP(hipEventElapsedTime(&ms, W->ev[0], W->ev[1]));
    W->kernel_ms += ms;
    for (int64_t k = 0; k < m; ++k) {
      gb_bsw_lpair &s = pairs[lo + k];
      const int32_t *o = ho + 8 * k;
      s.score = o[0], s.te = o[1], s.qe = o[2], s.score2 = o[3], s.te2 = o[4], s.tb = o[5], s.qb = o[6];
    }
  }
  return GB_OK;
}

}  // extern "C"
