// bsw_gencigar.hip -- MI355X (gfx950): bwa's packed reference on the device (gb_ref) and all of
// bwa_gen_cigar2 (tools/bwa/bwa.c:121-208) on top of it: kernels and C ABI.
//
// Per call of gb_bsw_gen_cigar:
//   fetch: one wave64 per accepted pair. A lane turns 16 bases of the 2-bit pac (two aligned 32-bit
//     words, funnel-shifted to the region's first base) into 16 byte codes and stores them with one
//     16-byte store into the pair's slice of the target staging buffer; slices start on 16-byte
//     boundaries and are padded to a multiple of 16, so every store is whole. For a reverse-strand
//     region (rb >= l_pac) bns_get_seq returns the complement read backwards and bwa_gen_cigar2 then
//     reverses it (bwa.c:138-139): the net effect, and what this kernel writes, is the complement in
//     FORWARD order, forward bases 2 l_pac - re .. 2 l_pac - rb - 1. The same wave writes the reversed
//     copy of such a pair's query (bwa.c:136-137) behind the caller's query bytes, and for a pair on
//     the reference's no-DP shortcut (bwa.c:141-149) the plain sum of mat.
//   fill, walk: the kernels of bsw_global.hip, unchanged, through gbbswg::run_resident, on the pairs
//     that are neither rejected nor on the shortcut.
//   md: one lane per pair walks the pair's CIGAR over target and query (bwa.c:169-198) twice: the first
//     pass measures the MD string (and counts mismatches), one atomic add reserves its bytes in the
//     chunk's MD pool, the second pass writes them. It runs once per chunk behind the walk kernel, and
//     once for the shortcut pairs, whose CIGAR is the single operation len2 M.
// Which pairs the reference rejects, and which take the shortcut, depends on rb, re, len2 and w alone
// and is decided on the host while the chunks are planned; such pairs never reach the DP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/gb_bsw.h"
#include "bsw_global_internal.h"
#include "bsw_ref_internal.h"
#include "gb_common.h"

static_assert(sizeof(gb_bsw_cpair) == 64, "gb_bsw_cpair is 64 bytes (include/gb_bsw.h)");

namespace gbgc {

constexpr int kMaxPenalty = 32768;
constexpr int kFetchWaves = 4;

enum : int32_t { kComplement = 1, kBackward = 2, kShortcut = 4 };

struct FetchItem {  // 48 B
  int64_t src;      // pac index of the base that lands in out[0]
  int64_t t_dst;    // 16-byte aligned offset in the target staging buffer
  int64_t q_src;    // offset of the query in the query buffer
  int64_t q_dst;    // 4-byte aligned offset of its reversed copy in the same buffer, -1: none
  int32_t len, qlen;
  int32_t flags, pad;
};

struct FetchArgs {
  const FetchItem *items;
  int64_t n;
  const uint32_t *pac;
  int64_t n_words;
  uint8_t *tgt;
  uint8_t *qry;
  int32_t *score;  // per item, written for kShortcut items only
  int8_t mat[28];
};

__global__ __launch_bounds__(64 * kFetchWaves) void bsw_gencigar_fetch_kernel(FetchArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * kFetchWaves + (threadIdx.x >> 6);
  if (p >= A.n) return;
  const FetchItem it = A.items[p];
  const uint32_t cx = (it.flags & kComplement) ? 0xFFFFFFFFu : 0u;  // 3 - x == ~x on two bits
  const bool back = (it.flags & kBackward) != 0;
  fetch_bases(A.pac, A.n_words, it.src, it.len, back, cx, A.tgt + it.t_dst, lane);
  const bool rev = it.q_dst >= 0;
  // the reversed query; the slice is padded to a multiple of 4
  if (rev) reverse_query(A.qry + it.q_src, it.qlen, A.qry + it.q_dst, lane);
  if (it.flags & kShortcut) {  // bwa.c:148-149 (len == qlen); the sum does not depend on the order
    const uint8_t *q = A.qry + it.q_src;
    int s = 0;
    for (int i = lane; i < it.qlen; i += 64) {
      const int64_t b = it.src + i;
      const int64_t wi = min(b >> 4, A.n_words - 1);
      const int t = (int)(((__builtin_bswap32(A.pac[wi]) >> (30 - 2 * (int)(b & 15))) ^ cx) & 3u);
      const int qb = min((int)(rev ? q[it.qlen - 1 - i] : q[i]), 4);
      s += A.mat[t * 5 + qb];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) A.score[p] = s;
  }
}

struct MdArgs {
  const gbbswg::Pair *pairs;
  int64_t n;
  const uint8_t *tgt, *qry;
  const int32_t *out4;    // per pair {score, n_cigar, nm, pool offset}; null: the one operation qlen M
  const uint32_t *pool;
  const uint8_t *rev;     // per pair: 1 = reverse strand, letters "TGCAN"
  char *md;               // the MD pool; null: measure and count only
  unsigned int *md_used;  // bytes reserved so far
  int32_t *md3;           // per pair {length, pool offset, mismatches}
};

template <bool WRITE>
__device__ __forceinline__ int put_count(int u, char *dst, int pos) {  // kputw of u >= 0
  const int d = u >= 1000 ? 4 : u >= 100 ? 3 : u >= 10 ? 2 : 1;
  if (WRITE) {
    for (int k = d - 1; k >= 0; --k) {
      dst[pos + k] = (char)('0' + u % 10);
      u /= 10;
    }
  }
  return pos + d;
}

// bwa.c:173-196. x, y stay inside the pair's query and target for a CIGAR that consumes exactly
// qlen and tlen; the clamps keep them there for any other. Returns the string's length.
template <bool WRITE>
__device__ __forceinline__ int md_walk(const uint32_t *ops, int n_ops, uint32_t one_op, const uint8_t *tgt, int tlen,
                                       const uint8_t *qry, int qlen, uint32_t letters, char *dst, int &n_mm) {
  int x = 0, y = 0, u = 0, pos = 0, mm = 0;
  for (int k = 0; k < n_ops; ++k) {
    const uint32_t o = ops ? ops[k] : one_op;
    const int op = (int)(o & 15u);
    int len = (int)(o >> 4);
    if (op == 0) {
      len = min(len, min(qlen - x, tlen - y));
      for (int i = 0; i < len; ++i) {
        const int t = tgt[y + i];
        if ((int)qry[x + i] != t) {
          pos = put_count<WRITE>(u, dst, pos);
          if (WRITE) dst[pos] = (char)((letters >> (8 * min(t, 3))) & 0xFF);
          ++pos, ++mm, u = 0;
        } else {
          ++u;
        }
      }
      x += len, y += len;
    } else if (op == 2) {
      len = min(len, tlen - y);
      if (k > 0 && k < n_ops - 1) {  // not for a D run that is the first or the last operation
        pos = put_count<WRITE>(u, dst, pos);
        if (WRITE) dst[pos] = '^';
        ++pos;
        for (int i = 0; i < len; ++i) {
          if (WRITE) dst[pos] = (char)((letters >> (8 * min((int)tgt[y + i], 3))) & 0xFF);
          ++pos;
        }
        u = 0;
      }
      y += len;
    } else {
      x += min(len, qlen - x);
    }
  }
  pos = put_count<WRITE>(u, dst, pos);
  n_mm = mm;
  return pos;
}

__global__ __launch_bounds__(64) void bsw_gencigar_md_kernel(MdArgs A) {
  const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (p >= A.n) return;
  const gbbswg::Pair P = A.pairs[p];
  const uint8_t *tgt = A.tgt + P.t_off, *qry = A.qry + P.q_off;
  const uint32_t *ops = nullptr;
  int n_ops = 1;
  if (A.out4) {
    n_ops = A.out4[4 * p + 1];
    ops = A.pool + (uint32_t)A.out4[4 * p + 3];
  }
  const uint32_t one_op = (uint32_t)P.qlen << 4;
  // "ACGT" / "TGCA" (bwa.c:172); the pac holds no N
  const uint32_t letters = A.rev[p] ? ('T' | 'G' << 8 | 'C' << 16 | 'A' << 24) : ('A' | 'C' << 8 | 'G' << 16 | 'T' << 24);
  int mm = 0, mm2 = 0;
  const int len = md_walk<false>(ops, n_ops, one_op, tgt, P.tlen, qry, P.qlen, letters, nullptr, mm);
  unsigned int base = 0;
  if (A.md) {
    // len <= 3 tlen + 1, and the pool holds the chunk's sum of that
    base = atomicAdd(A.md_used, (unsigned int)len);
    md_walk<true>(ops, n_ops, one_op, tgt, P.tlen, qry, P.qlen, letters, A.md + base, mm2);
  }
  int32_t *o = A.md3 + 3 * p;
  o[0] = len;
  o[1] = (int32_t)base;
  o[2] = mm;
}

struct GWs {  // the calling thread's, through gb::thread_ws
  int device = -1;
  gb::Event ev[4];  // fetch begin / end, md begin / end
  gb::DevBuf<uint8_t> d_tgt, d_qry, d_rev;
  gb::DevBuf<FetchItem> d_items;
  gb::DevBuf<int32_t> d_score, d_md3;
  gb::DevBuf<gbbswg::Pair> d_spairs;
  gb::DevBuf<char> d_md;
  gb::DevBuf<unsigned int> d_mctl;
  float fetch_ms = 0.f, fill_ms = 0.f, walk_ms = 0.f, md_ms = 0.f;
};

int get_gws(int dev, GWs **out) {
  return gb::thread_ws(dev, out, [](int dev, GWs **out) -> int {
    auto *G = new GWs();
    G->device = dev;
    hipError_t e = hipSuccess;
    for (auto &ev : G->ev)
      if (e == hipSuccess) e = ev.create();
    int st = GB_ERR_HIP;
    if (e == hipSuccess)
      st = G->d_mctl.reserve(4);
    else
      gb::set_error("gb_bsw_gen_cigar workspace: %s", hipGetErrorString(e));
    if (st) {
      delete G;
      return st;
    }
    *out = G;
    return GB_OK;
  });
}

// Upload on first use; afterwards the reference belongs to that device.
int ensure_device(gb_ref *R, int dev) {
  std::lock_guard<std::mutex> lock(R->mu);
  if (R->device == dev) return GB_OK;
  if (R->device >= 0) {
    gb::set_error("gb_ref: the reference lives on device %d, the calling thread uses device %d", R->device, dev);
    return GB_ERR_STATE;
  }
  const int64_t n_words = (R->l_pac + 15) / 16 + 2;
  int st = R->d_pac.reserve((size_t)n_words);
  if (st) return st;
  R->host.resize((size_t)n_words * 4, 0);  // zero-padded to whole words plus the slack
  const hipError_t e = gb::memcpy_big(R->d_pac, R->host.data(), (size_t)n_words * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    R->host.resize((size_t)((R->l_pac + 3) / 4));
    gb::set_error("gb_ref upload failed: %s", hipGetErrorString(e));
    return GB_ERR_HIP;
  }
  std::vector<uint8_t>().swap(R->host);
  R->n_words = n_words;
  R->device = dev;
  return GB_OK;
}

int launch_fetch(hipStream_t stream, GWs *G, const gb_ref *R, const std::vector<FetchItem> &items, const int8_t *mat) {
  const int64_t n = (int64_t)items.size();
  int st;
  if ((st = G->d_items.reserve((size_t)n))) return st;
  if ((st = G->d_score.reserve((size_t)n))) return st;
  GB_HIP(hipMemcpyAsync(G->d_items, items.data(), (size_t)n * sizeof(FetchItem), hipMemcpyHostToDevice, stream));
  FetchArgs F;
  F.items = G->d_items;
  F.n = n;
  F.pac = R->d_pac;
  F.n_words = R->n_words;
  F.tgt = G->d_tgt;
  F.qry = G->d_qry;
  F.score = G->d_score;
  std::memset(F.mat, 0, sizeof(F.mat));
  if (mat) std::memcpy(F.mat, mat, 25);
  GB_HIP(hipEventRecord(G->ev[0], stream));
  hipLaunchKernelGGL(bsw_gencigar_fetch_kernel, dim3((unsigned)((n + kFetchWaves - 1) / kFetchWaves)),
                     dim3(64 * kFetchWaves), 0, stream, F);
  GB_HIP(hipGetLastError());
  GB_HIP(hipEventRecord(G->ev[1], stream));
  return GB_OK;
}

// The MD kernel over m device-resident pair descriptors, and its results once the stream was
// synchronised. rev and tlen are the host's view of the same pairs.
struct MdPass {
  GWs *G = nullptr;
  bool write = false;
  std::vector<int32_t> md3;
  std::vector<char> bytes;
  unsigned int used = 0;
  int64_t cap = 0;

  int enqueue(hipStream_t stream, int64_t m, const gbbswg::Pair *d_pairs, const int32_t *d_out4, const uint32_t *d_pool,
              const uint8_t *rev, int64_t tlen_sum, const uint8_t *d_tgt, const uint8_t *d_qry) {
    int st;
    cap = 3 * tlen_sum + m;
    if ((st = G->d_rev.reserve((size_t)m))) return st;
    if ((st = G->d_md3.reserve((size_t)m * 3))) return st;
    if (write && (st = G->d_md.reserve((size_t)cap))) return st;
    GB_HIP(hipMemcpyAsync(G->d_rev, rev, (size_t)m, hipMemcpyHostToDevice, stream));
    GB_HIP(hipMemsetAsync(G->d_mctl, 0, 4 * sizeof(unsigned int), stream));
    MdArgs A;
    A.pairs = d_pairs;
    A.n = m;
    A.tgt = d_tgt;
    A.qry = d_qry;
    A.out4 = d_out4;
    A.pool = d_pool;
    A.rev = G->d_rev;
    A.md = write ? G->d_md.get() : nullptr;
    A.md_used = G->d_mctl;
    A.md3 = G->d_md3;
    GB_HIP(hipEventRecord(G->ev[2], stream));
    hipLaunchKernelGGL(bsw_gencigar_md_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, stream, A);
    GB_HIP(hipGetLastError());
    GB_HIP(hipEventRecord(G->ev[3], stream));
    md3.resize((size_t)m * 3);
    used = 0;
    GB_HIP(hipMemcpyAsync(md3.data(), G->d_md3, (size_t)m * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    GB_HIP(hipMemcpyAsync(&used, G->d_mctl, sizeof(used), hipMemcpyDeviceToHost, stream));
    return GB_OK;
  }

  int collect() {  // after the stream was synchronised
    float ms = 0.f;
    GB_HIP(hipEventElapsedTime(&ms, G->ev[2], G->ev[3]));
    G->md_ms += ms;
    if ((int64_t)used > cap) {
      gb::set_error("gb_bsw_gen_cigar: the device reserved %u MD bytes where at most %lld can be needed", used,
                    (long long)cap);
      return GB_ERR_STATE;
    }
    bytes.resize(used);
    if (write && used) GB_HIP(hipMemcpy(bytes.data(), G->d_md, used, hipMemcpyDeviceToHost));
    return GB_OK;
  }

  // pair k's string appended to out; its length (or a negative status)
  int append(int64_t k, std::vector<char> &out) const {
    const int64_t len = md3[3 * k], off = (int64_t)(uint32_t)md3[3 * k + 1];
    if (len < 1 || (write && off + len > (int64_t)used)) {
      gb::set_error("gb_bsw_gen_cigar: an MD string of %lld bytes at pool offset %lld of %u", (long long)len,
                    (long long)off, used);
      return GB_ERR_STATE;
    }
    if (write) out.insert(out.end(), bytes.begin() + off, bytes.begin() + off + len);
    return (int)len;
  }
};

enum Kind : uint8_t { kReject = 0, kShort = 1, kDp = 2 };

// bwa.c:132,134: rejected outright, or shortened by bns_get_seq's clamps
inline bool rejected(int64_t l_pac, int64_t rb, int64_t re) {
  return rb >= re || (rb < l_pac && re > l_pac) || rb < 0 || re > 2 * l_pac;
}

// Every refusal of include/gb_bsw.h, before any device work.
int validate(const char *who, const gb_bsw_params *params, const gb_ref *ref, const gb_bsw_cpair *pairs, int64_t n,
             const uint8_t *qer, int64_t qer_bytes, const uint32_t *cigar, int64_t cigar_cap, const char *md,
             int64_t md_cap) {
  GB_ARG(params && ref && n >= 0 && (n == 0 || pairs), "%s: bad arguments", who);
  GB_ARG(qer_bytes >= 0 && (qer_bytes == 0 || qer), "%s: bad sequence buffer", who);
  GB_ARG(!cigar || cigar_cap >= 0, "%s: negative cigar_cap", who);
  GB_ARG(!md || md_cap >= 0, "%s: negative md_cap", who);
  GB_ARG(!md || cigar, "%s: md needs cigar (scores only produces neither)", who);
  const int pen[4] = {params->o_del, params->e_del, params->o_ins, params->e_ins};
  for (int v : pen)
    GB_ARG(v >= 0 && v < kMaxPenalty, "%s: gap penalties (o_del %d, e_del %d, o_ins %d, e_ins %d) must lie in [0, %d)", who,
           pen[0], pen[1], pen[2], pen[3], kMaxPenalty);
  GB_ARG(params->e_del > 0 && params->e_ins > 0,
         "%s: gap extension penalties (e_del %d, e_ins %d) must be > 0, the band rule divides by them", who,
         params->e_del, params->e_ins);
  for (int64_t p = 0; p < n; ++p) {
    const gb_bsw_cpair &s = pairs[p];
    GB_ARG(s.len2 >= 1 && s.len2 <= GB_BSW_MAX_QLEN, "%s: pair %lld has len2=%d (need len2 in [1,%d])", who, (long long)p,
           s.len2, GB_BSW_MAX_QLEN);
    GB_ARG(s.w >= 0, "%s: pair %lld has w=%d below 0", who, (long long)p, s.w);
    GB_ARG(s.idq >= 0 && s.idq <= qer_bytes - s.len2, "%s: pair %lld has its query outside the sequence buffer", who,
           (long long)p);
    if (!rejected(ref->l_pac, s.rb, s.re))
      GB_ARG(s.re - s.rb <= GB_BSW_GLOBAL_MAX_TLEN, "%s: pair %lld has re - rb = %lld (need at most %d)", who, (long long)p,
             (long long)(s.re - s.rb), GB_BSW_GLOBAL_MAX_TLEN);
  }
  return GB_OK;
}

struct MdHook : gbbswg::ChunkHook {
  MdPass pass;
  const gb_bsw_gpair *dp = nullptr;  // the DP pairs run_resident works on
  const uint8_t *rev = nullptr;      // per DP pair
  const uint8_t *d_tgt = nullptr, *d_qry = nullptr;
  std::vector<int32_t> *md_len = nullptr;  // per DP pair
  std::vector<int64_t> *md_off = nullptr;  // into *out
  std::vector<char> *out = nullptr;

  int enqueue(hipStream_t stream, int64_t lo, int64_t m, const gbbswg::Pair *d_pairs, const int32_t *d_out4,
              const uint32_t *d_pool) override {
    int64_t tsum = 0;
    for (int64_t k = 0; k < m; ++k) tsum += dp[lo + k].len1;
    return pass.enqueue(stream, m, d_pairs, d_out4, d_pool, rev + lo, tsum, d_tgt, d_qry);
  }
  int collect(int64_t lo, int64_t m) override {
    int st = pass.collect();
    if (st) return st;
    for (int64_t k = 0; k < m; ++k) {
      (*md_off)[lo + k] = (int64_t)out->size();
      const int len = pass.append(k, *out);
      if (len < 0) return len;
      (*md_len)[lo + k] = len;
    }
    return GB_OK;
  }
};

inline int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// gb_bsw_gen_cigar behind its validation: per-pair fields written, operations and MD bytes appended
// to cig / mdv in pair order (cigar_off / md_off index those).
int run_core(const char *who, const gb_bsw_params *params, gb_ref *R, gb_bsw_cpair *pairs, int64_t n, const uint8_t *qer,
             int64_t qer_bytes, bool want_cigar, bool want_md, std::vector<uint32_t> &cig, std::vector<char> &mdv) {
  const int64_t l_pac = R->l_pac;
  std::vector<uint8_t> kind((size_t)n);
  std::vector<FetchItem> items;
  std::vector<int64_t> item_of((size_t)n, -1);
  int64_t t_bytes = 0, q_extra = 0, n_dp = 0, n_short = 0;
  const int64_t q_base = round_up(qer_bytes, 4);
  for (int64_t p = 0; p < n; ++p) {
    const gb_bsw_cpair &s = pairs[p];
    if (rejected(l_pac, s.rb, s.re)) {
      kind[p] = kReject;
      continue;
    }
    const int32_t len1 = (int32_t)(s.re - s.rb);
    const bool rev = s.rb >= l_pac;
    const bool shortcut = s.len2 == len1 && s.w == 0;
    kind[p] = shortcut ? kShort : kDp;
    shortcut ? ++n_short : ++n_dp;
    FetchItem it;
    it.src = rev ? 2 * l_pac - s.re : s.rb;
    it.t_dst = t_bytes;
    it.q_src = s.idq;
    it.q_dst = rev ? q_base + q_extra : -1;
    it.len = len1;
    it.qlen = s.len2;
    it.flags = (rev ? kComplement : 0) | (shortcut ? kShortcut : 0);
    it.pad = 0;
    t_bytes += round_up(len1, 16);
    if (rev) q_extra += round_up(s.len2, 4);
    item_of[p] = (int64_t)items.size();
    items.push_back(it);
  }

  std::vector<gb_bsw_gpair> dp;
  std::vector<uint8_t> dp_rev, sh_rev;
  std::vector<gbbswg::Pair> sh;
  std::vector<int32_t> sh_score, dp_md_len;
  std::vector<int64_t> dp_md_off;
  // the DP pairs' operations, packed from the front; sized for the worst case but not initialised, so
  // only the pages that receive operations are ever touched
  std::unique_ptr<uint32_t[]> dp_cig;
  std::vector<char> dp_md;
  MdPass sh_pass;
  int st = GB_OK;

  if (!items.empty()) {
    int dev = 0;
    GB_HIP(hipGetDevice(&dev));
    if ((st = ensure_device(R, dev))) return st;
    gbbswg::Ws *W = nullptr;
    GWs *G = nullptr;
    if ((st = gbbswg::get_ws(dev, &W))) return st;
    if ((st = get_gws(dev, &G))) return st;
    if ((st = G->d_tgt.reserve((size_t)t_bytes))) return st;
    if ((st = G->d_qry.reserve((size_t)(q_base + q_extra)))) return st;
    GB_HIP(hipMemcpyAsync(G->d_qry, qer, (size_t)qer_bytes, hipMemcpyHostToDevice, W->stream));
    if ((st = launch_fetch(W->stream, G, R, items, params->mat))) return st;

    dp.reserve((size_t)n_dp);
    int64_t worst = 0;
    for (int64_t p = 0; p < n; ++p) {
      if (kind[p] == kReject) continue;
      const FetchItem &it = items[(size_t)item_of[p]];
      const int64_t q_off = it.q_dst >= 0 ? it.q_dst : it.q_src;
      if (kind[p] == kDp) {
        gb_bsw_gpair g;
        std::memset(&g, 0, sizeof(g));
        g.idr = it.t_dst;
        g.idq = q_off;
        g.len1 = it.len;
        g.len2 = it.qlen;
        g.w = gb_bsw_global_band(params, it.qlen, it.len, pairs[p].w);
        dp.push_back(g);
        dp_rev.push_back(it.q_dst >= 0);
        worst += (int64_t)it.len + it.qlen;
      } else {
        sh.push_back(gbbswg::Pair{it.t_dst, q_off, 0, it.len, it.qlen, 0, 0});
        sh_rev.push_back(it.q_dst >= 0);
      }
    }

    if (n_short) {
      sh_score.resize((size_t)items.size());
      GB_HIP(hipMemcpyAsync(sh_score.data(), G->d_score, items.size() * sizeof(int32_t), hipMemcpyDeviceToHost, W->stream));
      if (want_cigar) {  // NM needs the mismatch count even when no MD is asked for
        if ((st = G->d_spairs.reserve((size_t)n_short))) return st;
        GB_HIP(hipMemcpyAsync(G->d_spairs, sh.data(), (size_t)n_short * sizeof(gbbswg::Pair), hipMemcpyHostToDevice,
                              W->stream));
        int64_t tsum = 0;
        for (const auto &s : sh) tsum += s.tlen;
        sh_pass.G = G;
        sh_pass.write = want_md;
        if ((st = sh_pass.enqueue(W->stream, n_short, G->d_spairs, nullptr, nullptr, sh_rev.data(), tsum, G->d_tgt, G->d_qry)))
          return st;
      }
      GB_HIP(hipStreamSynchronize(W->stream));
      if (want_cigar && (st = sh_pass.collect())) return st;
    }
    if (n_dp) {
      MdHook hook;
      hook.pass.G = G;
      hook.pass.write = true;
      hook.dp = dp.data();
      hook.rev = dp_rev.data();
      hook.d_tgt = G->d_tgt;
      hook.d_qry = G->d_qry;
      dp_md_len.assign((size_t)n_dp, 0);
      dp_md_off.assign((size_t)n_dp, 0);
      hook.md_len = &dp_md_len;
      hook.md_off = &dp_md_off;
      hook.out = &dp_md;
      if (want_cigar) dp_cig.reset(new uint32_t[(size_t)std::max<int64_t>(worst, 1)]);
      int64_t used = 0;
      if ((st = gbbswg::run_resident(W, who, params, dp.data(), n_dp, G->d_tgt, G->d_qry, want_cigar ? dp_cig.get() : nullptr,
                                     worst, &used, &G->fill_ms, &G->walk_ms, want_md ? &hook : nullptr)))
        return st;
    }
    float ms = 0.f;
    GB_HIP(hipEventElapsedTime(&ms, G->ev[0], G->ev[1]));  // every path above has synchronised the stream
    G->fetch_ms += ms;
  }

  // results in pair order
  int64_t k_dp = 0, k_sh = 0;
  for (int64_t p = 0; p < n; ++p) {
    gb_bsw_cpair &s = pairs[p];
    s.n_cigar = 0, s.nm = -1, s.md_len = 0;
    s.cigar_off = want_cigar ? (int64_t)cig.size() : 0;
    s.md_off = want_md ? (int64_t)mdv.size() : 0;
    if (kind[p] == kReject) continue;  // score stays as the caller set it
    if (kind[p] == kShort) {
      s.score = sh_score[(size_t)item_of[p]];
      if (want_cigar) {
        s.n_cigar = 1;
        cig.push_back((uint32_t)s.len2 << 4);
        s.nm = sh_pass.md3[3 * k_sh + 2];
        const int len = sh_pass.append(k_sh, mdv);
        if (len < 0) return len;
        if (want_md) s.md_len = len;
      }
      ++k_sh;
    } else {
      const gb_bsw_gpair &g = dp[(size_t)k_dp];
      s.score = g.score;
      if (want_cigar) {
        s.n_cigar = g.n_cigar;
        s.nm = g.nm;
        cig.insert(cig.end(), dp_cig.get() + g.cigar_off, dp_cig.get() + g.cigar_off + g.n_cigar);
        if (want_md) {
          s.md_len = dp_md_len[(size_t)k_dp];
          mdv.insert(mdv.end(), dp_md.begin() + dp_md_off[(size_t)k_dp], dp_md.begin() + dp_md_off[(size_t)k_dp] + s.md_len);
        }
      }
      ++k_dp;
    }
  }
  return GB_OK;
}

// The capacity rule of include/gb_bsw.h, then the copies.
int deliver(const char *who, const std::vector<uint32_t> &cig, const std::vector<char> &mdv, uint32_t *cigar,
            int64_t cigar_cap, int64_t *cigar_used, char *md, int64_t md_cap, int64_t *md_used) {
  if (cigar_used) *cigar_used = cigar ? (int64_t)cig.size() : 0;
  if (md_used) *md_used = md ? (int64_t)mdv.size() : 0;
  GB_ARG(!cigar || (int64_t)cig.size() <= cigar_cap, "%s: cigar_cap %lld is below the %lld operations of this call", who,
         (long long)cigar_cap, (long long)cig.size());
  GB_ARG(!md || (int64_t)mdv.size() <= md_cap, "%s: md_cap %lld is below the %lld MD bytes of this call", who,
         (long long)md_cap, (long long)mdv.size());
  if (cigar && !cig.empty()) std::memcpy(cigar, cig.data(), cig.size() * sizeof(uint32_t));
  if (md && !mdv.empty()) std::memcpy(md, mdv.data(), mdv.size());
  return GB_OK;
}

void reset_timing() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  if (GWs *G = gb::find_thread_ws<GWs>(dev)) G->fetch_ms = G->fill_ms = G->walk_ms = G->md_ms = 0.f;
}

}  // namespace gbgc

extern "C" {

int gb_ref_create(const uint8_t *pac, int64_t l_pac, gb_ref **out) {
  GB_ARG(pac && out && l_pac >= 1, "gb_ref_create: bad arguments (l_pac must be >= 1)");
  auto *R = new gb_ref();
  R->l_pac = l_pac;
  R->host.assign(pac, pac + (l_pac + 3) / 4);
  *out = R;
  return GB_OK;
}

int gb_ref_load_pac(const char *path, gb_ref **out) {
  GB_ARG(path && out, "gb_ref_load_pac: null argument");
  FILE *f = fopen(path, "rb");
  GB_ARG(f, "gb_ref_load_pac: cannot open %s", path);
  // The file is always l_pac / 4 + 2 bytes long and ends in l_pac % 4 (bntseq.c:317-324; bns_restore_core
  // reads the length back the same way): a zero byte stands before that one when l_pac % 4 == 0.
  int64_t size = -1;
  if (fseeko(f, 0, SEEK_END) == 0) size = (int64_t)ftello(f);
  unsigned char tail[2] = {0, 0};
  const bool ok = size >= 2 && fseeko(f, size - 2, SEEK_SET) == 0 && fread(tail, 1, 2, f) == 2 && tail[1] < 4 &&
                  (tail[1] != 0 || tail[0] == 0);
  const int64_t l_pac = ok ? (size - 2) * 4 + tail[1] : 0;
  if (l_pac < 1) {
    fclose(f);
    gb::set_error("gb_ref_load_pac: %s is not a .pac file (%lld bytes, last bytes %u %u)", path, (long long)size, tail[0],
                  tail[1]);
    return GB_ERR_ARG;
  }
  const int64_t bytes = (l_pac + 3) / 4;
  auto *R = new gb_ref();
  R->l_pac = l_pac;
  R->host.resize((size_t)bytes);
  const bool rd = fseeko(f, 0, SEEK_SET) == 0 && fread(R->host.data(), 1, (size_t)bytes, f) == (size_t)bytes;
  fclose(f);
  if (!rd) {
    delete R;
    gb::set_error("gb_ref_load_pac: short read on %s", path);
    return GB_ERR_ARG;
  }
  *out = R;
  return GB_OK;
}

int gb_ref_info(const gb_ref *ref, int64_t *l_pac) {
  GB_ARG(ref && l_pac, "gb_ref_info: null argument");
  *l_pac = ref->l_pac;
  return GB_OK;
}

int gb_ref_destroy(gb_ref *ref) {
  delete ref;
  return GB_OK;
}

int gb_ref_fetch(const gb_ref *ref, const int64_t *beg, const int64_t *end, int64_t n, uint8_t *out, int64_t out_cap,
                 int64_t *off, int32_t *len) {
  using namespace gbgc;
  GB_ARG(ref && n >= 0 && (n == 0 || (beg && end)) && out_cap >= 0 && (out_cap == 0 || out), "gb_ref_fetch: bad arguments");
  gb_ref *R = const_cast<gb_ref *>(ref);  // the lazy upload is not part of the reference's value
  const int64_t l_pac = R->l_pac;
  std::vector<FetchItem> items;
  std::vector<int64_t> offs((size_t)n);
  int64_t total = 0, t_bytes = 0;
  for (int64_t r = 0; r < n; ++r) {  // bntseq.c:407-423
    int64_t b = beg[r], e = end[r];
    if (e < b) std::swap(b, e);
    e = std::min(e, 2 * l_pac);
    b = std::max<int64_t>(b, 0);
    const int64_t L = (b >= l_pac || e <= l_pac) ? std::max<int64_t>(e - b, 0) : 0;
    GB_ARG(L <= INT32_MAX, "gb_ref_fetch: region %lld is %lld bases long", (long long)r, (long long)L);
    offs[(size_t)r] = total;
    total += L;
    if (L == 0) continue;
    FetchItem it;
    const bool rev = b >= l_pac;
    it.src = rev ? 2 * l_pac - 1 - b : b;  // reverse strand: out[i] = 3 - pac[2 l_pac - 1 - b - i]
    it.t_dst = t_bytes;
    it.q_src = 0;
    it.q_dst = -1;
    it.len = (int32_t)L;
    it.qlen = 0;
    it.flags = rev ? (kComplement | kBackward) : 0;
    it.pad = 0;
    t_bytes += round_up(L, 16);
    items.push_back(it);
  }
  for (int64_t r = 0; r < n; ++r) {
    if (off) off[r] = offs[(size_t)r];
    if (len) len[r] = (int32_t)((r + 1 < n ? offs[(size_t)r + 1] : total) - offs[(size_t)r]);
  }
  GB_ARG(total <= out_cap, "gb_ref_fetch: out_cap %lld is below the %lld bases of this call", (long long)out_cap,
         (long long)total);
  if (items.empty()) return GB_OK;

  int dev = 0, st;
  GB_HIP(hipGetDevice(&dev));
  if ((st = ensure_device(R, dev))) return st;
  gbbswg::Ws *W = nullptr;
  GWs *G = nullptr;
  if ((st = gbbswg::get_ws(dev, &W))) return st;
  if ((st = get_gws(dev, &G))) return st;
  if ((st = G->d_tgt.reserve((size_t)t_bytes))) return st;
  if ((st = launch_fetch(W->stream, G, R, items, nullptr))) return st;
  GB_HIP(hipStreamSynchronize(W->stream));
  std::vector<uint8_t> staged((size_t)t_bytes);
  GB_HIP(gb::memcpy_big(staged.data(), G->d_tgt, (size_t)t_bytes, hipMemcpyDeviceToHost));
  int64_t at = 0;
  for (const FetchItem &it : items) {  // region order; empty regions own no bytes
    std::memcpy(out + at, staged.data() + it.t_dst, (size_t)it.len);
    at += it.len;
  }
  return GB_OK;
}

int gb_bsw_gen_cigar(const gb_bsw_params *params, const gb_ref *ref, gb_bsw_cpair *pairs, int64_t n, const uint8_t *qer,
                     int64_t qer_bytes, uint32_t *cigar, int64_t cigar_cap, int64_t *cigar_used, char *md, int64_t md_cap,
                     int64_t *md_used) {
  using namespace gbgc;
  gb::Range range_("gb.bsw.gen_cigar");
  const char *who = "gb_bsw_gen_cigar";
  int st = validate(who, params, ref, pairs, n, qer, qer_bytes, cigar, cigar_cap, md, md_cap);
  if (st) return st;
  if (cigar_used) *cigar_used = 0;
  if (md_used) *md_used = 0;
  if (n == 0) return GB_OK;
  reset_timing();
  std::vector<uint32_t> cig;
  std::vector<char> mdv;
  if ((st = run_core(who, params, const_cast<gb_ref *>(ref), pairs, n, qer, qer_bytes, cigar != nullptr, md != nullptr, cig,
                     mdv)))
    return st;
  return deliver(who, cig, mdv, cigar, cigar_cap, cigar_used, md, md_cap, md_used);
}

int gb_bsw_gen_cigar_retry(const gb_bsw_params *params, const gb_ref *ref, gb_bsw_cpair *pairs, int64_t n,
                           const uint8_t *qer, int64_t qer_bytes, const int32_t *truesc, uint32_t *cigar, int64_t cigar_cap,
                           int64_t *cigar_used, char *md, int64_t md_cap, int64_t *md_used, int32_t *tries) {
  using namespace gbgc;
  gb::Range range_("gb.bsw.gen_cigar_retry");
  const char *who = "gb_bsw_gen_cigar_retry";
  int st = validate(who, params, ref, pairs, n, qer, qer_bytes, cigar, cigar_cap, md, md_cap);
  if (st) return st;
  GB_ARG(n == 0 || truesc, "%s: null truesc", who);
  GB_ARG(params->w >= 0 && params->w < (1 << 28), "%s: params->w = %d must lie in [0, 2^28)", who, params->w);
  if (cigar_used) *cigar_used = 0;
  if (md_used) *md_used = 0;
  if (n == 0) return GB_OK;
  reset_timing();
  gb_ref *R = const_cast<gb_ref *>(ref);
  const int w_cap = params->w << 2, a = params->mat[0];

  // bwamem.c:1154-1163, one round per try over the pairs still open
  struct Final {
    int round = 0;
    gb_bsw_cpair r;
  };
  std::vector<Final> fin((size_t)n);
  std::vector<int32_t> last_sc((size_t)n, -(1 << 30)), n_try((size_t)n, 0);
  std::vector<int64_t> open((size_t)n);
  for (int64_t p = 0; p < n; ++p) open[(size_t)p] = p;
  std::vector<uint32_t> cig[3];
  std::vector<char> mdv[3];
  std::vector<gb_bsw_cpair> sub;
  for (int round = 0; round < 3 && !open.empty(); ++round) {
    sub.clear();
    for (int64_t p : open) {
      gb_bsw_cpair s = round == 0 ? pairs[p] : fin[(size_t)p].r;
      if (round == 0) s.w = std::min(s.w, w_cap);
      sub.push_back(s);
    }
    if ((st = run_core(who, params, R, sub.data(), (int64_t)sub.size(), qer, qer_bytes, cigar != nullptr, md != nullptr,
                       cig[round], mdv[round])))
      return st;
    std::vector<int64_t> next;
    for (size_t k = 0; k < open.size(); ++k) {
      const int64_t p = open[k];
      Final &f = fin[(size_t)p];
      f.round = round;
      f.r = sub[k];
      n_try[(size_t)p] = round + 1;
      const gb_bsw_cpair &s = sub[k];
      if (rejected(R->l_pac, s.rb, s.re)) continue;
      if (s.score == last_sc[(size_t)p] || s.w == w_cap) continue;
      last_sc[(size_t)p] = s.score;
      if (round + 1 < 3 && s.score < truesc[p] - a) {
        f.r.w = std::min(s.w << 1, w_cap);
        next.push_back(p);
      }
    }
    open.swap(next);
  }

  std::vector<uint32_t> out_cig;
  std::vector<char> out_md;
  for (int64_t p = 0; p < n; ++p) {
    const Final &f = fin[(size_t)p];
    gb_bsw_cpair &s = pairs[p];
    const gb_bsw_cpair &r = f.r;
    s.w = r.w;
    s.score = r.score, s.n_cigar = r.n_cigar, s.nm = r.nm, s.md_len = r.md_len;
    s.cigar_off = cigar ? (int64_t)out_cig.size() : 0;
    s.md_off = md ? (int64_t)out_md.size() : 0;
    const auto &c = cig[f.round];
    const auto &m = mdv[f.round];
    out_cig.insert(out_cig.end(), c.begin() + r.cigar_off, c.begin() + r.cigar_off + r.n_cigar);
    out_md.insert(out_md.end(), m.begin() + r.md_off, m.begin() + r.md_off + r.md_len);
    if (tries) tries[p] = n_try[(size_t)p];
  }
  return deliver(who, out_cig, out_md, cigar, cigar_cap, cigar_used, md, md_cap, md_used);
}

int gb_bsw_gen_cigar_timing(float *fetch_ms, float *fill_ms, float *walk_ms, float *md_ms) {
  GB_ARG(fetch_ms && fill_ms && walk_ms && md_ms, "gb_bsw_gen_cigar_timing: null argument");
  const gbgc::GWs *G = nullptr;
  if (const int st = gb::ran_ws("gb_bsw_gen_cigar_timing", "gb_bsw_gen_cigar", &G)) return st;
  *fetch_ms = G->fetch_ms;
  *fill_ms = G->fill_ms;
  *walk_ms = G->walk_ms;
  *md_ms = G->md_ms;
  return GB_OK;
}

}  // extern "C"
