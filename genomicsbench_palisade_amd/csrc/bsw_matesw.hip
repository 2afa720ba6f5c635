// bsw_matesw.hip -- MI355X (gfx950): mate rescue on the device-resident packed reference, bwa's mem_pestat
// (tools/bwa/bwamem_pair.c:46-109) and the rescue loop of mem_sam_pe (:265-276) around mem_matesw (:111-180):
// kernels, host bookkeeping and C ABI.
//
// A task is (pair, side): the anchors of read i looking for read !i. A side reads and writes only the
// mate's region list, and its anchors come from a snapshot taken before any rescue, so the two sides of a
// pair and all pairs are independent; within a side the calls are sequential, because a call's skip test
// reads the regions earlier calls rescued. Round j therefore serves anchor j of every task that has one:
//   host: the skip test per task, one request (anchor rb, anchor rid, orientation, mate) per orientation
//     that is not skipped, written into page-locked staging;
//   window kernel, one lane per request: the window of bwamem_pair.c:137-145, bns_fetch_seq's clip to the
//     contig (or its reverse-strand mirror) that holds the window's middle, the rid and length tests. It
//     writes {rb, re, run} and the local kernel's descriptor; a request that does not run gets a target of
//     0 rows, which the local kernel answers without reading a target byte;
//   fetch kernel, one wave per request: the window's bases in bns_get_seq's form into the request's slot
//     (a fixed stride, 16-byte aligned);
//   the local DP of bsw_local.hip on those bytes, unchanged, through gbbswl::run_resident; the query is the
//     mate or its reverse complement, both resident since the call began;
//   region kernel, one lane per request: bwamem_pair.c:153-163;
//   one copy of the results back, and on the host per task and orientation the sorted insertion and
//     mem_sort_dedup_patch without mem_patch_reg (the per-read routine of bsw_regs_internal.h).
// The kernels are plain grids: no device-wide atomics but the DP's work counter, no loop whose trip
// count depends on another lane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <vector>

#include "../../include/gb_bsw.h"
#include "bsw_local_internal.h"
#include "bsw_matesw_internal.h"
#include "bsw_ref_internal.h"
#include "bsw_regs_internal.h"
#include "gb_common.h"

static_assert(sizeof(struct gb_bsw_pestat) == 32, "gb_bsw_pestat is 32 bytes (include/gb_bsw.h)");
static_assert(sizeof(gbms::Req) == 24 && sizeof(gbms::Out) == 40, "request and result records");

namespace gbms {

typedef gb_bsw_alnreg Reg;

constexpr int kMaxPenalty = 32768;
constexpr int kFetchWaves = 4;
constexpr int64_t kSlotBytes = 256ll << 20;  // windows of one chunk; GB_BSW_MATESW_CHUNK overrides
constexpr int64_t kMaxChunk = int64_t(1) << 20;

// mem_infer_dir: the orientation of a pair from its two rb, and the distance on read 1's strand
__host__ __device__ inline int infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t *dist) {
  const bool r1 = b1 >= l_pac, r2 = b2 >= l_pac;
  const int64_t p2 = r1 == r2 ? b2 : 2 * l_pac - 1 - b2;
  *dist = p2 > b1 ? p2 - b1 : b1 - p2;
  return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}

// ---- device ---------------------------------------------------------------------------------------

struct Win {  // 24 B
  int64_t rb, re;
  int32_t run, pad;
};

struct DevArgs {
  const Req *req;
  int64_t m;
  const int64_t *contig_end;  // n_contigs cumulative ends, the last l_pac
  int64_t n_contigs, l_pac;
  const int64_t *q_off;  // per read: its query in the query buffer; the reverse complement lies rev_base on
  const int32_t *l_query;
  int64_t rev_base, stride;
  int32_t low[4], high[4];
  int32_t min_seed_len, a;
  Win *win;
  gbbswl::Pair *pairs;
  const uint32_t *pac;
  int64_t n_words;
  uint8_t *tgt;
  const int32_t *out8;
  Out *out;
};

__global__ __launch_bounds__(256) void bsw_matesw_window_kernel(DevArgs A) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= A.m) return;
  const Req q = A.req[k];
  const int l_ms = A.l_query[q.read];
  const int r = q.r & 3;
  const bool is_rev = (r >> 1) != (r & 1), is_larger = !(r >> 1);
  // the mate lies low .. high beyond the anchor, or as far before it; a mate on the anchor's strand
  // ends l_ms later, one on the other strand starts l_ms earlier (in the doubled space)
  const int64_t near = is_larger ? A.low[r] : -(int64_t)A.high[r], far = is_larger ? A.high[r] : -(int64_t)A.low[r];
  int64_t rb = q.rb + near - (is_rev ? l_ms : 0), re = q.rb + far + (is_rev ? 0 : l_ms);
  rb = rb > 0 ? rb : 0;
  re = re < 2 * A.l_pac ? re : 2 * A.l_pac;
  int run = 0;
  if (rb < re) {
    const int64_t mid = (rb + re) >> 1;
    const bool rev = mid >= A.l_pac;
    const int64_t pos_f = rev ? 2 * A.l_pac - 1 - mid : mid;
    int64_t lo = 0, hi = A.n_contigs - 1;  // the first contig that ends beyond pos_f
    while (lo < hi) {
      const int64_t c = (lo + hi) >> 1;
      if (A.contig_end[c] > pos_f) hi = c;
      else lo = c + 1;
    }
    int64_t far_beg = lo ? A.contig_end[lo - 1] : 0, far_end = A.contig_end[lo];
    if (rev) {
      const int64_t t = far_beg;
      far_beg = 2 * A.l_pac - far_end;
      far_end = 2 * A.l_pac - t;
    }
    rb = rb > far_beg ? rb : far_beg;
    re = re < far_end ? re : far_end;
    // a window longer than its slot cannot pass the call's validation; it is not fetched in any case
    run = q.rid == (int32_t)lo && re - rb >= A.min_seed_len && re - rb <= A.stride;
  }
  A.win[k] = Win{rb, re, run, 0};
  const int xtra = GB_KSW_XSUBO | GB_KSW_XSTART | (l_ms * A.a < 250 ? GB_KSW_XBYTE : 0) | (A.min_seed_len * A.a);
  A.pairs[k] = gbbswl::Pair{k * A.stride, A.q_off[q.read] + (is_rev ? A.rev_base : 0), run ? (int32_t)(re - rb) : 0, l_ms,
                            xtra, 0};
}

__global__ __launch_bounds__(64 * kFetchWaves) void bsw_matesw_fetch_kernel(DevArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * kFetchWaves + (threadIdx.x >> 6);  // wave-uniform
  if (k >= A.m) return;
  const Win w = A.win[k];
  if (!w.run) return;
  const int32_t len = (int32_t)(w.re - w.rb);
  uint8_t *dst = A.tgt + k * A.stride;
  if (w.rb < A.l_pac)
    gbgc::fetch_bases(A.pac, A.n_words, w.rb, len, false, 0u, dst, lane);
  else  // the reverse strand: the complement read backwards (bntseq.c:414-418)
    gbgc::fetch_bases(A.pac, A.n_words, 2 * A.l_pac - 1 - w.rb, len, true, 0xFFFFFFFFu, dst, lane);
}

struct RcArgs {
  const int64_t *q_off;
  const int32_t *l_query;  // 0 for a read whose query was not uploaded
  int64_t n_reads, rev_base;
  uint8_t *qry;
};

// the reverse complement of every uploaded query, code 4 staying 4; one wave per read
__global__ __launch_bounds__(64 * kFetchWaves) void bsw_matesw_revcomp_kernel(RcArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kFetchWaves + (threadIdx.x >> 6);
  if (r >= A.n_reads) return;
  const int l = A.l_query[r];
  const uint8_t *q = A.qry + A.q_off[r];
  uint8_t *d = A.qry + A.rev_base + A.q_off[r];
  for (int i = lane; i < l; i += 64) {
    const uint8_t c = q[l - 1 - i];
    d[i] = c < 4 ? (uint8_t)(3 - c) : (uint8_t)4;
  }
}

__global__ __launch_bounds__(256) void bsw_matesw_region_kernel(DevArgs A) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= A.m) return;
  const Req q = A.req[k];
  const Win w = A.win[k];
  const int32_t *o = A.out8 + 8 * k;  // score, te, qe, score2, te2, tb, qb
  const int l_ms = A.l_query[q.read];
  const int r = q.r & 3;
  const bool is_rev = (r >> 1) != (r & 1);
  Out b = {};
  b.flags = w.run ? 1 : 0;
  if (w.run && o[0] >= A.min_seed_len && o[6] >= 0) {
    // on the other strand the alignment is that of the mate's reverse complement: mirrored back
    b.qb = is_rev ? l_ms - (o[2] + 1) : o[6];
    b.qe = is_rev ? l_ms - o[6] : o[2] + 1;
    b.rb = is_rev ? 2 * A.l_pac - (w.rb + o[1] + 1) : w.rb + o[5];
    b.re = is_rev ? 2 * A.l_pac - (w.rb + o[5]) : w.rb + o[1] + 1;
    b.score = o[0];
    b.csub = o[3];
    const int64_t lr = b.re - b.rb, lq = b.qe - b.qb;
    b.seedcov = (int32_t)((lr < lq ? lr : lq) >> 1);
    b.flags = 3;
  }
  A.out[k] = b;
}

// ---- host bookkeeping -----------------------------------------------------------------------------

// the orientations anchor a need not try: failed, or the mate already has a region at a proper distance
inline int skip_mask(const Rescue &C, const Reg &a, const std::vector<Reg> &ma) {
  int skip = 0;
  for (int r = 0; r < 4; ++r) skip |= (C.pes[r].failed ? 1 : 0) << r;
  for (const Reg &m : ma) {
    int64_t dist;
    const int r = infer_dir(C.l_pac, a.rb, m.rb, &dist);
    if (dist >= C.pes[r].low && dist <= C.pes[r].high) skip |= 1 << r;
  }
  return skip;
}

int rescue_rounds(Rescue &C, Aligner &A) {
  const char *who = "gb_bsw_mate_rescue";
  typedef std::chrono::steady_clock Clock;
  auto t0 = Clock::now();
  auto lap = [&] {
    const auto t = Clock::now();
    C.host_ms += std::chrono::duration<double, std::milli>(t - t0).count();
  };
  const int64_t n_reads = C.n_reads;
  // the anchors of read i: its regions within pen_unpaired of its first one, as they are before any rescue
  std::vector<int64_t> anc_off((size_t)n_reads + 1, 0);
  std::vector<int32_t> anc;
  for (int64_t i = 0; i < n_reads; ++i) {
    const int64_t off = C.reg_off[i], n = C.reg_off[i + 1] - off;
    int32_t got = 0;
    for (int64_t k = 0; k < n && got < C.opt.max_matesw; ++k)
      if (C.regs[off + k].score >= C.regs[off].score - C.opt.pen_unpaired) anc.push_back((int32_t)k), ++got;
    anc_off[(size_t)i + 1] = (int64_t)anc.size();
  }
  C.lists.resize((size_t)n_reads);
  for (int64_t i = 0; i < n_reads; ++i) C.lists[(size_t)i].assign(C.regs + C.reg_off[i], C.regs + C.reg_off[i + 1]);
  C.n_sw.assign((size_t)n_reads, 0);
  std::vector<int64_t> active;  // tasks, named by their anchor read; the mate is read ^ 1
  for (int64_t i = 0; i < n_reads; ++i)
    if (anc_off[(size_t)i + 1] > anc_off[(size_t)i]) active.push_back(i);
  gbrg::Opt dopt;
  std::memset(&dopt, 0, sizeof(dopt));
  dopt.max_chain_gap = C.opt.max_chain_gap, dopt.mask_level = C.opt.mask_level;
  dopt.mask_level_redun = C.opt.mask_level_redun, dopt.l_pac = C.l_pac, dopt.no_patch = 1;
  std::vector<int32_t> mask;
  std::vector<int64_t> base;
  std::vector<Req> req;
  std::vector<Out> out;
  int st = GB_OK, nth0 = 1;
  if ((st = gb::thread_count(who, "GB_BSW_MATESW_THREADS", &nth0))) return st;
  for (int32_t j = 0; !active.empty(); ++j) {
    const int64_t nt = (int64_t)active.size();
    const int nth = nt < 256 ? 1 : nth0;
    mask.resize((size_t)nt), base.resize((size_t)nt + 1);
    auto anchor_of = [&](int64_t i) -> const Reg & { return C.regs[C.reg_off[i] + anc[(size_t)(anc_off[(size_t)i] + j)]]; };
    st = gb::parallel(who, nth, [&](int t) {
      for (int64_t k = nt * t / nth; k < nt * (t + 1) / nth; ++k)
        mask[(size_t)k] = skip_mask(C, anchor_of(active[(size_t)k]), C.lists[(size_t)(active[(size_t)k] ^ 1)]);
    });
    if (st) return st;
    base[0] = 0;
    for (int64_t k = 0; k < nt; ++k) base[(size_t)k + 1] = base[(size_t)k] + (4 - __builtin_popcount(mask[(size_t)k]));
    const int64_t nq = base[(size_t)nt];
    req.resize((size_t)nq), out.resize((size_t)nq);
    st = gb::parallel(who, nth, [&](int t) {
      for (int64_t k = nt * t / nth; k < nt * (t + 1) / nth; ++k) {
        const int64_t i = active[(size_t)k];
        const Reg &a = anchor_of(i);
        int64_t at = base[(size_t)k];
        for (int r = 0; r < 4; ++r)
          if (!(mask[(size_t)k] >> r & 1)) req[(size_t)at++] = Req{a.rb, a.rid, r, (int32_t)(i ^ 1), 0};
      }
    });
    if (st) return st;
    lap();
    if (nq) {
      if ((st = A.run(req.data(), nq, out.data()))) return st;
      ++C.rounds;
      C.requests += nq;
    }
    t0 = Clock::now();
    st = gb::parallel(who, nth, [&](int t) {
      for (int64_t k = nt * t / nth; k < nt * (t + 1) / nth; ++k) {
        const int64_t i = active[(size_t)k];
        const Reg &a = anchor_of(i);
        std::vector<Reg> &ma = C.lists[(size_t)(i ^ 1)];
        int64_t at = base[(size_t)k];
        int n = 0;
        for (int r = 0; r < 4; ++r) {
          if (mask[(size_t)k] >> r & 1) continue;
          const Out &o = out[(size_t)at++];
          if (o.flags & 1) {
            if (o.flags & 2) {
              Reg b;
              std::memset(static_cast<void *>(&b), 0, sizeof(b));
              b.rid = a.rid, b.is_alt = a.is_alt;
              b.rb = o.rb, b.re = o.re, b.qb = o.qb, b.qe = o.qe;
              b.score = o.score, b.csub = o.csub, b.seedcov = o.seedcov;
              b.secondary = -1;
              // before the first of the entries that were there with a strictly smaller score
              size_t pos = 0;
              while (pos < ma.size() && !(ma[pos].score < b.score)) ++pos;
              ma.insert(ma.begin() + (std::ptrdiff_t)pos, b);
            }
            ++n;
          }
          if (n) {  // after every orientation that was tried once an alignment ran, also one that added nothing
            gbrg::State s;
            std::memset(&s, 0, sizeof(s));
            s.n = s.n_out = (int32_t)ma.size();
            gbrg::Request none{};
            gbrg::dedup_read(dopt, nullptr, ma.data(), s, false, 0, 0, &none);
            ma.resize((size_t)s.n_out);
          }
        }
        C.n_sw[(size_t)i] += n;
      }
    });
    if (st) return st;
    // the tasks that have an anchor j + 1
    size_t m = 0;
    for (size_t k = 0; k < active.size(); ++k)
      if (anc_off[(size_t)active[k] + 1] - anc_off[(size_t)active[k]] > j + 1) active[m++] = active[k];
    active.resize(m);
  }
  lap();
  return GB_OK;
}

// ---- device aligner ---------------------------------------------------------------------------------

using gb::round_up;

struct MWs {  // the calling thread's, through gb::thread_ws
  int device = -1;
  gb::Event ev[6];
  gb::PinnedBuf<Req> h_req;
  gb::PinnedBuf<Out> h_out;
  gb::PinnedBuf<uint8_t> h_in;
  gb::DevBuf<Req> d_req;
  gb::DevBuf<Out> d_out;
  gb::DevBuf<Win> d_win;
  gb::DevBuf<gbbswl::Pair> d_pairs;
  gb::DevBuf<int32_t> d_out8;
  gb::DevBuf<uint8_t> d_in, d_qry, d_tgt;
  float fetch_ms = 0.f, dp_ms = 0.f, region_ms = 0.f;
};

struct Timing {
  float fetch_ms, dp_ms, region_ms, host_ms;
  int32_t rounds;
  int64_t requests;
  bool valid;
};

thread_local Timing g_timing = {0.f, 0.f, 0.f, 0.f, 0, 0, false};  // of this thread's last call

int get_ws(int dev, MWs **out) {
  return gb::thread_ws(dev, out, [](int dev, MWs **out) {
    auto *W = new MWs();
    W->device = dev;
    hipError_t e = hipSuccess;
    for (auto &ev : W->ev)
      if (e == hipSuccess) e = ev.create();
    if (e != hipSuccess) {
      gb::set_error("gb_bsw_mate_rescue workspace: %s", hipGetErrorString(e));
      delete W;
      return GB_ERR_HIP;
    }
    *out = W;
    return GB_OK;
  });
}

struct DevAligner : Aligner {
  const Rescue *C = nullptr;
  gb_bsw_params dp;  // mat from params, the gap penalties from opt
  int max_mat = 1;
  gb_ref *R = nullptr;
  const int64_t *contig_end = nullptr;
  int64_t n_contigs = 0;
  const uint8_t *qer = nullptr;
  const int64_t *idq = nullptr;
  const int32_t *l_query = nullptr;
  int64_t max_win = 0;  // the longest window an open orientation can give
  // set at the first round
  MWs *W = nullptr;
  gbbswl::Ws *L = nullptr;
  DevArgs D{};
  int64_t chunk = 0;

  int begin() {  // the device, the reference, and the call's tables: queries, their reverse complements, contig ends
    const int64_t n_reads = C->n_reads;
    int dev = 0, st;
    GB_HIP(hipGetDevice(&dev));
    if ((st = get_ws(dev, &W))) return st;
    if ((st = gbbswl::get_ws(dev, &L))) return st;
    if ((st = gbgc::ensure_device(R, dev))) return st;
    W->fetch_ms = W->dp_ms = W->region_ms = 0.f;
    // one staging block: q_off (8 B per read), l_query (4 B), contig ends, the query bytes
    const int64_t o_qoff = 0, o_lq = o_qoff + round_up(n_reads * 8, 16), o_ce = o_lq + round_up(n_reads * 4, 16);
    const int64_t nc = contig_end ? n_contigs : 1;
    const int64_t o_q = o_ce + round_up(nc * 8, 16);
    int64_t q_half = 0;
    for (int64_t r = 0; r < n_reads; ++r)
      if (C->reg_off[(r ^ 1) + 1] > C->reg_off[r ^ 1]) q_half += round_up<int64_t>(l_query[r], 4);
    q_half = round_up(std::max<int64_t>(q_half, 1), 16);
    const int64_t bytes = o_q + q_half;
    if ((st = W->h_in.reserve((size_t)bytes, (size_t)bytes * 2))) return st;
    if ((st = W->d_in.reserve((size_t)bytes, (size_t)bytes * 2))) return st;
    if ((st = W->d_qry.reserve((size_t)(2 * q_half)))) return st;
    uint8_t *h = W->h_in;
    std::memset(h, 0, (size_t)bytes);
    auto *hq = reinterpret_cast<int64_t *>(h + o_qoff);
    auto *hl = reinterpret_cast<int32_t *>(h + o_lq);
    auto *hc = reinterpret_cast<int64_t *>(h + o_ce);
    int64_t qo = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
      hq[r] = 0, hl[r] = 0;
      if (C->reg_off[(r ^ 1) + 1] == C->reg_off[r ^ 1]) continue;  // nobody looks for this read
      hq[r] = qo, hl[r] = l_query[r];
      std::memcpy(h + o_q + qo, qer + idq[r], (size_t)l_query[r]);
      qo += round_up<int64_t>(l_query[r], 4);
    }
    if (contig_end)
      std::memcpy(hc, contig_end, (size_t)nc * 8);
    else
      hc[0] = C->l_pac;
    uint8_t *d = W->d_in;
    GB_HIP(hipMemcpyAsync(d, h, (size_t)bytes, hipMemcpyHostToDevice, L->stream));
    GB_HIP(hipMemcpyAsync(W->d_qry, d + o_q, (size_t)q_half, hipMemcpyDeviceToDevice, L->stream));
    RcArgs Rc{reinterpret_cast<const int64_t *>(d + o_qoff), reinterpret_cast<const int32_t *>(d + o_lq), n_reads, q_half,
              W->d_qry};
    GB_HIP(hipEventRecord(W->ev[4], L->stream));
    hipLaunchKernelGGL(bsw_matesw_revcomp_kernel, dim3((unsigned)((n_reads + kFetchWaves - 1) / kFetchWaves)),
                       dim3(64 * kFetchWaves), 0, L->stream, Rc);
    GB_HIP(hipGetLastError());
    GB_HIP(hipEventRecord(W->ev[5], L->stream));
    GB_HIP(hipStreamSynchronize(L->stream));
    float ms = 0.f;
    GB_HIP(hipEventElapsedTime(&ms, W->ev[4], W->ev[5]));
    W->fetch_ms += ms;
    D.contig_end = reinterpret_cast<const int64_t *>(d + o_ce);
    D.n_contigs = nc;
    D.l_pac = C->l_pac;
    D.q_off = Rc.q_off;
    D.l_query = Rc.l_query;
    D.rev_base = q_half;
    D.stride = round_up(std::max<int64_t>(max_win, 1), 16);
    for (int r = 0; r < 4; ++r) D.low[r] = C->pes[r].low, D.high[r] = C->pes[r].high;
    D.min_seed_len = C->opt.min_seed_len;
    D.a = C->opt.a;
    D.pac = R->d_pac;
    D.n_words = R->n_words;
    chunk = std::max<int64_t>(1, std::min(kMaxChunk, kSlotBytes / D.stride));
    if (const char *e = getenv("GB_BSW_MATESW_CHUNK")) chunk = std::max<int64_t>(1, std::min<int64_t>(atoll(e), kMaxChunk));
    return GB_OK;
  }

  int run(const Req *req, int64_t n, Out *out) override {
    int st;
    if (!W && (st = begin())) return st;
    for (int64_t lo = 0; lo < n; lo += chunk) {
      const int64_t m = std::min(chunk, n - lo);
      if ((st = W->h_req.reserve((size_t)m, (size_t)m * 2))) return st;
      if ((st = W->h_out.reserve((size_t)m, (size_t)m * 2))) return st;
      if ((st = W->d_req.reserve((size_t)m, (size_t)m * 2))) return st;
      if ((st = W->d_out.reserve((size_t)m, (size_t)m * 2))) return st;
      if ((st = W->d_win.reserve((size_t)m, (size_t)m * 2))) return st;
      if ((st = W->d_pairs.reserve((size_t)m, (size_t)m * 2))) return st;
      if ((st = W->d_out8.reserve((size_t)m * 8, (size_t)m * 16))) return st;
      // the slots are the one large buffer: no room beyond the chunk's, so that they stay under the byte budget
      if ((st = W->d_tgt.reserve((size_t)(m * D.stride + 16)))) return st;
      std::memcpy(static_cast<void *>(W->h_req.get()), req + lo, (size_t)m * sizeof(Req));
      hipStream_t s = L->stream;
      GB_HIP(hipMemcpyAsync(W->d_req, W->h_req, (size_t)m * sizeof(Req), hipMemcpyHostToDevice, s));
      DevArgs A = D;
      A.req = W->d_req;
      A.m = m;
      A.win = W->d_win;
      A.pairs = W->d_pairs;
      A.tgt = W->d_tgt;
      A.out8 = W->d_out8;
      A.out = W->d_out;
      GB_HIP(hipEventRecord(W->ev[0], s));
      hipLaunchKernelGGL(bsw_matesw_window_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, A);
      GB_HIP(hipGetLastError());
      hipLaunchKernelGGL(bsw_matesw_fetch_kernel, dim3((unsigned)((m + kFetchWaves - 1) / kFetchWaves)),
                         dim3(64 * kFetchWaves), 0, s, A);
      GB_HIP(hipGetLastError());
      GB_HIP(hipEventRecord(W->ev[1], s));
      if ((st = gbbswl::run_resident(L, &dp, max_mat, W->d_pairs, m, W->d_tgt, W->d_qry, W->d_out8,
                                     gbbswl::list_entries((int)D.stride), nullptr, nullptr)))
        return st;
      GB_HIP(hipEventRecord(W->ev[2], s));
      hipLaunchKernelGGL(bsw_matesw_region_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, A);
      GB_HIP(hipGetLastError());
      GB_HIP(hipEventRecord(W->ev[3], s));
      GB_HIP(hipMemcpyAsync(W->h_out, W->d_out, (size_t)m * sizeof(Out), hipMemcpyDeviceToHost, s));
      GB_HIP(hipStreamSynchronize(s));
      std::memcpy(static_cast<void *>(out + lo), W->h_out.get(), (size_t)m * sizeof(Out));
      float ms = 0.f;
      GB_HIP(hipEventElapsedTime(&ms, W->ev[0], W->ev[1]));
      W->fetch_ms += ms;
      GB_HIP(hipEventElapsedTime(&ms, W->ev[1], W->ev[2]));
      W->dp_ms += ms;
      GB_HIP(hipEventElapsedTime(&ms, W->ev[2], W->ev[3]));
      W->region_ms += ms;
    }
    return GB_OK;
  }
};

// ---- mem_pestat -------------------------------------------------------------------------------------

// cal_sub: the score of the first later region that overlaps the best one's query interval by mask_level of
// the shorter of the two, or min_seed_len * a
int cal_sub(const gb_bsw_pe_opt &o, const Reg *a, int64_t n) {
  int64_t j;
  for (j = 1; j < n; ++j) {
    const int b_max = std::max(a[j].qb, a[0].qb), e_min = std::min(a[j].qe, a[0].qe);
    if (e_min > b_max) {
      const int min_l = std::min(a[j].qe - a[j].qb, a[0].qe - a[0].qb);
      if ((float)(e_min - b_max) >= (float)min_l * o.mask_level) break;
    }
  }
  return j < n ? a[j].score : o.min_seed_len * o.a;
}

inline int round499(double x) { return (int)(x + .499); }

int pestat_impl(const gb_bsw_pe_opt *opt, int64_t l_pac, int64_t n_reads, const int64_t *reg_off, const Reg *regs,
                struct gb_bsw_pestat pes[4]) {
  const char *who = "gb_bsw_pestat";
  GB_ARG(opt && pes, "%s: null opt or pes", who);
  GB_ARG(n_reads >= 0 && n_reads % 2 == 0 && n_reads < (1ll << 31), "%s: n_reads = %lld (an even number of reads)", who,
         (long long)n_reads);
  GB_ARG(l_pac >= 1, "%s: l_pac = %lld", who, (long long)l_pac);
  GB_ARG(std::isfinite(opt->mask_level), "%s: mask_level is not finite", who);
  GB_ARG(n_reads == 0 || reg_off, "%s: null reg_off", who);
  if (n_reads) GB_ARG(reg_off[0] == 0, "%s: reg_off[0] = %lld", who, (long long)reg_off[0]);
  for (int64_t r = 0; r < n_reads; ++r)
    GB_ARG(reg_off[r + 1] >= reg_off[r], "%s: read %lld: reg_off decreases (%lld after %lld)", who, (long long)r,
           (long long)reg_off[r + 1], (long long)reg_off[r]);
  GB_ARG(n_reads == 0 || reg_off[n_reads] == 0 || regs, "%s: null regs", who);
  std::vector<uint64_t> isize[4];
  for (int64_t p = 0; p < n_reads / 2; ++p) {
    const Reg *a0 = regs + reg_off[2 * p], *a1 = regs + reg_off[2 * p + 1];
    const int64_t n0 = reg_off[2 * p + 1] - reg_off[2 * p], n1 = reg_off[2 * p + 2] - reg_off[2 * p + 1];
    if (n0 == 0 || n1 == 0) continue;
    if ((double)cal_sub(*opt, a0, n0) > 0.8 * a0[0].score) continue;  // MIN_RATIO: a unique hit
    if ((double)cal_sub(*opt, a1, n1) > 0.8 * a1[0].score) continue;
    if (a0[0].rid != a1[0].rid) continue;
    int64_t is;
    const int dir = infer_dir(l_pac, a0[0].rb, a1[0].rb, &is);
    if (is && is <= opt->max_ins) isize[dir].push_back((uint64_t)is);
  }
  struct gb_bsw_pestat out[4];
  std::memset(out, 0, sizeof(out));
  for (int d = 0; d < 4; ++d) {
    struct gb_bsw_pestat &r = out[d];
    std::vector<uint64_t> &q = isize[d];
    const size_t n = q.size();
    if (n < 10) {  // MIN_DIR_CNT
      r.failed = 1;
      continue;
    }
    std::sort(q.begin(), q.end());  // values only: any sort gives the reference's array
    const int p25 = (int)q[(size_t)(int)(.25 * n + .499)], p50 = (int)q[(size_t)(int)(.50 * n + .499)],
              p75 = (int)q[(size_t)(int)(.75 * n + .499)];
    (void)p50;
    r.low = round499(p25 - 2.0 * (p75 - p25));  // OUTLIER_BOUND
    if (r.low < 1) r.low = 1;
    r.high = round499(p75 + 2.0 * (p75 - p25));
    // the reference compares its unsigned sizes with these ints: the ints are converted
    const uint64_t lo = (uint64_t)(int64_t)r.low, hi = (uint64_t)(int64_t)r.high;
    int x = 0;
    r.avg = 0;
    for (size_t i = 0; i < n; ++i)
      if (q[i] >= lo && q[i] <= hi) r.avg += (double)q[i], ++x;
    r.avg /= x;
    r.std = 0;
    for (size_t i = 0; i < n; ++i)
      if (q[i] >= lo && q[i] <= hi) r.std += ((double)q[i] - r.avg) * ((double)q[i] - r.avg);
    r.std = std::sqrt(r.std / x);
    r.low = round499(p25 - 3.0 * (p75 - p25));  // MAPPING_BOUND
    r.high = round499(p75 + 3.0 * (p75 - p25));
    if (r.low > r.avg - 4.0 * r.std) r.low = round499(r.avg - 4.0 * r.std);  // MAX_STDDEV
    if (r.high < r.avg + 4.0 * r.std) r.high = round499(r.avg + 4.0 * r.std);
    if (r.low < 1) r.low = 1;
  }
  size_t mx = 0;
  for (int d = 0; d < 4; ++d) mx = std::max(mx, isize[d].size());
  for (int d = 0; d < 4; ++d)
    if (!out[d].failed && (double)isize[d].size() < (int)mx * 0.05) out[d].failed = 1;  // MIN_DIR_RATIO
  std::memcpy(pes, out, sizeof(out));
  return GB_OK;
}

// ---- the call -----------------------------------------------------------------------------------------

int rescue_impl(const gb_bsw_params *params, const gb_bsw_pe_opt *opt, const struct gb_bsw_pestat *pes, const gb_ref *ref,
                const int64_t *contig_end, int64_t n_contigs, const uint8_t *qer, int64_t qer_bytes, int64_t n_pairs,
                const int64_t *idq, const int32_t *l_query, const int64_t *reg_off, const Reg *regs, Reg *out_regs,
                int64_t out_cap, int64_t *out_off, int32_t *n_out, int32_t *n_sw, int64_t *out_used) {
  const char *who = "gb_bsw_mate_rescue";
  GB_ARG(params && opt && pes && ref, "%s: null params, opt, pes or ref", who);
  GB_ARG(n_pairs >= 0 && n_pairs < (1ll << 30), "%s: n_pairs = %lld", who, (long long)n_pairs);
  GB_ARG(n_contigs >= 1 && n_contigs < (1ll << 31), "%s: n_contigs = %lld", who, (long long)n_contigs);
  GB_ARG(qer_bytes >= 0 && (qer_bytes == 0 || qer), "%s: bad sequence buffer", who);
  GB_ARG(out_cap >= 0 && (out_cap == 0 || out_regs), "%s: bad region buffer", who);
  GB_ARG(opt->min_seed_len >= 1, "%s: min_seed_len = %d (need >= 1)", who, opt->min_seed_len);
  GB_ARG(opt->max_matesw >= 0, "%s: max_matesw = %d (need >= 0)", who, opt->max_matesw);
  GB_ARG(opt->pen_unpaired >= 0, "%s: pen_unpaired = %d (need >= 0)", who, opt->pen_unpaired);
  GB_ARG(opt->a >= 1 && (int64_t)opt->min_seed_len * opt->a <= 0xffff,
         "%s: a = %d, min_seed_len = %d (need a >= 1 and min_seed_len * a in 16 bits)", who, opt->a, opt->min_seed_len);
  GB_ARG(opt->max_chain_gap >= 0, "%s: max_chain_gap = %d", who, opt->max_chain_gap);
  GB_ARG(std::isfinite(opt->mask_level_redun), "%s: mask_level_redun is not finite", who);
  const int pen[4] = {opt->o_del, opt->e_del, opt->o_ins, opt->e_ins};
  GB_ARG(pen[0] >= 0 && pen[1] >= 0 && pen[2] >= 0 && pen[3] >= 0 && (int64_t)pen[0] + pen[1] < kMaxPenalty &&
             (int64_t)pen[2] + pen[3] < kMaxPenalty,
         "%s: gap penalties (o_del %d, e_del %d, o_ins %d, e_ins %d) must be >= 0 with o + e < %d", who, pen[0], pen[1],
         pen[2], pen[3], kMaxPenalty);
  int mx = params->mat[0], mn = params->mat[0];
  for (int k = 1; k < 25; ++k) mx = std::max<int>(mx, params->mat[k]), mn = std::min<int>(mn, params->mat[k]);
  GB_ARG(mx >= 1 && mn <= 0, "%s: the scoring matrix has max %d, min %d (need max >= 1, min <= 0)", who, mx, mn);
  const int64_t l_pac = ref->l_pac;
  if (contig_end) {
    for (int64_t k = 0; k < n_contigs; ++k)
      GB_ARG(contig_end[k] > (k ? contig_end[k - 1] : 0), "%s: contig_end[%lld] does not increase", who, (long long)k);
    GB_ARG(contig_end[n_contigs - 1] == l_pac, "%s: contig_end ends at %lld, l_pac is %lld", who,
           (long long)contig_end[n_contigs - 1], (long long)l_pac);
  }
  if (n_pairs == 0) {
    g_timing = Timing{0.f, 0.f, 0.f, 0.f, 0, 0, true};
    if (out_used) *out_used = 0;
    return GB_OK;
  }
  const int64_t n_reads = 2 * n_pairs;
  GB_ARG(idq && l_query && reg_off && out_off && n_out, "%s: null idq, l_query, reg_off, out_off or n_out", who);
  GB_ARG(reg_off[0] == 0, "%s: reg_off[0] = %lld", who, (long long)reg_off[0]);
  for (int64_t r = 0; r < n_reads; ++r) {
    GB_ARG(reg_off[r + 1] >= reg_off[r], "%s: read %lld: reg_off decreases (%lld after %lld)", who, (long long)r,
           (long long)reg_off[r + 1], (long long)reg_off[r]);
    GB_ARG(reg_off[r + 1] < (1ll << 31), "%s: read %lld: %lld regions (the call takes fewer than 2^31)", who, (long long)r,
           (long long)reg_off[r + 1]);
  }
  GB_ARG(reg_off[n_reads] == 0 || regs, "%s: null regs", who);
  int max_lms = 0;
  for (int64_t r = 0; r < n_reads; ++r) {
    const bool has = reg_off[r + 1] > reg_off[r], sought = reg_off[(r ^ 1) + 1] > reg_off[r ^ 1];
    if (!has && !sought) continue;
    const int lq = l_query[r];
    const long long rr = (long long)r;
    GB_ARG(lq >= 1 && lq <= GB_BSW_MAX_QLEN, "%s: read %lld: l_query = %d (need [1, %d])", who, rr, lq, GB_BSW_MAX_QLEN);
    GB_ARG(idq[r] >= 0 && idq[r] <= qer_bytes - lq, "%s: read %lld has its query outside the sequence buffer", who, rr);
    if (sought) {
      max_lms = std::max(max_lms, lq);
      if ((int64_t)lq * opt->a < 250) {  // the alignment will carry GB_KSW_XBYTE
        GB_ARG(pen[0] + pen[1] <= 255 && pen[2] + pen[3] <= 255,
               "%s: read %lld would be aligned with KSW_XBYTE and gap penalties o + e above 255", who, rr);
        GB_ARG(lq * mx - mn < 255,
               "%s: read %lld would be aligned with KSW_XBYTE and l_query * max(mat) - min(mat) = %d (need < 255)", who, rr,
               lq * mx - mn);
      }
    }
    for (int64_t k = reg_off[r]; k < reg_off[r + 1]; ++k) {
      const Reg &g = regs[k];
      const long long kk = (long long)(k - reg_off[r]);
      GB_ARG(g.qb >= 0 && g.qb < g.qe && g.qe <= lq, "%s: read %lld region %lld: [qb, qe) = [%d, %d), l_query = %d", who, rr,
             kk, g.qb, g.qe, lq);
      GB_ARG(g.rb >= 0 && g.rb < g.re && g.re <= 2 * l_pac && !(g.rb < l_pac && g.re > l_pac),
             "%s: read %lld region %lld: [rb, re) = [%lld, %lld) with l_pac = %lld", who, rr, kk, (long long)g.rb,
             (long long)g.re, (long long)l_pac);
      GB_ARG(g.rid >= 0 && g.rid < n_contigs, "%s: read %lld region %lld: rid = %d outside [0, %lld)", who, rr, kk, g.rid,
             (long long)n_contigs);
      GB_ARG(g.score >= 1, "%s: read %lld region %lld: score = %d", who, rr, kk, g.score);
      GB_ARG(g.seedcov >= 1, "%s: read %lld region %lld: seedcov = %d", who, rr, kk, g.seedcov);
      GB_ARG(g.w >= 0 && g.w < (1 << 28), "%s: read %lld region %lld: w = %d outside [0, 2^28)", who, rr, kk, g.w);
      GB_ARG(g.sub >= 0 && g.csub >= 0 && g.sub_n >= 0, "%s: read %lld region %lld: sub = %d, csub = %d, sub_n = %d", who, rr,
             kk, g.sub, g.csub, g.sub_n);
    }
  }
  int64_t max_win = 0;
  for (int r = 0; r < 4; ++r) {
    if (pes[r].failed) continue;
    GB_ARG(pes[r].low >= 0 && pes[r].high >= pes[r].low, "%s: orientation %d: low = %d, high = %d", who, r, pes[r].low,
           pes[r].high);
    GB_ARG((int64_t)pes[r].high - pes[r].low + max_lms <= GB_BSW_LOCAL_MAX_TLEN,
           "%s: orientation %d: a window of high - low + the longest mate = %lld bases (at most %d)", who, r,
           (long long)((int64_t)pes[r].high - pes[r].low + max_lms), GB_BSW_LOCAL_MAX_TLEN);
    max_win = std::max<int64_t>(max_win, (int64_t)pes[r].high - pes[r].low + max_lms);
  }

  int nth = 1;
  if (gb::thread_count(who, "GB_BSW_MATESW_THREADS", &nth)) return GB_ERR_ARG;  // refused here, before any device work
  g_timing = Timing{0.f, 0.f, 0.f, 0.f, 0, 0, true};
  Rescue C;
  C.opt = *opt;
  std::memcpy(C.pes, pes, sizeof(C.pes));
  C.l_pac = l_pac, C.n_reads = n_reads, C.reg_off = reg_off, C.regs = regs;
  DevAligner A;
  A.C = &C;
  A.dp = *params;
  A.dp.o_del = opt->o_del, A.dp.e_del = opt->e_del, A.dp.o_ins = opt->o_ins, A.dp.e_ins = opt->e_ins;
  A.max_mat = mx;
  A.R = const_cast<gb_ref *>(ref);
  A.contig_end = contig_end, A.n_contigs = n_contigs;
  A.qer = qer, A.idq = idq, A.l_query = l_query;
  A.max_win = max_win;
  int st;
  if ((st = rescue_rounds(C, A))) return st;
  if (A.W) g_timing.fetch_ms = A.W->fetch_ms, g_timing.dp_ms = A.W->dp_ms, g_timing.region_ms = A.W->region_ms;
  g_timing.host_ms = (float)C.host_ms, g_timing.rounds = C.rounds, g_timing.requests = C.requests;

  int64_t total = 0;
  for (int64_t r = 0; r < n_reads; ++r) total += (int64_t)C.lists[(size_t)r].size();
  if (out_used) *out_used = total;
  int64_t at = 0;
  for (int64_t r = 0; r < n_reads; ++r) {
    out_off[r] = at;
    n_out[r] = (int32_t)C.lists[(size_t)r].size();
    at += n_out[r];
  }
  if (n_sw)
    for (int64_t p = 0; p < n_pairs; ++p) n_sw[p] = C.n_sw[(size_t)(2 * p)] + C.n_sw[(size_t)(2 * p + 1)];
  GB_ARG(total <= out_cap, "%s: out_cap = %lld, the regions need %lld", who, (long long)out_cap, (long long)total);
  for (int64_t r = 0; r < n_reads; ++r)
    if (n_out[r])
      std::memcpy(static_cast<void *>(out_regs + out_off[r]), C.lists[(size_t)r].data(), (size_t)n_out[r] * sizeof(Reg));
  return GB_OK;
}

}  // namespace gbms

extern "C" {

void gb_bsw_pe_default_opt(gb_bsw_pe_opt *o) {
  if (!o) return;
  o->a = 1, o->b = 4, o->o_del = o->o_ins = 6, o->e_del = o->e_ins = 1;
  o->min_seed_len = 19, o->max_chain_gap = 10000, o->pen_unpaired = 17, o->max_matesw = 50, o->max_ins = 10000;
  o->mask_level = 0.50f, o->mask_level_redun = 0.95f;
}

int gb_bsw_pestat(const gb_bsw_pe_opt *opt, int64_t l_pac, int64_t n_reads, const int64_t *reg_off,
                  const gb_bsw_alnreg *regs, struct gb_bsw_pestat pes[4]) {
  try {
    return gbms::pestat_impl(opt, l_pac, n_reads, reg_off, regs, pes);
  } catch (const std::bad_alloc &) {
    gb::set_error("gb_bsw_pestat: out of host memory");
    return GB_ERR_NOMEM;
  }
}

// The C ABI lets no exception out: the lists, the requests and the host threads allocate.
int gb_bsw_mate_rescue(const gb_bsw_params *params, const gb_bsw_pe_opt *opt, const struct gb_bsw_pestat pes[4],
                       const gb_ref *ref, const int64_t *contig_end, int64_t n_contigs, const uint8_t *seq_buf_qer,
                       int64_t qer_bytes, int64_t n_pairs, const int64_t *idq, const int32_t *l_query,
                       const int64_t *reg_off, const gb_bsw_alnreg *regs, gb_bsw_alnreg *out_regs, int64_t out_cap,
                       int64_t *out_off, int32_t *n_out, int32_t *n_sw, int64_t *out_used) {
  gb::Range range_("gb.bsw.mate_rescue");
  try {
    return gbms::rescue_impl(params, opt, pes, ref, contig_end, n_contigs, seq_buf_qer, qer_bytes, n_pairs, idq, l_query,
                             reg_off, regs, out_regs, out_cap, out_off, n_out, n_sw, out_used);
  } catch (const std::bad_alloc &) {
    gb::set_error("gb_bsw_mate_rescue: out of host memory");
    return GB_ERR_NOMEM;
  } catch (const std::exception &e) {
    gb::set_error("gb_bsw_mate_rescue: %s", e.what());
    return GB_ERR_STATE;
  }
}

int gb_bsw_mate_rescue_timing(float *fetch_ms, float *dp_ms, float *region_ms, float *host_ms, int32_t *rounds,
                              int64_t *requests) {
  const gbms::Timing *W = &gbms::g_timing;
  if (!W->valid) {
    gb::set_error("gb_bsw_mate_rescue_timing: no gb_bsw_mate_rescue call on this thread");
    return GB_ERR_STATE;
  }
  if (fetch_ms) *fetch_ms = W->fetch_ms;
  if (dp_ms) *dp_ms = W->dp_ms;
  if (region_ms) *region_ms = W->region_ms;
  if (host_ms) *host_ms = W->host_ms;
  if (rounds) *rounds = W->rounds;
  if (requests) *requests = W->requests;
  return GB_OK;
}

}  // extern "C"
