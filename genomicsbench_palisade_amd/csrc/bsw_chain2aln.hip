// bsw_chain2aln.hip -- MI355X (gfx950): all of bwa's mem_chain2aln (tools/bwa/bwamem.c:632-824) on the
// device-resident packed reference (gb_ref): kernels and C ABI.
//
// Per chunk of reads of gb_bsw_chain2aln:
//   gather: one wave64 per chain fetches the chain's window [rmax0, rmax1) from the 2-bit pac in
//     bns_get_seq's form (16 bases per lane, 16-byte stores; the routine of bsw_ref_internal.h) and, in
//     the same wave, its reversal: both are direct fetches, the reversal reads the pac the other way.
//     One wave per read writes the reversed query behind the uploaded query bytes. After this no
//     per-seed bytes exist: a left extension's target is the slice of the reversed window that starts
//     at L - (rbeg - rmax0) and its query the slice of the reversed read at l_query - qbeg; a right
//     extension's are slices of the forward copies. The extension kernels read bytes, so a slice starts
//     where it starts.
//   extension: the kernels of bsw.hip, unchanged, through gbbsw::run_resident, in at most four rounds:
//     left at w, left at 2 w for the seeds MAX_BAND_TRY's rule sends there (bwamem.c:752), right at w
//     (its h0 is the left result, so out6 comes back to the host between the rounds, where the launch
//     plan's keys are built), right at 2 w. A round without seeds launches nothing.
//   finish: one lane per seed turns the two sides' results into qb, qe, rb, re, score, truesc, w
//     (bwamem.c:755-763, 802-809, 818-819) and sums seedcov over the chain's seeds (:813-817).
//   filter: one lane per read walks the read's chains in order and each chain's seeds by decreasing
//     score << 32 | index, and applies the containment test (:671-687) and the overlapping-seed check
//     that overrides it (:692-703) against the regions kept so far. A single-block scan turns the
//     reads' counts into offsets and an emit kernel writes the kept regions packed in read order.
// The windows (cal_max_gap, the clamps, the strand rule, the clip to the contig) and the seeds' order
// are host work done while the call is validated and cut into chunks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/gb_bsw.h"
#include "bsw_internal.h"
#include "bsw_ref_internal.h"
#include "gb_common.h"

static_assert(sizeof(gb_bsw_seed) == 24, "gb_bsw_seed is 24 bytes (include/gb_bsw.h)");
static_assert(sizeof(gb_bsw_region) == 56, "gb_bsw_region is 56 bytes (include/gb_bsw.h)");
static_assert(sizeof(gb_bsw_c2a_raw) == 64, "gb_bsw_c2a_raw is 64 bytes (include/gb_bsw.h)");

namespace gbc2a {

constexpr int kMaxPenalty = 32768;
constexpr int kGatherWaves = 4;
constexpr int kScanThreads = 1024;
constexpr int64_t kChunkBytes = 256ll << 20;  // GB_BSW_C2A_BYTES overrides

struct Opt {  // the fields of mem_opt_t that mem_chain2aln reads
  int a, o_del, e_del, o_ins, e_ins, w, pen_clip5, pen_clip3;
};

// cal_max_gap (bwamem.c:621-628) in the reference's double arithmetic: a division and an addition,
// nothing a contraction could fuse
__host__ __device__ inline int cal_max_gap(const Opt &o, int qlen) {
  const int l_del = (int)((double)(qlen * o.a - o.o_del) / o.e_del + 1.);
  const int l_ins = (int)((double)(qlen * o.a - o.o_ins) / o.e_ins + 1.);
  int l = l_del > l_ins ? l_del : l_ins;
  l = l > 1 ? l : 1;
  return l < o.w << 1 ? l : o.w << 1;
}

struct ChainItem {  // 32 B
  int64_t rmax0;    // first base of the window in the doubled coordinate space
  int64_t f_off;    // 16-byte aligned offsets of the forward and the reversed copy in the target buffer
  int64_t r_off;
  int32_t len, read;  // window length; the chain's read (chunk-local)
};

struct ReadItem {  // 16 B
  int64_t q_off;   // 4-byte aligned offset of the query; its reversal lies rev_base further on
  int32_t l_query, pad;
};

struct GatherArgs {
  const ChainItem *chains;
  const ReadItem *reads;
  int64_t n_chains, n_reads;
  const uint32_t *pac;
  int64_t n_words, l_pac;
  uint8_t *tgt, *qry;
  int64_t rev_base;
};

__global__ __launch_bounds__(64 * kGatherWaves) void bsw_c2a_gather_kernel(GatherArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t job = (int64_t)blockIdx.x * kGatherWaves + (threadIdx.x >> 6);  // wave-uniform
  if (job < A.n_chains) {
    const ChainItem it = A.chains[job];
    if (it.rmax0 < A.l_pac) {  // forward strand: the bases, and the same read backwards
      gbgc::fetch_bases(A.pac, A.n_words, it.rmax0, it.len, false, 0u, A.tgt + it.f_off, lane);
      gbgc::fetch_bases(A.pac, A.n_words, it.rmax0 + it.len - 1, it.len, true, 0u, A.tgt + it.r_off, lane);
    } else {  // reverse strand: the complement read backwards (bntseq.c:414-418), and its reversal
      gbgc::fetch_bases(A.pac, A.n_words, 2 * A.l_pac - 1 - it.rmax0, it.len, true, 0xFFFFFFFFu, A.tgt + it.f_off, lane);
      gbgc::fetch_bases(A.pac, A.n_words, 2 * A.l_pac - it.rmax0 - it.len, it.len, false, 0xFFFFFFFFu,
                        A.tgt + it.r_off, lane);
    }
  } else if (job < A.n_chains + A.n_reads) {
    const ReadItem it = A.reads[job - A.n_chains];
    gbgc::reverse_query(A.qry + it.q_off, it.l_query, A.qry + A.rev_base + it.q_off, lane);
  }
}

// After a round: the results of the round's k-th pair go to the raw record of seed list[k].
__global__ __launch_bounds__(256) void bsw_c2a_scatter_kernel(const int32_t *list, int64_t m, const int32_t *out6,
                                                              gb_bsw_c2a_raw *raw, int side) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  gb_bsw_c2a_raw *r = raw + list[k];
#pragma unroll
  for (int f = 0; f < 6; ++f) r->out6[side][f] = out6[6 * k + f];
  r->tries[side] += 1;
}

struct DevArgs {  // what finish, filter and emit share; every index is chunk-local
  const gb_bsw_seed *seeds;
  const int64_t *chain_seed_off;  // n_chains + 1
  const int64_t *read_chain_off;  // n_reads + 1
  const ChainItem *chains;
  const ReadItem *reads;
  const int32_t *seed_chain;  // the chain of every seed
  const uint32_t *srt;        // per chain: its seeds' local indices by increasing score << 32 | index
  gb_bsw_c2a_raw *raw;
  gb_bsw_region *cand;  // one finished region per seed
  int32_t *keep;        // per read, from its first seed's slot on: the seeds whose regions are kept
  int32_t *n_reg;
  int64_t *reg_off;  // n_reads + 1
  gb_bsw_region *out;
  int64_t n_seeds, n_chains, n_reads;
  int64_t seed_base, chain_base;  // the chunk's first seed / chain in the call
  Opt opt;
};

__global__ __launch_bounds__(256) void bsw_c2a_finish_kernel(DevArgs A) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n_seeds) return;
  const gb_bsw_seed s = A.seeds[i];
  const int c = A.seed_chain[i];
  const int l_query = A.reads[A.chains[c].read].l_query;
  const gb_bsw_c2a_raw r = A.raw[i];
  gb_bsw_region a;
  int aw0 = A.opt.w, aw1 = A.opt.w;
  if (s.qbeg) {  // bwamem.c:755-761
    const int *o = r.out6[0];  // score, qle, tle, gtle, gscore, max_off
    aw0 = A.opt.w << (r.tries[0] - 1);
    a.score = o[0];
    if (o[4] <= 0 || o[4] <= o[0] - A.opt.pen_clip5) {
      a.qb = s.qbeg - o[1], a.rb = s.rbeg - o[2];
      a.truesc = o[0];
    } else {
      a.qb = 0, a.rb = s.rbeg - o[3];
      a.truesc = o[4];
    }
  } else {
    a.score = a.truesc = s.len * A.opt.a, a.qb = 0, a.rb = s.rbeg;
  }
  if (s.qbeg + s.len != l_query) {  // bwamem.c:802-808
    const int *o = r.out6[1];
    const int sc0 = a.score, qe = s.qbeg + s.len;
    aw1 = A.opt.w << (r.tries[1] - 1);
    a.score = o[0];
    if (o[4] <= 0 || o[4] <= o[0] - A.opt.pen_clip3) {
      a.qe = qe + o[1], a.re = s.rbeg + s.len + o[2];
      a.truesc += o[0] - sc0;
    } else {
      a.qe = l_query, a.re = s.rbeg + s.len + o[3];
      a.truesc += o[4] - sc0;
    }
  } else {
    a.qe = l_query, a.re = s.rbeg + s.len;
  }
  a.seedcov = 0;
  for (int64_t k = A.chain_seed_off[c]; k < A.chain_seed_off[c + 1]; ++k) {  // bwamem.c:813-817
    const gb_bsw_seed t = A.seeds[k];
    if (t.qbeg >= a.qb && t.qbeg + t.len <= a.qe && t.rbeg >= a.rb && t.rbeg + t.len <= a.re) a.seedcov += t.len;
  }
  a.w = aw0 > aw1 ? aw0 : aw1;
  a.seedlen0 = s.len;
  a.chain = (int32_t)(A.chain_base + c);
  a.seed = (int32_t)(A.seed_base + i);
  a.pad = 0;
  A.cand[i] = a;
}

// One lane per read. Every loop runs over seeds of the read (its kept regions are among them).
__global__ __launch_bounds__(64) void bsw_c2a_filter_kernel(DevArgs A) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.n_reads) return;
  const int l_query = A.reads[r].l_query;
  const int64_t c0 = A.read_chain_off[r], c1 = A.read_chain_off[r + 1];
  int32_t *keep = A.keep + A.chain_seed_off[c0];
  int nk = 0;
  for (int64_t c = c0; c < c1; ++c) {
    const int64_t sb = A.chain_seed_off[c];
    const int n = (int)(A.chain_seed_off[c + 1] - sb);
    for (int k = n - 1; k >= 0; --k) {
      const int64_t si = sb + A.srt[sb + k];
      const gb_bsw_seed s = A.seeds[si];
      // The comparisons below are the reference's, doubles where it uses doubles. No addition stands
      // next to a multiplication in any of them (cal_max_gap divides and adds), so a contraction
      // into a fused multiply-add cannot change them; the build turns contraction off besides.
      int i;
      for (i = 0; i < nk; ++i) {  // bwamem.c:671-687
        const gb_bsw_region p = A.cand[keep[i]];
        if (s.rbeg < p.rb || s.rbeg + s.len > p.re || s.qbeg < p.qb || s.qbeg + s.len > p.qe) continue;
        if (s.len - p.seedlen0 > .1 * l_query) continue;
        int qd = s.qbeg - p.qb;
        int64_t rd = s.rbeg - p.rb;
        int max_gap = cal_max_gap(A.opt, (int)(qd < rd ? qd : rd));
        int w = max_gap < p.w ? max_gap : p.w;
        if (qd - rd < w && rd - qd < w) break;
        qd = p.qe - (s.qbeg + s.len), rd = p.re - (s.rbeg + s.len);
        max_gap = cal_max_gap(A.opt, (int)(qd < rd ? qd : rd));
        w = max_gap < p.w ? max_gap : p.w;
        if (qd - rd < w && rd - qd < w) break;
      }
      if (i < nk) {  // bwamem.c:692-703
        for (i = k + 1; i < n; ++i) {
          const int64_t ti = sb + A.srt[sb + i];
          if (A.raw[ti].skipped) continue;  // srt[i] == 0 in the reference
          const gb_bsw_seed t = A.seeds[ti];
          if (t.len < s.len * .95) continue;
          if (s.qbeg <= t.qbeg && s.qbeg + s.len - t.qbeg >= s.len >> 2 && t.qbeg - s.qbeg != t.rbeg - s.rbeg) break;
          if (t.qbeg <= s.qbeg && t.qbeg + t.len - s.qbeg >= s.len >> 2 && s.qbeg - t.qbeg != s.rbeg - t.rbeg) break;
        }
        if (i == n) {
          A.raw[si].skipped = 1;
          continue;
        }
      }
      keep[nk++] = (int32_t)si;
    }
  }
  A.n_reg[r] = nk;
}

// Exclusive prefix sum of n_reg into reg_off[0 .. n_reads], one block: a thread sums a contiguous
// slice of the reads, the block scans the slices' sums, the thread writes its slice.
__global__ __launch_bounds__(kScanThreads) void bsw_c2a_scan_kernel(DevArgs A) {
  __shared__ int64_t part[kScanThreads];
  const int t = threadIdx.x;
  const int64_t per = (A.n_reads + kScanThreads - 1) / kScanThreads;
  const int64_t lo = min(A.n_reads, t * per), hi = min(A.n_reads, lo + per);
  int64_t s = 0;
  for (int64_t r = lo; r < hi; ++r) s += A.n_reg[r];
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {
    const int64_t v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int64_t acc = part[t] - s;
  for (int64_t r = lo; r < hi; ++r) {
    A.reg_off[r] = acc;
    acc += A.n_reg[r];
  }
  if (t == kScanThreads - 1) A.reg_off[A.n_reads] = part[t];
}

__global__ __launch_bounds__(64) void bsw_c2a_emit_kernel(DevArgs A) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.n_reads) return;
  const int32_t *keep = A.keep + A.chain_seed_off[A.read_chain_off[r]];
  const int64_t o = A.reg_off[r];
  const int n = A.n_reg[r];
  for (int i = 0; i < n; ++i) A.out[o + i] = A.cand[keep[i]];
}

struct CWs {  // the calling thread's, through gb::thread_ws
  int device = -1;
  gb::Stream stream;
  gb::Event ev[6];  // gather, finish, filter begin / end
  gb::PinnedBuf<uint8_t> h_in;
  // host scratch that is read back here lives in ordinary memory (reads of page-locked memory are slow),
  // and in the workspace, so that a call does not fault its pages in again
  std::vector<int32_t> h_out6, list, again, sc0, hsc;
  std::vector<gb_seqpair> sp, sp2;
  std::vector<ChainItem> hc;
  std::vector<ReadItem> hr;
  gb::DevBuf<uint8_t> d_in, d_tgt, d_qry;
  gb::DevBuf<gb_bsw_c2a_raw> d_raw;
  gb::DevBuf<gb_bsw_region> d_cand, d_out;
  gb::DevBuf<int32_t> d_keep, d_nreg, d_list;
  gb::DevBuf<int64_t> d_regoff;
  float gather_ms = 0.f, ext_ms[4] = {0.f, 0.f, 0.f, 0.f}, finish_ms = 0.f, filter_ms = 0.f;
};

int get_ws(int dev, CWs **out) {
  return gb::thread_ws(dev, out, [](int dev, CWs **out) {
    auto *W = new CWs();
    W->device = dev;
    hipError_t e = W->stream.create();
    for (auto &ev : W->ev)
      if (e == hipSuccess) e = ev.create();
    if (e != hipSuccess) {
      gb::set_error("gb_bsw_chain2aln workspace: %s", hipGetErrorString(e));
      delete W;
      return GB_ERR_HIP;
    }
    *out = W;
    return GB_OK;
  });
}

struct Window {  // a chain's window after the clamps and the clip (bwamem.c:642-659)
  int64_t rmax0, rmax1;
};

struct Plan {
  int64_t n_reads = 0, n_chains = 0, n_seeds = 0;
  std::vector<Window> win;      // per chain
  std::vector<uint32_t> srt;    // per seed
  std::vector<int64_t> cuts;    // chunk c holds reads cuts[c] .. cuts[c + 1]
};

// Everything the call refuses, and the host part of mem_chain2aln: windows and seed order.
int make_plan(const gb_bsw_params *params, int32_t pen_clip5, int32_t pen_clip3, const gb_ref *ref,
              const int64_t *contig_end, int64_t n_contigs, const uint8_t *qer, int64_t qer_bytes, int64_t n_reads,
              const int64_t *idq, const int32_t *l_query, const int64_t *rco, const int64_t *cso,
              const gb_bsw_seed *seeds, Opt *opt, Plan *P) {
  const char *who = "gb_bsw_chain2aln";
  GB_ARG(params && ref && n_reads >= 0, "%s: bad arguments", who);
  GB_ARG(n_reads == 0 || (idq && l_query && rco && cso), "%s: null read or chain arrays", who);
  GB_ARG(qer_bytes >= 0 && (qer_bytes == 0 || qer), "%s: bad query buffer", who);
  GB_ARG(params->o_del >= 0 && params->o_del < kMaxPenalty && params->e_del >= 0 && params->e_del < kMaxPenalty &&
             params->o_ins >= 0 && params->o_ins < kMaxPenalty && params->e_ins >= 0 && params->e_ins < kMaxPenalty,
         "%s: gap penalties must lie in [0, %d)", who, kMaxPenalty);
  GB_ARG(params->e_del > 0 && params->e_ins > 0, "%s: gap extension must be > 0", who);
  GB_ARG(params->w >= 0 && params->w < (1 << 28), "%s: w = %d must lie in [0, 2^28)", who, params->w);
  const int64_t l_pac = ref->l_pac;
  if (contig_end) {
    GB_ARG(n_contigs >= 1, "%s: contig_end given with n_contigs = %lld", who, (long long)n_contigs);
    for (int64_t k = 0; k < n_contigs; ++k)
      GB_ARG(contig_end[k] > (k ? contig_end[k - 1] : 0), "%s: contig_end[%lld] does not increase", who, (long long)k);
    GB_ARG(contig_end[n_contigs - 1] == l_pac, "%s: contig_end ends at %lld, l_pac is %lld", who,
           (long long)contig_end[n_contigs - 1], (long long)l_pac);
  }
  *opt = Opt{params->mat[0], params->o_del, params->e_del, params->o_ins, params->e_ins, params->w, pen_clip5, pen_clip3};
  P->n_reads = n_reads;
  if (n_reads == 0) return GB_OK;
  GB_ARG(rco[0] == 0 && cso[0] == 0, "%s: read_chain_off[0] and chain_seed_off[0] must be 0", who);
  for (int64_t r = 0; r < n_reads; ++r)
    GB_ARG(rco[r + 1] >= rco[r], "%s: read_chain_off decreases at read %lld", who, (long long)r);
  P->n_chains = rco[n_reads];
  GB_ARG(P->n_chains == 0 || seeds, "%s: null seeds", who);
  for (int64_t c = 0; c < P->n_chains; ++c)
    GB_ARG(cso[c + 1] > cso[c], "%s: chain %lld is empty or chain_seed_off decreases", who, (long long)c);
  P->n_seeds = cso[P->n_chains];
  GB_ARG(P->n_seeds < (1ll << 31), "%s: %lld seeds (need fewer than 2^31)", who, (long long)P->n_seeds);
  P->win.resize((size_t)P->n_chains);
  P->srt.resize((size_t)P->n_seeds);
  const int amax = std::abs((int)params->mat[0]);
  const char *be = getenv("GB_BSW_C2A_BYTES");
  const int64_t bound = be ? std::max<int64_t>(1, atoll(be)) : kChunkBytes;
  // one read: what is refused, its chains' windows and seed orders, the bytes its gather needs
  std::vector<int64_t> rbytes_of((size_t)n_reads);
  auto plan_read = [&](int64_t r) -> int {
    const int lq = l_query[r];
    GB_ARG(lq >= 1, "%s: read %lld has l_query = %d (need >= 1)", who, (long long)r, lq);
    GB_ARG((int64_t)lq * std::max(amax, 1) < (1 << 30), "%s: read %lld: l_query = %d times the match score overflows", who,
           (long long)r, lq);
    GB_ARG(idq[r] >= 0 && idq[r] + lq <= qer_bytes, "%s: read %lld lies outside the query buffer", who, (long long)r);
    int64_t rbytes = 2 * gb::round_up<int64_t>(lq, 4);
    for (int64_t c = rco[r]; c < rco[r + 1]; ++c) {
      const gb_bsw_seed *cs = seeds + cso[c];
      const int n = (int)std::min<int64_t>(cso[c + 1] - cso[c], INT32_MAX);
      GB_ARG(cso[c + 1] - cso[c] <= INT32_MAX, "%s: chain %lld has too many seeds", who, (long long)c);
      int64_t rmax0 = l_pac << 1, rmax1 = 0;
      for (int j = 0; j < n; ++j) {
        const gb_bsw_seed &t = cs[j];
        const long long sid = (long long)(cso[c] + j);
        GB_ARG(t.len >= 1 && t.score >= 1 && t.qbeg >= 0 && (int64_t)t.qbeg + t.len <= lq,
               "%s: read %lld chain %lld seed %lld: qbeg = %d, len = %d, score = %d on a read of %d bases", who,
               (long long)r, (long long)c, sid, t.qbeg, t.len, t.score, lq);
        GB_ARG(t.qbeg <= GB_BSW_MAX_QLEN && lq - t.qbeg - t.len <= GB_BSW_MAX_QLEN,
               "%s: read %lld chain %lld seed %lld: an extension's query part (%d left, %d right) exceeds %d", who,
               (long long)r, (long long)c, sid, t.qbeg, lq - t.qbeg - t.len, GB_BSW_MAX_QLEN);
        GB_ARG(t.rbeg >= 0 && t.rbeg + t.len <= l_pac << 1,
               "%s: read %lld chain %lld seed %lld: [%lld, %lld) lies outside [0, 2 l_pac = %lld]", who, (long long)r,
               (long long)c, sid, (long long)t.rbeg, (long long)(t.rbeg + t.len), (long long)(l_pac << 1));
        GB_ARG(!(t.rbeg < l_pac && t.rbeg + t.len > l_pac), "%s: read %lld chain %lld seed %lld bridges l_pac", who,
               (long long)r, (long long)c, sid);
        GB_ARG((t.rbeg >= l_pac) == (cs[0].rbeg >= l_pac),
               "%s: read %lld chain %lld seed %lld lies on the other strand than the chain's first seed", who,
               (long long)r, (long long)c, sid);
        // bwamem.c:644-650
        const int64_t b = t.rbeg - (t.qbeg + cal_max_gap(*opt, t.qbeg));
        const int64_t e = t.rbeg + t.len + ((lq - t.qbeg - t.len) + cal_max_gap(*opt, lq - t.qbeg - t.len));
        rmax0 = rmax0 < b ? rmax0 : b;
        rmax1 = rmax1 > e ? rmax1 : e;
      }
      rmax0 = rmax0 > 0 ? rmax0 : 0;
      rmax1 = rmax1 < l_pac << 1 ? rmax1 : l_pac << 1;
      if (rmax0 < l_pac && l_pac < rmax1) {  // bwamem.c:654-657
        if (cs[0].rbeg < l_pac)
          rmax1 = l_pac;
        else
          rmax0 = l_pac;
      }
      {  // bns_fetch_seq's clip to the contig of seeds[0].rbeg (bntseq.c:435-444)
        const int64_t mid = cs[0].rbeg;
        const bool is_rev = mid >= l_pac;
        const int64_t pos_f = is_rev ? (l_pac << 1) - 1 - mid : mid;
        int64_t far_beg = 0, far_end = l_pac;
        if (contig_end) {
          const int64_t *it = std::upper_bound(contig_end, contig_end + n_contigs, pos_f);
          far_end = *it;
          far_beg = it == contig_end ? 0 : it[-1];
        }
        if (is_rev) {
          const int64_t tmp = far_beg;
          far_beg = (l_pac << 1) - far_end;
          far_end = (l_pac << 1) - tmp;
        }
        rmax0 = rmax0 > far_beg ? rmax0 : far_beg;
        rmax1 = rmax1 < far_end ? rmax1 : far_end;
      }
      for (int j = 0; j < n; ++j)
        GB_ARG(cs[j].rbeg >= rmax0 && cs[j].rbeg + cs[j].len <= rmax1,
               "%s: read %lld chain %lld seed %lld lies outside the chain's window [%lld, %lld) on the contig of its "
               "first seed",
               who, (long long)r, (long long)c, (long long)(cso[c] + j), (long long)rmax0, (long long)rmax1);
      GB_ARG(rmax1 - rmax0 < (1ll << 31), "%s: read %lld chain %lld: a window of %lld bases", who, (long long)r,
             (long long)c, (long long)(rmax1 - rmax0));
      P->win[(size_t)c] = Window{rmax0, rmax1};
      rbytes += 2 * gb::round_up<int64_t>(rmax1 - rmax0, 16);
      // bwamem.c:662-665: by increasing score << 32 | index, that is by score and, among equal scores,
      // by index; the keys are distinct, so any sort gives the reference's order (chains are short:
      // insertion)
      uint32_t *srt = P->srt.data() + cso[c];
      if (n <= 32) {
        for (int j = 0; j < n; ++j) {
          int k = j;
          for (; k > 0 && cs[srt[k - 1]].score > cs[j].score; --k) srt[k] = srt[k - 1];
          srt[k] = (uint32_t)j;
        }
      } else {
        for (int j = 0; j < n; ++j) srt[j] = (uint32_t)j;
        std::stable_sort(srt, srt + n, [cs](uint32_t x, uint32_t y) { return cs[x].score < cs[y].score; });
      }
    }
    rbytes_of[(size_t)r] = rbytes;
    return GB_OK;
  };
  // big calls plan their reads on several threads; the lowest read that is refused is then planned
  // again on this thread, which leaves its message in gb_last_error()
  const int nth = n_reads >= (1 << 14) ? (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency())) : 1;
  std::atomic<int64_t> bad{n_reads};
  auto plan_range = [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi && r < bad.load(std::memory_order_relaxed); ++r)
      if (plan_read(r)) {
        int64_t b = bad.load();
        while (r < b && !bad.compare_exchange_weak(b, r)) {
        }
        return;
      }
  };
  if (const int st = gb::parallel(who, nth, [&](int t) { plan_range(n_reads * t / nth, n_reads * (t + 1) / nth); }))
    return st;
  if (bad.load() < n_reads) return plan_read(bad.load());
  int64_t bytes = 0;
  P->cuts.push_back(0);
  for (int64_t r = 0; r < n_reads; ++r) {
    if (bytes > 0 && bytes + rbytes_of[(size_t)r] > bound) {
      P->cuts.push_back(r);
      bytes = 0;
    }
    bytes += rbytes_of[(size_t)r];
  }
  P->cuts.push_back(n_reads);
  return GB_OK;
}

struct Blob {  // offsets of the chunk's uploaded arrays inside one staging block
  int64_t size = 0;
  int64_t take(int64_t bytes) {
    const int64_t at = size;
    size += gb::round_up<int64_t>(std::max<int64_t>(bytes, 1), 16);
    return at;
  }
};

// The descriptors of one side's first round: fill(k, &pair) returns whether seed k has that side. Big
// chunks are cut into ranges that threads count, then fill at their offsets, so the order is by seed.
template <class Fill>
int build_round(int64_t ns, Fill fill, std::vector<int32_t> *list, std::vector<gb_seqpair> *sp) {
  const char *who = "gb_bsw_chain2aln";
  const int nth = ns >= (1 << 16) ? (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency())) : 1;
  std::vector<int64_t> at((size_t)nth + 1, 0);
  int st = gb::parallel(who, nth, [&](int t) {
    gb_seqpair x{};
    int64_t n = 0;
    for (int64_t k = ns * t / nth; k < ns * (t + 1) / nth; ++k) n += fill(k, &x) ? 1 : 0;
    at[(size_t)t + 1] = n;
  });
  if (st) return st;
  for (int t = 0; t < nth; ++t) at[(size_t)t + 1] += at[(size_t)t];
  list->resize((size_t)at[(size_t)nth]);
  sp->resize((size_t)at[(size_t)nth]);
  return gb::parallel(who, nth, [&](int t) {
    int64_t o = at[(size_t)t];
    gb_seqpair x{};
    for (int64_t k = ns * t / nth; k < ns * (t + 1) / nth; ++k)
      if (fill(k, &x)) {
        (*list)[(size_t)o] = (int32_t)k;
        (*sp)[(size_t)o++] = x;
      }
  });
}

// One round of extensions: the seeds of `list` (chunk-local), whose descriptors are sp, on `side` at
// band w. The results come back in W->h_out6 in list order (the next round is planned from them) and
// are scattered into the raw records on the device.
int run_round(CWs *W, const gb_bsw_params *params, int side, int w, int end_bonus, const std::vector<int32_t> &list,
              const std::vector<gb_seqpair> &sp, int64_t tgt_bytes, int64_t qry_bytes, float *ms) {
  const int64_t m = (int64_t)list.size();
  if (m == 0) return GB_OK;  // an empty round costs no launch
  gb_bsw_params pl = *params;
  pl.w = w;
  pl.end_bonus = end_bonus;
  if (W->h_out6.size() < (size_t)m * 6) W->h_out6.resize((size_t)m * 6);
  int st = W->d_list.reserve((size_t)m, (size_t)m * 2);
  if (st) return st;
  const int32_t *d_out6 = nullptr;
  if ((st = gbbsw::run_resident(&pl, sp.data(), m, W->d_tgt, tgt_bytes, W->d_qry, qry_bytes, W->h_out6.data(), &d_out6, ms)))
    return st;
  GB_HIP(hipMemcpyAsync(W->d_list, list.data(), (size_t)m * 4, hipMemcpyHostToDevice, W->stream));
  hipLaunchKernelGGL(bsw_c2a_scatter_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, W->stream, W->d_list, m,
                     d_out6, W->d_raw.get(), side);
  GB_HIP(hipGetLastError());
  // the next round replaces the results the scatter reads, and the caller reuses `list`
  GB_HIP(hipStreamSynchronize(W->stream));
  return GB_OK;
}

}  // namespace gbc2a

extern "C" {

int gb_bsw_chain2aln(const gb_bsw_params *params, int32_t pen_clip5, int32_t pen_clip3, const gb_ref *ref,
                     const int64_t *contig_end, int64_t n_contigs, const uint8_t *qer, int64_t qer_bytes,
                     int64_t n_reads, const int64_t *idq, const int32_t *l_query, const int64_t *rco,
                     const int64_t *cso, const gb_bsw_seed *seeds, gb_bsw_region *regs, int64_t reg_cap,
                     int64_t *reg_off, int32_t *n_reg, int64_t *reg_used, gb_bsw_c2a_raw *raw_out) {
  using namespace gbc2a;
  gb::Range range_("gb.bsw.chain2aln");
  Opt opt;
  Plan P;
  // GB_BSW_C2A_PROF=1: host milliseconds per phase on stderr (development aid)
  const char *pe = getenv("GB_BSW_C2A_PROF");
  const bool prof = pe && *pe == '1';
  auto t_last = std::chrono::steady_clock::now();
  auto mark = [&](const char *what) {
    if (!prof) return;
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[c2a prof] %-8s %.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
    t_last = t;
  };
  int st = make_plan(params, pen_clip5, pen_clip3, ref, contig_end, n_contigs, qer, qer_bytes, n_reads, idq, l_query,
                     rco, cso, seeds, &opt, &P);
  if (st) return st;
  mark("plan");
  GB_ARG(reg_cap >= 0 && (reg_cap == 0 || regs), "gb_bsw_chain2aln: bad region buffer");
  GB_ARG(n_reads == 0 || (reg_off && n_reg), "gb_bsw_chain2aln: null reg_off or n_reg");
  if (reg_used) *reg_used = 0;
  if (n_reads == 0) return GB_OK;
  int dev = 0;
  GB_HIP(hipGetDevice(&dev));
  CWs *W = nullptr;
  if ((st = get_ws(dev, &W))) return st;
  gb_ref *R = const_cast<gb_ref *>(ref);
  if ((st = gbgc::ensure_device(R, dev))) return st;
  W->gather_ms = W->finish_ms = W->filter_ms = 0.f;
  for (float &x : W->ext_ms) x = 0.f;
  const int64_t l_pac = R->l_pac;
  int64_t total = 0;  // regions so far
  // The number of seeds always suffices, so with that much room the chunks' regions go straight to
  // regs; a smaller reg_cap is known to be enough only after the last chunk, and regs stays untouched
  // when it is not, so the regions wait in `held`.
  const bool direct = reg_cap >= P.n_seeds;
  std::vector<gb_bsw_region> held;
  for (size_t ck = 0; ck + 1 < P.cuts.size(); ++ck) {
    const int64_t r0 = P.cuts[ck], r1 = P.cuts[ck + 1], nr = r1 - r0;
    const int64_t c0 = rco[r0], nc = rco[r1] - c0;
    const int64_t s0 = cso[c0], ns = cso[c0 + nc] - s0;
    // layout of the target and query buffers
    int64_t tgt_bytes = 0, q_half = 0;
    Blob B;
    const int64_t o_chain = B.take(nc * (int64_t)sizeof(ChainItem)), o_read = B.take(nr * (int64_t)sizeof(ReadItem)),
                  o_cso = B.take((nc + 1) * 8), o_rco = B.take((nr + 1) * 8), o_sc = B.take(ns * 4),
                  o_srt = B.take(ns * 4), o_seed = B.take(ns * (int64_t)sizeof(gb_bsw_seed));
    for (int64_t r = r0; r < r1; ++r) q_half += gb::round_up<int64_t>(l_query[r], 4);
    q_half = gb::round_up<int64_t>(std::max<int64_t>(q_half, 1), 16);
    const int64_t o_qry = B.take(q_half);
    if ((st = W->h_in.reserve((size_t)B.size, (size_t)B.size * 2))) return st;
    if ((st = W->d_in.reserve((size_t)B.size, (size_t)B.size * 2))) return st;
    uint8_t *h = W->h_in;
    W->hc.resize((size_t)std::max<int64_t>(nc, 1)), W->hr.resize((size_t)nr), W->hsc.resize((size_t)std::max<int64_t>(ns, 1));
    ChainItem *hc = W->hc.data();
    ReadItem *hr = W->hr.data();
    int32_t *hsc = W->hsc.data();
    auto *hcso = reinterpret_cast<int64_t *>(h + o_cso);
    auto *hrco = reinterpret_cast<int64_t *>(h + o_rco);
    int64_t qo = 0;
    for (int64_t r = r0; r < r1; ++r) {
      hr[r - r0] = ReadItem{qo, l_query[r], 0};
      std::memcpy(h + o_qry + qo, qer + idq[r], (size_t)l_query[r]);
      qo += gb::round_up<int64_t>(l_query[r], 4);
      hrco[r - r0] = rco[r] - c0;
      for (int64_t c = rco[r]; c < rco[r + 1]; ++c) {
        const Window &wn = P.win[(size_t)c];
        const int64_t L = wn.rmax1 - wn.rmax0, Lp = gb::round_up<int64_t>(L, 16);
        hc[c - c0] = ChainItem{wn.rmax0, tgt_bytes, tgt_bytes + Lp, (int32_t)L, (int32_t)(r - r0)};
        tgt_bytes += 2 * Lp;
        hcso[c - c0] = cso[c] - s0;
        for (int64_t k = cso[c]; k < cso[c + 1]; ++k) hsc[k - s0] = (int32_t)(c - c0);
      }
    }
    hrco[nr] = nc;
    hcso[nc] = ns;
    std::memcpy(h + o_chain, hc, (size_t)nc * sizeof(ChainItem));
    std::memcpy(h + o_read, hr, (size_t)nr * sizeof(ReadItem));
    if (ns) {
      std::memcpy(h + o_sc, hsc, (size_t)ns * 4);
      std::memcpy(h + o_srt, P.srt.data() + s0, (size_t)ns * 4);
      std::memcpy(h + o_seed, seeds + s0, (size_t)ns * sizeof(gb_bsw_seed));
    }
    // 16 bytes of slack: the extension kernels read the first target byte of a pair whose target is
    // empty, and such a slice can start at the very end
    const int64_t tgt_cap = tgt_bytes, nsz = std::max<int64_t>(ns, 1);
    if ((st = W->d_tgt.reserve((size_t)tgt_bytes + 16))) return st;
    if ((st = W->d_qry.reserve((size_t)(2 * q_half)))) return st;
    if ((st = W->d_raw.reserve((size_t)nsz))) return st;
    if ((st = W->d_cand.reserve((size_t)nsz))) return st;
    if ((st = W->d_out.reserve((size_t)nsz))) return st;
    if ((st = W->d_keep.reserve((size_t)nsz))) return st;
    if ((st = W->d_nreg.reserve((size_t)nr))) return st;
    if ((st = W->d_regoff.reserve((size_t)nr + 1))) return st;
    uint8_t *d = W->d_in;
    mark("stage");
    GB_HIP(hipMemcpyAsync(d, h, (size_t)B.size, hipMemcpyHostToDevice, W->stream));
    if (prof) {
      GB_HIP(hipStreamSynchronize(W->stream));
      mark("upload");
    }
    GB_HIP(hipMemcpyAsync(W->d_qry, d + o_qry, (size_t)q_half, hipMemcpyDeviceToDevice, W->stream));
    GatherArgs G;
    G.chains = reinterpret_cast<const ChainItem *>(d + o_chain);
    G.reads = reinterpret_cast<const ReadItem *>(d + o_read);
    G.n_chains = nc;
    G.n_reads = nr;
    G.pac = R->d_pac;
    G.n_words = R->n_words;
    G.l_pac = l_pac;
    G.tgt = W->d_tgt;
    G.qry = W->d_qry;
    G.rev_base = q_half;
    GB_HIP(hipEventRecord(W->ev[0], W->stream));
    hipLaunchKernelGGL(bsw_c2a_gather_kernel, dim3((unsigned)((nc + nr + kGatherWaves - 1) / kGatherWaves)),
                       dim3(64 * kGatherWaves), 0, W->stream, G);
    GB_HIP(hipGetLastError());
    GB_HIP(hipEventRecord(W->ev[1], W->stream));
    if (ns) GB_HIP(hipMemsetAsync(W->d_raw, 0, (size_t)ns * sizeof(gb_bsw_c2a_raw), W->stream));
    // while the gather runs: the left round's descriptors
    std::vector<int32_t> &list = W->list, &again = W->again, &sc0 = W->sc0;  // sc0: the score the right side starts from
    std::vector<gb_seqpair> &sp = W->sp, &sp2 = W->sp2;
    sc0.resize((size_t)nsz);
    st = build_round(ns, [&](int64_t k, gb_seqpair *x) {
      const gb_bsw_seed &s = seeds[s0 + k];
      sc0[(size_t)k] = s.len * opt.a;
      if (!s.qbeg) return false;
      const ChainItem &c = hc[hsc[k]];
      const ReadItem &rd = hr[c.read];
      const int64_t tl = s.rbeg - c.rmax0;
      x->idr = c.r_off + c.len - tl, x->len1 = (int32_t)tl;
      x->idq = q_half + rd.q_off + rd.l_query - s.qbeg, x->len2 = s.qbeg;
      x->h0 = s.len * opt.a;
      return true;
    }, &list, &sp);
    if (st) return st;
    mark("pairs_l");
    GB_HIP(hipStreamSynchronize(W->stream));  // the extension kernels run on the batch's own streams
    mark("gather");
    float ms = 0.f;
    GB_HIP(hipEventElapsedTime(&ms, W->ev[0], W->ev[1]));
    W->gather_ms += ms;
    const int thr = (opt.w >> 1) + (opt.w >> 2);  // bwamem.c:752: a second try when max_off reaches it at w
    // the seeds of a round that take a second try: not (score == prev || max_off < thr)
    auto second = [&](const int32_t *prev) {
      again.clear(), sp2.clear();
      for (size_t k = 0; k < list.size(); ++k) {
        const int32_t *o = W->h_out6.data() + 6 * k;
        if (o[0] == (prev ? prev[list[k]] : -1) || o[5] < thr) continue;
        again.push_back(list[k]);
        sp2.push_back(sp[k]);
      }
    };
    if ((st = run_round(W, params, 0, opt.w, pen_clip5, list, sp, tgt_cap, 2 * q_half, &W->ext_ms[0]))) return st;
    for (size_t k = 0; k < list.size(); ++k) sc0[(size_t)list[k]] = W->h_out6[6 * k];
    second(nullptr);  // prev is -1 before the first left try (bwamem.c:711,724)
    if ((st = run_round(W, params, 0, opt.w << 1, pen_clip5, again, sp2, tgt_cap, 2 * q_half, &W->ext_ms[1]))) return st;
    for (size_t k = 0; k < again.size(); ++k) sc0[(size_t)again[k]] = W->h_out6[6 * k];
    mark("left");
    st = build_round(ns, [&](int64_t k, gb_seqpair *x) {
      const gb_bsw_seed &s = seeds[s0 + k];
      const ChainItem &c = hc[hsc[k]];
      const ReadItem &rd = hr[c.read];
      if (s.qbeg + s.len == rd.l_query) return false;
      const int64_t re = s.rbeg + s.len - c.rmax0;
      x->idr = c.f_off + re, x->len1 = (int32_t)(c.len - re);
      x->idq = rd.q_off + s.qbeg + s.len, x->len2 = rd.l_query - s.qbeg - s.len;
      x->h0 = sc0[(size_t)k];
      return true;
    }, &list, &sp);
    if (st) return st;
    mark("pairs_r");
    if ((st = run_round(W, params, 1, opt.w, pen_clip3, list, sp, tgt_cap, 2 * q_half, &W->ext_ms[2]))) return st;
    second(sc0.data());  // prev is the left score (bwamem.c:771,799)
    if ((st = run_round(W, params, 1, opt.w << 1, pen_clip3, again, sp2, tgt_cap, 2 * q_half, &W->ext_ms[3]))) return st;
    mark("right");
    DevArgs A;
    A.seeds = reinterpret_cast<const gb_bsw_seed *>(d + o_seed);
    A.chain_seed_off = reinterpret_cast<const int64_t *>(d + o_cso);
    A.read_chain_off = reinterpret_cast<const int64_t *>(d + o_rco);
    A.chains = G.chains;
    A.reads = G.reads;
    A.seed_chain = reinterpret_cast<const int32_t *>(d + o_sc);
    A.srt = reinterpret_cast<const uint32_t *>(d + o_srt);
    A.raw = W->d_raw;
    A.cand = W->d_cand;
    A.keep = W->d_keep;
    A.n_reg = W->d_nreg;
    A.reg_off = W->d_regoff;
    A.out = W->d_out;
    A.n_seeds = ns;
    A.n_chains = nc;
    A.n_reads = nr;
    A.seed_base = s0;
    A.chain_base = c0;
    A.opt = opt;
    GB_HIP(hipEventRecord(W->ev[2], W->stream));
    if (ns) {
      hipLaunchKernelGGL(bsw_c2a_finish_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, W->stream, A);
      GB_HIP(hipGetLastError());
    }
    GB_HIP(hipEventRecord(W->ev[3], W->stream));
    GB_HIP(hipEventRecord(W->ev[4], W->stream));
    hipLaunchKernelGGL(bsw_c2a_filter_kernel, dim3((unsigned)((nr + 63) / 64)), dim3(64), 0, W->stream, A);
    GB_HIP(hipGetLastError());
    hipLaunchKernelGGL(bsw_c2a_scan_kernel, dim3(1), dim3(kScanThreads), 0, W->stream, A);
    GB_HIP(hipGetLastError());
    hipLaunchKernelGGL(bsw_c2a_emit_kernel, dim3((unsigned)((nr + 63) / 64)), dim3(64), 0, W->stream, A);
    GB_HIP(hipGetLastError());
    GB_HIP(hipEventRecord(W->ev[5], W->stream));
    std::vector<int64_t> off((size_t)nr + 1);
    GB_HIP(hipMemcpyAsync(off.data(), W->d_regoff, (size_t)(nr + 1) * 8, hipMemcpyDeviceToHost, W->stream));
    GB_HIP(hipMemcpyAsync(n_reg + r0, W->d_nreg, (size_t)nr * 4, hipMemcpyDeviceToHost, W->stream));
    if (raw_out && ns)
      GB_HIP(hipMemcpyAsync(raw_out + s0, W->d_raw, (size_t)ns * sizeof(gb_bsw_c2a_raw), hipMemcpyDeviceToHost, W->stream));
    GB_HIP(hipStreamSynchronize(W->stream));
    GB_HIP(hipEventElapsedTime(&ms, W->ev[2], W->ev[3]));
    W->finish_ms += ms;
    GB_HIP(hipEventElapsedTime(&ms, W->ev[4], W->ev[5]));
    W->filter_ms += ms;
    mark("finish");
    const int64_t m = off[(size_t)nr];
    for (int64_t r = 0; r < nr; ++r) reg_off[r0 + r] = total + off[(size_t)r];
    if (!direct) held.resize((size_t)(total + m));
    if (m)
      GB_HIP(hipMemcpy(direct ? regs + total : held.data() + total, W->d_out, (size_t)m * sizeof(gb_bsw_region),
                       hipMemcpyDeviceToHost));
    total += m;
    mark("regs");
  }
  if (reg_used) *reg_used = total;
  GB_ARG(total <= reg_cap, "gb_bsw_chain2aln: reg_cap = %lld, the regions need %lld", (long long)reg_cap,
         (long long)total);
  if (!direct && total) std::memcpy(regs, held.data(), (size_t)total * sizeof(gb_bsw_region));
  return GB_OK;
}

int gb_bsw_chain2aln_timing(float *gather_ms, float ext_ms[4], float *finish_ms, float *filter_ms) {
  int dev = 0;
  GB_HIP(hipGetDevice(&dev));
  gbc2a::CWs *W = gb::find_thread_ws<gbc2a::CWs>(dev);
  if (!W) {
    gb::set_error("gb_bsw_chain2aln_timing: no gb_bsw_chain2aln call on this thread and device");
    return GB_ERR_STATE;
  }
  if (gather_ms) *gather_ms = W->gather_ms;
  if (ext_ms)
    for (int k = 0; k < 4; ++k) ext_ms[k] = W->ext_ms[k];
  if (finish_ms) *finish_ms = W->finish_ms;
  if (filter_ms) *filter_ms = W->filter_ms;
  return GB_OK;
}

}  // extern "C"
