// bsw_abea_hmm.hip -- gb_abea_hmm_score: the methylation profile-HMM forward score (f5c / nanopolish
// profile_hmm_score, hmm.c:301-727).
//
// An item is a matrix of rows (events) by k-mer blocks of three states K, B, M. M and B of a row read the row
// above; K reads its own row's previous block, and the table-driven log-sum is not associative, so the only
// parallel order is the anti-diagonal. A lane owns NK consecutive k-mers (NK = 1, 2, 4 by size class, so 256
// k-mers fit one wave64); at step t lane l computes row t - l for its k-mers in order, which resolves the
// same-row K chain inside the lane, and takes M, B, K of lane l-1's last k-mer for rows t-l and t-l-1 from that
// lane's two previous steps by a one-lane DPP shift. The event, and the post-flank value of its row, move down
// the lanes one per step; lane 0 takes them from windows that the lanes load ahead. Items of at most 16 k-mers
// share a wave: four 16-lane rows with row_shr:1. No matrix is stored; the log-sum table lives in LDS. Waves
// take slots (one item, or four small ones) of a sorted list from an atomic work counter; an item never spans
// waves and no wave waits for another. GB_ABEA_HOST=1 runs the plain C++ restatement below instead; both paths
// share the cell, emission, log-sum and end-update functions.
#include <cstring>

#include "bsw_abea_hmm_internal.h"

namespace gbhmm {

constexpr int kTbl = GB_ABEA_HMM_LOGSUM_TBL;
constexpr int kBlocksPerCU = 2;  // 64 000 B of table per block, 160 KB of LDS per CU
constexpr int kWavesSmall = 16, kWavesLarge = 8;  // per block: one k-mer per lane stays under 64 VGPRs

// ---- the fold, one text for host and device; the emission and the rest are bsw_abea_hmm_internal.h's ----

// p7_FLogsum (logsum.h:61-71). The table is read at 0 where the reference reads nothing.
GB_HD float logsum(const float *tbl, float a, float b) {
  const float mx = a > b ? a : b;
  const float mn = a < b ? a : b;
  const float d = mx - mn;
  const bool cut = mn == kNegInf || d >= 15.7f;
  const int idx = cut ? 0 : (int)(d * 1000.f);
  const float t = tbl[idx];
  return cut ? mx : mx + t;
}

// update_cell (hmm.c:558-566): the six terms in the order SAME_M, PREV_M, SAME_B, PREV_B, PREV_K, SOFT
GB_HD float fold6(const float *tbl, float x0, float x1, float x2, float x3, float x4, float x5, float em) {
  float s = x0;
  s = logsum(tbl, s, x1);
  s = logsum(tbl, s, x2);
  s = logsum(tbl, s, x3);
  s = logsum(tbl, s, x4);
  s = logsum(tbl, s, x5);
  return s + em;
}

// M and B of a cell from the row above: `up` is this k-mer's block, `lu` the previous k-mer's (hmm.c:441-465)
GB_HD void cell_mb(const float *tbl, const Trans &T, const State &up, const State &lu, float soft, float em, float *m,
                   float *b) {
  *m = fold6(tbl, T.mm_self + up.m, T.mm_next + lu.m, T.bm_self + up.b, T.bm_next + lu.b, T.km + lu.k, soft, em);
  *b = fold6(tbl, T.mb + up.m, kNegInf, T.bb + up.b, kNegInf, kNegInf, kNegInf, 0.0f);
}
// K of a cell from the previous k-mer's block of the same row (hmm.c:468-474)
GB_HD float cell_k(const float *tbl, const Trans &T, const State &left) {
  return fold6(tbl, kNegInf, T.mk + left.m, kNegInf, T.bk + left.b, T.kk + left.k, kNegInf, 0.0f);
}
// the three update_end calls of a row (hmm.c:479-487): M, B, K, with lp_ms = 0.0f
GB_HD float end_update(const float *tbl, float lp_end, const State &s, float post) {
  lp_end = logsum(tbl, lp_end, 0.0f + s.m + post);
  lp_end = logsum(tbl, lp_end, 0.0f + s.b + post);
  lp_end = logsum(tbl, lp_end, 0.0f + s.k + post);
  return lp_end;
}

GB_HD int base_rank5(char b) { return b == 'C' ? 1 : b == 'G' ? 2 : b == 'M' ? 3 : b == 'T' ? 4 : 0; }
GB_HD int kmer_rank5(const char *s) {
  int r = 0;
#pragma unroll
  for (int i = 0; i < kK; ++i) r = r * 5 + base_rank5(s[i]);
  return r;
}

// ---- host tables: everything that calls libm, once per process or once per read ----

struct Tables {
  float logsum[kTbl];
  std::vector<float> flank;  // pre_flank[i]; post_flank[i] == pre_flank[n_events - 1 - i] (hmm.c:132-205)
  Trans trans;               // the eight transitions that do not depend on the read
  Tables() : flank((size_t)kMaxRows) {
    for (int i = 0; i < kTbl; ++i) logsum[i] = (float)log(1. + exp((double)-i / 1000.f));
    flank[0] = (float)log(1 - 0.5);
    flank[1] = (float)(log(0.5) + -3.0f + log(1 - 0.9));
    for (int i = 2; i < kMaxRows; ++i) flank[(size_t)i] = (float)(log(0.9) + -3.0f + flank[(size_t)i - 1]);
    float p_next;
    make_trans(2.0, &trans, &p_next);
  }
};
static const Tables &tables() {
  static const Tables *T = new Tables();
  return *T;
}

// ---- host path: profile_hmm_fill_generic_r9 restated over two rolling rows ----

static float host_score(const Model *model, const Tables &tb, const char *seq, const gb_abea_hmm_item &it,
                        const float *read_events, const gb_abea_hmm_read &rd, const Trans &T, std::vector<State> *rows,
                        std::vector<Kmer> *kmers) {
  const float *tbl = tb.logsum;
  const int nk = it.seq_len - kK + 1, n = item_rows(it), stride = it.rc ? -1 : 1;
  const bool pre_clip = it.flags & GB_ABEA_HMM_PRE_CLIP, post_clip = it.flags & GB_ABEA_HMM_POST_CLIP;
  kmers->resize((size_t)nk);
  for (int ki = 0; ki < nk; ++ki)
    (*kmers)[(size_t)ki] =
        make_kmer(model[kmer_rank5(kmer_at(seq, it.seq_len, it.rc, ki))], rd.scale, rd.shift, rd.var, rd.log_var);
  rows->assign((size_t)2 * (nk + 1), State{kNegInf, kNegInf, kNegInf});  // block 0 is the start block
  State *prev = rows->data(), *cur = prev + (nk + 1);
  float lp_end = kNegInf;
  for (int r = 1; r <= n; ++r) {
    const float x = read_events[(int64_t)it.event_start + (int64_t)(r - 1) * stride];
    for (int ki = 0; ki < nk; ++ki) {
      const float soft = ki == 0 && (r == 1 || pre_clip) ? 0.0f + tb.flank[(size_t)r - 1] : kNegInf;
      State s;
      cell_mb(tbl, T, prev[ki + 1], prev[ki], soft, emission(x, (*kmers)[(size_t)ki]), &s.m, &s.b);
      s.k = cell_k(tbl, T, cur[ki]);
      cur[ki + 1] = s;
    }
    if (post_clip || r == n) lp_end = end_update(tbl, lp_end, cur[nk], tb.flank[(size_t)(n - r)]);
    std::swap(prev, cur);
  }
  return lp_end;
}

// ---- device path ----

struct DItem {
  int64_t seq_off, ev_first;  // ev_first: the index of row 1's event in the events of the call
  int32_t seq_len, n_rows, out, misc;  // out: index into scores[], -1 for a filler; misc: rc | flags << 1
  float scale, shift, var, log_var, lp_mm_self, lp_mm_next;
};

struct Args {
  const Model *model;
  const char *seqs;
  const float *events;
  const float *flank;
  const float *logsum;
  const DItem *items;  // this launch's slots in order: one item each, or four with fillers at the end
  int64_t n_slots;
  float *scores;
  unsigned int *next;
  Trans T;
};

struct Win {  // of the rows tb + 1 .. tb + G, one per lane of the group
  float ev, pre, post;
};

template <int NK, bool PACK>
__device__ __forceinline__ void score_slot(const Args &A, const float *tbl, int64_t slot, int lane) {
  constexpr int G = PACK ? 16 : 64;
  const int lg = lane & (G - 1), gbase = lane & ~(G - 1);
  const DItem I = A.items[PACK ? slot * 4 + (lane >> 4) : slot];
  const int nk = I.seq_len - kK + 1, n = I.n_rows;  // a filler has neither k-mers nor rows
  const int rc = I.misc & 1, stride = rc ? -1 : 1;
  const bool pre_clip = (I.misc >> 1) & GB_ABEA_HMM_PRE_CLIP, post_clip = (I.misc >> 1) & GB_ABEA_HMM_POST_CLIP;
  const char *seq = A.seqs + I.seq_off;
  const float *evs = A.events + I.ev_first;
  Trans T = A.T;
  T.mm_self = I.lp_mm_self, T.mm_next = I.lp_mm_next;

  // this lane's k-mers; anything finite for a k-mer past the item's (nothing reads what such a cell holds)
  Kmer km[NK];
#pragma unroll
  for (int j = 0; j < NK; ++j) {
    const int ki = lg * NK + j;
    km[j] = Kmer{0.f, 1.f, 0.f};
    if (ki < nk) km[j] = make_kmer(A.model[kmer_rank5(kmer_at(seq, I.seq_len, rc, ki))], I.scale, I.shift, I.var, I.log_var);
  }
  const int last = nk > 0 ? nk - 1 : 0, llast = last / NK;
  const int myj = lg == llast ? last % NK : -1;  // the k-mer whose block feeds the end state, in its lane
  int steps = nk > 0 ? n + llast : 0;            // lane llast computes row n at step n + llast
  if (PACK)
    steps = max(max(__builtin_amdgcn_readlane(steps, 0), __builtin_amdgcn_readlane(steps, 16)),
                max(__builtin_amdgcn_readlane(steps, 32), __builtin_amdgcn_readlane(steps, 48)));
  else
    steps = __builtin_amdgcn_readfirstlane(steps);

  // Row t's event, its SOFT term (pre_flank[t-1] where the start state may enter, hmm.c:452-454) and its end
  // term (post_flank[t-1] == flank[n - t] where the end state may be entered, hmm.c:479). A row outside 1..n
  // gets -infinity for both: its cells then change nothing.
  auto load_win = [&](int tb) {
    const int t = tb + lg + 1;
    const bool in = t <= n;
    Win w;
    w.ev = in ? evs[(int64_t)(t - 1) * stride] : 0.f;
    w.pre = in && (t == 1 || pre_clip) ? 0.0f + A.flank[t - 1] : kNegInf;
    w.post = in && (t == n || post_clip) ? A.flank[n - t] : kNegInf;
    return w;
  };

  State S[NK];
#pragma unroll
  for (int j = 0; j < NK; ++j) S[j] = State{kNegInf, kNegInf, kNegInf};
  State nprev{kNegInf, kNegInf, kNegInf};  // lane l-1's last k-mer, one row above this step's
  float ev = 0.f, post = kNegInf, lp_end = kNegInf;
  Win w = load_win(0), wn = load_win(G);
  for (int t = 1; t <= steps; ++t) {
    const int jw = (t - 1) & (G - 1);
    if (jw == 0 && t > 1) {
      w = wn;
      wn = load_win(t - 1 + G);
    }
    // lane l now holds row t - l's event and end term
    const float pre_t = pick<PACK>(w.pre, jw, gbase);
    ev = shr1<PACK>(ev, pick<PACK>(w.ev, jw, gbase));
    post = shr1<PACK>(post, pick<PACK>(w.post, jw, gbase));
    // lane l-1 computed row t - l in the step before this one
    State ncur;
    ncur.m = shr1<PACK>(S[NK - 1].m, kNegInf);
    ncur.b = shr1<PACK>(S[NK - 1].b, kNegInf);
    ncur.k = shr1<PACK>(S[NK - 1].k, kNegInf);
    State lu = nprev, lc = ncur;
#pragma unroll
    for (int j = 0; j < NK; ++j) {
      const State up = S[j];
      const float soft = j == 0 && lg == 0 ? pre_t : kNegInf;
      State s;
      cell_mb(tbl, T, up, lu, soft, emission(ev, km[j]), &s.m, &s.b);
      s.k = cell_k(tbl, T, lc);
      S[j] = s, lu = up, lc = s;
    }
    State se = S[0];
#pragma unroll
    for (int j = 1; j < NK; ++j) {
      se.m = myj == j ? S[j].m : se.m;
      se.b = myj == j ? S[j].b : se.b;
      se.k = myj == j ? S[j].k : se.k;
    }
    lp_end = end_update(tbl, lp_end, se, myj >= 0 ? post : kNegInf);
    nprev = ncur;
  }
  // stored by lane 1 of the group, never lane 0 (see bsw_global.hip on stores next to the work counter)
  const float score = pick<PACK>(lp_end, PACK ? llast : __builtin_amdgcn_readfirstlane(llast), gbase);
  if (lg == 1 && I.out >= 0) A.scores[I.out] = score;
}

template <int NK, bool PACK, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void abea_hmm_kernel(Args A) {
  __shared__ __attribute__((aligned(16))) float stbl[kTbl];
  for (int i = threadIdx.x; i < kTbl / 4; i += 64 * WAVES)
    reinterpret_cast<float4 *>(stbl)[i] = reinterpret_cast<const float4 *>(A.logsum)[i];
  __syncthreads();  // the kernel's only block-wide meeting
  const int lane = threadIdx.x & 63;
  for (;;) {
    unsigned int p = 0;
    if (lane == 0) p = atomicAdd(A.next, 1u);
    p = __builtin_amdgcn_readfirstlane(p);
    if ((int64_t)p >= A.n_slots) break;
    score_slot<NK, PACK>(A, stbl, (int64_t)p, lane);
    // the whole wave meets here before any lane fetches the next slot (see bsw_global.hip)
    __builtin_amdgcn_wave_barrier();
  }
}

static_assert(sizeof(Model) == 12, "gb_abea_model is three floats");
static_assert(sizeof(DItem) == 56, "DItem is packed");
static_assert(sizeof(gb_abea_hmm_read) == 40 && sizeof(gb_abea_hmm_item) == 32, "the header's records");
static_assert(kTbl % 4 == 0 && kTbl * sizeof(float) <= 64 * 1024, "the table is staged as float4 into 64 KB");

struct Ws : gb::WsBase<2> {  // the calling thread's, through gb::get_ws
  gb::DevBuf<Model> d_model;
  gb::DevBuf<char> d_seqs;
  gb::DevBuf<float> d_events, d_flank, d_logsum, d_scores;
  gb::DevBuf<DItem> d_items;
  gb::DevBuf<unsigned int> d_ctl;
  gb::PinnedBuf<DItem> h_items;
  gb::PinnedBuf<float> h_scores;
  float kernel_ms = 0.f;
  int64_t cells = 0, calls = 0;
};

static int make_tables(Ws *W) {  // the workspace's own part of gb::get_ws: the control words and the two tables
  const Tables &tb = tables();
  int st;
  if ((st = W->d_ctl.reserve(kClasses)) || (st = W->d_flank.reserve((size_t)kMaxRows)) ||
      (st = W->d_logsum.reserve((size_t)kTbl)))
    return st;
  hipError_t e = hipMemcpy(W->d_flank, tb.flank.data(), (size_t)kMaxRows * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(W->d_logsum, tb.logsum, (size_t)kTbl * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) return GB_OK;
  gb::set_error("gb_abea_hmm_score tables: %s", hipGetErrorString(e));
  return GB_ERR_HIP;
}

static int run_device(Ws *W, const gb_abea_hmm_read *reads, const gb_abea_hmm_item *items, int64_t n_items,
                      const std::vector<Trans> &trans, float *scores) {
  // The items by size class, each class with the most rows first, so that the items of a packed slot are of
  // like length and the long ones do not start last. A packed class is filled up to a multiple of four.
  std::vector<int32_t> order((size_t)n_items);
  for (int64_t i = 0; i < n_items; ++i) order[(size_t)i] = (int32_t)i;
  auto key = [&](int32_t i) {
    const gb_abea_hmm_item &it = items[i];
    return ((int64_t)size_class(it.seq_len - kK + 1) << 32) | (int64_t)(kMaxRows - item_rows(it));
  };
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key(a) < key(b); });
  int64_t count[kClasses] = {0, 0, 0, 0}, first[kClasses], slots[kClasses];
  for (int64_t i = 0; i < n_items; ++i) count[size_class(items[i].seq_len - kK + 1)] += 1;
  const int64_t fill0 = gb::round_up(count[0], 4) - count[0], total = n_items + fill0;
  int st;
  if ((st = W->h_items.reserve((size_t)total)) || (st = W->d_items.reserve((size_t)total)) ||
      (st = W->h_scores.reserve((size_t)n_items)) || (st = W->d_scores.reserve((size_t)n_items)))
    return st;
  DItem *hi = W->h_items;
  int64_t pos = 0, k = 0;
  W->cells = 0;
  for (int c = 0; c < kClasses; ++c) {
    first[c] = pos;
    for (int64_t j = 0; j < count[c]; ++j, ++k) {
      const int32_t i = order[(size_t)k];
      const gb_abea_hmm_item &it = items[i];
      const gb_abea_hmm_read &rd = reads[it.read];
      const Trans &T = trans[(size_t)it.read];
      hi[pos++] = DItem{it.seq_off, rd.event_off + it.event_start, it.seq_len, item_rows(it), i, it.rc | (it.flags << 1),
                        rd.scale, rd.shift, rd.var, rd.log_var, T.mm_self, T.mm_next};
      W->cells += (int64_t)item_rows(it) * (it.seq_len - kK + 1);
    }
    if (c == 0)
      for (int64_t j = 0; j < fill0; ++j) hi[pos++] = DItem{0, 0, kK - 1, 0, -1, 0, 1.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    slots[c] = c == 0 ? (count[0] + fill0) / 4 : count[c];
  }
  GB_HIP(hipMemcpyAsync(W->d_items, hi, (size_t)total * sizeof(DItem), hipMemcpyHostToDevice, W->stream));
  GB_HIP(hipMemsetAsync(W->d_ctl, 0, kClasses * sizeof(unsigned int), W->stream));
  Args A;
  A.model = W->d_model, A.seqs = W->d_seqs, A.events = W->d_events, A.flank = W->d_flank, A.logsum = W->d_logsum;
  A.scores = W->d_scores, A.T = tables().trans;
  GB_HIP(hipEventRecord(W->ev[0], W->stream));
  for (int c = 0; c < kClasses; ++c) {
    if (!slots[c]) continue;
    A.items = W->d_items.get() + first[c], A.n_slots = slots[c], A.next = W->d_ctl.get() + c;
    const int waves = c < 2 ? kWavesSmall : kWavesLarge;
    const int64_t want = (slots[c] + waves - 1) / waves;
    const dim3 grid((unsigned)std::min<int64_t>(want, (int64_t)W->num_cus * kBlocksPerCU)), block(64 * waves);
    if (c == 0)
      hipLaunchKernelGGL((abea_hmm_kernel<1, true, kWavesSmall>), grid, block, 0, W->stream, A);
    else if (c == 1)
      hipLaunchKernelGGL((abea_hmm_kernel<1, false, kWavesSmall>), grid, block, 0, W->stream, A);
    else if (c == 2)
      hipLaunchKernelGGL((abea_hmm_kernel<2, false, kWavesLarge>), grid, block, 0, W->stream, A);
    else
      hipLaunchKernelGGL((abea_hmm_kernel<4, false, kWavesLarge>), grid, block, 0, W->stream, A);
    GB_HIP(hipGetLastError());
  }
  GB_HIP(hipEventRecord(W->ev[1], W->stream));
  GB_HIP(hipMemcpyAsync(W->h_scores, W->d_scores, (size_t)n_items * sizeof(float), hipMemcpyDeviceToHost, W->stream));
  GB_HIP(hipStreamSynchronize(W->stream));
  GB_HIP(hipEventElapsedTime(&W->kernel_ms, W->ev[0], W->ev[1]));
  std::memcpy(scores, W->h_scores.get(), (size_t)n_items * sizeof(float));
  return GB_OK;
}

}  // namespace gbhmm

extern "C" {

int gb_abea_hmm_logsum_table(float *out) {
  GB_ARG(out, "gb_abea_hmm_logsum_table: null argument");
  std::memcpy(out, gbhmm::tables().logsum, sizeof(float) * gbhmm::kTbl);
  return GB_OK;
}

int gb_abea_hmm_timing(float *kernel_ms, int64_t *cells) {
  GB_ARG(kernel_ms && cells, "gb_abea_hmm_timing: null argument");
  const gbhmm::Ws *W = nullptr;
  if (const int st = gb::ran_ws("gb_abea_hmm_timing", "gb_abea_hmm_score", &W, &gbhmm::Ws::calls)) return st;
  *kernel_ms = W->kernel_ms, *cells = W->cells;
  return GB_OK;
}

int gb_abea_hmm_score(const gb_abea_model *cpg_model, const char *seqs, int64_t seq_bytes, const float *event_mean,
                      int64_t n_event_total, const gb_abea_hmm_read *reads, int64_t n_reads,
                      const gb_abea_hmm_item *items, int64_t n_items, float *scores) {
  using namespace gbhmm;
  const char *who = "gb_abea_hmm_score";
  gb::Range range_("gb.abea.hmm_score");
  try {
    std::vector<Trans> trans;
    int st = validate(who, cpg_model, GB_ABEA_HMM_MODEL_SIZE, 1, 3, seqs, seq_bytes, event_mean, n_event_total, reads, n_reads,
                      items, n_items, scores, &trans);
    if (st || n_items == 0) return st;
    if (gb::env_flag("GB_ABEA_HOST")) {
      int nth = 1;
      if ((st = gb::thread_count(who, "GB_ABEA_THREADS", &nth))) return st;
      const Tables &tb = tables();
      std::vector<float> out((size_t)n_items);
      std::atomic<int64_t> next{0};
      if ((st = gb::parallel(who, (int)std::min<int64_t>(nth, n_items), [&](int) {
             std::vector<State> rows;
             std::vector<Kmer> kmers;
             for (int64_t i; (i = next.fetch_add(1)) < n_items;) {
               const gb_abea_hmm_item &it = items[i];
               const gb_abea_hmm_read &rd = reads[it.read];
               out[(size_t)i] = host_score(cpg_model, tb, seqs + it.seq_off, it, event_mean + rd.event_off, rd,
                                           trans[(size_t)it.read], &rows, &kmers);
             }
           })))
        return st;
      std::memcpy(scores, out.data(), (size_t)n_items * sizeof(float));
      return GB_OK;
    }
    int dev = 0;
    GB_HIP(hipGetDevice(&dev));
    Ws *W = nullptr;
    if ((st = gb::get_ws(who, dev, &W, make_tables))) return st;
    W->calls = 0;
    if ((st = W->d_model.reserve(GB_ABEA_HMM_MODEL_SIZE)) || (st = W->d_seqs.reserve((size_t)seq_bytes)) ||
        (st = W->d_events.reserve((size_t)n_event_total)))
      return st;
    GB_HIP(hipMemcpyAsync(W->d_model, cpg_model, GB_ABEA_HMM_MODEL_SIZE * sizeof(Model), hipMemcpyHostToDevice, W->stream));
    GB_HIP(hipMemcpyAsync(W->d_seqs, seqs, (size_t)seq_bytes, hipMemcpyHostToDevice, W->stream));
    GB_HIP(hipMemcpyAsync(W->d_events, event_mean, (size_t)n_event_total * sizeof(float), hipMemcpyHostToDevice,
                          W->stream));
    if ((st = run_device(W, reads, items, n_items, trans, scores))) return st;
    W->calls = 1;
    return GB_OK;
  } catch (const std::bad_alloc &) {
    gb::set_error("%s: out of host memory", who);
    return GB_ERR_NOMEM;
  }
}

}  // extern "C"
