// bsw_abea.hip -- gb_abea_align: adaptive banded event alignment (f5c / nanopolish align(), align.c:169-548).
//
// One read per wave64 from a persistent grid with an atomic work counter. A band of 100 cells is two
// adjacent offsets per lane (lanes 0..49); the last two bands, the lanes' event means and their k-mers'
// model values live in registers and move by wave-wide one-lane shifts, since a band step moves the whole
// band one event down or one k-mer right. The trace is 32 bytes per band in the wave's workspace slice
// (four 64-bit bit planes, two per offset parity, with the band's count of right moves in their spare top
// bits); the same wave walks it back right after its fill. A chunk's reads run longest first, one launch per
// length class, so that the slices are sized by the class and not by the chunk. GB_ABEA_HOST=1 runs the plain C++ restatement
// below instead; both paths share the cell, emission, trim and end-score functions.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/gb_bsw_abea.h"
#include "gb_common.h"
#include "gb_common_wave.h"

namespace gbabea {

constexpr int kBW = GB_ABEA_BANDWIDTH, kK = GB_ABEA_K, kHalf = kBW / 2;
constexpr int kFromD = 0, kFromU = 1, kFromL = 2;
constexpr int kWavesPerBlock = 4, kBlocksPerCU = 3;  // 48 KB of model per block, 160 KB of LDS per CU
constexpr int kTraceWords = 8;                       // 32 bytes per band
constexpr int64_t kDefaultWsBytes = int64_t(1) << 30;
constexpr float kNegInf = -INFINITY;

using Model = gb_abea_model;

struct Consts {  // align.c:196-205, host libm in double
  double lp_skip, lp_stay, lp_step, lp_trim;
};

// ---- the arithmetic, one text for host and device (no contraction: -ffp-contract=off) ----

#define GB_HD __host__ __device__ __forceinline__

GB_HD float gp_mean(float scale, float shift, float level_mean) { return scale * level_mean + shift; }

// log_normal_pdf (align.c:99-106), f32 throughout, correctly rounded division
GB_HD float emission(float x, float mean, float stdv, float log_stdv) {
  const float a = (x - mean) / stdv;
  return -0.918938f - log_stdv + (-0.5f * a * a);
}

// align.c:371-381: the sums are double, each score is rounded to float; D first, U replaces on >, from is U
// on ==, then the same for L
GB_HD float cell(float diag, float up, float left, float em, const Consts &c, int *from) {
  const float score_d = (float)((double)diag + c.lp_step + (double)em);
  const float score_u = (float)((double)up + c.lp_stay + (double)em);
  const float score_l = (float)((double)left + c.lp_skip);
  float m = score_d;
  int f = kFromD;
  m = score_u > m ? score_u : m;
  f = m == score_u ? kFromU : f;
  m = score_l > m ? score_l : m;
  f = m == score_l ? kFromL : f;
  *from = f;
  return m;
}

GB_HD float trim_score(double lp_trim, int event_idx) { return (float)(lp_trim * (double)((int64_t)event_idx + 1)); }

GB_HD float end_score(float band, int events_left, double lp_trim) {
  return (float)((double)band + (double)events_left * lp_trim);
}

GB_HD int base_rank(char b) { return b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 0; }

GB_HD int kmer_rank(const char *s) {
  int r = 0;
#pragma unroll
  for (int i = 0; i < kK; ++i) r = (r << 2) | base_rank(s[i]);
  return r;
}

static Consts make_consts(int n_events, int n_kmers) {
  Consts c;
  const double events_per_kmer = (double)n_events / n_kmers;
  const double p_stay = 1 - (1 / (events_per_kmer + 1));
  const double epsilon = 1e-10;
  c.lp_skip = log(epsilon);
  c.lp_stay = log(p_stay);
  c.lp_step = log(1.0 - exp(c.lp_skip) - exp(c.lp_stay));
  c.lp_trim = log(0.01);
  return c;
}

// align.c:515-532 on what a walk leaves; host side for both paths
static void finish_stat(gb_abea_stat *s) {
  s->pad = 0, s->pad2 = 0.f;
  if (s->no_end_cell) {
    s->n_raw = s->n_pairs = 0;
    return;
  }
  const double avg_log_emission = s->sum_emission / (double)s->n_raw;
  const bool fail = avg_log_emission < -5.0 || !s->spanned || s->max_gap > 50;
  s->n_pairs = fail ? 0 : s->n_raw;
}

// ---- host path: align() restated, with rolling bands, one trace byte per cell and k_b per band ----

struct HostScratch {
  std::vector<uint8_t> trace;
  std::vector<int32_t> kll;
  std::vector<int32_t> ranks;
};

// Writes the walk backwards from region[cap - 1], so region[cap - n_raw .. cap) is the final order.
static void host_align(const Model *model, const char *seq, int seq_len, const float *ev, int n_events, float scale,
                       float shift, gb_abea_pair *region, int64_t cap, gb_abea_stat *st, HostScratch *S) {
  const int n_kmers = seq_len - kK + 1;
  const int n_bands = n_events + n_kmers + 2;
  const Consts C = make_consts(n_events, n_kmers);
  S->trace.assign((size_t)n_bands * kBW, 0);
  S->kll.assign((size_t)n_bands, 0);
  S->ranks.resize((size_t)n_kmers);
  for (int i = 0; i < n_kmers; ++i) S->ranks[(size_t)i] = kmer_rank(seq + i);
  float bands[3][kBW];
  for (auto &b : bands)
    for (float &v : b) v = kNegInf;
  int e_b = kHalf - 1, k_b = -1 - kHalf;
  S->kll[0] = k_b;
  bands[0][kHalf] = 0.0f;  // the start cell (-1, -1)
  e_b += 1;
  S->kll[1] = k_b;
  bands[1][kHalf] = (float)C.lp_trim;  // band 1: the first event is trimmed
  S->trace[(size_t)kBW + kHalf] = kFromU;
  int fills = 0;
  float best = kNegInf;
  int best_ev = 0;
  for (int b = 2; b < n_bands; ++b) {
    const float *P = bands[(b - 1) % 3], *Q = bands[(b - 2) % 3];
    float *N = bands[b % 3];
    const float ll = P[0], ur = P[kBW - 1];
    const bool right = (ll == kNegInf && ur == kNegInf) ? (b % 2 == 1) : ll < ur;
    if (right)
      k_b += 1;
    else
      e_b += 1;
    S->kll[(size_t)b] = k_b;
    const int e_p = right ? e_b : e_b - 1, k_p = right ? k_b - 1 : k_b;  // band b - 1
    const int k_q = S->kll[(size_t)b - 2];
    uint8_t *T = &S->trace[(size_t)b * kBW];
    for (int o = 0; o < kBW; ++o) N[o] = kNegInf;
    const int trim_off = -1 - k_b;
    if (trim_off >= 0 && trim_off < kBW) {
      const int event_idx = e_b - trim_off;
      if (event_idx >= 0 && event_idx < n_events) {
        N[trim_off] = trim_score(C.lp_trim, event_idx);
        T[trim_off] = kFromU;
      }
    }
    const int min_off = std::max(std::max(-k_b, e_b - (n_events - 1)), 0);
    const int max_off = std::min(std::min(n_kmers - k_b, e_b + 1), kBW);
    for (int o = min_off; o < max_off; ++o) {
      const int event_idx = e_b - o, kmer_idx = k_b + o;
      const int o_up = e_p - (event_idx - 1), o_left = (kmer_idx - 1) - k_p, o_diag = (kmer_idx - 1) - k_q;
      const float up = o_up >= 0 && o_up < kBW ? P[o_up] : kNegInf;
      const float left = o_left >= 0 && o_left < kBW ? P[o_left] : kNegInf;
      const float diag = o_diag >= 0 && o_diag < kBW ? Q[o_diag] : kNegInf;
      const Model &m = model[S->ranks[(size_t)kmer_idx]];
      const float em = emission(ev[event_idx], gp_mean(scale, shift, m.level_mean), m.level_stdv, m.level_log_stdv);
      int from;
      N[o] = cell(diag, up, left, em, C, &from);
      T[o] = (uint8_t)from;
      fills += 1;
    }
    // the end scan (align.c:418-434), folded in: this band's (event, last k-mer) cell, events ascending
    const int ev_end = b - 1 - n_kmers, o_end = n_kmers - 1 - k_b;
    if (ev_end >= 0 && ev_end < n_events && o_end >= 0 && o_end < kBW) {
      const float s = end_score(N[o_end], n_events - ev_end, C.lp_trim);
      if (s > best) best = s, best_ev = ev_end;
    }
  }
  std::memset(st, 0, sizeof(*st));
  st->fills = fills;
  st->end_score = best;
  st->end_event = best_ev;
  if (!(best > kNegInf)) {
    st->no_end_cell = 1;
    finish_stat(st);
    return;
  }
  int ev_i = best_ev, km_i = n_kmers - 1, n = 0, gap = 0, max_gap = 0;
  const int max_steps = n_events + n_kmers;
  double sum = 0;
  while (n < max_steps && km_i >= 0 && ev_i >= 0) {
    region[cap - 1 - n] = gb_abea_pair{km_i, ev_i};
    ++n;
    const Model &m = model[S->ranks[(size_t)km_i]];
    sum += emission(ev[ev_i], gp_mean(scale, shift, m.level_mean), m.level_stdv, m.level_log_stdv);
    const int b = ev_i + km_i + 2;
    const int from = S->trace[(size_t)b * kBW + (size_t)(km_i - S->kll[(size_t)b])];
    if (from == kFromD) {
      km_i -= 1, ev_i -= 1, gap = 0;
    } else if (from == kFromU) {
      ev_i -= 1, gap = 0;
    } else {
      km_i -= 1, gap += 1;
      max_gap = std::max(gap, max_gap);
    }
  }
  st->n_raw = n;
  st->max_gap = max_gap;
  st->spanned = km_i < 0 || region[cap - n].ref_pos == 0;
  st->sum_emission = sum;
  finish_stat(st);
}

// ---- device path ----

struct DRead {
  int64_t seq_off, event_off, region_end;  // the walk's first pair goes to pairs[region_end - 1]
  int32_t seq_len, n_events;
  float scale, shift;
  double lp_stay, lp_step;
};

struct Args {
  const Model *model;
  const char *seqs;
  const float *events;
  const DRead *reads;
  const int32_t *order;  // this launch's reads, longest first
  int64_t n;
  gb_abea_pair *pairs;
  uint32_t *stats;  // 12 words per read, gb_abea_stat's layout
  uint32_t *trace;
  int64_t slot_words;
  int n_waves;
  unsigned int *next;
  unsigned long long *cycles;  // per wave: fill, walk, summed over a chunk's launches
  double lp_skip, lp_trim;
};

__device__ __forceinline__ float readlane_f(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
// lane l takes lane l-1's v, lane 0 takes lane0
__device__ __forceinline__ float shr1_f(float v, float lane0) {
  return __int_as_float(gb::wave_shr1(__float_as_int(v), __float_as_int(lane0)));
}
// lane l takes lane l+1's v, lane 63 takes lane63 (wave_shl:1, bound_ctrl off)
__device__ __forceinline__ float shl1_f(float v, float lane63) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(lane63), __float_as_int(v), 0x130, 0xF, 0xF, false));
}

// model values of k-mer `kmer` as the cells use them; anything for a k-mer outside the read (such cells are
// outside [min_offset, max_offset) and never computed into a band)
__device__ __forceinline__ void load_kmer(const char *seq, const Model *sm, int kmer, int n_kmers, float scale,
                                          float shift, float *gm, float *sd, float *ls) {
  *gm = 0.f, *sd = 1.f, *ls = 0.f;
  if (kmer >= 0 && kmer < n_kmers) {
    const Model m = sm[kmer_rank(seq + kmer)];
    *gm = gp_mean(scale, shift, m.level_mean), *sd = m.level_stdv, *ls = m.level_log_stdv;
  }
}
__device__ __forceinline__ float load_event(const float *evs, int idx, int n_events) {
  return idx >= 0 && idx < n_events ? evs[idx] : 0.f;
}

__device__ __forceinline__ void align_wave(const Args &A, const Model *sm, const DRead &R, uint32_t *tr, int lane,
                                           uint32_t *stat_out, unsigned long long *t_fill,
                                           unsigned long long *t_walk) {
  const long long t0 = clock64();
  const int n_events = R.n_events, n_kmers = R.seq_len - kK + 1;
  const int n_bands = n_events + n_kmers + 2;  // the trip count of the fill, known before it starts
  const char *seq = A.seqs + R.seq_off;
  const float *evs = A.events + R.event_off;
  const float scale = R.scale, shift = R.shift;
  const Consts C{A.lp_skip, R.lp_stay, R.lp_step, A.lp_trim};
  const int o0 = 2 * lane, o1 = 2 * lane + 1;

  // bands 0 (Q) and 1 (P); lanes 50..63 hold -inf for good
  float Q0 = o0 == kHalf ? 0.0f : kNegInf, Q1 = kNegInf;
  float P0 = o0 == kHalf ? (float)C.lp_trim : kNegInf, P1 = kNegInf;
  int e_b = kHalf, k_b = -1 - kHalf;  // band 1's lower left
  int r_prev = 0, rights = 0;
  // the lanes' events and k-mers at band 1
  float ev0 = load_event(evs, e_b - o0, n_events), ev1 = load_event(evs, e_b - o1, n_events);
  float gm0, sd0, ls0, gm1, sd1, ls1;
  load_kmer(seq, sm, k_b + o0, n_kmers, scale, shift, &gm0, &sd0, &ls0);
  load_kmer(seq, sm, k_b + o1, n_kmers, scale, shift, &gm1, &sd1, &ls1);
  // windows of what enters next: the event at offset 0 after a down move, the k-mer at offset 99 after a
  // right move; lane j holds index base + j
  int fe_base = e_b + 1, fk_base = k_b + kBW;
  float wev = load_event(evs, fe_base + lane, n_events);
  float wgm, wsd, wls;
  load_kmer(seq, sm, fk_base + lane, n_kmers, scale, shift, &wgm, &wsd, &wls);
  if (lane < 2 * kTraceWords) tr[lane] = 0;  // bands 0 and 1 hold no cell a walk visits

  int fills = 0, best_ev = 0;
  float best = kNegInf;
  for (int b = 2; b < n_bands; ++b) {
    // placement (align.c:289-311): from band b-1's offsets 0 and 99, after its fill
    const float ll = readlane_f(P0, 0), ur = readlane_f(P1, kHalf - 1);
    const bool right = (ll == kNegInf && ur == kNegInf) ? (b & 1) : ll < ur;
    float up0, up1, left0, left1;
    if (right) {
      k_b += 1, rights += 1;
      int j = k_b + kBW - 1 - fk_base;
      if (j >= 64) {
        fk_base += 64, j -= 64;
        load_kmer(seq, sm, fk_base + lane, n_kmers, scale, shift, &wgm, &wsd, &wls);
      }
      const float ngm = readlane_f(wgm, j), nsd = readlane_f(wsd, j), nls = readlane_f(wls, j);
      const float tg = shl1_f(gm0, 0.f), ts = shl1_f(sd0, 1.f), tl = shl1_f(ls0, 0.f);
      gm0 = gm1, sd0 = sd1, ls0 = ls1;
      gm1 = lane == kHalf - 1 ? ngm : tg, sd1 = lane == kHalf - 1 ? nsd : ts, ls1 = lane == kHalf - 1 ? nls : tl;
      up0 = P1, up1 = shl1_f(P0, kNegInf), left0 = P0, left1 = P1;
    } else {
      e_b += 1;
      int j = e_b - fe_base;
      if (j >= 64) {
        fe_base += 64, j -= 64;
        wev = load_event(evs, fe_base + lane, n_events);
      }
      const float nev = readlane_f(wev, j);
      const float t = shr1_f(ev1, nev);
      ev1 = ev0, ev0 = t;
      up0 = P0, up1 = P1, left0 = shr1_f(P1, kNegInf), left1 = P0;
    }
    const int r2 = (right ? 1 : 0) + r_prev;
    float d0, d1;
    if (r2 == 0)
      d0 = shr1_f(Q1, kNegInf), d1 = Q0;
    else if (r2 == 1)
      d0 = Q0, d1 = Q1;
    else
      d0 = Q1, d1 = shl1_f(Q0, kNegInf);

    const int min_off = max(max(-k_b, e_b - (n_events - 1)), 0);
    const int max_off = min(min(n_kmers - k_b, e_b + 1), kBW);
    const int trim_off = -1 - k_b, trim_ev = e_b - trim_off;
    const bool trim_ok = trim_off >= 0 && trim_off < kBW && trim_ev >= 0 && trim_ev < n_events;
    const float trim_val = trim_score(C.lp_trim, trim_ev);
    int f0, f1;
    const float c0 = cell(d0, up0, left0, emission(ev0, gm0, sd0, ls0), C, &f0);
    const float c1 = cell(d1, up1, left1, emission(ev1, gm1, sd1, ls1), C, &f1);
    const bool in0 = o0 >= min_off && o0 < max_off, in1 = o1 >= min_off && o1 < max_off;
    const bool tr0 = trim_ok && o0 == trim_off, tr1 = trim_ok && o1 == trim_off;
    const float N0 = in0 ? c0 : tr0 ? trim_val : kNegInf, N1 = in1 ? c1 : tr1 ? trim_val : kNegInf;
    f0 = in0 ? f0 : tr0 ? kFromU : 0, f1 = in1 ? f1 : tr1 ? kFromU : 0;
    fills += max(max_off - min_off, 0);

    // the band's trace: four bit planes over the lanes, the count of right moves in the spare top bits
    const unsigned long long m0 = __ballot(f0 & 1), m1 = __ballot(f0 & 2), m2 = __ballot(f1 & 1),
                             m3 = __ballot(f1 & 2);
    const uint32_t w1 = (uint32_t)(m0 >> 32) | ((uint32_t)(rights & 0x3fff) << 18);
    const uint32_t w3 = (uint32_t)(m1 >> 32) | ((uint32_t)((rights >> 14) & 0x3fff) << 18);
    uint32_t w = (uint32_t)m0;
    w = lane == 1 ? w1 : w;
    w = lane == 2 ? (uint32_t)m1 : w;
    w = lane == 3 ? w3 : w;
    w = lane == 4 ? (uint32_t)m2 : w;
    w = lane == 5 ? (uint32_t)(m2 >> 32) : w;
    w = lane == 6 ? (uint32_t)m3 : w;
    w = lane == 7 ? (uint32_t)(m3 >> 32) : w;
    if (lane < kTraceWords) tr[(int64_t)b * kTraceWords + lane] = w;

    // the end scan (align.c:418-434), folded in: events ascend with the bands, first maximum wins
    const int ev_end = b - 1 - n_kmers, o_end = n_kmers - 1 - k_b;
    if (ev_end >= 0 && ev_end < n_events && o_end >= 0 && o_end < kBW) {
      const float bv = readlane_f((o_end & 1) ? N1 : N0, o_end >> 1);
      const float s = end_score(bv, n_events - ev_end, C.lp_trim);
      if (s > best) best = s, best_ev = ev_end;
    }
    Q0 = P0, Q1 = P1, P0 = N0, P1 = N1;
    r_prev = right ? 1 : 0;
  }
  __threadfence_block();  // lanes 0..7 stored the trace, every lane loads it
  const long long t1 = clock64();

  const bool no_end = !(best > kNegInf);
  int n = 0, max_gap = 0, km_i = n_kmers - 1, ev_i = best_ev, last_km = -1;
  double sum = 0;
  if (!no_end) {
    // The walk. A finite cell's chosen predecessor is finite and was read from inside its band, so from
    // a finite end cell only finite in-band cells are visited. Windows of 64 bands' trace, 64 events and 64
    // k-mers' model values, lane j holding index lo + j, refilled as the walk passes below them.
    const int max_steps = n_events + n_kmers;
    int wlo = INT_MAX, ewlo = INT_MAX, kwlo = INT_MAX, gap = 0;
    uint4 ta = make_uint4(0, 0, 0, 0), tb = ta;
    float xw = 0.f, kgm = 0.f, ksd = 1.f, kls = 0.f;
    int pk = 0, pe = 0;
    for (; n < max_steps && km_i >= 0 && ev_i >= 0; ++n) {
      const int b = ev_i + km_i + 2;
      if (b < wlo) {
        wlo = b - 63;
        if (wlo + lane >= 0) {
          const uint4 *src = reinterpret_cast<const uint4 *>(tr + (int64_t)(wlo + lane) * kTraceWords);
          ta = src[0], tb = src[1];
        }
      }
      if (ev_i < ewlo) {
        ewlo = ev_i - 63;
        xw = load_event(evs, ewlo + lane, n_events);
      }
      if (km_i < kwlo) {
        kwlo = km_i - 63;
        load_kmer(seq, sm, kwlo + lane, n_kmers, scale, shift, &kgm, &ksd, &kls);
      }
      if (lane == (n & 63)) pk = km_i, pe = ev_i;
      last_km = km_i;
      if ((n & 63) == 63) A.pairs[R.region_end - 1 - (int64_t)(n - 63 + lane)] = gb_abea_pair{pk, pe};
      const int kj = km_i - kwlo;
      const float em =
          emission(readlane_f(xw, ev_i - ewlo), readlane_f(kgm, kj), readlane_f(ksd, kj), readlane_f(kls, kj));
      sum += (double)em;
      // every lane decodes its own band at the offset the cell would have there; lane b - wlo is right
      const int own_rights = (int)(ta.y >> 18) | ((int)(ta.w >> 18) << 14);
      const int o = km_i - (own_rights - 1 - kHalf);
      const int l = (o >> 1) & 63;
      const unsigned long long lo_pl = (o & 1) ? ((unsigned long long)tb.y << 32 | tb.x)
                                               : ((unsigned long long)ta.y << 32 | ta.x);
      const unsigned long long hi_pl = (o & 1) ? ((unsigned long long)tb.w << 32 | tb.z)
                                               : ((unsigned long long)ta.w << 32 | ta.z);
      const int own_from = (int)((lo_pl >> l) & 1) | ((int)((hi_pl >> l) & 1) << 1);
      const int from = __builtin_amdgcn_readlane(own_from, b - wlo);
      if (from == kFromD) {
        km_i -= 1, ev_i -= 1, gap = 0;
      } else if (from == kFromU) {
        ev_i -= 1, gap = 0;
      } else {
        km_i -= 1, gap += 1;
        max_gap = max(gap, max_gap);
      }
    }
    if (lane < (n & 63)) A.pairs[R.region_end - 1 - (int64_t)((n & ~63) + lane)] = gb_abea_pair{pk, pe};
  }
  // gb_abea_stat, one word per lane (no store under `lane == 0` next to the work counter's branch, see
  // bsw_global.hip); n_pairs and the pads are the host's
  const unsigned long long sum_bits = (unsigned long long)__double_as_longlong(sum);
  uint32_t v = 0;
  v = lane == 1 ? (uint32_t)n : v;
  v = lane == 2 ? (uint32_t)max_gap : v;
  v = lane == 3 ? (uint32_t)(last_km == 0) : v;
  v = lane == 4 ? (uint32_t)best_ev : v;
  v = lane == 5 ? (uint32_t)no_end : v;
  v = lane == 6 ? (uint32_t)fills : v;
  v = lane == 8 ? (uint32_t)__float_as_int(best) : v;
  v = lane == 10 ? (uint32_t)sum_bits : v;
  v = lane == 11 ? (uint32_t)(sum_bits >> 32) : v;
  if (lane < 12) stat_out[lane] = v;
  const long long t2 = clock64();
  *t_fill += (unsigned long long)(t1 - t0);
  *t_walk += (unsigned long long)(t2 - t1);
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void abea_fill_kernel(Args A) {
  __shared__ Model smodel[GB_ABEA_MODEL_SIZE];
  for (int i = threadIdx.x; i < GB_ABEA_MODEL_SIZE; i += 64 * kWavesPerBlock) smodel[i] = A.model[i];
  __syncthreads();  // the kernel's only block-wide meeting; waves beyond the grid's count leave after it
  const int lane = threadIdx.x & 63;
  const int wave = (int)blockIdx.x * kWavesPerBlock + (int)(threadIdx.x >> 6);
  if (wave >= A.n_waves) return;
  uint32_t *tr = A.trace + (int64_t)wave * A.slot_words;
  unsigned long long t_fill = 0, t_walk = 0;
  for (;;) {
    unsigned int p = 0;
    if (lane == 0) p = atomicAdd(A.next, 1u);
    p = __builtin_amdgcn_readfirstlane(p);
    if ((int64_t)p >= A.n) break;
    const int32_t r = A.order[p];
    const DRead R = A.reads[r];
    align_wave(A, smodel, R, tr, lane, A.stats + 12 * (int64_t)r, &t_fill, &t_walk);
    // the whole wave meets here before any lane fetches the next read (see bsw_global.hip)
    __builtin_amdgcn_wave_barrier();
  }
  // launches of one chunk follow each other on one stream, and a slot of the sums is its wave's alone
  if (lane >= 1 && lane < 3) A.cycles[2 * (int64_t)wave + (lane - 1)] += lane == 1 ? t_fill : t_walk;
}

static_assert(sizeof(gb_abea_stat) == 48, "gb_abea_stat is 12 words on the device");
static_assert(sizeof(Model) == 12, "gb_abea_model is three floats");

struct Ws : gb::WsBase<2> {  // the calling thread's, through gb::get_ws
  gb::DevBuf<Model> d_model;
  gb::DevBuf<char> d_seqs;
  gb::DevBuf<float> d_events;
  gb::DevBuf<DRead> d_reads;
  gb::DevBuf<int32_t> d_order;
  gb::PinnedBuf<int32_t> h_order;
  gb::DevBuf<gb_abea_pair> d_pairs;
  gb::DevBuf<uint32_t> d_stats, d_trace;
  gb::DevBuf<unsigned int> d_ctl;
  gb::DevBuf<unsigned long long> d_cycles;
  gb::PinnedBuf<DRead> h_reads;
  gb::PinnedBuf<gb_abea_pair> h_pairs;
  gb::PinnedBuf<uint32_t> h_stats;
  gb::PinnedBuf<unsigned long long> h_cycles;
  float fill_ms = 0.f, trace_ms = 0.f;
  int64_t cells = 0, chunks = 0, waves = 0, ws_bytes = 0;
};

struct Need {  // of a read: its bands, n_events + n_kmers + 2, a pair each in the chunk's pair region
  int64_t bands;
  int64_t bytes() const { return bands * (int64_t)sizeof(gb_abea_pair); }
  void operator+=(const Need &o) { bands += o.bands; }
};
using Chunk = gb::Chunk<Need>;  // of the call's reads

static inline int64_t read_bands(const gb_abea_read &r) { return (int64_t)r.n_events + (r.seq_len - kK + 1) + 2; }

// Every refusal of include/gb_bsw_abea.h, before any device work.
static int validate(const gb_abea_model *model, const char *seqs, int64_t seq_bytes, const float *event_mean,
                    int64_t n_event_total, const gb_abea_read *reads, int64_t n_reads, const gb_abea_pair *pairs,
                    int64_t pair_cap, const int64_t *pair_off, const gb_abea_stat *stats) {
  const char *who = "gb_abea_align";
  GB_ARG(n_reads >= 0 && (n_reads == 0 || (reads && stats && model)) && pair_off, "%s: bad arguments", who);
  GB_ARG(seq_bytes >= 0 && n_event_total >= 0 && (seq_bytes == 0 || seqs) && (n_event_total == 0 || event_mean),
         "%s: bad sequence or event buffers", who);
  GB_ARG(pair_cap >= 0 && (pair_cap == 0 || pairs), "%s: bad pair buffer", who);
  if (n_reads == 0) return GB_OK;
  for (int k = 0; k < GB_ABEA_MODEL_SIZE; ++k) {
    const gb_abea_model &m = model[k];
    GB_ARG(std::isfinite(m.level_stdv) && m.level_stdv > 0.f,
           "%s: model entry %d has level_stdv %g (need finite and > 0)", who, k, (double)m.level_stdv);
    GB_ARG(std::isfinite(m.level_mean) && std::isfinite(m.level_log_stdv), "%s: model entry %d is not finite", who, k);
  }
  for (int64_t r = 0; r < n_reads; ++r) {
    const gb_abea_read &s = reads[r];
    GB_ARG(s.seq_len >= kK && s.seq_len <= GB_ABEA_MAX_SEQ_LEN, "%s: read %lld has seq_len %d (need %d..%d)", who,
           (long long)r, s.seq_len, kK, GB_ABEA_MAX_SEQ_LEN);
    GB_ARG(s.n_events >= 1 && s.n_events <= GB_ABEA_MAX_EVENTS, "%s: read %lld has n_events %d (need 1..%d)", who,
           (long long)r, s.n_events, GB_ABEA_MAX_EVENTS);
    GB_ARG(s.seq_off >= 0 && s.seq_off <= seq_bytes - s.seq_len && s.event_off >= 0 &&
               s.event_off <= n_event_total - s.n_events,
           "%s: read %lld lies outside the sequence or event buffer", who, (long long)r);
    GB_ARG(std::isfinite(s.scale) && std::isfinite(s.shift), "%s: read %lld has scale %g, shift %g (need finite)", who,
           (long long)r, (double)s.scale, (double)s.shift);
    const float *e = event_mean + s.event_off;
    for (int32_t i = 0; i < s.n_events; ++i)
      GB_ARG(std::isfinite(e[i]), "%s: read %lld has event %d with a mean that is not finite", who, (long long)r, i);
  }
  return GB_OK;
}

// Chunks of reads whose pair regions (8 bytes per band) fit region_bytes, one read at the least: a read whose
// region alone does not fit is a chunk of its own.
static std::vector<Chunk> make_chunks(const gb_abea_read *reads, int64_t n_reads, int64_t region_bytes) {
  std::vector<Chunk> out;
  (void)gb::cut_chunks(n_reads, region_bytes, [&](int64_t r) { return Need{read_bands(reads[r])}; }, &out);
  return out;
}

static int run_chunk_device(Ws *W, const gb_abea_read *reads, const Chunk &c, int64_t slice_bytes, gb_abea_stat *stats) {
  int st;
  const int64_t m = c.last - c.first;
  if ((st = W->h_reads.reserve((size_t)m)) || (st = W->d_reads.reserve((size_t)m))) return st;
  if ((st = W->h_pairs.reserve((size_t)c.need.bands)) || (st = W->d_pairs.reserve((size_t)c.need.bands))) return st;
  if ((st = W->h_stats.reserve((size_t)m * 12)) || (st = W->d_stats.reserve((size_t)m * 12))) return st;
  if ((st = W->h_order.reserve((size_t)m)) || (st = W->d_order.reserve((size_t)m))) return st;
  // The reads longest first, cut into launches by length class (bands up to 4096, then per power of two): a
  // launch's trace slices are sized by its own longest read, so the short reads, which are most reads, run
  // on a full grid. Per launch the grid is what the device holds, what the launch can use, and what the
  // trace half of the budget holds, one wave at the least.
  struct Launch {
    int64_t first, count, slot_words, n_waves;
  };
  std::vector<Launch> launches;
  int32_t *order = W->h_order;
  for (int64_t k = 0; k < m; ++k) order[k] = (int32_t)k;
  std::stable_sort(order, order + m, [&](int32_t a, int32_t b) { return read_bands(reads[c.first + a]) > read_bands(reads[c.first + b]); });
  int64_t cur_class = -1, max_waves = 1, trace_words = 0;
  for (int64_t k = 0; k < m; ++k) {
    const int64_t nb = read_bands(reads[c.first + order[k]]);
    int64_t cls = 4096;
    while (cls < nb) cls *= 2;
    if (cls != cur_class) {
      launches.push_back(Launch{k, 0, nb * kTraceWords, 0});
      cur_class = cls;
    }
    launches.back().count += 1;
  }
  for (Launch &l : launches) {
    const int64_t want = std::min<int64_t>((int64_t)W->num_cus * kBlocksPerCU * kWavesPerBlock, l.count);
    const int64_t fit = slice_bytes / (l.slot_words * (int64_t)sizeof(uint32_t));
    l.n_waves = std::max<int64_t>(1, std::min(want, fit));
    max_waves = std::max(max_waves, l.n_waves);
    trace_words = std::max(trace_words, l.n_waves * l.slot_words);
  }
  if ((st = W->d_trace.reserve((size_t)trace_words))) return st;
  if ((st = W->d_cycles.reserve((size_t)max_waves * 2)) || (st = W->h_cycles.reserve((size_t)max_waves * 2))) return st;
  W->waves = std::max(W->waves, max_waves);
  W->ws_bytes = std::max<int64_t>(
      W->ws_bytes, trace_words * (int64_t)sizeof(uint32_t) + c.need.bands * (int64_t)sizeof(gb_abea_pair));
  DRead *hr = W->h_reads;
  int64_t end = 0;
  for (int64_t k = 0; k < m; ++k) {
    const gb_abea_read &s = reads[c.first + k];
    const Consts C = make_consts(s.n_events, s.seq_len - kK + 1);
    end += read_bands(s);
    hr[k] = DRead{s.seq_off, s.event_off, end, s.seq_len, s.n_events, s.scale, s.shift, C.lp_stay, C.lp_step};
  }
  const Consts C0 = make_consts(1, 1);
  GB_HIP(hipMemcpyAsync(W->d_reads, hr, (size_t)m * sizeof(DRead), hipMemcpyHostToDevice, W->stream));
  GB_HIP(hipMemcpyAsync(W->d_order, order, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, W->stream));
  GB_HIP(hipMemsetAsync(W->d_cycles, 0, (size_t)max_waves * 2 * sizeof(unsigned long long), W->stream));
  Args A;
  A.model = W->d_model, A.seqs = W->d_seqs, A.events = W->d_events, A.reads = W->d_reads;
  A.pairs = W->d_pairs, A.stats = W->d_stats, A.trace = W->d_trace;
  A.next = W->d_ctl, A.cycles = W->d_cycles;
  A.lp_skip = C0.lp_skip, A.lp_trim = C0.lp_trim;
  GB_HIP(hipEventRecord(W->ev[0], W->stream));
  for (const Launch &l : launches) {
    GB_HIP(hipMemsetAsync(W->d_ctl, 0, 4 * sizeof(unsigned int), W->stream));
    A.order = W->d_order.get() + l.first, A.n = l.count, A.slot_words = l.slot_words, A.n_waves = (int)l.n_waves;
    const int64_t blocks = (l.n_waves + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(abea_fill_kernel, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0, W->stream, A);
    GB_HIP(hipGetLastError());
  }
  GB_HIP(hipEventRecord(W->ev[1], W->stream));
  GB_HIP(hipMemcpyAsync(W->h_stats, W->d_stats, (size_t)m * 12 * sizeof(uint32_t), hipMemcpyDeviceToHost, W->stream));
  GB_HIP(hipMemcpyAsync(W->h_cycles, W->d_cycles, (size_t)max_waves * 2 * sizeof(unsigned long long),
                        hipMemcpyDeviceToHost, W->stream));
  GB_HIP(hipMemcpyAsync(W->h_pairs, W->d_pairs, (size_t)c.need.bands * sizeof(gb_abea_pair), hipMemcpyDeviceToHost,
                        W->stream));
  GB_HIP(hipStreamSynchronize(W->stream));
  float ms = 0.f;
  GB_HIP(hipEventElapsedTime(&ms, W->ev[0], W->ev[1]));
  double cf = 0, cw = 0;
  for (int64_t k = 0; k < max_waves; ++k) cf += (double)W->h_cycles[2 * k], cw += (double)W->h_cycles[2 * k + 1];
  const double share = cf + cw > 0 ? cf / (cf + cw) : 1.0;
  W->fill_ms += (float)(ms * share), W->trace_ms += (float)(ms * (1.0 - share));
  for (int64_t k = 0; k < m; ++k) {
    std::memcpy(&stats[c.first + k], W->h_stats.get() + 12 * k, sizeof(gb_abea_stat));
    finish_stat(&stats[c.first + k]);
    W->cells += stats[c.first + k].fills;
  }
  return GB_OK;
}

}  // namespace gbabea

extern "C" {

int gb_abea_align_timing(float *fill_ms, float *trace_ms, int64_t *cells) {
  GB_ARG(fill_ms && trace_ms && cells, "gb_abea_align_timing: null argument");
  const gbabea::Ws *W = nullptr;
  if (const int st = gb::ran_ws("gb_abea_align_timing", "gb_abea_align", &W, &gbabea::Ws::chunks)) return st;
  *fill_ms = W->fill_ms, *trace_ms = W->trace_ms, *cells = W->cells;
  return GB_OK;
}

int gb_abea_align_plan(int64_t *chunks, int64_t *waves, int64_t *ws_bytes) {
  GB_ARG(chunks && waves && ws_bytes, "gb_abea_align_plan: null argument");
  const gbabea::Ws *W = nullptr;
  if (const int st = gb::ran_ws("gb_abea_align_plan", "gb_abea_align", &W, &gbabea::Ws::chunks)) return st;
  *chunks = W->chunks, *waves = W->waves, *ws_bytes = W->ws_bytes;
  return GB_OK;
}

int gb_abea_align(const gb_abea_model *model, const char *seqs, int64_t seq_bytes, const float *event_mean,
                  int64_t n_event_total, const gb_abea_read *reads, int64_t n_reads, gb_abea_pair *pairs,
                  int64_t pair_cap, int64_t *pair_off, gb_abea_stat *stats, int64_t *pairs_used) {
  using namespace gbabea;
  const char *who = "gb_abea_align";
  gb::Range range_("gb.abea.align");
  int st = validate(model, seqs, seq_bytes, event_mean, n_event_total, reads, n_reads, pairs, pair_cap, pair_off, stats);
  if (st) return st;
  if (pairs_used) *pairs_used = 0;
  pair_off[0] = 0;
  if (n_reads == 0) return GB_OK;
  int64_t budget = 0;
  if ((st = gb::env_number(who, "GB_ABEA_WS_BYTES", 1, INT64_MAX, kDefaultWsBytes, &budget))) return st;
  const std::vector<Chunk> chunks = make_chunks(reads, n_reads, budget / 2);
  const bool host = gb::env_flag("GB_ABEA_HOST");

  // the pairs of all chunks in their final, packed order; they reach pairs[] only once the need is known
  std::vector<gb_abea_pair> packed;
  int64_t used = 0;
  auto pack = [&](const Chunk &c, const gb_abea_pair *region) {
    int64_t end = 0;
    for (int64_t r = c.first; r < c.last; ++r) {
      end += read_bands(reads[r]);
      const int64_t n = stats[r].n_raw;
      pair_off[r] = used;
      packed.insert(packed.end(), region + end - n, region + end);
      used += n;
    }
  };
  try {
    if (host) {
      int nth = 1;
      if ((st = gb::thread_count(who, "GB_ABEA_THREADS", &nth))) return st;
      std::vector<gb_abea_pair> region;
      for (const Chunk &c : chunks) {
        region.resize((size_t)c.need.bands);
        std::vector<int64_t> ends((size_t)(c.last - c.first));
        int64_t end = 0;
        for (int64_t r = c.first; r < c.last; ++r) ends[(size_t)(r - c.first)] = end += read_bands(reads[r]);
        std::atomic<int64_t> next{c.first};
        const int use = (int)std::min<int64_t>(nth, c.last - c.first);
        if ((st = gb::parallel(who, use, [&](int) {
               HostScratch S;
               for (int64_t r; (r = next.fetch_add(1)) < c.last;) {
                 const gb_abea_read &s = reads[r];
                 host_align(model, seqs + s.seq_off, s.seq_len, event_mean + s.event_off, s.n_events, s.scale, s.shift,
                            region.data(), ends[(size_t)(r - c.first)], &stats[r], &S);
               }
             })))
          return st;
        pack(c, region.data());
      }
    } else {
      int dev = 0;
      GB_HIP(hipGetDevice(&dev));
      Ws *W = nullptr;
      if ((st = gb::get_ws(who, dev, &W, [](Ws *W) { return W->d_ctl.reserve(4); }))) return st;
      W->fill_ms = W->trace_ms = 0.f;
      W->cells = W->chunks = W->waves = W->ws_bytes = 0;
      if ((st = W->d_model.reserve(GB_ABEA_MODEL_SIZE)) || (st = W->d_seqs.reserve((size_t)seq_bytes)) ||
          (st = W->d_events.reserve((size_t)n_event_total)))
        return st;
      GB_HIP(hipMemcpyAsync(W->d_model, model, GB_ABEA_MODEL_SIZE * sizeof(Model), hipMemcpyHostToDevice, W->stream));
      GB_HIP(hipMemcpyAsync(W->d_seqs, seqs, (size_t)seq_bytes, hipMemcpyHostToDevice, W->stream));
      GB_HIP(hipMemcpyAsync(W->d_events, event_mean, (size_t)n_event_total * sizeof(float), hipMemcpyHostToDevice,
                            W->stream));
      for (const Chunk &c : chunks) {
        if ((st = run_chunk_device(W, reads, c, budget / 2, stats))) return st;
        pack(c, W->h_pairs);
      }
      W->chunks = (int64_t)chunks.size();
    }
  } catch (const std::bad_alloc &) {
    gb::set_error("%s: out of host memory", who);
    return GB_ERR_NOMEM;
  }
  pair_off[n_reads] = used;
  if (pairs_used) *pairs_used = used;
  GB_ARG(used <= pair_cap, "%s: pair_cap %lld is too small, the call needs %lld", who, (long long)pair_cap,
         (long long)used);
  if (used) std::memcpy(pairs, packed.data(), (size_t)used * sizeof(gb_abea_pair));
  return GB_OK;
}

}  // extern "C"
