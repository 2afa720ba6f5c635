// bsw_abea_hmm_internal.h -- what the two profile-HMM legs share: gb_abea_hmm_score (bsw_abea_hmm.hip, the
// forward score) and gb_abea_hmm_align (bsw_abea_viterbi.hip, Viterbi with traceback). The emission, the ten
// transitions, the size classes, the one-lane shifts of the anti-diagonal sweep and the refusals are one text;
// the fold of a cell's six terms (log-sum or max/argmax), the k-mer rank and what a cell leaves behind are each
// leg's own.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "../../include/gb_bsw_abea_hmm.h"
#include "gb_common.h"
#include "gb_common_wave.h"

namespace gbhmm {

constexpr int kK = GB_ABEA_K, kMaxRows = GB_ABEA_HMM_MAX_EVENTS;
constexpr int kClasses = 4;  // packed 16, then 1, 2, 4 k-mers per lane
constexpr float kNegInf = -INFINITY;

using Model = gb_abea_model;

struct Trans {  // BlockTransitions (hmm.c:212-229): the same for every k-mer of a call
  float mm_self, mb, mk, mm_next, bb, bk, bm_next, bm_self, kk, km;
};
struct State {
  float m, b, k;
};
struct Kmer {  // gp_mean, gp_stdv and log_inv_sqrt_2pi - gp_log_stdv of log_probability_match_r9
  float gm, sd, c;
};

// ---- the arithmetic, one text for host and device (no contraction: -ffp-contract=off) ----

#define GB_HD __host__ __device__ __forceinline__

GB_HD Kmer make_kmer(const Model &m, float scale, float shift, float var, float log_var) {
  Kmer k;
  k.gm = scale * m.level_mean + shift;
  k.sd = m.level_stdv * var;
  k.c = -0.918938f - (m.level_log_stdv + log_var);
  return k;
}
// log_normal_pdf (hmm.c:55-62), correctly rounded division
GB_HD float emission(float x, const Kmer &k) {
  const float a = (x - k.gm) / k.sd;
  return k.c + (-0.5f * a * a);
}

// k-mer ki of the string the reference reads (hmm.c:382-393)
GB_HD const char *kmer_at(const char *seq, int seq_len, int rc, int ki) {
  return rc ? seq + seq_len - ki - kK : seq + ki;
}

// ---- host ----

// calculate_transitions (hmm.c:231-298); false where the library refuses the read
inline bool make_trans(double events_per_base, Trans *T, float *p_next) {
  const float p_stay = (float)(1 - (1 / events_per_base));
  const float p_skip = (float)0.0025, p_bad = (float)0.001, p_bad_self = p_bad, p_skip_self = (float)0.3;
  const float p_mk = p_skip, p_mb = p_bad, p_mm_self = p_stay;
  const float p_mm_next = 1.0f - p_mm_self - p_mk - p_mb;
  const float p_bb = p_bad_self;
  const float p_bk = (1.0f - p_bb) / 3, p_bm_next = p_bk, p_bm_self = p_bk;
  const float p_kk = p_skip_self, p_km = 1.0f - p_kk;
  *p_next = p_mm_next;
  if (!(p_mm_next > 0.f) || !(p_mm_self >= 0.f)) return false;
  T->mk = (float)log((double)p_mk), T->mb = (float)log((double)p_mb);
  T->mm_self = (float)log((double)p_mm_self), T->mm_next = (float)log((double)p_mm_next);
  T->bb = (float)log((double)p_bb), T->bk = (float)log((double)p_bk);
  T->bm_next = (float)log((double)p_bm_next), T->bm_self = (float)log((double)p_bm_self);
  T->kk = (float)log((double)p_kk), T->km = (float)log((double)p_km);
  return true;
}

inline int item_rows(const gb_abea_hmm_item &it) {
  return (int)std::min<int64_t>(std::llabs((int64_t)it.event_stop - it.event_start) + 1, (int64_t)kMaxRows + 1);
}

GB_HD int size_class(int nk) { return nk <= 16 ? 0 : nk <= 64 ? 1 : nk <= 128 ? 2 : 3; }

// Every refusal of include/gb_bsw_abea_hmm.h, before any device work, for a model of model_size entries, items
// of at least min_rows rows and flags up to max_flags. trans[r] is read r's transitions. `out` is the call's
// output buffer, tested for null only.
inline int validate(const char *who, const Model *model, int model_size, int min_rows, int max_flags, const char *seqs,
                    int64_t seq_bytes, const float *event_mean, int64_t n_event_total, const gb_abea_hmm_read *reads,
                    int64_t n_reads, const gb_abea_hmm_item *items, int64_t n_items, const void *out,
                    std::vector<Trans> *trans) {
  GB_ARG(n_items >= 0 && n_reads >= 0 && (n_items == 0 || (items && out && model && reads)), "%s: bad arguments", who);
  GB_ARG(seq_bytes >= 0 && n_event_total >= 0 && (seq_bytes == 0 || seqs) && (n_event_total == 0 || event_mean),
         "%s: bad sequence or event buffers", who);
  GB_ARG(n_items < (int64_t(1) << 31) - 4, "%s: %lld items in one call (need fewer than 2^31 - 4)", who, (long long)n_items);
  if (n_items == 0) return GB_OK;
  for (int k = 0; k < model_size; ++k) {
    const Model &m = model[k];
    GB_ARG(std::isfinite(m.level_stdv) && m.level_stdv > 0.f, "%s: model entry %d has level_stdv %g (need finite and > 0)",
           who, k, (double)m.level_stdv);
    GB_ARG(std::isfinite(m.level_mean) && std::isfinite(m.level_log_stdv), "%s: model entry %d is not finite", who, k);
  }
  trans->resize((size_t)n_reads);
  for (int64_t r = 0; r < n_reads; ++r) {
    const gb_abea_hmm_read &s = reads[r];
    GB_ARG(s.n_events >= 0 && s.event_off >= 0 && s.event_off <= n_event_total - s.n_events,
           "%s: read %lld lies outside the event buffer", who, (long long)r);
    GB_ARG(std::isfinite(s.scale) && std::isfinite(s.shift), "%s: read %lld has scale %g, shift %g (need finite)", who,
           (long long)r, (double)s.scale, (double)s.shift);
    GB_ARG(std::isfinite(s.var) && s.var > 0.f && std::isfinite(s.log_var),
           "%s: read %lld has var %g, log_var %g (need finite, var > 0)", who, (long long)r, (double)s.var,
           (double)s.log_var);
    GB_ARG(std::isfinite(s.events_per_base) && s.events_per_base >= 1.0,
           "%s: read %lld has events_per_base %g (need finite and >= 1)", who, (long long)r, s.events_per_base);
    float p_next = 0.f;
    GB_ARG(make_trans(s.events_per_base, &(*trans)[(size_t)r], &p_next),
           "%s: read %lld has events_per_base %g, which leaves p_mm_next = %g (need > 0)", who, (long long)r,
           s.events_per_base, (double)p_next);
    const float *e = event_mean + s.event_off;
    for (int32_t i = 0; i < s.n_events; ++i)
      GB_ARG(std::isfinite(e[i]), "%s: read %lld has event %d with a mean that is not finite", who, (long long)r, i);
  }
  for (int64_t i = 0; i < n_items; ++i) {
    const gb_abea_hmm_item &it = items[i];
    GB_ARG(it.seq_len >= kK && it.seq_len - kK + 1 <= GB_ABEA_HMM_MAX_KMERS,
           "%s: item %lld has seq_len %d (need %d..%d)", who, (long long)i, it.seq_len, kK, GB_ABEA_HMM_MAX_KMERS + kK - 1);
    GB_ARG(it.seq_off >= 0 && it.seq_off <= seq_bytes - it.seq_len, "%s: item %lld lies outside the sequence buffer", who,
           (long long)i);
    GB_ARG(it.read >= 0 && it.read < n_reads, "%s: item %lld names read %d of %lld", who, (long long)i, it.read,
           (long long)n_reads);
    const int32_t ne = reads[it.read].n_events;
    GB_ARG(it.event_start >= 0 && it.event_start < ne && it.event_stop >= 0 && it.event_stop < ne,
           "%s: item %lld has events %d..%d outside its read's %d", who, (long long)i, it.event_start, it.event_stop, ne);
    GB_ARG(it.rc <= 1 && it.flags <= max_flags, "%s: item %lld has rc %d, flags %d (need 0..1, 0..%d)", who, (long long)i,
           it.rc, it.flags, max_flags);
    GB_ARG(it.rc ? it.event_start >= it.event_stop : it.event_start <= it.event_stop,
           "%s: item %lld has rc %d with events %d..%d (rc 0 runs up, rc 1 down)", who, (long long)i, it.rc,
           it.event_start, it.event_stop);
    GB_ARG(item_rows(it) >= min_rows, "%s: item %lld has %d rows (need at least %d)", who, (long long)i, item_rows(it),
           min_rows);
    GB_ARG(item_rows(it) <= kMaxRows, "%s: item %lld has more than %d rows", who, (long long)i, kMaxRows);
  }
  return GB_OK;
}

// ---- device: the one-lane moves of the sweep ----

// lane l of a group (a 16-lane row, or the wave) takes lane l-1's v, lane 0 takes first
template <bool PACK>
__device__ __forceinline__ float shr1(float v, float first) {
  if (PACK)
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(first), __float_as_int(v), 0x111, 0xF, 0xF, false));
  return __int_as_float(gb::wave_shr1(__float_as_int(v), __float_as_int(first)));
}
// every lane takes lane j of its group
template <bool PACK>
__device__ __forceinline__ float pick(float v, int j, int gbase) {
  if (PACK) return __int_as_float(__builtin_amdgcn_ds_bpermute((gbase + j) * 4, __float_as_int(v)));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

}  // namespace gbhmm
