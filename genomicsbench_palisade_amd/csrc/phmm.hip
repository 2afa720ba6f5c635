// phmm.hip -- MI355X (gfx950) PairHMM forward pass: host tables, batch packing, HIP kernels, C ABI.
//
// Arithmetic contract: the GKL recurrence
//   M[r][c] = ((M[r-1][c-1]*pMM + X[r-1][c-1]*pGAPM) + Y[r-1][c-1]*pGAPM) * dist(r,c)
//   X[r][c] = M[r-1][c]*pMX + X[r-1][c]*pXX
//   Y[r][c] = M[r][c-1]*pMY + Y[r][c-1]*pYY
// (tools/GKL/src/main/native/pairhmm/avx-pairhmm-template.h:183-198) with Y[0][*] = 2^120/haplen
// (f32) or 2^1020/haplen (f64), every other boundary 0, result = sum_c M[R][c] + sum_c X[R][c]
// (:299-344), f64 recomputation when the f32 result < 1e-28f (IntelPairHmmCSource.cpp:70-79).
// Must be built with -ffp-contract=off: no FMA anywhere, so every cell is bit-identical to the
// reference's AVX kernels.
//
// MI355X design: one stack of testcases sharing a haplotype per wave64 (phmm_stack: reads stacked
// vertically, each behind two virtual rows that reproduce the initial row); the stack is cut into
// stripes of 64 rows, lane k owns row r0+k and the wave sweeps anti-diagonals (step t: lane k is at
// column t-k+1). Values move one lane
// down per step with DPP wave_shr:1 (no LDS round trip); lane 0 takes the row above the stripe from
// one uniform LDS record per step, every lane reads the haplotype code of its own column from an
// LDS byte array, and lane 63 writes the stripe's last row back into the records (in place: the
// write index trails the read index by 63 columns). A second, persistent kernel recomputes in f64
// the testcases whose f32 result fell below MIN_ACCEPTED, stack by stack. Stacks are ordered by
// descending cost so the dispatcher balances waves.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <functional>
#include <future>
#include <limits>
#include <mutex>
#include <string>
#include <unordered_map>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/gb_phmm.h"
#include "gb_common.h"
#include "gb_common_wave.h"
#include "phmm_internal.h"

using namespace gb::phmm;

namespace {

constexpr int kBndPad = 72;  // boundary records beyond column C (see phmm_stripe reads)
constexpr int kRecPad = 16;  // boundary records below column 0 (phmm_stripe's lane 63 writes from column -2 on,
                             // phmm_rolled's from column -(kRollGroup - 1))
constexpr int kQualTab = 128;
// the batch's device counter words (d_count): [0..7] the passes' counters, then the f64 plan's
// bucket counts, bucket cursors and its number of units with work (f64_plan)
constexpr int kPlanBuckets = 128;
constexpr int kPlanCount = 8, kPlanCursor = kPlanCount + kPlanBuckets, kPlanTotal = kPlanCursor + kPlanBuckets;
constexpr int kCountWords = kPlanTotal + 8;
// behind the plan's total, the predictor's words: the gate's sample (testcases, predicted), testcases
// predicted, confirmed and redone
constexpr int kPredSampled = kPlanTotal + 1, kPredSamplePred = kPlanTotal + 2, kPredPredicted = kPlanTotal + 3;
constexpr int kPredConfirmed = kPlanTotal + 4, kPredRedone = kPlanTotal + 5;
static_assert(kPredRedone < kCountWords, "counter words");
constexpr int kM2M = ((127 * 128) >> 1) + 128;  // set_mm_prob indices for quals < 128

// ---------------------------------------------------------------------------------------------
// Host tables: Context<float>/Context<double> (Context.h:13-190), restated.
// ---------------------------------------------------------------------------------------------
constexpr int kMaxQual = 254;
constexpr double kJacTol = 8.0;
constexpr double kJacStep = 0.0001;
#define GB_JAC_INV_STEP (1.0 / kJacStep)
constexpr int kJacSize = (int)(kJacTol / kJacStep) + 1;

template <typename T>
struct HostTables {
  T ph2pr[kQualTab];
  T one_minus[kQualTab];  // 1 - ph2pr[x]: pGAPM (template.h:119) and 1-distm (template.h:152)
  T div3[kQualTab];       // ph2pr[x] / 3: mismatch distm (template.h:154)
  T m2m[kM2M];            // matchToMatchProb (Context.h:50-61) for quals < 128
  T init_const;           // INITIAL_CONSTANT
  T log10_init;           // LOG10_INITIAL_CONSTANT
};

template <typename T>
static int fast_round(T d) {
  return (d > (T)0.0) ? (int)(d + (T)0.5) : (int)(d - (T)0.5);
}

template <typename T>
static T log10sum(const std::vector<T> &jac, T small, T big) {
  if (small > big) std::swap(small, big);
  T diff = big - small;
  if (diff >= (T)kJacTol) return big;
  int ind = fast_round<T>((T)(diff * (T)GB_JAC_INV_STEP));
  return big + jac[ind];
}

template <typename T>
static void build_tables(HostTables<T> &t) {
  std::vector<T> jac(kJacSize);
  for (int k = 0; k < kJacSize; k++) jac[k] = (T)(log10(1.0 + pow(10.0, -((double)k) * kJacStep)));
  const double inv_ln10 = 1.0 / log(10);
  std::vector<T> m2m_full(((kMaxQual + 1) * (kMaxQual + 2)) >> 1);
  for (int i = 0, off = 0; i <= kMaxQual; off += ++i)
    for (int j = 0; j <= i; j++) {
      double s = log10sum<T>(jac, (T)(-0.1 * i), (T)(-0.1 * j));
      double l = log1p(-std::min(1.0, pow(10, s))) * inv_ln10;
      m2m_full[off + j] = (T)(pow(10, l));
    }
  for (int k = 0; k < kM2M; k++) t.m2m[k] = m2m_full[k];
  for (int x = 0; x < kQualTab; x++) {
    if constexpr (sizeof(T) == 4)
      t.ph2pr[x] = powf(10.f, -((float)x) / 10.f);
    else
      t.ph2pr[x] = pow(10.0, -((double)x) / 10.0);
    t.one_minus[x] = (T)1.0 - t.ph2pr[x];
    t.div3[x] = t.ph2pr[x] / (T)3.0;
  }
  if constexpr (sizeof(T) == 4) {
    t.init_const = ldexpf(1.f, 120);
    t.log10_init = log10f(t.init_const);
  } else {
    t.init_const = ldexp(1.0, 1020);
    t.log10_init = log10(t.init_const);
  }
}

// ConvertChar (pairhmm_common.h:30-39): A0 C1 T2 G3 N4, every other byte 0.
static uint8_t base_code(char ch) {
  switch ((uint8_t)ch) {
    case 'A': return 0;
    case 'C': return 1;
    case 'T': return 2;
    case 'G': return 3;
    case 'N': return 4;
    default: return 0;
  }
}
// Bit h set when a read base of this code matches a haplotype base of code h: equal codes, or
// either is N (mask construction in avx-pairhmm-template.h:5-27).
static uint8_t read_match_mask(uint8_t rc) { return rc == 4 ? 0x1F : (uint8_t)((1u << rc) | 0x10); }

// The early exit's gate (phmm_stack, "Early exit"). exit_growth: G >= prod_k max(1, g_k) over the rows
// k of a packed read (rmatch[R] q[R] i[R] d[R] c[R]) that have a row below them, g_k the most the
// crossing mass can grow from the crossing into row k to the crossing out of it, whatever the
// haplotype; from the f32 table values the kernel multiplies by, in double. +inf when a row's gap
// mass does not decay (ph2pr[c_k] = 1: its geometric sum is the haplotype's length, which a read
// shared between haplotypes does not know) yet leaks into the row below. A read may exit when
// G <= kExitGrowthMax; the pack sets kMayExit in every row's match mask then.
constexpr double kExitGrowthMax = 2.0;
static double exit_growth(const HostTables<float> &t, const uint8_t *rec, int R) {
  const double inf = std::numeric_limits<double>::infinity();
  double G = 1.0;
  for (int k = 0; k + 1 < R; k++) {
    const int qd = rec[3 * R + k] & 127, qc = rec[4 * R + k] & 127;  // own row: pMY, pYY
    const int ni = rec[2 * R + k + 1] & 127, nd = rec[3 * R + k + 1] & 127, nc = rec[4 * R + k + 1] & 127;
    const int mn = std::min(ni, nd), mx = std::max(ni, nd);
    const double nMM = t.m2m[((mx * (mx + 1)) >> 1) + mn], nMX = t.ph2pr[ni];
    const double nGAPM = t.one_minus[nc], nXX = t.ph2pr[nc];
    const double pYY = t.ph2pr[qc], leak = (double)t.ph2pr[qd] * nGAPM;
    if (leak > 0 && pYY >= 1.0) return inf;
    const double gM = nMM + nMX + (leak > 0 ? leak / (1.0 - pYY) : 0.0), gX = nGAPM + nXX;
    const double g = std::max(gM, gX);
    if (g > 1.0) G *= g;
    if (G > 1e30) return inf;
  }
  return G;
}

// The predictor's certificate (phmm_predict, verify_unit). A predicted testcase skips the f32 pass and is
// taken by the f64 pass; verify_unit then needs the f64 result to prove that the f32 result, which nobody
// computed, is below MIN_ACCEPTED. Both results are sums over the same alignment paths of products of
// table entries, times INITIAL_CONSTANT / haplen: f32 of the f32 tables' entries with f32 roundings, f64
// of the f64 tables'. A path visits at most R + C cells and takes at most two entries per cell (a
// transition and, in M, the emission), so with rho >= 1 the largest ratio of an f32 entry to its f64 entry
// among the entries the read's rows use, the exact f32-table sum is at most rho^(2 (R + C) + 2) times the
// exact f64-table sum. Every f32 operation on these non-negative terms gives at most its exact value
// times 1 + 2^-24 (plus 2^-150 where it rounds into the denormals: below 4e-35 over a whole matrix, see
// the early exit), every f64 operation at least its exact value times 1 - 2^-53 (f64 results of interest
// are ~2^800: its underflow is nowhere near), and a result depends on at most D = 4 (R + C) + C + 4
// operations in a chain: 4 a cell (the emission product, a transition product, the bracket's two sums),
// the last row's C + 1 additions, the division of the initial constant. Hence
//   f32_result <= K * f64_result * 2^-900 + 4e-35,  K = rho^(2 (R + C) + 2) * ((1 + 2^-24) / (1 - 2^-53))^D.
// cert_log_rho: log(rho) of a read, or +inf for a read that is never certified: an entry that is 0 in
// f64 and positive in f32, an insertion or deletion quality of 0..3 (where GKL clamps pMM at 0 and a
// state's outflow exceeds 1), a base or continuation quality of 0 (ph2pr = 1). cert_K: the bound for a
// haplotype of C columns. The pack certifies a read (kMayPredict in its first quality byte, whose bit 7
// no kernel reads) when cert_K(R, kMaxHaplen) <= kCertMax: K grows with C, so the flag holds for every
// haplotype the read meets. log(rho), rounded up to f32, follows the read's five byte rows in the pool, and
// verify_unit computes the testcase's own K from it.
constexpr double kCertMax = 2.0;
// CertTab: per quality value the largest f32 / f64 ratio of the entries a row takes with it (+inf for an
// entry that is 0 in f64 and positive in f32), so that a row costs five lookups at pack time.
struct CertTab {
  double q[kQualTab];  // one_minus[q], div3[q]
  double p[kQualTab];  // ph2pr[i], ph2pr[d]
  double c[kQualTab];  // ph2pr[c], one_minus[c]
  double m[kM2M];      // m2m
};
static void build_cert_tab(const HostTables<float> &tf, const HostTables<double> &td, CertTab &T) {
  auto ratio = [](float f, double d) {
    return d > 0 ? std::max(1.0, (double)f / d) : (f > 0 ? std::numeric_limits<double>::infinity() : 1.0);
  };
  for (int x = 0; x < kQualTab; x++) {
    T.q[x] = std::max(ratio(tf.one_minus[x], td.one_minus[x]), ratio(tf.div3[x], td.div3[x]));
    T.p[x] = ratio(tf.ph2pr[x], td.ph2pr[x]);
    T.c[x] = std::max(T.p[x], ratio(tf.one_minus[x], td.one_minus[x]));
  }
  for (int k = 0; k < kM2M; k++) T.m[k] = ratio(tf.m2m[k], td.m2m[k]);
}
static double cert_log_rho(const CertTab &T, const uint8_t *q, const uint8_t *qi, const uint8_t *qd,
                           const uint8_t *qc, int R) {
  double rho = 1.0;
  for (int r = 0; r < R; r++) {
    const int a = q[r] & 127, i = qi[r] & 127, d = qd[r] & 127, c = qc[r] & 127;
    if (i <= 3 || d <= 3 || a == 0 || c == 0) return std::numeric_limits<double>::infinity();
    const int mn = std::min(i, d), mx = std::max(i, d), m = ((mx * (mx + 1)) >> 1) + mn;
    rho = std::max(rho, std::max(std::max(T.q[a], T.p[i]), std::max(std::max(T.p[d], T.c[c]), T.m[m])));
  }
  return std::log(rho);
}
__host__ __device__ inline double cert_K(double log_rho, int R, int C) {
  const double steps = (double)R + (double)C, D = 4.0 * steps + (double)C + 4.0;
  return exp((2.0 * steps + 2.0) * log_rho + D * 5.9604644e-8);  // >= log1p(2^-24) - log1p(-2^-53)
}

// ---------------------------------------------------------------------------------------------
// Device side
// ---------------------------------------------------------------------------------------------
template <typename T>
struct DevTab {
  const T *ph2pr, *one_minus, *div3, *m2m;
  T init_const;
};

// the tables of upload_tables' blob at `base`
template <typename T>
__host__ __device__ inline DevTab<T> dev_tab(const T *base, T init_const) {
  DevTab<T> t;
  t.ph2pr = base;
  t.one_minus = base + kQualTab;
  t.div3 = base + 2 * kQualTab;
  t.m2m = base + 3 * kQualTab;
  t.init_const = init_const;
  return t;
}

// Boundary record per column c (stripe above the current one): the two partial sums the first
// row of the current stripe needs from the row above, already multiplied by THAT first row's
// transition probabilities, plus the haplotype base code of column c:
//   z = (M*pMM + X*pGAPM) + Y*pGAPM   (the M recurrence's bracket, used one column later)
//   w = M*pMX + X*pXX                 (= X of the next row at the same column)
// Read by lane 0 with one uniform ds_read per step. The haplotype codes live in a separate byte
// array that every lane reads at its own column (no cross-lane traffic, no VALU).
template <typename T>
struct __attribute__((aligned(2 * sizeof(T)))) Brec {
  T z, w;
};

template <int (*F)(int, int)>
__device__ __forceinline__ float dpp(float v, float keep) {
  return __builtin_bit_cast(float, F(__builtin_bit_cast(int, v), __builtin_bit_cast(int, keep)));
}
template <int (*F)(int, int)>
__device__ __forceinline__ double dpp(double v, double keep) {
  long long vb = __builtin_bit_cast(long long, v), kb = __builtin_bit_cast(long long, keep);
  int lo = F((int)(vb & 0xffffffffll), (int)(kb & 0xffffffffll));
  int hi = F((int)(vb >> 32), (int)(kb >> 32));
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
template <int (*F)(int, int)>
__device__ __forceinline__ uint32_t dpp(uint32_t v, uint32_t keep) {
  return (uint32_t)F((int)v, (int)keep);
}

// dist select without a compare: sign-extend bit `h` of the lane's match mask (0 or ~0) and
// bit-insert between the two candidates.
__device__ __forceinline__ float select_dist(uint32_t rmask, uint32_t h, float dmatch, float dmis) {
  uint32_t m = (uint32_t)__builtin_amdgcn_sbfe((int)rmask, h, 1);
  uint32_t r = (m & __builtin_bit_cast(uint32_t, dmatch)) | (~m & __builtin_bit_cast(uint32_t, dmis));
  return __builtin_bit_cast(float, r);
}
// f64: the same mask applied to both halves. The mask comes from inline asm because hipcc 7.2
// mis-derives the high word of a sign-extended sbfe mask and constant-folds it; asm is opaque.
__device__ __forceinline__ double select_dist(uint32_t rmask, uint32_t h, double dmatch, double dmis) {
  uint32_t m;
  asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(rmask), "v"(h));
  const uint64_t a = __builtin_bit_cast(uint64_t, dmatch), b = __builtin_bit_cast(uint64_t, dmis);
  const uint32_t lo = (m & (uint32_t)a) | (~m & (uint32_t)b);
  const uint32_t hi = (m & (uint32_t)(a >> 32)) | (~m & (uint32_t)(b >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// The wave's sum in every lane by the butterfly acc += partner(lane ^ o), o = 32, 16 .. 1 (the early exit's
// test: the order fixes the rounding). The exchanges below 32 go through ds_swizzle, whose lane pattern
// is an immediate; as bpermutes each keeps an index register alive across the whole sweep.
template <int O>
__device__ __forceinline__ float swz_xor(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), (O << 10) | 0x1F));
}
template <int O>
__device__ __forceinline__ double swz_xor(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_ds_swizzle((int)(b & 0xffffffffll), (O << 10) | 0x1F);
  const int hi = __builtin_amdgcn_ds_swizzle((int)(b >> 32), (O << 10) | 0x1F);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
template <typename T>
__device__ __forceinline__ T wave_sum_xor(T acc) {
  acc += __shfl_xor(acc, 32);
  acc += swz_xor<16>(acc);
  acc += swz_xor<8>(acc);
  acc += swz_xor<4>(acc);
  acc += swz_xor<2>(acc);
  acc += swz_xor<1>(acc);
  return acc;
}

// A value the optimiser takes as new where it stands. The exit kernel runs at the 64 registers of 8 waves
// per SIMD: a per-lane address or offset that depends on the lane alone is otherwise computed once at
// the kernel's top, kept for the whole stack, and spilled.
__device__ __forceinline__ int fresh(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// A lane's haplotype code of one column. The empty asm keeps the zero extension in the load's basic
// block, where the byte load gives it for free; left to the optimiser it sinks to the step that uses
// the code, behind lane 63's record write, and the code crosses the blocks as a byte that is masked
// again there (a v_and_b32 0xff per code, 3 of the 70 VALU instructions of a 4-step f32 block).
__device__ __forceinline__ uint32_t load_code(const uint8_t *p) {
  uint32_t h = *p;
  asm volatile("" : "+v"(h));
  return h;
}

// Per-lane constants of one stripe (initializeVectors, avx-pairhmm-template.h:83-128): the lane's
// own row (Y recurrence, emission) and the NEXT row's transitions (the partials z/w it hands down).
// nGAPMx is nGAPM for the X term of the bracket; a separate register so that the virtual row 0 of
// a stacked testcase (phmm_stack) can drop the X it receives from the testcase above it.
template <typename T>
struct RowParams {
  T pMY, pYY, dmatch, dmis;              // own row
  T nMM, nGAPM, nGAPMx, nMX, nXX;        // row below (lane+1; lane 63: first row of next stripe)
  uint32_t rmask;
};

// Lane state between steps. Row r = lane's row, column c = step - lane + 1:
//   Mp, Yp : M[r][c-1], Y[r][c-1]           zo, wo : this lane's z/w of column c-1
//   zd     : z of row r-1 at column c-1 (= the M bracket of this lane's next cell), shifted in
template <typename T>
struct LaneState {
  T Mp, Yp, zo, wo, zd;
};

// One anti-diagonal step. Arithmetic per cell is exactly the reference's (no FMA, same order):
//   X = M[r-1][c]*pMX + X[r-1][c]*pXX         computed by lane-1 as w, shifted in
//   M = ((M*pMM + X*pGAPM) + Y*pGAPM)[r-1][c-1] * dist    bracket computed by lane-1 as z
//   Y = M[r][c-1]*pMY + Y[r][c-1]*pYY
// kSum: accumulate the row sums (a testcase's last row is in the stripe); kWrite: lane 63 hands its
// row's partials to the next stripe through the LDS records.
template <typename T, bool kSum, bool kWrite>
__device__ __forceinline__ void phmm_step(const Brec<T> &rec, uint32_t h, LaneState<T> &st,
                                          const RowParams<T> &P, T &sumM, T &sumX, Brec<T> *wr, bool last_lane) {
  const T X = dpp<gb::wave_shr1>(st.wo, rec.w);          // X[r][c]
  const T zdn = dpp<gb::wave_shr1>(st.zo, rec.z);        // bracket for column c+1
  const T dist = select_dist(P.rmask, h, P.dmatch, P.dmis);
  const T M = st.zd * dist;
  const T Y = st.Mp * P.pMY + st.Yp * P.pYY;
  st.zo = (M * P.nMM + X * P.nGAPMx) + Y * P.nGAPM;
  st.wo = M * P.nMX + X * P.nXX;
  if constexpr (kSum) {
    sumM = sumM + M;
    sumX = sumX + X;
  }
  if constexpr (kWrite) {
    // lane 63 hands its row's z/w (the next stripe's brackets) to LDS; columns < 1 land in the pad
    if (last_lane) {
      Brec<T> b;
      b.z = st.zo;
      b.w = st.wo;
      *wr = b;
    }
  }
  st.zd = zdn;
  st.Mp = M;
  st.Yp = Y;
}

// Sweep `steps` anti-diagonals of one stripe, 4 per iteration, the boundary records of the next
// block prefetched before this block runs. Reads are at columns > t; lane 63 writes column t-62 of
// the row below at step t from step 60 on (bnd has kRecPad pad records below column 0).
// kSum: the lanes in `lastmask` hold the last row of a testcase; lane k reaches column C at step
// C + k - 1, where its row sum is final, so that step runs singly and lane k stores sumM + sumX
// (later steps add columns beyond C). The check is a uniform scalar compare per 4 steps.
template <typename T, bool kSum, bool kWrite>
__device__ __forceinline__ void phmm_stripe(int steps, LaneState<T> &st, const RowParams<T> &P,
                                            T &sumM, T &sumX, Brec<T> *__restrict__ bnd,
                                            const uint8_t *__restrict__ hcol, int C, int lane,
                                            uint64_t lastmask, T *__restrict__ out) {
  // hcol[c] = haplotype code of column c (valid for c in [-63, C+kBndPad)); lane's column at step
  // t is t - lane + 1.
  const uint8_t *hl = hcol + 1 - lane;
  const bool last_lane = lane == kWave - 1;
  constexpr int U = 4;
  // lane 63 reaches column 0 at step 62: its records for earlier (negative) columns are dropped by
  // running the first 60 steps without writes (the pad holds columns -2, -1)
  constexpr int kNoWrite = 60;
  uint64_t pend = lastmask;
  int target = (kSum && pend) ? C + __builtin_ctzll(pend) - 1 : INT_MAX;
  auto single = [&](int tt, auto wr_tag) {
    constexpr bool W = decltype(wr_tag)::value;
    phmm_step<T, kSum, W>(bnd[tt + 1], load_code(hl + tt), st, P, sumM, sumX, bnd + (tt - (kWave - 2)), last_lane);
    if (kSum && tt == target) {
      if (lane == __builtin_ctzll(pend)) *out = sumM + sumX;
      pend &= pend - 1;
      target = pend ? C + __builtin_ctzll(pend) - 1 : INT_MAX;
    }
  };
  // The block's record reads and writes go through one VGPR address with immediate offsets (an
  // SGPR base costs a v_mov per access); the asm zero keeps the compiler from rematerialising it.
  int vzero;
  asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
  Brec<T> *wb = bnd - (kWave - 2) + vzero;
  auto run = [&](int t, int end, auto wr_tag) {
    constexpr bool W = decltype(wr_tag)::value;
    for (; t + U <= end; t += U) {
      if (kSum && target < t + U) {
        for (int u = 0; u < U; u++) single(t + u, wr_tag);
        continue;
      }
      // records land directly in the DPP "old" registers (no rotation copies); the LDS latency is
      // covered by the other waves on the SIMD
      Brec<T> *wr = wb + t;
      const Brec<T> c0 = wr[kWave - 1], c1 = wr[kWave], c2 = wr[kWave + 1], c3 = wr[kWave + 2];
      const uint32_t h0 = load_code(hl + t), h1 = load_code(hl + t + 1);
      const uint32_t h2 = load_code(hl + t + 2), h3 = load_code(hl + t + 3);
      phmm_step<T, kSum, W>(c0, h0, st, P, sumM, sumX, wr, last_lane);
      phmm_step<T, kSum, W>(c1, h1, st, P, sumM, sumX, wr + 1, last_lane);
      phmm_step<T, kSum, W>(c2, h2, st, P, sumM, sumX, wr + 2, last_lane);
      phmm_step<T, kSum, W>(c3, h3, st, P, sumM, sumX, wr + 3, last_lane);
    }
    for (; t < end; t++) single(t, wr_tag);
  };
  if constexpr (kWrite) {
    const int a = min(steps, kNoWrite);
    run(0, a, std::false_type{});
    run(a, steps, std::true_type{});
  } else {
    run(0, steps, std::false_type{});
  }
}

template <typename T>
__device__ __forceinline__ void load_row(const uint8_t *__restrict__ rbase, int R, int row,
                                         const DevTab<T> &tab, T &pMM, T &pGAPM, T &pMX, T &pXX,
                                         T &pMY, T &pYY, T &dmatch, T &dmis, uint32_t &rmask) {
  rmask = rbase[row];
  const int q = rbase[R + row] & 127, qi = rbase[2 * R + row] & 127;
  const int qd = rbase[3 * R + row] & 127, qc = rbase[4 * R + row] & 127;
  const int mn = qi <= qd ? qi : qd, mx = qi <= qd ? qd : qi;
  pMM = tab.m2m[((mx * (mx + 1)) >> 1) + mn];
  pGAPM = tab.one_minus[qc];
  pMX = tab.ph2pr[qi];
  pXX = tab.ph2pr[qc];
  pMY = tab.ph2pr[qd];
  pYY = tab.ph2pr[qc];
  dmatch = tab.one_minus[q];
  dmis = tab.div3[q];
}

// Stacks: testcases that share a haplotype are stacked into one tall matrix, so a wave sweeps
// 64-row stripes of the stack and a read's rows need not start at a stripe boundary: the partial
// last stripe of every testcase (a quarter of all lane steps for 100-250-row reads) disappears.
// Each read is preceded by two virtual rows, ordinary lanes whose constants make the shared step
// code produce the reference's initial row (M = X = 0, Y = INITIAL_CONSTANT / haplen) exactly, and
// zeros at the columns a lane sweeps before its column 1 (so nothing leaks into column 0):
//   va: dist = 0 (M = 0), Y = init_Y * 1 at every step, partials z = (0*0 + X*0) + init_Y*1 and
//       w = 0*0 + X*0 = 0, whatever the testcase above hands it;
//   v0: dist = 1 at columns >= 0 and 0 before (column codes 5 at column 0, 6 below it, matched by
//       v0's mask only up to 5), so M = init_Y from column 0 on, and its partials are
//       z = (M*pGAPM + X*0) + 0*0 = init_Y*pGAPM (the reference's (0*pMM + 0*pGAPM) + init_Y*pGAPM)
//       and w = 0 (its 0*pMX + 0*pXX), zero before column 0.
// Lanes beyond the stack's last row compute zeros.
struct __attribute__((aligned(16))) StackEnt {
  int start;  // stacked row of the testcase's first virtual row
  int R;
  uint32_t read_off, out_idx;
};

// ---------------------------------------------------------------------------------------------
// Rolled stripes. A 64-row stripe costs C + 63 wave steps for 64 x C cells: the anti-diagonal fill.
// Here the wave does not wait for lane 63 before it starts the next 64 rows ("turn"): lanes move on
// in groups of kRollGroup at 4-step block boundaries. With P = roundup4(C + kRollGroup + 1) the
// period of a turn, group k (lanes k*G .. k*G + G - 1) moves from turn s - 1 to turn s at step
// s*P + k*G, and lane l of turn s is at column t - l - s*P at step t: every lane stays one column
// behind the lane above it, so phmm_step and its two DPP shifts are unchanged. A group's last lane
// has passed column C + 1 when the group moves on, so the lane below it has consumed its column-C
// outputs; between column C and its switch a lane computes garbage columns (code 0), as a lane of
// phmm_stripe does beyond column C, and after the switch its negative columns give zeros through
// the column codes 6 and 5. A switch replaces the lane's RowParams and state by the next turn's.
// When the last group has moved, every lane finds its row of the turn after (the binary search over
// the entry table) and loads that row's quality bytes and those of the row below it: two registers
// per lane (RowDesc: seven 7-bit qualities, with i and d of the row below already folded into their
// m2m index, the match mask and the row's kind), held through the turn. The group's own switch
// expands them straight into the live registers. It is a divergent branch taken by the group's 16
// lanes (the other 48 are masked off by exec; no longer selects in a straight-line block): eight
// independent table loads (the entries load_row reads; a va, v0 or dead lane loads entry 0 and drops
// it) and a select per constant for the va / v0 / last / dead kinds, about 40 VALU instructions
// for f32. No byte load -> table load chain is left at a switch, and no second set of constants for
// 64 lanes lives through the turn (with one the f32 exit kernel spilled 40 registers and reloaded
// them at every switch). Lane 0 passes through column 0 itself, so it needs no special initial state
// and takes the record of column 0 like any other.
// Records: lane 63 writes its row's z / w in place at its column, lane 0 reads the row above at its
// own; lane 0 reads column c P - 63 steps after lane 63 wrote it (4 records are fetched a block
// ahead: P >= 72, given by C >= 64) and lane 63 overwrites it 63 steps after that. Both go through
// one per-lane address register: every lane holds lane 0's read address, lane 63 its own write
// address. After a switch lane 63 is at column -(kRollGroup - 1), inside the kRecPad pad records, so
// every block writes; the sweep's first 48 steps, lane 63 at columns -63 .. -16, write into the end
// of the pad beyond column C instead, which only garbage columns read.
// Row sums: last rows complete in stacked-row order, which is time order (turn s, lane l reaches
// column C at step s*P + l + C), so the next one comes from the entry table; the summing block
// variant runs from that row's switch to its column C.
// Early exit: the test of phmm_stack, on the same rows with the same sum, at the first block
// boundary after lane 63's row has written column C (44 or 48 steps into the next turn); lane 63's
// row and testcase are read from the entry table as scalars when the last group switches. No lane of
// the next turn has reached column C then (P > 63), so nothing of the dying testcase has been
// stored: the rows in flight are abandoned and the sweep starts again at the next testcase's first
// row, a va row, which ignores the records it is handed.
// (kRollGroup and the sweeps' cost in wave steps, stack_steps: phmm_internal.h)

// The rolled sweep of a stack's rows from `base` (at least two turns, C >= 64). Returns the stacked
// row the stack goes on from: T_rows, or the next testcase's first row after an early exit.
template <typename T, bool kExit>
__device__ __forceinline__ int phmm_rolled(const int base, const int T_rows, const int na, const int C, const int lane,
                                           const int e_start, const int e_R, const uint32_t e_read,
                                           const uint32_t e_out, const uint8_t *__restrict__ pool,
                                           const DevTab<T> &tab, const T init_Y, Brec<T> *bnd, const uint8_t *hcol,
                                           T *raw_out, unsigned long long *exit_stats) {
  constexpr int G = kRollGroup, NG = kWave / G, U = 4;
  static_assert(G % U == 0 && G <= kRecPad, "lane 63 writes from its switch on, at columns >= -(G - 1)");
  const int Pd = (C + G + 1 + 3) & ~3;
  const int nturn = (T_rows - base + kWave - 1) / kWave;
  const int t_end = (nturn - 1) * Pd + C + (T_rows - base - kWave * (nturn - 1));
  const bool last_lane = lane == kWave - 1;
  struct L63 {
    int r, R, start, out, may;
  };
  // A lane's row of turn s, described in two registers (the binary search over the entry table and the
  // row's quality bytes, once per turn for all 64 lanes); `expand` turns it into constants and state.
  //   own: rmask | q << 8 | d << 16 | c << 24 of the lane's own row (rmask 0x3F for v0, all 0 for va / dead)
  //   nxt: the row below in the same testcase: its m2m index (14 bits) | i << 14 | c << 21, and the row's
  //        kind in the top four bits
  constexpr uint32_t kReal = 1u << 28, kNext = 1u << 29, kVa = 1u << 30, kV0 = 1u << 31;
  struct RowDesc {
    uint32_t own, nxt;
  };
  auto describe = [&](int s) -> RowDesc {
    const int g = base + kWave * s + lane;
    int lo = 0, hi = na - 1;
    while (__builtin_amdgcn_ballot_w64(lo < hi)) {
      const int mid = (lo + hi + 1) >> 1;
      const int sm = __shfl(e_start, mid);
      if (lo < hi) {
        if (sm <= g) lo = mid; else hi = mid - 1;
      }
    }
    const int start = __shfl(e_start, lo), R = __shfl(e_R, lo);
    const uint8_t *rb = pool + (uint32_t)__shfl((int)e_read, lo);
    const int r = g - start;  // 0: va, 1: v0, 2..R+1: read row r-2
    const bool live = g < T_rows;
    const bool real = live && r >= 2, below = live && r >= 1 && r <= R;  // a row of the read below it
    RowDesc D;
    D.own = (live && r == 1) ? 0x3Fu : 0u;
    D.nxt = real ? kReal : (live ? (r == 0 ? kVa : kV0) : 0u);
    if (real) {
      const uint8_t *p = rb + (r - 2);
      D.own = (uint32_t)p[0] | (uint32_t)(p[R] & 127) << 8 | (uint32_t)(p[3 * R] & 127) << 16 |
              (uint32_t)(p[4 * R] & 127) << 24;
    }
    if (below) {
      const uint8_t *p = rb + (r - 1);
      const uint32_t qi = p[2 * R] & 127, qd = p[3 * R] & 127, qc = p[4 * R] & 127;
      const uint32_t mn = qi <= qd ? qi : qd, mx = qi <= qd ? qd : qi;
      D.nxt |= (((mx * (mx + 1)) >> 1) + mn) | qi << 14 | qc << 21 | (real ? kNext : 0u);
    }
    return D;
  };
  // The switch proper: the lanes in `mine` take their row's constants (the table entries load_row reads)
  // and initial state (phmm_stack's, for a row that does not start at column 1), in place.
  auto expand = [&](const RowDesc &D, bool mine, RowParams<T> &P, LaneState<T> &st) {
    if (mine) {
      const T zero = (T)0, one = (T)1;
      const bool real = D.nxt & kReal, nextr = D.nxt & kNext, va = D.nxt & kVa, v0 = D.nxt & kV0;
      const uint32_t q = (D.own >> 8) & 127, qd = (D.own >> 16) & 127, qc = D.own >> 24;
      const uint32_t nqi = (D.nxt >> 14) & 127, nqc = (D.nxt >> 21) & 127;
      const T tMY = tab.ph2pr[qd], tYY = tab.ph2pr[qc], tdm = tab.one_minus[q], tdx = tab.div3[q];
      const T tMM = tab.m2m[D.nxt & 0x3FFF], tGAPM = tab.one_minus[nqc], tMX = tab.ph2pr[nqi], tXX = tab.ph2pr[nqc];
      P.rmask = D.own & 0xFF;
      P.pMY = real ? tMY : zero;
      P.pYY = real ? tYY : (va ? one : zero);
      P.dmatch = real ? tdm : (v0 ? one : zero);
      P.dmis = real ? tdx : zero;
      P.nMM = nextr ? tMM : (v0 ? tGAPM : zero);
      P.nGAPMx = nextr ? tGAPM : zero;
      P.nGAPM = nextr ? tGAPM : (va ? one : zero);
      P.nMX = nextr ? tMX : zero;
      P.nXX = nextr ? tXX : zero;
      st.Mp = st.wo = zero;
      st.Yp = st.zo = va ? init_Y : zero;  // va hands init_Y down from its first step: (0*0 + 0*0) + init_Y*1
      st.zd = v0 ? init_Y : zero;          // va's output at the column before
    }
  };
  // lane 63's row of turn s for the early exit, as scalars: its entry is the last one starting at or
  // before it (the entries are in stacked-row order)
  auto row63 = [&](int s, const RowParams<T> &P) -> L63 {
    const int g = base + kWave * s + kWave - 1;
    const int e = __builtin_popcountll(__builtin_amdgcn_ballot_w64(lane < na && e_start <= g)) - 1;
    L63 L;
    L.start = __builtin_amdgcn_readlane(e_start, e);
    L.R = __builtin_amdgcn_readlane(e_R, e);
    L.out = __builtin_amdgcn_readlane((int)e_out, e);
    L.r = g - L.start;
    L.may = __builtin_amdgcn_readlane((int)P.rmask, 63) & kMayExit;
    return L;
  };
  auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };  // wave-uniform, for the compiler
  RowParams<T> P;
  LaneState<T> st;
  expand(describe(0), true, P, st);
  L63 c63 = {0, 0, 0, 0, 0};
  if constexpr (kExit) c63 = row63(0, P);
  RowDesc nd = describe(1);  // the next turn's rows
  T sumM = (T)0, sumX = (T)0;
  const int ln = fresh(lane);
  const uint8_t *hl = hcol - ln;  // hl[t]: the code of the lane's column at step t
  // pp[t]: lane 0's record in every lane but 63, which holds its own. Lane 63's first columns of the
  // sweep, -63 .. -16, have no record: until step kFirst they go to the last records of the pad
  // beyond column C, which are read as garbage columns only
  constexpr int kFirst = kWave - kRecPad;
  Brec<T> *pp = ln == kWave - 1 ? bnd + (C + kBndPad - kFirst) : bnd;
  int first_t = kFirst;
  int s3 = 0;         // the turn lane 63 is in
  int sw = 0;         // next switch: group `sw` moves to turn s3 + 1 at step sw_t
  int sw_t = Pd;      // (nturn >= 2)
  int chk_s = 0;      // next turn whose lane-63 row is tested, at step chk_t
  int chk_t = kExit ? (kWave + C + 3) & ~3 : INT_MAX;
  // the next last row to complete: entry `ent`'s, in lane tg.lane at step tg.t, summed from step tg.from
  // (its group's switch) and stored at tg.out; all wave-uniform
  struct Target {
    int t, from, lane;
    uint32_t out;
  };
  auto target_of = [&](int en) -> Target {
    const int ec = min(en, na - 1);
    const int d = __builtin_amdgcn_readlane(e_start, ec) + __builtin_amdgcn_readlane(e_R, ec) + 1 - base;
    const int s = d / kWave, l = d % kWave;
    Target g;
    g.lane = l;
    g.t = uni(en < na ? s * Pd + l + C : INT_MAX);
    g.from = uni(en < na ? (s ? s * Pd + (l / G) * G : 0) : INT_MAX);
    g.out = (uint32_t)__builtin_amdgcn_readlane((int)e_out, ec);
    return g;
  };
  int ent = uni((int)__builtin_ctzll(__builtin_amdgcn_ballot_w64(lane < na && e_start + e_R + 1 >= base) | (1ull << 63)));
  Target tg = target_of(ent);
  for (int t = 0; t < t_end;) {
    if constexpr (kExit) {
      if (t == chk_t) {
        if (c63.r >= 2 && c63.r <= c63.R && c63.may) {
          __syncthreads();
          T acc = (T)0;
#pragma unroll 1
          for (int c = 1 + fresh(lane); c <= C; c += kWave) acc += bnd[c].z + bnd[c].w;
          acc = wave_sum_xor(acc);
          if (__builtin_amdgcn_readfirstlane(acc < (T)0.25e-28f ? 1 : 0)) {
            const int next = c63.start + c63.R + 2;
            if (lane == 0) {
              raw_out[(uint32_t)c63.out] = (T)0;
              atomicAdd(exit_stats, 1ull);
              atomicAdd(exit_stats + 1,
                        (unsigned long long)(next - (base + kWave * (chk_s + 1))) * (unsigned long long)C);
            }
            return next;
          }
        }
        chk_s = uni(chk_s + 1);
        chk_t = uni(chk_s + 1 < nturn ? chk_t + Pd : INT_MAX);
      }
    }
    if (t == first_t) {
      if (last_lane) pp = bnd - (kWave - 1);
      first_t = INT_MAX;
    }
    if (t == sw_t) {
      // group `sw` takes the next turn's constants and state
      const bool mine = lane / G == sw;
      expand(nd, mine, P, st);
      if (mine) {
        sumM = sumX = (T)0;
        hl -= Pd;
      }
      if (sw == 0) pp -= last_lane ? 0 : fresh(Pd);
      if (sw == NG - 1) {
        // lane 63 is at column -(G - 1) >= -kRecPad and goes on writing. The turn after this one is
        // set up now (beyond the last turn: dead rows, never switched to)
        s3 = uni(s3 + 1);
        if (last_lane) pp = bnd - (kWave - 1) - s3 * Pd;
        if constexpr (kExit) c63 = row63(s3, P);
        nd = describe(s3 + 1);
        sw = 0;
        sw_t = uni(s3 + 1 < nturn ? (s3 + 1) * Pd : INT_MAX);
      } else {
        sw = uni(sw + 1);
        sw_t = uni(sw_t + G);
      }
    }
    // blocks of one variant up to the next event: a switch, the exit test, the block in which the
    // next last row completes, the step its sums start at, or the sweep's last whole block
    const bool sum = t >= tg.from;
    int stop = min(min(min(chk_t, sw_t), first_t), min(t_end & ~(U - 1), tg.t & ~(U - 1)));
    if (!sum) stop = min(stop, tg.from);
    stop = uni(stop);
    if (t < stop) {
      auto run = [&](auto sum_tag) {
        constexpr bool S = decltype(sum_tag)::value;
        do {
          Brec<T> *wp = pp + t;
          const uint8_t *hp = hl + t;
          const Brec<T> c0 = wp[0], c1 = wp[1], c2 = wp[2], c3 = wp[3];
          const uint32_t h0 = load_code(hp), h1 = load_code(hp + 1), h2 = load_code(hp + 2), h3 = load_code(hp + 3);
          phmm_step<T, S, true>(c0, h0, st, P, sumM, sumX, wp, last_lane);
          phmm_step<T, S, true>(c1, h1, st, P, sumM, sumX, wp + 1, last_lane);
          phmm_step<T, S, true>(c2, h2, st, P, sumM, sumX, wp + 2, last_lane);
          phmm_step<T, S, true>(c3, h3, st, P, sumM, sumX, wp + 3, last_lane);
          t += U;
        } while (t < stop);
      };
      if (sum) run(std::true_type{}); else run(std::false_type{});
    } else {
      // a last row reaches column C in this block (its sum is final at that step), or the sweep ends in it
      const int n = min(U, t_end - t);
      Brec<T> *wp = pp + t;
      const uint8_t *hp = hl + t;
#pragma unroll 1
      for (int u = 0; u < n; u++) {
        const Brec<T> c = wp[u];
        const uint32_t h = load_code(hp + u);
        phmm_step<T, true, true>(c, h, st, P, sumM, sumX, wp + u, last_lane);
        if (t + u == tg.t) {
          if (lane == tg.lane) raw_out[tg.out] = sumM + sumX;
          ent = uni(ent + 1);
          tg = target_of(ent);
        }
      }
      t += n;
    }
  }
  return T_rows;
}

// One stack. f32 pass: every testcase `sel` selects (kExit: with the early exit below); f64 pass: those
// whose f32 result is below MIN_ACCEPTED (all of them when `force`). Returns the number of testcases computed.
// kRoll && roll: the stack's runs of at least two turns over C >= 64 columns take phmm_rolled.
template <typename T, bool kF64Pass, bool kExit = false, bool kRoll = false>
__device__ __forceinline__ int phmm_stack(const Stack &S, const uint32_t *__restrict__ stk_tc, const TcDesc *__restrict__ descs,
                          const uint8_t *__restrict__ pool, const DevTab<T> &tab, T *__restrict__ raw_out,
                          const float *__restrict__ raw_f, bool force, uint8_t *smem_raw, int part = 0,
                          int parts = 1, unsigned long long *exit_stats = nullptr, bool roll = false,
                          const uint8_t *__restrict__ sel = nullptr, int sel_want = 0) {
  const int lane = threadIdx.x;
  const int C = (int)S.C;
  // LDS: boundary records for columns [-kRecPad, C+kBndPad) and the haplotype codes for columns
  // [-kWave, C+kBndPad). The stack's testcase table lives in lanes (lane a: entry a), read with
  // cross-lane shuffles.
  Brec<T> *bnd = reinterpret_cast<Brec<T> *>(smem_raw) + kRecPad;
  uint8_t *hcol = smem_raw + sizeof(Brec<T>) * (size_t)(C + kBndPad + kRecPad) + kWave;

  // the stack's testcases, compacted to those computed in this pass
  TcDesc d = {0, 0, 0, 0};
  // the f64 pass may take a stack in `parts` work units: unit `part` takes the stack's entries
  // [part * count / parts, (part + 1) * count / parts)
  bool act = lane < (int)S.count;
  if (parts > 1) act = act && lane >= part * (int)S.count / parts && lane < (part + 1) * (int)S.count / parts;
  if (act) {
    d = descs[stk_tc[S.first + lane]];
    if constexpr (kF64Pass) act = force || raw_f[d.out_idx] < 1e-28f;  // MIN_ACCEPTED, pairhmm_common.h:16
    // f32 pass: without the testcases phmm_predict took (sel = pred, 0); the redo inside the f64 pass: only
    // those verify_unit sent back (sel = redo, 1)
    else if (sel) act = sel[d.out_idx] == (uint8_t)sel_want;
  }
  const uint64_t am = __builtin_amdgcn_ballot_w64(act);
  if (!am) return 0;
  const int na = __builtin_popcountll(am);
  const int rows = act ? (int)(d.dims & 0xffff) + 2 : 0;
  const int incl = gb::scan_add(rows);
  const int T_rows = __builtin_amdgcn_readlane(incl, 63);
  // compaction: entry a = the a-th computed testcase (lane order), gathered into lane a
  int src = 0;
  {
    uint64_t m = am;
    for (int a = 0; a < lane && m; a++) m &= m - 1;  // drop the first `lane` active lanes
    src = m ? __builtin_ctzll(m) : 63;
  }
  const int e_start = __shfl(incl - rows, src), e_R = __shfl(rows - 2, src);
  const uint32_t e_read = (uint32_t)__shfl((int)d.read_off, src), e_out = (uint32_t)__shfl((int)d.out_idx, src);
  const T init_Y = tab.init_const / (T)C;
  const uint8_t *hcode = pool + S.hap_off;
  for (int c = lane; c < C + kBndPad; c += kWave) {
    Brec<T> b;
    b.z = (T)0;
    b.w = (T)0;
    bnd[c] = b;
  }
  // column codes: the haplotype's at 1..C, 5 at column 0 and 6 below it (see va / v0), 0 beyond C
  for (int c = lane - kWave; c < C + kBndPad; c += kWave)
    hcol[c] = (c >= 1 && c <= C) ? hcode[c - 1] : (c == 0 ? 5 : (c < 0 ? 6 : 0));
  __syncthreads();

  // the stripe loop walks stacked rows from `base`; an early exit (f32 pass, `force` set) can skip the
  // rest of a testcase, so the stripes are not at fixed multiples of 64
  for (int base = 0; base < T_rows;) {
    if constexpr (kRoll) {
      if (roll && C >= kWave && T_rows - base > kWave) {
        base = phmm_rolled<T, kExit && !kF64Pass>(base, T_rows, na, C, lane, e_start, e_R, e_read, e_out, pool, tab,
                                                  init_Y, bnd, hcol, raw_out, exit_stats);
        __syncthreads();
        continue;
      }
    }
    const int g = base + lane;
    // the lane's testcase: the last entry starting at or before row g
    int lo = 0, hi = na - 1;
    while (__builtin_amdgcn_ballot_w64(lo < hi)) {  // per-lane binary search over lanes' starts
      const int mid = (lo + hi + 1) >> 1;
      const int sm = __shfl(e_start, mid);
      if (lo < hi) {
        if (sm <= g) lo = mid; else hi = mid - 1;
      }
    }
    StackEnt e;
    e.start = __shfl(e_start, lo);
    e.R = __shfl(e_R, lo);
    e.read_off = (uint32_t)__shfl((int)e_read, lo);
    e.out_idx = (uint32_t)__shfl((int)e_out, lo);
    const int r = g - e.start;  // 0: va, 1: v0, 2..R+1: read row r-2
    const bool dead = g >= T_rows;
    const uint8_t *rbase = pool + e.read_off;
    RowParams<T> P;
    LaneState<T> st;
    st.Mp = st.zo = st.wo = (T)0;
    st.Yp = (T)0;
    // bracket at column 0 of the row above: lane 0 takes it from the record lane 63 wrote there
    st.zd = lane == 0 ? bnd[0].z : (T)0;
    {
      T pMM, pGAPM, pMX, pXX, a, b, dm, dx;
      uint32_t f;
      const T zero = (T)0, one = (T)1;
      P.nMM = P.nGAPM = P.nGAPMx = P.nMX = P.nXX = zero;
      if (dead) {
        P.pMY = P.pYY = P.dmatch = P.dmis = zero;
        P.rmask = 0;
      } else if (r == 0) {  // va
        P.pMY = zero;
        P.pYY = one;
        P.dmatch = P.dmis = zero;
        P.rmask = 0;
        P.nGAPM = one;
        st.Yp = init_Y;
        // the state of a lane that has swept the columns before its first one: va's outputs are
        // constant, so it hands init_Y down from its first step
        st.zo = (zero * zero + zero * zero) + init_Y * one;
      } else if (r == 1) {  // v0
        P.pMY = P.pYY = zero;
        P.dmatch = one;
        P.dmis = zero;
        P.rmask = 0x3F;
        load_row(rbase, e.R, 0, tab, pMM, pGAPM, pMX, pXX, a, b, dm, dx, f);
        P.nMM = pGAPM;
        st.zd = init_Y;  // va's output at the column before
        // lane 0 starts at column 1: the row below takes v0's column-0 bracket from its initial zo
        if (lane == 0) st.zo = (init_Y * P.nMM + zero * zero) + zero * zero;
      } else {
        load_row(rbase, e.R, r - 2, tab, pMM, pGAPM, pMX, pXX, P.pMY, P.pYY, P.dmatch, P.dmis, P.rmask);
        if (r - 1 < e.R) {
          load_row(rbase, e.R, r - 1, tab, P.nMM, P.nGAPM, P.nMX, P.nXX, a, b, dm, dx, f);
          P.nGAPMx = P.nGAPM;
        }  // the last row: nothing below it in this testcase (zero partials)
      }
    }
    const bool last_row = !dead && r == e.R + 1;
    const uint64_t lastmask = __builtin_amdgcn_ballot_w64(last_row);
    const bool more = base + kWave < T_rows;
    const int steps = more ? C + kWave - 1 : C + (T_rows - base) - 1;
    T sumM = (T)0, sumX = (T)0;
    T *out = raw_out + e.out_idx;
    // lane 63's row and testcase for the early exit below, taken before the sweep into scalars
    int r63 = 0, R63 = 0, start63 = 0, out63 = 0;
    if (kExit && more) {
      r63 = __builtin_amdgcn_readlane(r, 63);
      R63 = __builtin_amdgcn_readlane(e.R, 63);
      start63 = __builtin_amdgcn_readlane(e.start, 63);
      out63 = __builtin_amdgcn_readlane((int)e.out_idx, 63);
    }
    if (lastmask) {
      if (more)
        phmm_stripe<T, true, true>(steps, st, P, sumM, sumX, bnd, hcol, C, lane, lastmask, out);
      else
        phmm_stripe<T, true, false>(steps, st, P, sumM, sumX, bnd, hcol, C, lane, lastmask, out);
    } else {
      phmm_stripe<T, false, true>(steps, st, P, sumM, sumX, bnd, hcol, C, lane, 0, out);
    }
    __syncthreads();
    int next = base + kWave;
    if constexpr (!kF64Pass && kExit) {
      // Early exit (GB_PHMM_EXIT). Every path of a testcase crosses from its row r to row r+1 once. The
      // crossing mass A_r = sum_c (z + w) of row r is what lane 63 just wrote for the next stripe,
      // already multiplied by row r+1's transitions. Row r+1 takes M = z * dist and X = w from it, so
      // its entering mass E = sum_c (M + X) is <= A_r (dist <= 1), and the result is the last row's E.
      // In between the mass can GROW: every single transition is <= 1, a state's total outflow is
      // not. Out of row k (its own pMY, pYY; row k+1's nMM, nMX, nGAPM, nXX) a unit of M sends
      // nMM + nMX straight down and pMY into Y, which hands pMY * nGAPM * sum_{j<C} pYY^j down along
      // the row; a unit of X sends nGAPM + nXX. So
      //   A_k <= g_k * E_k,   g_k = max(nMM + nMX + pMY * nGAPM / (1 - pYY), nGAPM + nXX),
      // and g_k > 1 on inputs the reference accepts:
      //   * clamped pMM: GKL clamps 1 - (10^(-i/10) + 10^(-d/10)) at 0 and does not renormalise, so
      //     for i, d of 0..3 nMM + nMX + pMY reaches 2;
      //   * the Y leak: Y stays with row k's ph2pr[c_k] and leaves with 1 - ph2pr[c_{k+1}], which sum
      //     to 1 only when c_k = c_{k+1}; with ph2pr[c_k] = 1 the geometric sum is C;
      //   * pMY is row k's while nMM, nMX are row k+1's: 10^(-d_k/10) - 10^(-d_{k+1}/10) is left over
      //     where the deletion quality falls from a row to the next (6.8e-5 a row for d of 40..45);
      //   * the rounding of the f32 tables (5.1e-8 where pMM > 0).
      // With G >= prod_k max(1, g_k) over the read's rows (exit_growth: the f32 table values used
      // here, in double; +inf where unbounded), result <= A_r * G in exact arithmetic. In f32 every
      // product and sum of these non-negative terms is at most its exact value times 1 + 2^-24, plus
      // 2^-150 where it rounds into the denormals. A path takes at most 4 roundings through a row
      // besides the Y chain's 2 per column, which act on the geometric sum like
      // pYY * (1 + 2^-24)^2 <= 0.7944: < (1 + 2^-24)^15 a row, < 1.07 over 65535 rows; the last row's
      // sums add (1 + 2^-24)^(C+1) < 1.004, this block's own sum < 1.0001; the denormal terms of a
      // whole 65535 x 65535 matrix, 12 operations a cell, sum to < 4e-35, each growing by at most G
      // afterwards. Hence the f32 result is < 1.08 * G * (A_r + 4e-35). The pack lets a read exit only
      // when its G <= kExitGrowthMax = 2 (kMayExit in its rows' match masks; benchmark-range reads, i
      // and d of 40..45 with one c, have G < 1.02 at 250 rows), so the test A_r < MIN_ACCEPTED / 4 gives
      // a result < 2.16 * (0.25e-28 + 4e-35) < MIN_ACCEPTED: the testcase must fail the f32 test. Its
      // remaining rows are skipped, its f32 result is written as 0, and the f64 pass computes it as it
      // would have anyway. Only rows with a row of the same testcase below them are tested.
      if (r63 >= 2 && r63 <= R63 && (__builtin_amdgcn_readlane((int)P.rmask, 63) & kMayExit)) {
        T acc = (T)0;
#pragma unroll 1
        for (int c = 1 + fresh(lane); c <= C; c += kWave) acc += bnd[c].z + bnd[c].w;
        acc = wave_sum_xor(acc);
        // the sum is the same in every lane; readfirstlane tells the compiler so (a divergent loop
        // bound would turn the whole stripe loop into per-lane control flow)
        if (__builtin_amdgcn_readfirstlane(acc < (T)0.25e-28f ? 1 : 0)) {
          next = start63 + R63 + 2;  // the next testcase's first (virtual) row
          if (lane == 0) {
            raw_out[(uint32_t)out63] = (T)0;
            // exit_stats[0] testcases dropped, [1] their cells not computed (real rows from the next
            // stripe's first row to the testcase's last)
            atomicAdd(exit_stats, 1ull);
            atomicAdd(exit_stats + 1, (unsigned long long)(next - (base + kWave)) * (unsigned long long)C);
          }
        }
        __syncthreads();
      }
    }
    base = next;
  }
  return na;
}

// cert_K as a call: inlined into the f64 pass's persistent loop, exp's polynomial constants are hoisted
// out of that loop into 28 registers that live through the f64 sweeps, which have 21 to spare
__device__ __attribute__((noinline)) double cert_K_call(double log_rho, int R, int C) { return cert_K(log_rho, R, C); }

// After a unit of the f64 pass, by the wave that computed it (lane a: the stack's entry a, as in
// phmm_stack): a predicted testcase whose f64 result proves the f32 result below MIN_ACCEPTED (cert_K) is
// confirmed and counts, with all its cells, in the early exit's statistics (nok, okcells); every other
// predicted testcase is marked in `redo` and counted in nre. A predicted testcase holds raw f32 0, so the
// unit has just computed it. Returns whether the unit has a testcase to redo.
__device__ __forceinline__ bool verify_unit(const Stack &S, int part, int parts, const uint32_t *__restrict__ stk_tc,
                                            const TcDesc *__restrict__ descs, const uint8_t *__restrict__ pool,
                                            const uint8_t *__restrict__ pred, const double *rd, uint8_t *redo,
                                            int &nok, int &nre, unsigned long long &okcells) {
  const int lane = threadIdx.x;
  bool act = lane < (int)S.count;
  if (parts > 1) act = act && lane >= part * (int)S.count / parts && lane < (part + 1) * (int)S.count / parts;
  bool ok = false, re = false;
  unsigned long long cells = 0;
  if (act) {
    const TcDesc d = descs[stk_tc[S.first + lane]];
    if (pred[d.out_idx]) {
      const int R = (int)(d.dims & 0xffff), C = (int)(d.dims >> 16);
      const uint8_t *lp = pool + d.read_off + 5 * (size_t)R;  // the read's log(rho), unaligned
      const uint32_t lb = (uint32_t)lp[0] | (uint32_t)lp[1] << 8 | (uint32_t)lp[2] << 16 | (uint32_t)lp[3] << 24;
      const double K = cert_K_call((double)__builtin_bit_cast(float, lb), R, C);
      ok = rd[d.out_idx] * 0x1p-900 * K + 4e-35 < (double)1e-28f;
      re = !ok;
      if (ok) cells = (unsigned long long)R * (unsigned long long)C;
      else redo[d.out_idx] = 1;
    }
  }
  const uint64_t okm = __builtin_amdgcn_ballot_w64(ok), rem = __builtin_amdgcn_ballot_w64(re);
  if (okm) {
    for (int o = 32; o >= 1; o >>= 1) cells += __shfl_xor(cells, o);
    okcells += (unsigned long long)__builtin_amdgcn_readfirstlane((int)(cells & 0xffffffffu)) |
               (unsigned long long)__builtin_amdgcn_readfirstlane((int)(cells >> 32)) << 32;
    nok += __builtin_popcountll(okm);
  }
  nre += __builtin_popcountll(rem);
  return rem != 0;
}

// f32 pass: one stack per workgroup (LPT order). f64 pass: a persistent grid takes stacks through
// counter[1] and recomputes their testcases whose f32 result fell below MIN_ACCEPTED; counter[0]
// counts them.
// kLong: stacks whose haplotype is longer than kLdsHaplen; their boundary records and codes live in
// `scratch` (scratch_stride bytes per workgroup, global memory: lane 63's record stores and lane 0's
// loads of the next stripe are ordered by the stripe's __syncthreads), and both passes take the
// stacks through a persistent grid (counter[2] f32, counter[3] f64).
// The LDS kernels' registers are held to the waves per SIMD their LDS allows (f32 8, f64 4). As built
// by the Makefile (-O3 -ffp-contract=off -fno-slp-vectorize -mllvm -amdgpu-sched-strategy=max-ilp)
// the f32 kernels take 59 and, with the exit, 64 registers without a spill (phmm_rolled's RowDesc,
// fresh(), wave_sum_xor) and the f64 kernel 113 of 128 (107 before it took the f32 sweep in); without the
// max-ilp scheduler the parent's were 58 / 64 / 94.
// The f64 pass over the LDS stacks also settles the predictor's testcases (`sel` = pred, set when the
// batch predicted): after each unit the wave confirms its predicted entries from the f64 results it has
// just stored (verify_unit) and, where one is not confirmed, sweeps those entries in f32 at once (the
// tables at `tabf`, into `raw_f`, sel = redo), in the same LDS; the SIMD's other waves hide that single
// wave's latency. No list, and no wave waits on another.
template <typename T, bool kF64Pass, bool kLong = false, bool kExit = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kLong ? 1 : (sizeof(T) == 4 ? 8 : 4), 8))) void phmm_forward(
    const Stack *__restrict__ stacks, int nstacks,
                                                    const uint32_t *__restrict__ stk_tc,
                                                    const TcDesc *__restrict__ descs,
                                                    const uint8_t *__restrict__ pool, DevTab<T> tab,
                                                    T *__restrict__ raw_out, const float *raw_f,
                                                    int *__restrict__ counter, int force, uint8_t *scratch,
                                                    size_t scratch_stride, const uint32_t *__restrict__ units,
                                                    const uint8_t *__restrict__ sel, int sel_want,
                                                    const float *tabf, uint8_t *redo) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  uint8_t *rec = kLong ? scratch + (size_t)blockIdx.x * scratch_stride : smem_raw;
  const bool roll = (force >> 16) & 1;  // the LDS stacks' rolled sweep (phmm_rolled; GB_PHMM_ROLL)
  if constexpr (kF64Pass || kLong) {
    int done = 0;
    // the predictor's totals of this wave (wave-uniform): confirmed, their cells, redone
    int nok = 0, nre = 0;
    unsigned long long okcells = 0;
    int *next = counter + (kLong ? (kF64Pass ? 3 : 2) : 1);
    // f64 pass over the LDS stacks: `parts` work units per stack (the top byte of `force`), so a job
    // of few stacks per worker balances its fallback work finer
    const int parts = (kF64Pass && !kLong) ? max(1, (force >> 8) & 0xFF) : 1;
    // with a plan (f64_plan / f64_plan_order): only the units that have work, costliest first
    const int nwork = units ? __builtin_amdgcn_readfirstlane(counter[kPlanTotal]) : nstacks * parts;
    while (true) {
      int k = 0;
      if (threadIdx.x == 0) k = atomicAdd(next, 1);
      k = __builtin_amdgcn_readfirstlane(__shfl(k, 0));
      if (k >= nwork) break;
      if (units) k = __builtin_amdgcn_readfirstlane((int)units[k]);
      const int nf = phmm_stack<T, kF64Pass, false, !kLong>(stacks[k / parts], stk_tc, descs, pool, tab, raw_out, raw_f,
                                                            (force & 0xFF) != 0, rec, k % parts, parts, nullptr, roll);
      done += nf;
      __syncthreads();  // the next stack re-initialises the records
      if constexpr (kF64Pass && !kLong) {
        // (the barrier above has also waited for the unit's result stores: verify_unit reads them back)
        if (sel && nf) {
          if (verify_unit(stacks[k / parts], k % parts, parts, stk_tc, descs, pool, sel, raw_out, redo, nok, nre,
                          okcells)) {
            __syncthreads();
            phmm_stack<float, false, false, true>(stacks[k / parts], stk_tc, descs, pool, dev_tab(tabf, 0x1p120f),
                                                  const_cast<float *>(raw_f), nullptr, false, rec, k % parts, parts,
                                                  nullptr, roll, redo, 1);
            __syncthreads();
          }
        }
      }
    }
    if (kF64Pass && threadIdx.x == 0) {
      if (done) atomicAdd(counter, done);
      if (nok) {
        atomicAdd(counter + kPredConfirmed, nok);
        atomicAdd(reinterpret_cast<unsigned long long *>(counter + 4), (unsigned long long)nok);
        atomicAdd(reinterpret_cast<unsigned long long *>(counter + 4) + 1, okcells);
      }
      if (nre) atomicAdd(counter + kPredRedone, nre);
    }
  } else {
    phmm_stack<T, false, kExit, true>(stacks[blockIdx.x], stk_tc, descs, pool, tab, raw_out, nullptr, false, rec, 0, 1,
                                      reinterpret_cast<unsigned long long *>(counter + 4), roll, sel, sel_want);
  }
}

// f64 pass plan: the persistent grid's units (stack parts) ordered by their cost, costliest first, so
// the grid's tail is its cheapest units -- a 1/8 shard's f64 pass has only ~8 units per resident
// wave, and ordered by the f32 pass's stack order (its rows, not the fallback's) its last units were
// as long as any. f64_plan: per unit the stripes of its fallback rows times the columns a stripe
// sweeps, as a bucket key (0: no fallback row), and the buckets' counts; f64_plan_order: the units
// with work into `units`, by descending key (any order inside a bucket: a unit's outputs do not
// depend on when it runs).
__global__ __launch_bounds__(256) void f64_plan(const Stack *__restrict__ stacks, int nunits, int parts,
                                                const uint32_t *__restrict__ stk_tc, const TcDesc *__restrict__ descs,
                                                const float *__restrict__ raw_f, int force, int roll,
                                                uint8_t *__restrict__ ukey, int *__restrict__ counter) {
  __shared__ int hist[kPlanBuckets];
  for (int i = threadIdx.x; i < kPlanBuckets; i += blockDim.x) hist[i] = 0;
  __syncthreads();
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < nunits) {
    const Stack S = stacks[u / parts];
    const int part = u % parts, lo = part * (int)S.count / parts, hi = (part + 1) * (int)S.count / parts;
    int rows = 0;
    for (int a = lo; a < hi; a++) {
      const TcDesc d = descs[stk_tc[S.first + a]];
      if (force || raw_f[d.out_idx] < 1e-28f) rows += (int)(d.dims & 0xffff) + 2;  // as phmm_stack's `act`
    }
    int key = 0;
    if (rows) {
      key = (int)((stack_steps(rows, (int)S.C, kWave, roll != 0) + 63) / 64);
      key = key < 1 ? 1 : (key > kPlanBuckets - 1 ? kPlanBuckets - 1 : key);
      atomicAdd(&hist[key], 1);
    }
    ukey[u] = (uint8_t)key;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kPlanBuckets; i += blockDim.x)
    if (hist[i]) atomicAdd(&counter[kPlanCount + i], hist[i]);
}

__global__ __launch_bounds__(256) void f64_plan_order(int nunits, const uint8_t *__restrict__ ukey,
                                                      int *__restrict__ counter, uint32_t *__restrict__ units) {
  __shared__ int cnt[kPlanBuckets], off[kPlanBuckets], hist[kPlanBuckets], base[kPlanBuckets];
  for (int i = threadIdx.x; i < kPlanBuckets; i += blockDim.x) {
    cnt[i] = counter[kPlanCount + i];
    hist[i] = 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // bucket offsets, descending key
    int sum = 0;
    for (int k = kPlanBuckets - 1; k >= 1; k--) {
      off[k] = sum;
      sum += cnt[k];
    }
    if (blockIdx.x == 0) counter[kPlanTotal] = sum;
  }
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  const int key = u < nunits ? ukey[u] : 0;
  int rank = 0;
  if (key) rank = atomicAdd(&hist[key], 1);
  __syncthreads();
  for (int i = threadIdx.x; i < kPlanBuckets; i += blockDim.x)
    if (hist[i]) base[i] = atomicAdd(&counter[kPlanCursor + i], hist[i]);
  __syncthreads();
  if (key) units[off[key] + base[key] + rank] = (uint32_t)u;
}

// ---------------------------------------------------------------------------------------------
// Fallback predictor. A testcase whose f32 result is below MIN_ACCEPTED is computed twice: by the f32
// pass, which throws the result away, and by the f64 pass. phmm_predict picks such testcases before the
// f32 pass from an integer estimate of the likelihood (tests/phmm_predict_ref.py restates it in numpy,
// decision for decision): the cheapest ungapped diagonal among -63 .. C - R + 63, a mismatch costing
// 1.4 / 2.5 / 3.9 (base quality below 14 / below 28 / from 28) and an overhang of n rows 4.5 + (n - 1), in
// units of 0.01 log10; predicted when the cost exceeds -log10(MIN_ACCEPTED * 2^-120 * C) + kPredMargin.
// A predicted testcase gets pred = 1 and raw f32 = 0: the f32 pass compacts it out of its stack and the
// f64 pass takes it. The estimate is not a bound. The f64 pass confirms a prediction from the f64 result
// and the read's certificate (verify_unit; cert_K: f32 <= K * f64 * 2^-900 + 4e-35, so f32 < MIN_ACCEPTED
// is proved); what it cannot confirm is marked `redo`, and the wave that computed the unit sweeps those
// testcases in f32 after all, inside the f64 pass's grid, as if they had never been
// predicted. Only certified reads are predicted.
// The kernel: a wave per stack. The haplotype's columns become four bit planes in LDS (base A / C / T /
// G, each also set for N and outside the haplotype, whose rows cost their overhang), column c at bit c + 64. Per testcase, 64 rows at a time, the
// read's rows become seven wave-uniform bit planes by ballot (the row's match-mask bits 0..3, three
// quality classes). A lane owns one diagonal of a 64-diagonal chunk: for 32 rows the haplotype planes'
// bits of its diagonal are a funnel shift of two LDS words (three words serve 64 rows), mismatch =
// ~OR(read_b & hap_b), three popcounts: about 18 VALU instructions per 32 rows x 64 diagonals.
// Gate: whether a batch falls back at all is a property of its packed testcases, so it is decided where
// they are packed. batch_fill launches the kernel in kPredSample mode behind its uploads: kGateTake
// testcases of one stack in 16 (of every stack up to kGateAll stacks; chosen by the stack's place in the
// testcase list, so both sweeps' launch orders sample alike; positions that move through the stack with
// that place, since a stack's first testcases are the first of its haplotype in input order; a
// wave's time is the latency of its testcases one after the other, so it takes few), counted with their
// predictions and nothing else written, read back at the synchronisation the fill ends with. With fewer
// than 1 in kGateDen predicted the gate is closed and gb_phmm_batch_run launches exactly what it launched
// without the predictor: a batch that does not fall back pays nothing per step. A one-shot call
// (gb_phmm_compute) pays the sample at every fill and the redone testcases' latency at every step, about
// 0.5 ms, so there the predictor is used from kPredMinCells cells a call only; a batch made by
// gb_phmm_batch_create is sampled once and run many times, and is predicted at any size.
// kPredOpen: everything with no gate (GB_PHMM_PREDICT=open), kPredAll: every certified testcase.
constexpr int kPredMargin = -100, kPredThresh = 6412, kPredPad = 63;
constexpr int kPredMaxRows = 2046;
constexpr int kPlaneWords = 320;  // >= (kLdsHaplen + 64 + 256) / 32 + 3, even
constexpr int kPredChunks = 4;    // 64-diagonal chunks sharing one pass over the read's rows
constexpr int kGateDen = 8, kGateTake = 2, kGateAll = 1024;  // (one stack in 16: the top 4 bits of a hash)
constexpr int64_t kPredMinCells = 5000000000ll;  // one-shot calls: 0.5 ms fixed against 12 % of a 4 ms step
static_assert(kPlaneWords % 2 == 0 && kPlaneWords >= (kLdsHaplen + 64 + 256) / 32 + 3, "plane words");
enum PredictMode { kPredSample = 0, kPredAll = 2, kPredOpen = 3 };

__device__ __forceinline__ int pred_overhang(int n) { return n > 0 ? 350 + 100 * n : 0; }

__global__ __launch_bounds__(64) void phmm_predict(const Stack *__restrict__ stacks, int nstacks,
                                                   const uint32_t *__restrict__ stk_tc,
                                                   const TcDesc *__restrict__ descs, const uint8_t *__restrict__ pool,
                                                   float *__restrict__ raw_f, uint8_t *__restrict__ pred,
                                                   int *__restrict__ counter, int mode) {
  __shared__ uint32_t plane[4][kPlaneWords];
  const int lane = threadIdx.x;
  const int first = (int)blockIdx.x, stride = (int)gridDim.x;
  int seen = 0, npred = 0;
  for (int k = first; k < nstacks; k += stride) {
    const Stack S = stacks[k];
    const int C = (int)S.C;
    // the sample takes kGateTake of the stack's testcases, half a stack apart, from a position that moves
    // with the stack's index
    const int cnt = (int)S.count;
    // which stacks and testcases the sample takes depends on the stack's place in the testcase list, not
    // on the launch order (which differs between the two sweeps): the same batch, the same gate
    if (mode == kPredSample && nstacks > kGateAll && ((S.first * 2654435761u) >> 28) != 0) continue;
    const int n_take = mode == kPredSample ? min(kGateTake, cnt) : cnt;
    const int a_first = mode == kPredSample ? (int)((S.first >> 4) % (uint32_t)cnt) : 0;
    const int a_step = mode == kPredSample ? (cnt + 1) / 2 : 1;
    seen += n_take;
    if (C > kLdsHaplen) continue;
    const uint8_t *hcode = pool + S.hap_off;
    const int nw = (C + 64 + 256) / 32 + 2;
    __syncthreads();
    for (int j = 0; 2 * j < nw; j++) {
      const int c = 64 * j + lane - 64;
      const uint32_t code = (c >= 0 && c < C) ? hcode[c] : 255u;
      // outside the haplotype every base "matches": those rows cost their overhang, added per diagonal
      uint64_t m[4];
      for (int b = 0; b < 4; b++) m[b] = __builtin_amdgcn_ballot_w64(code == (uint32_t)b || code >= 4u);
      if (lane < 8) {
        const uint64_t v = lane < 2 ? m[0] : lane < 4 ? m[1] : lane < 6 ? m[2] : m[3];
        plane[lane >> 1][2 * j + (lane & 1)] = (uint32_t)(v >> (32 * (lane & 1)));
      }
    }
    __syncthreads();
    const int lcC = [&]() {
      const int msb = 31 - __builtin_clz((uint32_t)C);
      const uint32_t l2 = ((uint32_t)msb << 8) | ((((uint32_t)C << (31 - msb)) >> 23) & 0xFFu);
      return (int)((l2 * 7706u) >> 16);
    }();
    const int thr = kPredThresh - lcC + kPredMargin;
    for (int j = 0; j < n_take; j++) {
      const int a = (a_first + j * a_step) % cnt;
      const TcDesc d = descs[stk_tc[S.first + a]];
      const int R = (int)(d.dims & 0xffff);
      const uint8_t *rb = pool + d.read_off;
      if (!(rb[R] & kMayPredict) || R > kPredMaxRows) continue;
      // only `best > thr` leaves the kernel, and every term of a diagonal's cost is non-negative: a chunk
      // with no diagonal at or below thr after some rows is left (`alive`, wave-uniform, looked at after every
      // 64 rows that have rows below them; both overhangs are known before row 0 and count from there), and
      // a group that ends with a diagonal at or below thr decides "not predicted" for the testcase
      bool low = false;
      if (mode != kPredAll) {
        const int dhi = C - R + kPredPad;
        for (int g0 = 0; g0 - kPredPad <= dhi && !low; g0 += 64 * kPredChunks) {
          const int nch = min(kPredChunks, (dhi + kPredPad - g0) / 64 + 1);
          const int e0 = 1 + g0 + lane;  // the lane's diagonal of chunk 0, + 64: its bit at row 0
          const uint32_t sh = (uint32_t)e0 & 31u;
          const uint32_t *w0 = &plane[0][e0 >> 5];
          uint32_t n0[kPredChunks], n1[kPredChunks], n2[kPredChunks];
          for (int c = 0; c < kPredChunks; c++) n0[c] = n1[c] = n2[c] = 0;
          // chunk c's diagonal of this lane at or below thr, with the rows counted so far
          auto at_or_below = [&](int c) {
            const int dg = g0 + 64 * c + lane - kPredPad;
            const int n_lo = min(R, max(0, -dg)), n_hi = min(R - n_lo, max(0, R + dg - C));
            const int cost = 140 * (int)n0[c] + 250 * (int)n1[c] + 390 * (int)n2[c] + pred_overhang(n_lo) +
                             pred_overhang(n_hi);
            return dg <= dhi && cost <= thr;
          };
          uint32_t alive = (1u << nch) - 1u;
          for (int r64 = 0; r64 < R && alive; r64 += 64) {
            const int row = r64 + lane;
            const bool in = row < R;
            const uint32_t rm = in ? rb[row] : 0u, qv = in ? (uint32_t)(rb[R + row] & 127) : 0u;
            uint64_t rp[4], qp[3];
            for (int b = 0; b < 4; b++) rp[b] = __builtin_amdgcn_ballot_w64((rm >> b) & 1u);
            qp[0] = __builtin_amdgcn_ballot_w64(in && qv < 14u);
            qp[1] = __builtin_amdgcn_ballot_w64(in && qv >= 14u && qv < 28u);
            qp[2] = __builtin_amdgcn_ballot_w64(in && qv >= 28u);
            // rows r64 .. r64 + 31 take the planes' words j, j + 1 of the lane's diagonal, rows r64 + 32 ..
            // words j + 1, j + 2; rows from R on are in no quality class
            const uint32_t *w = w0 + (r64 >> 5);
            const bool two = r64 + 32 < R;
#pragma unroll
            for (int c = 0; c < kPredChunks; c++) {
              if ((alive >> c) & 1u) {
                uint32_t ha[4], hb[4];
#pragma unroll
                for (int p = 0; p < 4; p++) {
                  const uint32_t x0 = w[p * kPlaneWords + 2 * c], x1 = w[p * kPlaneWords + 2 * c + 1];
                  const uint32_t x2 = w[p * kPlaneWords + 2 * c + 2];
                  ha[p] = __builtin_amdgcn_alignbit(x1, x0, sh);
                  hb[p] = __builtin_amdgcn_alignbit(x2, x1, sh);
                }
                const uint32_t ma = ~(((uint32_t)rp[0] & ha[0]) | ((uint32_t)rp[1] & ha[1]) | ((uint32_t)rp[2] & ha[2]) |
                                      ((uint32_t)rp[3] & ha[3]));
                n0[c] += __builtin_popcount(ma & (uint32_t)qp[0]);
                n1[c] += __builtin_popcount(ma & (uint32_t)qp[1]);
                n2[c] += __builtin_popcount(ma & (uint32_t)qp[2]);
                if (two) {
                  const uint32_t mb = ~(((uint32_t)(rp[0] >> 32) & hb[0]) | ((uint32_t)(rp[1] >> 32) & hb[1]) |
                                        ((uint32_t)(rp[2] >> 32) & hb[2]) | ((uint32_t)(rp[3] >> 32) & hb[3]));
                  n0[c] += __builtin_popcount(mb & (uint32_t)(qp[0] >> 32));
                  n1[c] += __builtin_popcount(mb & (uint32_t)(qp[1] >> 32));
                  n2[c] += __builtin_popcount(mb & (uint32_t)(qp[2] >> 32));
                }
              }
            }
            if (r64 + 64 < R) {
#pragma unroll
              for (int c = 0; c < kPredChunks; c++)
                if (((alive >> c) & 1u) && !__builtin_amdgcn_ballot_w64(at_or_below(c))) alive &= ~(1u << c);
            }
          }
          // a chunk that stayed alive has swept all rows: its costs are final (a dead one's are above thr)
#pragma unroll
          for (int c = 0; c < kPredChunks; c++)
            if ((alive >> c) & 1u) low = low || at_or_below(c);
          low = __builtin_amdgcn_ballot_w64(low) != 0;
        }
      }
      if (!low) {
        npred++;
        if (lane == 0 && mode != kPredSample) {
          pred[d.out_idx] = 1;
          raw_f[d.out_idx] = 0.f;
        }
      }
    }
  }
  if (lane == 0) {
    if (mode == kPredSample && seen) atomicAdd(counter + kPredSampled, seen);
    if (mode == kPredSample && npred) atomicAdd(counter + kPredSamplePred, npred);
    if (mode != kPredSample && npred) atomicAdd(counter + kPredPredicted, npred);
  }
}

// gb_phmm_init's warm-up launch (no work)
__global__ void phmm_warm(int *count) {
  if (threadIdx.x == 0 && blockIdx.x == 0) count[3] = 0;
}

// Device log10 epilogue (IntelPairHmmCSource.cpp:73-79); the host path recomputes it bit-exactly.
// After a predicted run (`redo` set): a redone testcase whose f32 result passes MIN_ACCEPTED is answered from
// f32, as in the reference: its f64 result reads 0 like that of any testcase that never fell back, and it
// leaves the count of fallbacks (counter[0], gb_phmm_batch_stats).
__global__ void phmm_finalize(const float *__restrict__ rf, double *__restrict__ rd,
                              const uint8_t *__restrict__ redo, double *__restrict__ out, int n,
                              float log10_init_f, double log10_init_d, int *__restrict__ counter) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (redo && redo[i] && rf[i] >= 1e-28f) {
    rd[i] = 0.0;
    atomicSub(counter, 1);
  }
  out[i] = (rf[i] < 1e-28f) ? (log10(rd[i]) - log10_init_d) : (double)(log10f(rf[i]) - log10_init_f);
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Host state
// ---------------------------------------------------------------------------------------------
// The host tables, built once (ensure_host_tables); the pack reads hf and cert.
struct gb::phmm::PackTables {
  HostTables<float> hf;
  HostTables<double> hd;
  CertTab cert;
};

namespace {

struct DeviceTables {
  int device = -1;
  float *f = nullptr;   // ph2pr | one_minus | div3 | m2m
  double *d = nullptr;
  HostTables<float> hf;
  HostTables<double> hd;
};

std::mutex g_mu;
PackTables *g_host = nullptr;
std::unordered_map<int, DeviceTables *> g_dev;

int ensure_host_tables() {
  if (!g_host) {
    auto *t = new PackTables();
    build_tables(t->hf);
    build_tables(t->hd);
    build_cert_tab(t->hf, t->hd, t->cert);
    g_host = t;
  }
  return GB_OK;
}

// The device tables live as long as the process and are shared by every batch and thread, behind
// g_mu: raw pointers that are never freed (a free at process exit could run after the HIP runtime
// is torn down, and an owning buffer may not have static storage duration).
template <typename T>
int upload_tables(const HostTables<T> &h, T **dst) {
  const size_t nel = 3 * kQualTab + kM2M;
  std::vector<T> blob(nel);
  std::memcpy(blob.data(), h.ph2pr, sizeof(T) * kQualTab);
  std::memcpy(blob.data() + kQualTab, h.one_minus, sizeof(T) * kQualTab);
  std::memcpy(blob.data() + 2 * kQualTab, h.div3, sizeof(T) * kQualTab);
  std::memcpy(blob.data() + 3 * kQualTab, h.m2m, sizeof(T) * kM2M);
  GB_HIP(hipMalloc(dst, sizeof(T) * nel));
  GB_HIP(hipMemcpy(*dst, blob.data(), sizeof(T) * nel, hipMemcpyHostToDevice));
  return GB_OK;
}

int get_device_tables(DeviceTables **out) {
  std::lock_guard<std::mutex> lk(g_mu);
  ensure_host_tables();
  int dev = -1;
  GB_HIP(hipGetDevice(&dev));
  auto it = g_dev.find(dev);
  if (it != g_dev.end()) {
    *out = it->second;
    return GB_OK;
  }
  auto *t = new DeviceTables();
  t->device = dev;
  t->hf = g_host->hf;
  t->hd = g_host->hd;
  int st = upload_tables(g_host->hf, &t->f);
  if (st) return st;
  st = upload_tables(g_host->hd, &t->d);
  if (st) return st;
  for (auto fn : {(const void *)phmm_forward<float, false>, (const void *)phmm_forward<float, false, false, true>,
                  (const void *)phmm_forward<double, true>})
    GB_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  g_dev[dev] = t;
  *out = t;
  return GB_OK;
}

// Deduplication keys: the caller shares read/haplotype buffers across the R x H cross product
// (PairHMMUnitTest.cpp:564-579); identical pointers + length => identical packed record.
struct ReadKey {
  const char *rs, *q, *i, *d, *c;
  int len;
  bool operator==(const ReadKey &o) const {
    return rs == o.rs && q == o.q && i == o.i && d == o.d && c == o.c && len == o.len;
  }
};
struct KeyHash {
  size_t mix(size_t a, size_t b) const { return a ^ (b + 0x9e3779b97f4a7c15ull + (a << 6) + (a >> 2)); }
  size_t operator()(const ReadKey &k) const {
    size_t h = std::hash<const void *>()(k.rs);
    for (const void *p : {(const void *)k.q, (const void *)k.i, (const void *)k.d, (const void *)k.c})
      h = mix(h, std::hash<const void *>()(p));
    return mix(h, (size_t)k.len);
  }
  size_t operator()(const HapKey &k) const { return mix(std::hash<const void *>()(k.h), (size_t)k.len); }
};

}  // namespace

struct gb_phmm_batch {
  DeviceTables *tabs = nullptr;
  gb::Stream stream;
  gb::Event ev[4];
  int n = 0;
  int max_haplen = 0;
  int64_t cells = 0;
  gb::PinnedBuf<uint8_t> h_stage;  // upload staging (grow-only)
  gb::DevBuf<uint8_t> d_arena;     // holds d_desc, d_rf, d_rd, d_out, d_stk_tc, d_stacks, d_units, d_ukey
  TcDesc *d_desc = nullptr;
  gb::DevBuf<uint8_t> d_pool;
  float *d_rf = nullptr;
  double *d_rd = nullptr;
  double *d_out = nullptr;
  uint32_t *d_stk_tc = nullptr;  // testcase indices, stack by stack
  Stack *d_stacks = nullptr;     // LPT order
  int nstacks = 0;                 // stacks whose haplotype fits the LDS (the first nstacks)
  int n_long = 0;                  // stacks behind them whose haplotype does not (kLong kernels)
  int long_grid = 0;               // their persistent grid
  gb::DevBuf<uint8_t> d_scratch;   // their boundary records, scratch_stride bytes per workgroup
  size_t scratch_stride = 0;
  gb::DevBuf<int> d_count;  // [0] testcases recomputed by the f64 pass, [1] its stack counter,
                           // [4..7] the f32 early exit's two u64 counts (testcases, cells skipped),
                           // [2] / [3] the kLong f32 / f64 stack counters, then the f64 plan's words
                           // (kCountWords in all)
  uint32_t *d_units = nullptr;  // f64 plan: units with work, costliest first (kMaxF64Parts per testcase)
  uint8_t *d_ukey = nullptr;    // f64 plan: per unit its cost bucket
  int f64_grid = 0;                // persistent f64 grid: resident workgroups of the device
  int cus = 256;                   // compute units of the device (stack height rule)
  bool ran = false;
  bool force_f64 = false;
  Knobs knobs;  // the last fill's (read_knobs); the launches read f64_parts, f64_plan, f32_exit, roll and predict
  bool resident = false;  // made by gb_phmm_batch_create (packed once, run many times), not a one-shot workspace
  bool gate_open = false; // batch_fill's sample: enough of the batch is predicted for the predictor to run
  int gate_n = 0, gate_pred = 0;  // the sample's testcases and predictions
  uint8_t *d_pred = nullptr;  // per testcase: predicted (skips the f32 pass), and behind it d_redo
  uint8_t *d_redo = nullptr;  // per testcase: prediction not confirmed, f32 result computed after all, inside the f64 pass
  size_t pred_bytes = 0;      // of d_rd, d_pred and d_redo together (adjacent in the arena)
  // host scratch of the fills (grow-only, host_reserve)
  std::vector<uint32_t> hid;
  std::vector<Stack> stacks;
  std::vector<uint64_t> skeys;
  std::vector<std::vector<uint8_t>> pools;
};

namespace {
int warm_up(DeviceTables *t);
}

extern "C" {

int gb_phmm_init(void) {
  DeviceTables *t = nullptr;
  int st = get_device_tables(&t);
  if (st) return st;
  return warm_up(t);
}

}  // extern "C"

namespace {

// Device buffers of a batch for n testcases and a pool of pool_bytes (grow-only). The pipelined path
// reserves every chunk's buffers before its first launch: an allocation that grows a buffer frees
// the old one, and hipFree waits for the device.
int batch_reserve(gb_phmm_batch *b, int n, size_t pool_bytes) {
  const ArenaLayout A = arena_layout(std::max(n, 1));
  // every array grows with n, so an arena that holds this total was carved for at least these sizes
  if (A.total > b->d_arena.capacity()) {
    // the per-testcase arrays carved from one allocation (a cold process pays per hipMalloc)
    b->d_desc = nullptr;
    b->d_rf = nullptr;
    b->d_rd = b->d_out = nullptr;
    b->d_stk_tc = nullptr;
    b->d_stacks = nullptr;
    b->d_units = nullptr;
    b->d_ukey = nullptr;
    b->d_pred = b->d_redo = nullptr;
    if (int st = b->d_arena.reserve(A.total)) return st;
    uint8_t *a = b->d_arena;
    b->d_desc = (TcDesc *)(a + A.desc);
    b->d_rf = (float *)(a + A.rf);
    b->d_rd = (double *)(a + A.rd);
    b->d_pred = a + A.pred;
    b->d_redo = a + A.redo;
    b->pred_bytes = A.out - A.rd;  // d_rd, d_pred and d_redo are zeroed by one fill
    b->d_out = (double *)(a + A.out);
    b->d_stk_tc = (uint32_t *)(a + A.stk_tc);
    b->d_stacks = (Stack *)(a + A.stacks);
    b->d_units = (uint32_t *)(a + A.units);
    b->d_ukey = a + A.ukey;
  }
  if (int st = b->d_pool.reserve(pool_bytes)) return st;
  return b->d_count.reserve(kCountWords);
}

// grow-only pinned staging buffer of a batch (uploads, results); its first `keep` bytes survive a growth
int stage_reserve(gb_phmm_batch *b, size_t bytes, size_t keep = 0) {
  if (bytes <= b->h_stage.capacity()) return GB_OK;
  gb::PinnedBuf<uint8_t> h;
  if (int st = h.reserve(bytes)) return st;
  if (keep && b->h_stage) std::memcpy(h, b->h_stage, std::min(keep, b->h_stage.capacity()));
  b->h_stage = std::move(h);
  return GB_OK;
}

// Host scratch of a batch's fills for n testcases and pack pools of pool_bytes in all, kept across
// fills and touched here: a fresh vector pays a page fault per 4 KiB at its first write, and several
// fills faulting at once serialise on the process's memory map.
void host_reserve(gb_phmm_batch *b, size_t n, size_t pool_bytes, int threads) {
  if (b->hid.size() < n) b->hid.assign(n, 0);
  if (b->stacks.size() < n) b->stacks.assign(n, Stack{});
  if (b->skeys.size() < 2 * n) b->skeys.assign(2 * n, 0);
  if ((int)b->pools.size() < threads) b->pools.resize(threads);
  for (int t = 0; t < threads; t++) {
    auto &P = b->pools[t];
    const size_t want = pool_bytes / threads + 4096;
    if (P.capacity() < want) {
      P.clear();
      P.shrink_to_fit();
      P.resize(want);  // touch
    }
    P.clear();
  }
}

// Staging layout of a fill of n testcases and a pool of pool_bytes: descriptors | stack testcase
// lists | stacks (at most one per testcase) | pool
struct StageLayout {
  size_t o_tc, o_stk, o_pool, total;
  StageLayout(size_t n, size_t pool_bytes) {
    auto up = [](size_t x) { return gb::round_up<size_t>(x, 256); };
    o_tc = up(sizeof(TcDesc) * n);
    o_stk = o_tc + up(sizeof(uint32_t) * n);
    o_pool = o_stk + up(sizeof(Stack) * n);
    total = o_pool + up(pool_bytes) + 256;
  }
};

// The limits of include/gb_phmm.h, checked before any device work; the error names the first bad
// testcase by its index in the caller's array.
int validate_testcases(const gb_testcase *tcs, int n) {
  for (int k = 0; k < n; k++) {
    const gb_testcase &t = tcs[k];
    GB_ARG(t.rslen >= 1 && t.rslen <= 65535, "testcase %d: rslen %d outside [1,65535]", k, t.rslen);
    GB_ARG(t.haplen >= 1 && t.haplen <= kMaxHaplen, "testcase %d: haplen %d outside [1,%d]", k,
           t.haplen, kMaxHaplen);
    GB_ARG(t.rs && t.q && t.i && t.d && t.c && t.hap, "testcase %d: null sequence pointer", k);
  }
  return GB_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// A fill's host steps (phmm_internal.h): knobs, pack, merge, plan. No HIP call, no batch.
// ---------------------------------------------------------------------------------------------
namespace gb {
namespace phmm {

const PackTables &host_tables() {
  std::lock_guard<std::mutex> lk(g_mu);
  ensure_host_tables();
  return *g_host;
}

Knobs read_knobs() {
  Knobs K;
  // calls from 8 K testcases pack on several threads (2 K testcases each at least): the reference's
  // per-batch calls (PairHMMUnitTest.cpp:549-593) are mostly 5-45 K testcases
  if (const char *e = getenv("GB_PHMM_PACK_MIN")) K.pack_min = std::max(1, atoi(e));  // probes
  // work units per stack in the f64 pass: in stack order, two units per stack took the 1/8 shard's
  // f64 pass 2.28 -> 2.00 ms (profiles/r05e_phmm_f64_parts.log); ordered by cost (f64_plan) one unit
  // per stack is best: the shard 1.93 (stack order, two) -> 1.82 (plan, two) -> 1.78 ms (plan, one), the
  // whole job 13.19 -> 13.07 -> 12.95 ms (profiles/r06x_phmm_f64_plan.log)
  if (const char *e = getenv("GB_PHMM_F64_PARTS")) K.f64_parts = std::max(1, std::min(kMaxF64Parts, atoi(e)));
  if (const char *e = getenv("GB_PHMM_F64_PLAN")) K.f64_plan = atoi(e) != 0;
  // the f32 pass drops a testcase's remaining rows once its crossing mass proves it falls back to f64
  // (phmm_stack kExit): f32 pass 19.05 -> 18.40 ms, step +2.0 % (profiles/r05zzi_phmm_exit_ab.log);
  // finals, raw f64 and the fallback choice unchanged, a dropped testcase's raw f32 reads 0
  if (const char *e = getenv("GB_PHMM_EXIT")) K.f32_exit = atoi(e) != 0;
  // rolled stripes (phmm_rolled) in both passes
  if (const char *e = getenv("GB_PHMM_ROLL")) K.roll = atoi(e) != 0;
  // the fallback predictor (phmm_predict): on; GB_PHMM_PREDICT=0 off, =all every certified testcase with
  // the gate off (tests: every passing testcase then takes the verify -> redo path), =open the estimate
  // with the gate off (tests of jobs too small for the gate's sample)
  if (const char *e = getenv("GB_PHMM_PREDICT"))
    K.predict = strcmp(e, "all") == 0 ? 2 : strcmp(e, "open") == 0 ? 3 : (atoi(e) != 0 ? 1 : 0);
  if (const char *e = getenv("GB_PHMM_STACK_ROWS")) K.stack_rows_forced = std::max(1, atoi(e));  // probes
  // GB_PHMM_TAIL=frac:rows (0 = off) for probes of plan_stacks' tail split
  if (const char *te = getenv("GB_PHMM_TAIL")) {
    K.tail_frac = std::max(0.0, atof(te));  // (anything not above 0 is off)
    const char *cm = strchr(te, ':');
    if (cm) K.tail_rows = std::max(1, atoi(cm + 1));
  }
  return K;
}

// One chunk of the pack. The reference driver's r-major loop repeats a read for every haplotype and cycles
// the haplotypes: a last-read check and a small direct-mapped haplotype cache skip most hash lookups.
static void pack_chunk(const gb_testcase *tcs, PackChunk &C, bool cert_wanted, const PackTables &tables,
                       TcDesc *desc, uint32_t *hid) {
  std::unordered_map<ReadKey, uint32_t, KeyHash> read_at;
  std::unordered_map<HapKey, uint32_t, KeyHash> hap_at;
  ReadKey last_rk{nullptr, nullptr, nullptr, nullptr, nullptr, -1};
  uint32_t last_roff = 0;
  struct HapSlot {
    const char *h = nullptr;
    int len = -1;
    uint32_t id = 0;
  };
  HapSlot hcache[256];
  std::vector<uint8_t> &pool = *C.pool;
  for (int k = C.lo; k < C.hi; k++) {
    const gb_testcase &t = tcs[k];
    const ReadKey rk{t.rs, t.q, t.i, t.d, t.c, t.rslen};
    uint32_t roff;
    if (rk == last_rk) {
      roff = last_roff;
    } else {
      auto ri = read_at.find(rk);
      if (ri != read_at.end()) {
        roff = ri->second;
      } else {
        roff = (uint32_t)pool.size();
        pool.resize(pool.size() + 5 * (size_t)t.rslen + sizeof(float));  // and the certificate's log(rho)
        uint8_t *rec = pool.data() + roff;
        for (int r = 0; r < t.rslen; r++) {
          rec[r] = read_match_mask(base_code(t.rs[r]));
          rec[t.rslen + r] = (uint8_t)t.q[r];
          rec[2 * t.rslen + r] = (uint8_t)t.i[r];
          rec[3 * t.rslen + r] = (uint8_t)t.d[r];
          rec[4 * t.rslen + r] = (uint8_t)t.c[r];
        }
        // the early exit's gate: bit 7 of every row's match mask (select_dist reads bits 0..6)
        if (exit_growth(tables.hf, rec, t.rslen) <= kExitGrowthMax)
          for (int r = 0; r < t.rslen; r++) rec[r] |= kMayExit;
        // the predictor's certificate: bit 7 of the first quality byte (the kernels read bits 0..6)
        if (t.rslen > 0) rec[t.rslen] &= 127;
        // (a call that will not be predicted, see batch_fill's may_predict, certifies nothing)
        const double lr = cert_wanted ? cert_log_rho(tables.cert, rec + t.rslen, rec + 2 * t.rslen, rec + 3 * t.rslen,
                                                     rec + 4 * t.rslen, t.rslen)
                                      : std::numeric_limits<double>::infinity();
        float lrf = 0.f;
        if (t.rslen > 0 && cert_K(lr, t.rslen, kMaxHaplen) <= kCertMax) {
          rec[t.rslen] |= kMayPredict;
          lrf = (float)lr;
          if ((double)lrf < lr) lrf = std::nextafterf(lrf, 1.f);
        }
        std::memcpy(rec + 5 * (size_t)t.rslen, &lrf, sizeof(float));
        read_at.emplace(rk, roff);
      }
    }
    last_rk = rk;
    last_roff = roff;
    const HapKey hk{t.hap, t.haplen};
    HapSlot &hs = hcache[(((uintptr_t)t.hap) >> 4) & 255];
    uint32_t id;
    if (hs.h == t.hap && hs.len == t.haplen) {
      id = hs.id;
    } else {
      auto hi = hap_at.find(hk);
      if (hi != hap_at.end()) {
        id = hi->second;
      } else {
        id = (uint32_t)C.hap_off.size();
        const uint32_t hoff = (uint32_t)pool.size();
        pool.resize(pool.size() + (size_t)t.haplen);
        for (int c = 0; c < t.haplen; c++) pool[hoff + c] = base_code(t.hap[c]);
        hap_at.emplace(hk, id);
        C.hap_off.push_back(hoff);
        C.hap_key.push_back(hk);
      }
      hs.h = t.hap;
      hs.len = t.haplen;
      hs.id = id;
    }
    hid[k] = id;  // local until the merge
    // read offset chunk-relative and the local haplotype id until the merge
    desc[k] = TcDesc{roff, 0, (uint32_t)t.rslen | ((uint32_t)t.haplen << 16), (uint32_t)k};
    C.cells += (int64_t)t.rslen * t.haplen;
  }
}

// Pack: deduplicate reads and haplotypes by pointer (the driver shares them across the R x H cross
// product, PairHMMUnitTest.cpp:564-579), convert bases to codes once. Big jobs pack in contiguous chunks
// on several threads, each with its own pool and maps (a read shared across a chunk edge is stored once
// per chunk).
int pack_testcases(const gb_testcase *tcs, int n, int nth, bool cert_wanted, const PackTables &tables,
                   std::vector<std::vector<uint8_t>> &pools, TcDesc *desc, uint32_t *hid,
                   std::vector<PackChunk> *chunks) {
  std::vector<PackChunk> &ch = *chunks;
  ch.assign(nth, PackChunk{});
  for (int t = 0; t < nth; t++) {
    ch[t].lo = (int)((int64_t)n * t / nth);
    ch[t].hi = (int)((int64_t)n * (t + 1) / nth);
    ch[t].pool = &pools[t];
    ch[t].pool->clear();
  }
  return gb::parallel("gb_phmm_batch_create", nth,
                      [&](int t) { pack_chunk(tcs, ch[t], cert_wanted, tables, desc, hid); });
}

int merged_pool_bytes(const std::vector<PackChunk> &chunks, size_t *pool_bytes) {
  size_t sum = 0;
  for (const PackChunk &C : chunks) sum += C.pool->size();
  GB_ARG(sum < (1ull << 32), "batch pool exceeds 4 GiB");
  *pool_bytes = std::max<size_t>(gb::round_up<size_t>(sum, 16), 16);
  return GB_OK;
}

// Merge: chunk pool bases, global haplotype ids in first-appearance order, which is the id order a
// single pass gives, one pool.
int merge_pools(const std::vector<PackChunk> &ch, TcDesc *desc, uint32_t *hid, uint8_t *h_pool, size_t pool_bytes,
                std::vector<uint32_t> *hap_off_of_, int64_t *cells) {
  const int nth = (int)ch.size();
  std::vector<uint32_t> &hap_off_of = *hap_off_of_;
  hap_off_of.clear();
  std::vector<size_t> base(nth + 1, 0);
  for (int t = 0; t < nth; t++) base[t + 1] = base[t] + ch[t].pool->size();
  std::vector<std::vector<uint32_t>> gid(nth);
  {
    std::unordered_map<HapKey, uint32_t, KeyHash> hap_at;
    for (int t = 0; t < nth; t++) {
      gid[t].resize(ch[t].hap_off.size());
      for (size_t h = 0; h < ch[t].hap_off.size(); h++) {
        auto it = hap_at.find(ch[t].hap_key[h]);
        if (it == hap_at.end()) {
          it = hap_at.emplace(ch[t].hap_key[h], (uint32_t)hap_off_of.size()).first;
          hap_off_of.push_back((uint32_t)(base[t] + ch[t].hap_off[h]));
        }
        gid[t][h] = it->second;
      }
    }
  }
  *cells = 0;
  for (int t = 0; t < nth; t++) *cells += ch[t].cells;
  auto merge_chunk = [&](int t) {
    if (!ch[t].pool->empty()) std::memcpy(h_pool + base[t], ch[t].pool->data(), ch[t].pool->size());
    for (int k = ch[t].lo; k < ch[t].hi; k++) {
      hid[k] = gid[t][hid[k]];
      desc[k].read_off += (uint32_t)base[t];
      desc[k].hap_off = hap_off_of[hid[k]];
    }
  };
  if (int st = gb::parallel("gb_phmm_batch_create", nth, merge_chunk)) return st;
  std::memset(h_pool + base[nth], 0, pool_bytes - base[nth]);
  return GB_OK;
}

// Plan. Stacks (phmm_stack): testcases grouped by haplotype, stacked up to stack_rows rows (R + 2 per
// testcase) and 64 testcases; longest-processing-time first (the dispatcher hands out workgroups in grid
// order).
Plan plan_stacks(const TcDesc *desc, int n, const uint32_t *hid, int n_haps, const Knobs &knobs, int cus,
                 uint32_t *order, Stack *stacks, uint64_t *key, Stack *h_stacks, HostClock &clk) {
  auto rows_of = [&](uint32_t at) { return (int)(desc[order[at]].dims & 0xffff) + 2; };  // of order[at], stacked
  auto stack_rows_of = [&](const Stack &S) {
    int rows = 0;
    for (uint32_t t = 0; t < S.count; t++) rows += rows_of(S.first + t);
    return rows;
  };
  {  // counting sort by haplotype (stable: testcases keep their order within a haplotype)
    std::vector<int> first((size_t)n_haps + 1, 0);
    for (int k = 0; k < n; k++) first[hid[k] + 1]++;
    for (int h = 0; h < n_haps; h++) first[h + 1] += first[h];
    for (int k = 0; k < n; k++) order[first[hid[k]]++] = (uint32_t)k;
  }
  clk.mark("haplotype order");
  // Stack height adapts to the job: tall stacks waste the least on partial stripes, but a job of
  // few stacks per resident wave leaves the grid's tail -- one whole stack -- exposed, and the f64
  // pass's persistent grid balances finer pieces better. 2048 rows from 4 stacks per resident wave
  // (32 per CU) up, 512 below 16 stacks per CU, 1024 between. Measured (tools/phmm_shard_probe.py,
  // profiles/r05w_phmm_rows.log, r05x): the 'large' job 2048 / 1024 / 512 rows 32.3 / 32.6 / 33.6 ms,
  // its 1/2, 1/4 and 1/8 shards best at 1024 (1/4: 8.57 ms against 8.76-8.80 at 512 / 2048; 1/8:
  // 4.48 against 4.53 / 4.74), the 'small' job 1024 (4.27 against 4.41 at 512) and its 1/8 shard,
  // 2.75 M rows, 512 (0.83 ms against 0.90 at 1024).
  int64_t total_rows = 0;
  for (int k = 0; k < n; k++) total_rows += (int64_t)(desc[k].dims & 0xffff) + 2;
  int stack_rows = kStackRows;
  if (total_rows / stack_rows < 4ll * 32 * cus) stack_rows = 1024;
  if (stack_rows == 1024 && total_rows / stack_rows < 16ll * cus) stack_rows = 512;
  // a small call (one of the reference's per-batch calls) is its longest stack: below 2 stacks per
  // SIMD the stacks shrink further, to 128 rows
  while (stack_rows > 128 && total_rows / stack_rows < 8ll * cus) stack_rows /= 2;
  if (knobs.stack_rows_forced) stack_rows = knobs.stack_rows_forced;
  // sort keys: long-haplotype stacks last (they run on the kLong kernels), then decreasing cost,
  // then stack index (so the order is the stable one)
  uint64_t *key2 = key + n;
  Plan P;
  for (int k = 0; k < n;) {
    const uint32_t h = desc[order[k]].hap_off;
    const int C = (int)(desc[order[k]].dims >> 16);
    Stack S{(uint32_t)k, 0, h, (uint32_t)C};
    int rows = 0;
    while (k < n && desc[order[k]].hap_off == h && S.count < (uint32_t)kWave &&
           (S.count == 0 || rows + rows_of(k) <= stack_rows)) {
      rows += rows_of(k);
      S.count++;
      k++;
    }
    const bool is_long = C > kLdsHaplen;
    if (is_long) {
      P.n_long++;
      P.max_h_long = std::max(P.max_h_long, C);
    } else {
      P.max_h_short = std::max(P.max_h_short, C);
    }
    const uint64_t cost = std::min<uint64_t>(stack_steps(rows, C, kWave, false), 0x7fffffffu);
    key[P.ns_all] = ((uint64_t)is_long << 63) | ((0x7fffffffu - cost) << 32) | (uint32_t)P.ns_all;
    stacks[P.ns_all++] = S;
  }
  clk.mark("stack build");
  // LSD radix sort of the keys' upper 32 bits, 8 bits a pass (the low 32 bits are the index)
  auto sort_keys = [&](int ns) {
    uint32_t cnt[256];
    for (int shift = 32; shift < 64; shift += 8) {
      const uint64_t d0 = ns ? (key[0] >> shift) & 255 : 0;
      bool same = true;
      for (int k = 1; k < ns && same; k++) same = ((key[k] >> shift) & 255) == d0;
      if (same) continue;
      std::memset(cnt, 0, sizeof(cnt));
      for (int k = 0; k < ns; k++) cnt[(key[k] >> shift) & 255]++;
      for (uint32_t d = 0, sum = 0; d < 256; d++) {
        const uint32_t c = cnt[d];
        cnt[d] = sum;
        sum += c;
      }
      for (int k = 0; k < ns; k++) key2[cnt[(key[k] >> shift) & 255]++] = key[k];
      std::swap(key, key2);
    }
  };
  sort_keys(P.ns_all);
  for (int k = 0; k < P.ns_all; k++) h_stacks[k] = stacks[(uint32_t)key[k]];
  // Tail split: the stacks holding the last 10 % of the LPT order's cost are cut into stacks of at
  // most 512 rows (taller stacks waste less on the anti-diagonal fill; shorter ones let the grid's
  // last waves end together). Measured (tools/phmm_shard_probe.py, profiles/r06h/r06i): the 'large'
  // job 31.93-32.00 -> 31.65 ms, its 1/8 shard 4.47-4.49 -> 4.41-4.46 ms; 5 / 15 / 20 / 30 % and
  // 128 / 256 / 384-row pieces no better on the job.
  const double frac = knobs.tail_frac >= 0 ? knobs.tail_frac : (stack_rows > 512 ? 0.10 : 0.0);
  const int trows = knobs.tail_rows;
  if (frac > 0) {
    const int ns_short = P.ns_all - P.n_long;
    auto cost_of = [&](const Stack &S) -> uint64_t { return stack_steps(stack_rows_of(S), (int)S.C, kWave, false); };
    uint64_t total = 0;
    for (int k = 0; k < ns_short; k++) total += cost_of(h_stacks[k]);
    uint64_t acc = 0;
    int t0 = ns_short;
    while (t0 > 0 && (double)acc < frac * (double)total) acc += cost_of(h_stacks[--t0]);
    std::vector<std::pair<uint64_t, Stack>> pieces;
    for (int k = t0; k < ns_short; k++) {
      const Stack S = h_stacks[k];
      uint32_t t = 0;
      while (t < S.count) {
        Stack Q{S.first + t, 0, S.hap_off, S.C};
        int rows = 0;
        while (t < S.count && (Q.count == 0 || rows + rows_of(S.first + t) <= trows)) {
          rows += rows_of(S.first + t);
          Q.count++;
          t++;
        }
        pieces.push_back({stack_steps(rows, (int)S.C, kWave, false), Q});
      }
    }
    std::stable_sort(pieces.begin(), pieces.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
    std::vector<Stack> longs(h_stacks + ns_short, h_stacks + P.ns_all);
    int k = t0;
    for (const auto &pc : pieces) h_stacks[k++] = pc.second;
    for (const auto &ls : longs) h_stacks[k++] = ls;
    P.ns_all = k;
  }
  // Which testcases share a stack is decided above by the fill-per-stripe cost, whatever the sweep (a
  // dropped testcase's raw f32 depends on where the early exit's stripes fall in its stack). The launch
  // order of the LDS stacks is by the cost of the sweep they take: the rolled one's wave steps.
  if (knobs.roll) {
    const int ns_short = P.ns_all - P.n_long;
    for (int k = 0; k < ns_short; k++) {
      const Stack &S = h_stacks[k];
      const uint64_t cost = std::min<uint64_t>(stack_steps(stack_rows_of(S), (int)S.C, kWave, true), 0x7fffffffu);
      key[k] = ((0x7fffffffu - cost) << 32) | (uint32_t)k;
      stacks[k] = S;
    }
    sort_keys(ns_short);
    for (int k = 0; k < ns_short; k++) h_stacks[k] = stacks[(uint32_t)key[k]];
  }
  clk.mark("stacks");
  return P;
}

}  // namespace phmm
}  // namespace gb

namespace {

// Fill: pack the testcases (deduplicated reads/haplotypes, stacks in LPT order) into b's pinned staging
// buffer and upload them, growing its buffers when they are too small; b's stream/events exist
// already. threads: host threads of the pack and merge phases (0: up to 8 from pack_min testcases).
// validated: the caller has run validate_testcases over the whole call (compute_pipelined, whose
// chunks would otherwise name a testcase by its index in the chunk). Inputs are validated first
// (sequentially, so the error names the first bad testcase). Descriptors, stack lists, stacks and pool
// are written straight into the pinned staging buffer.
int batch_fill(gb_phmm_batch *b, const gb_testcase *tcs, int n, int threads = 0, bool validated = false) {
  HostClock clk;
  if (!validated)
    if (int st = validate_testcases(tcs, n)) return st;
  clk.mark("validate");
  const Knobs K = b->knobs = read_knobs();
  int nth = n >= K.pack_min ? (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency())) : 1;
  if (threads > 0) nth = std::max(1, std::min(threads, n / 4096));
  nth = std::max(1, std::min(nth, n / 2048));
  const size_t nn = std::max(n, 1);
  host_reserve(b, nn, 0, nth);
  // descriptors are written by the pack (a bigger pool than guessed grows the buffer after it)
  if (int st = stage_reserve(b, StageLayout(nn, 32 * nn).total)) return st;
  uint32_t *hid = b->hid.data();  // dense haplotype index of each testcase (stack grouping)
  // one-shot calls below kPredMinCells do without the predictor (phmm_predict, "Gate")
  int64_t pre_cells = 0;
  for (int k = 0; k < n; k++) pre_cells += (int64_t)tcs[k].rslen * tcs[k].haplen;
  const bool cert_wanted = b->resident || pre_cells >= kPredMinCells;
  std::vector<PackChunk> ch;
  if (int st = pack_testcases(tcs, n, nth, cert_wanted, *g_host, b->pools, (TcDesc *)b->h_stage.get(), hid, &ch))
    return st;
  clk.mark("pack");
  size_t pool_bytes = 0;
  if (int st = merged_pool_bytes(ch, &pool_bytes)) return st;
  const StageLayout L(nn, pool_bytes);
  if (int st = stage_reserve(b, L.total, sizeof(TcDesc) * nn)) return st;
  TcDesc *desc = (TcDesc *)b->h_stage.get();
  uint32_t *order = (uint32_t *)(b->h_stage + L.o_tc);  // the stacks' testcase lists
  Stack *h_stacks = (Stack *)(b->h_stage + L.o_stk);
  uint8_t *h_pool = b->h_stage + L.o_pool;
  std::vector<uint32_t> hap_off_of;
  int64_t cells = 0;
  if (int st = merge_pools(ch, desc, hid, h_pool, pool_bytes, &hap_off_of, &cells)) return st;
  clk.mark("merge");
  const Plan P = plan_stacks(desc, n, hid, (int)hap_off_of.size(), K, b->cus, order, b->stacks.data(),
                             b->skeys.data(), h_stacks, clk);
  const int ns_short = P.ns_all - P.n_long;
  if (int st = batch_reserve(b, n, pool_bytes)) return st;
  if (P.n_long) {
    // records + codes of one long stack per workgroup of the persistent kLong grid
    b->long_grid = std::min(P.n_long, b->f64_grid);
    b->scratch_stride = gb::round_up<size_t>(sizeof(Brec<double>) * (size_t)(P.max_h_long + kBndPad + kRecPad) +
                                                 (size_t)(P.max_h_long + kBndPad + kWave) + 16, 256);
    const size_t need = b->scratch_stride * (size_t)b->long_grid;
    if (int st = b->d_scratch.reserve(need)) return st;
  }
  // the uploads go through the pinned staging buffer: a pageable copy is staged by the runtime, and
  // while an earlier chunk's kernels held the GPU one chunk's upload waited 10-15 ms for it
  // (profiles/r05j_phmm_cli.log); a pinned copy is a plain DMA
  if (n) {
    GB_HIP(hipMemcpyAsync(b->d_desc, desc, sizeof(TcDesc) * n, hipMemcpyHostToDevice, b->stream));
    GB_HIP(hipMemcpyAsync(b->d_stk_tc, order, sizeof(uint32_t) * n, hipMemcpyHostToDevice, b->stream));
    GB_HIP(hipMemcpyAsync(b->d_stacks, h_stacks, sizeof(Stack) * P.ns_all, hipMemcpyHostToDevice, b->stream));
  }
  GB_HIP(hipMemcpyAsync(b->d_pool, h_pool, pool_bytes, hipMemcpyHostToDevice, b->stream));
  // the predictor's gate (phmm_predict): sampled here, behind the uploads, and read at the fill's own
  // synchronisation; one-shot calls below kPredMinCells do without the predictor
  const bool may_predict = K.predict && K.f32_exit && ns_short > 0 && cert_wanted;
  int gate[2] = {0, 0};
  b->gate_open = may_predict && K.predict >= 2;
  if (may_predict && K.predict == 1) {
    GB_HIP(hipMemsetAsync(b->d_count, 0, kCountWords * sizeof(int), b->stream));
    const int sg = std::min(ns_short, b->cus * 16);
    hipLaunchKernelGGL(phmm_predict, dim3(sg), dim3(kWave), 0, b->stream, (const Stack *)b->d_stacks, ns_short,
                       (const uint32_t *)b->d_stk_tc, (const TcDesc *)b->d_desc, (const uint8_t *)b->d_pool.get(),
                       b->d_rf, b->d_pred, b->d_count.get(), (int)kPredSample);
    GB_HIP(hipGetLastError());
    GB_HIP(hipMemcpyAsync(gate, b->d_count + kPredSampled, sizeof(gate), hipMemcpyDeviceToHost, b->stream));
  }
  GB_HIP(hipStreamSynchronize(b->stream));  // the staging buffer is reused by the next fill
  b->gate_n = gate[0];
  b->gate_pred = gate[1];
  if (may_predict && K.predict == 1) b->gate_open = (int64_t)gate[1] * kGateDen >= (int64_t)gate[0] && gate[1] > 0;
  clk.mark("upload");
  b->n = n;
  b->nstacks = ns_short;
  b->n_long = P.n_long;
  b->max_haplen = P.max_h_short;
  b->cells = cells;
  b->ran = false;
  return GB_OK;
}

int batch_new(DeviceTables *tabs, gb_phmm_batch **out) {
  auto *b = new gb_phmm_batch();
  b->tabs = tabs;
  int cus = 256;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, tabs->device) != hipSuccess) cus = 256;
  b->f64_grid = cus * 16;
  if (const char *e = getenv("GB_PHMM_F64_GRID")) b->f64_grid = cus * std::max(1, std::min(32, atoi(e)));  // probe
  b->cus = cus;
  hipError_t e = b->stream.create();
  for (auto &ev : b->ev)
    if (e == hipSuccess) e = ev.create();
  if (e != hipSuccess) {
    gb::set_error("gb_phmm_batch_create: %s", hipGetErrorString(e));
    gb_phmm_batch_destroy(b);
    return GB_ERR_HIP;
  }
  *out = b;
  return GB_OK;
}

// gb_phmm_compute's workspaces: the calling thread's batch for (device, slot), refilled on every call
// so the reference's once-per-batch computelikelihoodsboth does not create streams, events and
// buffers each time.
gb_phmm_batch *thread_workspace(DeviceTables *tabs, int *st, int slot = 0) {
  gb_phmm_batch *b = nullptr;
  *st = gb::thread_ws(tabs->device, slot, &b, [tabs](int, gb_phmm_batch **out) { return batch_new(tabs, out); });
  return b;
}

constexpr int kPipeMinChunk = 65536;  // testcases per chunk from three chunks on
constexpr int kPipeMin2 = 16384;      // the smallest call pipelined (two chunks)
constexpr int kPipeMaxChunks = 4;

// gb_phmm_init (the reference's initPairHMM, called before its timed loop) also readies what the
// first computation would otherwise pay for inside it: the code objects of the kernels (loaded at
// their first launch: empty launches here) and this thread's pipeline workspaces (streams, events).
int warm_up(DeviceTables *t) {
  int st = GB_OK;
  gb_phmm_batch *b = thread_workspace(t, &st, 0);
  if (!b) return st;
  if ((st = batch_reserve(b, 1, 16))) return st;
  // one launch of a no-op kernel of this module loads the module's code object (every phmm kernel);
  // a no-op of its own keeps the profiles' per-kernel statistics free of empty dispatches
  hipLaunchKernelGGL(phmm_warm, dim3(1), dim3(kWave), 0, b->stream, b->d_count);
  GB_HIP(hipGetLastError());
  GB_HIP(hipStreamSynchronize(b->stream));
  // the runtime creates a stream's hardware queue at its first command (~10-15 ms, measured inside
  // bin/phmm's timed region as a chunk upload): give each workspace stream one here
  for (int c = 1; c < kPipeMaxChunks; c++) {
    gb_phmm_batch *w = thread_workspace(t, &st, c);
    if (!w) return st;
    if ((st = batch_reserve(w, 1, 16))) return st;
    GB_HIP(hipMemsetAsync(w->d_count, 0, 8 * sizeof(int), w->stream));
    GB_HIP(hipEventRecord(w->ev[0], w->stream));
  }
  for (int c = 1; c < kPipeMaxChunks; c++) GB_HIP(hipStreamSynchronize(thread_workspace(t, &st, c)->stream));
  // buffers for a job of GB_PHMM_PREALLOC testcases (default 1 M; 0: none) in the pipeline's chunk
  // proportions: allocating them inside the first call cost bin/phmm ~14 ms of its timed region
  // (device ~90 B, pinned ~70 B and host scratch ~70 B per testcase; all grow on demand past it)
  int64_t pre = 1 << 20;
  if (const char *e = getenv("GB_PHMM_PREALLOC")) pre = std::max(0ll, atoll(e));
  if (pre > 0) {
    const int64_t W = (int64_t)kPipeMaxChunks * (kPipeMaxChunks + 1) / 2;
    for (int c = 0; c < kPipeMaxChunks; c++) {
      gb_phmm_batch *w = thread_workspace(t, &st, c);
      const int64_t m = pre * (c + 1) / W + 1;
      const size_t pool = 32 * (size_t)m;
      if ((st = batch_reserve(w, (int)std::min<int64_t>(m, 1 << 30), pool))) return st;
      if ((st = stage_reserve(w, StageLayout((size_t)m, pool).total))) return st;
      host_reserve(w, (size_t)m, pool, 4);
    }
  }
  return GB_OK;
}

// Pipelined one-call path for big calls: the testcases are cut into contiguous chunks of growing size
// (weights 1, 2, .., k), each packed into its own workspace batch (own stream). The first, small
// chunk is packed on the calling thread and launched at once; the others are packed meanwhile on
// worker threads and launched in order as they become ready, so the host's packing hides behind the
// kernels, and chunk c's results (D2H + log10) overlap the kernels of the chunks after it. Chunks are
// independent jobs, so results are those of one job.
int compute_pipelined(DeviceTables *tabs, const gb_testcase *tcs, int n, double *results, float *raw_f,
                      double *raw_d, uint8_t *used_double) {
  const char *e = getenv("GB_PHMM_PIPE");  // probes: the chunk count (1 = one job, no overlap)
  // two chunks from kPipeMin2 testcases (the reference's bigger per-batch calls), up to four
  int k = std::min(kPipeMaxChunks, std::max(2, n / kPipeMinChunk));
  if (e) k = std::max(1, std::min(16, atoi(e)));
  std::vector<gb_phmm_batch *> B(k);
  std::vector<int> lo(k + 1);
  const int64_t W = (int64_t)k * (k + 1) / 2;
  for (int c = 0; c <= k; c++) lo[c] = (int)((int64_t)n * ((int64_t)c * (c + 1) / 2) / W);
  int st = GB_OK;
  for (int c = 0; c < k; c++) {
    B[c] = thread_workspace(tabs, &st, c);
    if (!B[c]) return st;
    B[c]->force_f64 = false;
  }
  HostClock clk;
  // the whole call is validated here, before any chunk is packed or launched: a bad testcase fails the
  // call with its index in the caller's array and nothing on the device
  if ((st = validate_testcases(tcs, n))) return st;
  // host threads: about 12 over the concurrent fills (GB_PHMM_FILL_THREADS: per fill)
  int fill_threads = std::max(1, 12 / k);
  if (const char *f = getenv("GB_PHMM_FILL_THREADS")) fill_threads = std::max(1, atoi(f));
  const int device = tabs->device;
  auto fill = [&, device](int c) -> std::pair<int, std::string> {
    if (hipSetDevice(device) != hipSuccess) return {GB_ERR_HIP, "gb_phmm_compute: hipSetDevice failed"};
    const int s = batch_fill(B[c], tcs + lo[c], lo[c + 1] - lo[c], fill_threads, true);
    return {s, s ? std::string(gb::last_error()) : std::string()};
  };
  // the workers' futures join on destruction, also on an early return
  std::vector<std::future<std::pair<int, std::string>>> ready;
  for (int c = 1; c < k; c++) ready.push_back(std::async(std::launch::async, fill, c));
  auto fetch = [&](int c) {
    const int o = lo[c];
    return gb_phmm_batch_results(B[c], results ? results + o : nullptr, raw_f ? raw_f + o : nullptr,
                                 raw_d ? raw_d + o : nullptr, used_double ? used_double + o : nullptr, nullptr);
  };
  // on an error, the chunks already launched are waited for before the call returns, so no kernel
  // of this call is left in flight (results are undefined on a nonzero status) and the next call
  // refills those workspaces behind nothing
  int launched = 0;
  auto fail = [&](int s) {
    const std::string msg = gb::last_error();
    for (int c = 0; c < launched; c++) (void)hipStreamSynchronize(B[c]->stream);
    for (size_t c = 0; c < ready.size(); c++)
      if (ready[c].valid()) ready[c].wait();
    gb::set_error("%s", msg.c_str());
    return s;
  };
  if ((st = batch_fill(B[0], tcs, lo[1], fill_threads, true))) return fail(st);
  clk.mark("chunk 0 filled");
  if ((st = gb_phmm_batch_run(B[0]))) return fail(st);
  launched = 1;
  // chunk c - 2's results are fetched after chunk c is launched: the host never waits on the chunk
  // the GPU has just started, only on one queued behind it
  int fetched = 0;
  for (int c = 1; c < k; c++) {
    const auto r = ready[c - 1].get();
    if (r.first) {
      gb::set_error("%s", r.second.c_str());
      return fail(r.first);
    }
    clk.mark("chunk ready");
    if ((st = gb_phmm_batch_run(B[c]))) return fail(st);
    launched = c + 1;
    if (c >= 2) {
      if ((st = fetch(fetched++))) return fail(st);
      clk.mark("chunk fetched");
    }
  }
  while (fetched < k)
    if ((st = fetch(fetched++))) return fail(st);
  clk.mark("last chunks fetched");
  return st;
}

}  // namespace

extern "C" {

int gb_phmm_batch_create(const gb_testcase *tcs, int n, gb_phmm_batch **out) {
  GB_ARG(out, "gb_phmm_batch_create: null out");
  GB_ARG(n >= 0 && (n == 0 || tcs), "gb_phmm_batch_create: bad testcase array (n=%d)", n);
  *out = nullptr;
  DeviceTables *tabs = nullptr;
  int st = get_device_tables(&tabs);
  if (st) return st;
  gb_phmm_batch *b = nullptr;
  if ((st = batch_new(tabs, &b))) return st;
  b->resident = true;
  if ((st = batch_fill(b, tcs, n))) {
    gb_phmm_batch_destroy(b);
    return st;
  }
  *out = b;
  return GB_OK;
}

int gb_phmm_batch_run(gb_phmm_batch *b) {
  gb::Range range_("gb.phmm.batch_run");
  GB_ARG(b, "gb_phmm_batch_run: null batch");
  DeviceTables *t = b->tabs;
  GB_HIP(hipSetDevice(t->device));
  const int n = b->n;
  GB_HIP(hipEventRecord(b->ev[0], b->stream));
  GB_HIP(hipMemsetAsync(b->d_count, 0, kCountWords * sizeof(int), b->stream));
  // (a run with the predictor zeroes d_rd together with d_pred and d_redo behind it)
  const bool predict = n > 0 && b->gate_open && b->knobs.f32_exit && !b->force_f64 && b->nstacks > 0;
  GB_HIP(hipMemsetAsync(b->d_rd, 0, predict ? b->pred_bytes : sizeof(double) * std::max(n, 1), b->stream));
  if (n > 0) {
    const size_t rec = (size_t)(b->max_haplen + kBndPad + kRecPad), codes = (size_t)(b->max_haplen + kBndPad + kWave);
    const size_t lds_f = sizeof(Brec<float>) * rec + codes + 16;
    const size_t lds_d = sizeof(Brec<double>) * rec + codes + 16;
    auto f32k = phmm_forward<float, false>;
    auto f64k = phmm_forward<double, true>;
    const int ns = b->nstacks, nl = b->n_long;
    const Stack *d_long = b->d_stacks + ns;
    if (b->knobs.f32_exit) f32k = phmm_forward<float, false, false, true>;
    // the fallback predictor, on the exit's switch too (GB_PHMM_EXIT=0 keeps every raw f32), when the
    // fill's sample opened the gate; the f32 pass then leaves the predicted testcases out
    const uint8_t *skip = predict ? b->d_pred : nullptr;
    // its f64 pass confirms the predictions, or computes the f32 result after all (verify_unit)
    if (predict) {
      const int pg = std::min(ns, b->cus * 16);
      hipLaunchKernelGGL(phmm_predict, dim3(pg), dim3(kWave), 0, b->stream, b->d_stacks, ns, b->d_stk_tc, b->d_desc,
                         b->d_pool, b->d_rf, b->d_pred, b->d_count, b->knobs.predict == 2 ? (int)kPredAll : (int)kPredOpen);
      GB_HIP(hipGetLastError());
    }
    if (!b->force_f64) {
      if (ns > 0)
        hipLaunchKernelGGL(f32k, dim3(ns), dim3(kWave), lds_f, b->stream, b->d_stacks, ns, b->d_stk_tc, b->d_desc,
                           b->d_pool, dev_tab<float>(t->f, t->hf.init_const), b->d_rf, (const float *)nullptr,
                           b->d_count, b->knobs.roll ? 1 << 16 : 0, (uint8_t *)nullptr, (size_t)0, (const uint32_t *)nullptr,
                           skip, 0, (const float *)nullptr, (uint8_t *)nullptr);
      if (nl > 0)
        hipLaunchKernelGGL((phmm_forward<float, false, true>), dim3(b->long_grid), dim3(kWave), 0, b->stream, d_long,
                           nl, b->d_stk_tc, b->d_desc, b->d_pool, dev_tab<float>(t->f, t->hf.init_const), b->d_rf,
                           (const float *)nullptr, b->d_count, 0, b->d_scratch, b->scratch_stride,
                           (const uint32_t *)nullptr, (const uint8_t *)nullptr, 0, (const float *)nullptr, (uint8_t *)nullptr);
      GB_HIP(hipGetLastError());
    }
    GB_HIP(hipEventRecord(b->ev[1], b->stream));
    // f64 fallback: persistent grid over the stacks, each recomputing its flagged testcases
    if (ns > 0) {
      const int nunits = ns * b->knobs.f64_parts;
      const int g64 = std::min(nunits, b->f64_grid);
      if (b->knobs.f64_plan) {
        const dim3 pg((unsigned)((nunits + 255) / 256)), pb(256);
        hipLaunchKernelGGL(f64_plan, pg, pb, 0, b->stream, b->d_stacks, nunits, b->knobs.f64_parts, b->d_stk_tc, b->d_desc,
                           (const float *)b->d_rf, b->force_f64 ? 1 : 0, b->knobs.roll ? 1 : 0, b->d_ukey, b->d_count);
        hipLaunchKernelGGL(f64_plan_order, pg, pb, 0, b->stream, nunits, (const uint8_t *)b->d_ukey, b->d_count,
                           b->d_units);
      }
      hipLaunchKernelGGL(f64k, dim3(g64), dim3(kWave), lds_d, b->stream, b->d_stacks, ns, b->d_stk_tc, b->d_desc,
                         b->d_pool, dev_tab<double>(t->d, t->hd.init_const), b->d_rd, (const float *)b->d_rf,
                         b->d_count, (b->force_f64 ? 1 : 0) | (b->knobs.f64_parts << 8) | (b->knobs.roll ? 1 << 16 : 0),
                         (uint8_t *)nullptr, (size_t)0,
                         b->knobs.f64_plan ? (const uint32_t *)b->d_units : nullptr, skip, 0,
                         (const float *)t->f, predict ? b->d_redo : nullptr);
    }
    if (nl > 0)
      hipLaunchKernelGGL((phmm_forward<double, true, true>), dim3(b->long_grid), dim3(kWave), 0, b->stream, d_long,
                         nl, b->d_stk_tc, b->d_desc, b->d_pool, dev_tab<double>(t->d, t->hd.init_const), b->d_rd,
                         (const float *)b->d_rf, b->d_count, b->force_f64 ? 1 : 0, b->d_scratch, b->scratch_stride,
                         (const uint32_t *)nullptr, (const uint8_t *)nullptr, 0, (const float *)nullptr, (uint8_t *)nullptr);
    GB_HIP(hipGetLastError());
    GB_HIP(hipEventRecord(b->ev[2], b->stream));
    hipLaunchKernelGGL(phmm_finalize, dim3((n + 255) / 256), dim3(256), 0, b->stream, b->d_rf, b->d_rd,
                       predict ? (const uint8_t *)b->d_redo : nullptr, b->d_out, n, t->hf.log10_init,
                       t->hd.log10_init, b->d_count);
    GB_HIP(hipGetLastError());
  } else {
    GB_HIP(hipEventRecord(b->ev[1], b->stream));
    GB_HIP(hipEventRecord(b->ev[2], b->stream));
  }
  GB_HIP(hipEventRecord(b->ev[3], b->stream));
  b->ran = true;
  return GB_OK;
}

int gb_phmm_batch_sync(gb_phmm_batch *b) {
  GB_ARG(b, "gb_phmm_batch_sync: null batch");
  GB_HIP(hipStreamSynchronize(b->stream));
  return GB_OK;
}

int gb_phmm_batch_results(gb_phmm_batch *b, double *results, float *raw_f, double *raw_d,
                          uint8_t *used_double, double *dev_results) {
  GB_ARG(b, "gb_phmm_batch_results: null batch");
  if (!b->ran) {
    gb::set_error("gb_phmm_batch_results: batch has not been run");
    return GB_ERR_STATE;
  }
  GB_HIP(hipSetDevice(b->tabs->device));
  GB_HIP(hipStreamSynchronize(b->stream));
  const int n = b->n;
  if (n == 0) return GB_OK;
  // raw likelihoods back through the pinned staging buffer when it is big enough (a pageable copy is
  // staged by the runtime)
  std::vector<float> rf_v;
  std::vector<double> rd_v;
  const float *rf;
  const double *rd;
  const size_t off_d = gb::round_up<size_t>(sizeof(float) * (size_t)n, 256);
  if (b->h_stage && b->h_stage.capacity() >= off_d + sizeof(double) * (size_t)n) {
    GB_HIP(hipMemcpyAsync(b->h_stage, b->d_rf, sizeof(float) * n, hipMemcpyDeviceToHost, b->stream));
    GB_HIP(hipMemcpyAsync(b->h_stage + off_d, b->d_rd, sizeof(double) * n, hipMemcpyDeviceToHost, b->stream));
    GB_HIP(hipStreamSynchronize(b->stream));
    rf = (const float *)b->h_stage.get();
    rd = (const double *)(b->h_stage + off_d);
  } else {
    rf_v.resize(n);
    rd_v.resize(n);
    GB_HIP(hipMemcpy(rf_v.data(), b->d_rf, sizeof(float) * n, hipMemcpyDeviceToHost));
    GB_HIP(hipMemcpy(rd_v.data(), b->d_rd, sizeof(double) * n, hipMemcpyDeviceToHost));
    rf = rf_v.data();
    rd = rd_v.data();
  }
  if (dev_results) GB_HIP(hipMemcpy(dev_results, b->d_out, sizeof(double) * n, hipMemcpyDeviceToHost));
  const float l10f = b->tabs->hf.log10_init;
  const double l10d = b->tabs->hd.log10_init;
  auto part = [&](int lo, int hi) {
    for (int k = lo; k < hi; k++) {
      const bool ud = rf[k] < 1e-28f;
      if (results) results[k] = ud ? (log10(rd[k]) - l10d) : (double)(log10f(rf[k]) - l10f);
      if (raw_f) raw_f[k] = rf[k];
      if (raw_d) raw_d[k] = rd[k];
      if (used_double) used_double[k] = ud ? 1 : 0;
    }
  };
  // the host log10 epilogue (bit-exact, unlike the device one) over a few threads for big jobs
  const int nt = n >= (1 << 16) ? (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency())) : 1;
  return gb::parallel("gb_phmm_batch_results", nt,
                      [&](int t) { part((int)((int64_t)n * t / nt), (int)((int64_t)n * (t + 1) / nt)); });
}

int gb_phmm_batch_timing(gb_phmm_batch *b, float *f32_ms, float *f64_ms, float *total_ms) {
  GB_ARG(b && b->ran, "gb_phmm_batch_timing: batch has not been run");
  GB_HIP(hipEventSynchronize(b->ev[3]));
  float a = 0, c = 0, tot = 0;
  GB_HIP(hipEventElapsedTime(&a, b->ev[0], b->ev[1]));
  GB_HIP(hipEventElapsedTime(&c, b->ev[1], b->ev[2]));
  GB_HIP(hipEventElapsedTime(&tot, b->ev[0], b->ev[3]));
  if (f32_ms) *f32_ms = a;
  if (f64_ms) *f64_ms = c;
  if (total_ms) *total_ms = tot;
  return GB_OK;
}

int gb_phmm_batch_stats(gb_phmm_batch *b, int64_t *testcases, int64_t *cells, int64_t *n_f64) {
  GB_ARG(b, "gb_phmm_batch_stats: null batch");
  if (testcases) *testcases = b->n;
  if (cells) *cells = b->cells;
  if (n_f64) {
    int c = 0;
    if (b->ran) {
      GB_HIP(hipStreamSynchronize(b->stream));
      GB_HIP(hipMemcpy(&c, b->d_count, sizeof(int), hipMemcpyDeviceToHost));
    }
    *n_f64 = c;
  }
  return GB_OK;
}

int gb_phmm_batch_exit_stats(gb_phmm_batch *b, int64_t *dropped, int64_t *cells_skipped) {
  GB_ARG(b, "gb_phmm_batch_exit_stats: null batch");
  unsigned long long c[2] = {0, 0};
  if (b->ran) {
    GB_HIP(hipStreamSynchronize(b->stream));
    GB_HIP(hipMemcpy(c, b->d_count + 4, sizeof(c), hipMemcpyDeviceToHost));
  }
  if (dropped) *dropped = (int64_t)c[0];
  if (cells_skipped) *cells_skipped = (int64_t)c[1];
  return GB_OK;
}

int gb_phmm_batch_predict_stats(gb_phmm_batch *b, int64_t *sampled, int64_t *predicted, int64_t *confirmed,
                                int64_t *redone) {
  GB_ARG(b, "gb_phmm_batch_predict_stats: null batch");
  int c[kCountWords] = {0};
  if (b->ran) {
    GB_HIP(hipStreamSynchronize(b->stream));
    GB_HIP(hipMemcpy(c, b->d_count, sizeof(c), hipMemcpyDeviceToHost));
  }
  if (sampled) *sampled = b->gate_n;
  if (predicted) *predicted = c[kPredPredicted];
  if (confirmed) *confirmed = c[kPredConfirmed];
  if (redone) *redone = c[kPredRedone];
  return GB_OK;
}

int gb_phmm_batch_stacks(gb_phmm_batch *b, int64_t *stacks) {
  GB_ARG(b && stacks, "gb_phmm_batch_stacks: null argument");
  *stacks = (int64_t)b->nstacks + b->n_long;
  return GB_OK;
}

int gb_phmm_batch_predicted(gb_phmm_batch *b, uint8_t *pred) {
  GB_ARG(b && pred, "gb_phmm_batch_predicted: null argument");
  if (!b->ran) {
    gb::set_error("gb_phmm_batch_predicted: batch has not been run");
    return GB_ERR_STATE;
  }
  if (b->n == 0) return GB_OK;
  GB_HIP(hipStreamSynchronize(b->stream));
  int c[kCountWords] = {0};
  GB_HIP(hipMemcpy(c, b->d_count, sizeof(c), hipMemcpyDeviceToHost));
  // a run without the predictor leaves d_pred as it was: nothing predicted
  if (c[kPredPredicted] == 0)
    std::memset(pred, 0, (size_t)b->n);
  else
    GB_HIP(hipMemcpy(pred, b->d_pred, (size_t)b->n, hipMemcpyDeviceToHost));
  return GB_OK;
}

int gb_phmm_certificate(const gb_testcase *tcs, int n, double *K, uint8_t *certified) {
  GB_ARG(n >= 0 && (n == 0 || tcs), "gb_phmm_certificate: bad testcase array (n=%d)", n);
  if (int st = validate_testcases(tcs, n)) return st;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    ensure_host_tables();
  }
  for (int k = 0; k < n; k++) {
    const gb_testcase &t = tcs[k];
    const double lr = cert_log_rho(g_host->cert, (const uint8_t *)t.q, (const uint8_t *)t.i, (const uint8_t *)t.d,
                                   (const uint8_t *)t.c, t.rslen);
    if (K) K[k] = cert_K(lr, t.rslen, t.haplen);
    if (certified) certified[k] = cert_K(lr, t.rslen, kMaxHaplen) <= kCertMax ? 1 : 0;
  }
  return GB_OK;
}

int gb_phmm_batch_destroy(gb_phmm_batch *b) {
  if (!b) return GB_OK;
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  delete b;  // the events, the stream and the buffers go with it
  return GB_OK;
}

int gb_phmm_compute(const gb_testcase *tcs, int n, double *results, float *raw_f, double *raw_d,
                    uint8_t *used_double) {
  gb::Range range_("gb.phmm.compute");
  GB_ARG(n >= 0 && (n == 0 || tcs), "gb_phmm_compute: bad testcase array (n=%d)", n);
  if (n == 0) return GB_OK;
  DeviceTables *tabs = nullptr;
  int st = get_device_tables(&tabs);
  if (st) return st;
  if (n >= kPipeMin2 || getenv("GB_PHMM_PIPE"))
    return compute_pipelined(tabs, tcs, n, results, raw_f, raw_d, used_double);
  gb_phmm_batch *b = thread_workspace(tabs, &st);
  if (!b) return st;
  b->force_f64 = false;
  if ((st = batch_fill(b, tcs, n))) return st;
  HostClock clk;
  st = gb_phmm_batch_run(b);
  if (!st) st = gb_phmm_batch_sync(b);
  clk.mark("kernels");
  if (!st) st = gb_phmm_batch_results(b, results, raw_f, raw_d, used_double, nullptr);
  clk.mark("results");
  return st;
}

int gb_phmm_compute_f64(const gb_testcase *tcs, int n, double *raw_d) {
  GB_ARG(n >= 0 && raw_d && (n == 0 || tcs), "gb_phmm_compute_f64: bad arguments");
  if (n == 0) return GB_OK;
  DeviceTables *tabs = nullptr;
  int st = get_device_tables(&tabs);
  if (st) return st;
  gb_phmm_batch *b = thread_workspace(tabs, &st);
  if (!b) return st;
  if ((st = batch_fill(b, tcs, n))) return st;
  b->force_f64 = true;
  st = gb_phmm_batch_run(b);
  b->force_f64 = false;
  if (!st) st = gb_phmm_batch_results(b, nullptr, nullptr, raw_d, nullptr, nullptr);
  return st;
}

int gb_phmm_compute_f32(const gb_testcase *tcs, int n, float *raw_f) {
  gb::Range range_("gb.phmm.compute_f32");
  GB_ARG(n >= 0 && raw_f && (n == 0 || tcs), "gb_phmm_compute_f32: bad arguments");
  if (n == 0) return GB_OK;
  DeviceTables *tabs = nullptr;
  int st = get_device_tables(&tabs);
  if (st) return st;
  gb_phmm_batch *b = thread_workspace(tabs, &st);
  if (!b) return st;
  b->force_f64 = false;
  if ((st = batch_fill(b, tcs, n))) return st;
  b->knobs.f32_exit = false;  // every testcase's f32 probability in full, also those that fall back
  st = gb_phmm_batch_run(b);
  if (!st) st = gb_phmm_batch_sync(b);
  if (!st) st = gb_phmm_batch_results(b, nullptr, raw_f, nullptr, nullptr, nullptr);
  return st;
}

}  // extern "C"
