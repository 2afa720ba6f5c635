// phmm_internal.h -- the host steps of a PairHMM fill that need no device (pack, merge, plan), the knobs they
// and the launches read, and the layouts they share with the kernels; one copy for csrc/phmm.hip and for
// tests/cpp/phmm_host_check.cpp.
#pragma once
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/gb_phmm.h"

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace gb {
namespace phmm {

constexpr int kWave = 64;
// Longest haplotype a stack keeps in LDS: the f64 kernel's LDS (16-B boundary record + 1 code byte
// per column, plus kBndPad + kWave pad columns) must fit the 160 KB of one CU. Stacks of longer
// haplotypes (up to kMaxHaplen, the 16-bit field of TcDesc::dims) keep the same records in a global
// scratch area per workgroup instead (phmm_forward<.., kLong>): the reference GKL has no cap.
constexpr int kLdsHaplen = 9400;
constexpr int kMaxHaplen = 65535;
constexpr int kStackRows = 2048;  // rows per stack (a testcase taller than this gets its own)
constexpr int kMaxF64Parts = 8;
constexpr int kRollGroup = 16;  // lanes that move on to the next turn together (phmm_rolled)
// bit 7 of every row's match mask: the read may leave the f32 pass early (exit_growth); bit 7 of the
// first quality byte: the read is certified for the predictor (cert_K). No kernel reads either as data.
constexpr uint8_t kMayExit = 0x80;
constexpr uint8_t kMayPredict = 0x80;

struct __attribute__((aligned(16))) TcDesc {
  uint32_t read_off;  // pool offset: rmatch[R] (| kMayExit) q[R] i[R] d[R] c[R], then the certificate's f32 log(rho)
  uint32_t hap_off;   // pool offset: hcode[C]
  uint32_t dims;      // rslen | haplen << 16
  uint32_t out_idx;   // position in the caller's testcase array
};

// Testcases that share a haplotype, stacked into one tall matrix (phmm_stack)
struct __attribute__((aligned(16))) Stack {
  uint32_t first;  // first entry in the stack's testcase index list
  uint32_t count;  // testcases (<= 64)
  uint32_t hap_off;
  uint32_t C;
};

// wave steps of a stack (or an f64 work unit) of `rows` stacked rows over C columns with stripes of
// `sh` rows (every caller's are kWave; as a constant it changes one instruction of f64_plan): the rolled
// sweep where phmm_stack takes it, else a fill per stripe
__host__ __device__ inline uint64_t stack_steps(int rows, int C, int sh, bool roll) {
  const int turns = (rows + sh - 1) / sh;
  if (roll && sh == kWave && C >= kWave && C <= kLdsHaplen && turns >= 2) {
    const int P = (C + kRollGroup + 1 + 3) & ~3;
    return (uint64_t)(turns - 1) * (uint64_t)P + (uint64_t)(C + rows - kWave * (turns - 1));
  }
  return (uint64_t)turns * (uint64_t)(C + sh);
}

// The environment's knobs of a fill and of the runs that follow it, read once per fill (read_knobs);
// the batch keeps the copy its launches read.
struct Knobs {
  int f64_parts = 1;          // GB_PHMM_F64_PARTS: work units per stack in the f64 pass
  bool f64_plan = true;       // GB_PHMM_F64_PLAN=0: the f64 pass's units in stack order, not by cost
  bool f32_exit = true;       // GB_PHMM_EXIT=0: the f32 pass without its early exit
  bool roll = true;           // GB_PHMM_ROLL=0: a fill per stripe in both passes, no rolled sweep
  int predict = 1;            // GB_PHMM_PREDICT: 0 off, 1 behind the gate, 2 "all", 3 "open"
  int stack_rows_forced = 0;  // GB_PHMM_STACK_ROWS: rows per stack (0: plan_stacks' rule)
  double tail_frac = -1;      // GB_PHMM_TAIL=frac:rows, the tail split (< 0: plan_stacks' rule, 0: off)
  int tail_rows = 512;
  int pack_min = 1 << 13;     // GB_PHMM_PACK_MIN: the smallest call packed on several threads
};
Knobs read_knobs();

// GB_PHMM_HOSTPROF=1: host phase times of the drop-in path on stderr (development aid)
struct HostClock {
  bool on;
  std::chrono::steady_clock::time_point t0;
  HostClock() : on(getenv("GB_PHMM_HOSTPROF") != nullptr), t0(std::chrono::steady_clock::now()) {}
  void mark(const char *what) {
    if (!on) return;
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[phmm host] %s %.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t0).count());
    t0 = t;
  }
};

// The host tables the pack reads (the f32 probabilities, the certificate's ratios): built on first use,
// for the life of the process.
struct PackTables;
const PackTables &host_tables();

struct HapKey {
  const char *h;
  int len;
  bool operator==(const HapKey &o) const { return h == o.h && len == o.len; }
};
// One thread's share of a pack: testcases [lo, hi), its pool, its haplotypes in first-appearance order
struct PackChunk {
  int lo = 0, hi = 0;
  std::vector<uint8_t> *pool = nullptr;
  std::vector<uint32_t> hap_off;  // local haplotype id -> offset in this chunk's pool
  std::vector<HapKey> hap_key;    // local haplotype id -> key
  int64_t cells = 0;
};

// Pack: testcases [n * t / nth, n * (t + 1) / nth) on thread t into pools[t] (nth <= pools.size()), reads and
// haplotypes deduplicated by pointer and length, bases converted to codes, the exit and certificate flags set
// (the latter only when cert_wanted). desc[k] gets a chunk-relative read offset and hid[k] the chunk's local
// haplotype id, both until merge_pools; desc and hid hold n. The inputs have passed validate_testcases.
int pack_testcases(const gb_testcase *tcs, int n, int nth, bool cert_wanted, const PackTables &tables,
                   std::vector<std::vector<uint8_t>> &pools, TcDesc *desc, uint32_t *hid,
                   std::vector<PackChunk> *chunks);

// Bytes of the merged pool: the chunk pools end to end, rounded up to 16 and at least 16. Refuses 4 GiB.
int merged_pool_bytes(const std::vector<PackChunk> &chunks, size_t *pool_bytes);
// Merge: the chunk pools into h_pool (merged_pool_bytes of it, the padding zeroed), desc's offsets made
// absolute, hid made global: haplotype ids in order of first appearance in the call, hap_off_of[id] the
// haplotype's pool offset. cells: the call's R x C sum.
int merge_pools(const std::vector<PackChunk> &chunks, TcDesc *desc, uint32_t *hid, uint8_t *h_pool, size_t pool_bytes,
                std::vector<uint32_t> *hap_off_of, int64_t *cells);

struct Plan {
  int ns_all = 0;       // stacks: the LDS ones in launch order, then n_long long ones
  int n_long = 0;       // stacks of haplotypes longer than kLdsHaplen
  int max_h_short = 0;  // the longest haplotype of either kind (0: none)
  int max_h_long = 0;
};
// Plan: order[0 .. n) the testcases grouped by haplotype id (stable), cut into stacks in h_stacks (room for n;
// Stack::first indexes order). stacks_scratch holds n, keys_scratch 2 n. cus: compute units of the device.
Plan plan_stacks(const TcDesc *desc, int n, const uint32_t *hid, int n_haps, const Knobs &knobs, int cus,
                 uint32_t *order, Stack *stacks_scratch, uint64_t *keys_scratch, Stack *h_stacks, HostClock &clk);

// The per-testcase device arrays of a batch, carved from one allocation in this order (offsets in bytes,
// each a multiple of 256). d_rd, d_pred and d_redo are adjacent: a predicted run zeroes them with one fill.
struct ArenaLayout {
  size_t desc, rf, rd, pred, redo, out, stk_tc, stacks, units, ukey, total;
};
inline ArenaLayout arena_layout(size_t n) {
  size_t off = 0;
  auto carve = [&off](size_t bytes) {
    const size_t at = off;
    off += (bytes + 255) / 256 * 256;
    return at;
  };
  ArenaLayout A;
  A.desc = carve(sizeof(TcDesc) * n);
  A.rf = carve(sizeof(float) * n);
  A.rd = carve(sizeof(double) * n);
  A.pred = carve(n);
  A.redo = carve(n);
  A.out = carve(sizeof(double) * n);
  A.stk_tc = carve(sizeof(uint32_t) * n);
  A.stacks = carve(sizeof(Stack) * n);  // at most one stack per testcase
  A.units = carve(sizeof(uint32_t) * n * kMaxF64Parts);
  A.ukey = carve(n * kMaxF64Parts);
  A.total = off;
  return A;
}

}  // namespace phmm
}  // namespace gb
