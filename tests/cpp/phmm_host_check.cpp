// phmm_host_check.cpp -- stand-alone host program over the host steps of a PairHMM fill (csrc/phmm.hip through
// csrc/phmm_internal.h: pack_testcases, merge_pools, plan_stacks, arena_layout), meant to be built with the address
// and undefined-behaviour sanitizers on the host side (`make phmm-sanitize` builds it together with the library's
// source file and runs it). It touches no device: the steps write into plain vectors. Seeded jobs (none, one and two
// testcases; a cross product of read and haplotype lengths around the stripe, stack and LDS edges; 12 288
// testcases packed on one and on three threads) under every combination of the planner's knobs: the packed pool
// decodes back to the inputs, the stacks are well formed, cover the testcases once and are in launch order, and
// the arena's offsets are those of the hand-summed table it replaced. Prints "ok" and returns 0.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../genomicsbench_palisade_amd/csrc/phmm_internal.h"

using namespace gb::phmm;

#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      printf("%s:%d: ", __FILE__, __LINE__);  \
      printf(__VA_ARGS__);                    \
      printf("\n");                           \
      return 1;                               \
    }                                         \
  } while (0)

struct Job {
  // the caller's buffers: a read is five strings of one length, shared by the testcases that use it
  std::vector<std::string> rs, q, i, d, c, hap;
  std::vector<gb_testcase> tcs;
  void add(int r, int h) {
    gb_testcase t;
    t.rslen = (int)rs[r].size(), t.haplen = (int)hap[h].size();
    t.rs = rs[r].data(), t.q = q[r].data(), t.i = i[r].data(), t.d = d[r].data(), t.c = c[r].data();
    t.hap = hap[h].data();
    tcs.push_back(t);
  }
};

static std::string bases(std::mt19937 &rng, int len) {
  static const char kAlpha[] = "ACGTACGTACGTACGTNx";  // a few N and a byte that is no base
  std::string s((size_t)len, 'A');
  for (auto &ch : s) ch = kAlpha[rng() % (sizeof(kAlpha) - 1)];
  return s;
}
static std::string quals(std::mt19937 &rng, int len, int lo, int hi) {
  std::string s((size_t)len, 0);
  for (auto &ch : s) ch = (char)(lo + (int)(rng() % (uint32_t)(hi - lo + 1)));
  return s;
}
static void add_read(Job &J, std::mt19937 &rng, int len) {
  J.rs.push_back(bases(rng, len));
  // base qualities over the whole byte (bit 7 of the first is the pack's flag), the others in the usual range
  J.q.push_back(quals(rng, len, 0, 255));
  J.i.push_back(quals(rng, len, 2, 60));
  J.d.push_back(quals(rng, len, 2, 60));
  J.c.push_back(quals(rng, len, 1, 40));
}

// the pack's encodings, restated (ConvertChar; the match mask of a read base)
static uint8_t code_of(char ch) { return ch == 'C' ? 1 : ch == 'T' ? 2 : ch == 'G' ? 3 : ch == 'N' ? 4 : 0; }
static uint8_t mask_of(char ch) { return code_of(ch) == 4 ? 0x1F : (uint8_t)((1u << code_of(ch)) | 0x10); }

struct Packed {
  std::vector<TcDesc> desc;
  std::vector<uint32_t> hid, hap_off_of;
  std::vector<uint8_t> pool;
  int64_t cells = 0;
};

static int pack(const Job &J, int nth, bool cert, Packed &P) {
  const int n = (int)J.tcs.size();
  P.desc.assign((size_t)std::max(n, 1), TcDesc{});
  P.hid.assign((size_t)std::max(n, 1), 0);
  std::vector<std::vector<uint8_t>> pools((size_t)nth);
  std::vector<PackChunk> ch;
  CHECK(pack_testcases(J.tcs.data(), n, nth, cert, host_tables(), pools, P.desc.data(), P.hid.data(), &ch) == 0,
        "pack_testcases failed");
  CHECK((int)ch.size() == nth, "chunks");
  for (int t = 0; t < nth; t++)
    CHECK(ch[t].lo == (int)((int64_t)n * t / nth) && ch[t].hi == (int)((int64_t)n * (t + 1) / nth), "chunk edges");
  size_t bytes = 0;
  CHECK(merged_pool_bytes(ch, &bytes) == 0 && bytes >= 16 && bytes % 16 == 0, "merged_pool_bytes");
  P.pool.assign(bytes, 0xAA);  // exactly the bytes asked for: a write past them is the sanitizer's
  CHECK(merge_pools(ch, P.desc.data(), P.hid.data(), P.pool.data(), bytes, &P.hap_off_of, &P.cells) == 0,
        "merge_pools failed");
  return 0;
}

// every descriptor decodes to its testcase; haplotype ids are dense and in order of first appearance
static int check_decode(const Job &J, const Packed &P) {
  const int n = (int)J.tcs.size();
  int64_t cells = 0;
  uint32_t next_id = 0;
  for (int k = 0; k < n; k++) {
    const gb_testcase &t = J.tcs[k];
    const TcDesc &D = P.desc[k];
    const int R = t.rslen, C = t.haplen;
    CHECK(D.dims == ((uint32_t)R | (uint32_t)C << 16) && D.out_idx == (uint32_t)k, "testcase %d: dims / out_idx", k);
    CHECK((size_t)D.read_off + 5 * (size_t)R + 4 <= P.pool.size(), "testcase %d: read record outside the pool", k);
    CHECK((size_t)D.hap_off + (size_t)C <= P.pool.size(), "testcase %d: haplotype outside the pool", k);
    const uint8_t *rec = P.pool.data() + D.read_off;
    for (int r = 0; r < R; r++) {
      CHECK((rec[r] & 0x7F) == mask_of(t.rs[r]), "testcase %d row %d: match mask", k, r);
      const uint8_t keep = r == 0 ? 0x7F : 0xFF;
      CHECK((rec[R + r] & keep) == ((uint8_t)t.q[r] & keep), "testcase %d row %d: base quality", k, r);
      CHECK(rec[2 * R + r] == (uint8_t)t.i[r] && rec[3 * R + r] == (uint8_t)t.d[r] && rec[4 * R + r] == (uint8_t)t.c[r],
            "testcase %d row %d: gap qualities", k, r);
      CHECK((rec[r] & kMayExit) == (rec[0] & kMayExit), "testcase %d: the exit flag is per read", k);
    }
    const uint8_t *hc = P.pool.data() + D.hap_off;
    for (int c = 0; c < C; c++) CHECK(hc[c] == code_of(t.hap[c]), "testcase %d column %d: haplotype code", k, c);
    CHECK(P.hid[k] <= next_id, "testcase %d: haplotype id %u before %u", k, P.hid[k], next_id);
    if (P.hid[k] == next_id) next_id++;
    CHECK(P.hap_off_of[P.hid[k]] == D.hap_off, "testcase %d: hap_off_of", k);
    cells += (int64_t)R * C;
  }
  CHECK(next_id == P.hap_off_of.size() && cells == P.cells, "haplotype count / cells");
  return 0;
}

// the stack height rule of plan_stacks, restated from its comment
static int rule_rows(const Packed &P, int n, int cus) {
  int64_t total = 0;
  for (int k = 0; k < n; k++) total += (int64_t)(P.desc[k].dims & 0xffff) + 2;
  int rows = 2048;
  if (total / rows < 4ll * 32 * cus) rows = 1024;
  if (rows == 1024 && total / rows < 16ll * cus) rows = 512;
  while (rows > 128 && total / rows < 8ll * cus) rows /= 2;
  return rows;
}

struct Planned {
  Plan P;
  std::vector<uint32_t> order;
  std::vector<Stack> stacks;
};
static Planned plan(const Packed &K, int n, const Knobs &knobs, int cus) {
  Planned R;
  const size_t nn = (size_t)std::max(n, 1);
  R.order.assign(nn, 0xFFFFFFFFu);
  R.stacks.assign(nn, Stack{});
  std::vector<Stack> scratch(nn);
  std::vector<uint64_t> keys(2 * nn);
  HostClock clk;
  R.P = plan_stacks(K.desc.data(), n, K.hid.data(), (int)K.hap_off_of.size(), knobs, cus, R.order.data(), scratch.data(),
                    keys.data(), R.stacks.data(), clk);
  return R;
}

static int check_plan(const Packed &K, int n, const Knobs &knobs, int cus) {
  const Planned R = plan(K, n, knobs, cus);
  Knobs whole = knobs;
  whole.tail_frac = 0;
  const Planned W = plan(K, n, whole, cus);  // the same plan before the tail split: what is not in it is a tail piece
  std::set<std::pair<uint32_t, uint32_t>> uncut;
  for (int s = 0; s < W.P.ns_all; s++) uncut.insert({W.stacks[s].first, W.stacks[s].count});
  const Plan &P = R.P;
  CHECK(P.ns_all >= 0 && P.ns_all <= n && P.n_long >= 0 && P.n_long <= P.ns_all, "counts %d %d", P.ns_all, P.n_long);
  std::vector<char> seen((size_t)std::max(n, 1), 0);
  for (int k = 0; k < n; k++) {
    CHECK(R.order[k] < (uint32_t)n && !seen[R.order[k]], "order is no permutation at %d", k);
    seen[R.order[k]] = 1;
  }
  const int stack_rows = knobs.stack_rows_forced ? knobs.stack_rows_forced : rule_rows(K, n, cus);
  const int ns_short = P.ns_all - P.n_long;
  int max_short = 0, max_long = 0;
  uint64_t prev = ~0ull;
  std::vector<std::pair<uint32_t, uint32_t>> spans;
  for (int s = 0; s < P.ns_all; s++) {
    const Stack &S = R.stacks[s];
    CHECK(S.count >= 1 && S.count <= 64 && (uint64_t)S.first + S.count <= (uint64_t)n, "stack %d: count %u", s, S.count);
    int rows = 0;
    for (uint32_t t = 0; t < S.count; t++) {
      const TcDesc &D = K.desc[R.order[S.first + t]];
      CHECK(D.hap_off == S.hap_off && (D.dims >> 16) == S.C, "stack %d entry %u: another haplotype", s, t);
      rows += (int)(D.dims & 0xffff) + 2;
    }
    const bool piece = !uncut.count({S.first, S.count});
    const int limit = piece ? std::min(stack_rows, knobs.tail_rows) : stack_rows;
    CHECK(S.count == 1 || rows <= limit, "stack %d: %d rows over the limit %d", s, rows, limit);
    const bool is_long = (int)S.C > kLdsHaplen;
    CHECK(is_long == (s >= ns_short), "stack %d: LDS stacks first, long ones last", s);
    CHECK(!(piece && is_long), "stack %d: a long stack was cut", s);
    (is_long ? max_long : max_short) = std::max(is_long ? max_long : max_short, (int)S.C);
    // launch order: the LDS stacks by the cost of the sweep the knobs select, the long ones by the fill per stripe
    if (s == ns_short) prev = ~0ull;
    const uint64_t cost = std::min<uint64_t>(stack_steps(rows, (int)S.C, kWave, !is_long && knobs.roll), 0x7fffffffu);
    CHECK(cost <= prev, "stack %d: cost %llu after %llu", s, (unsigned long long)cost, (unsigned long long)prev);
    prev = cost;
    spans.push_back({S.first, S.count});
  }
  CHECK(max_short == P.max_h_short && max_long == P.max_h_long, "max_h %d %d", P.max_h_short, P.max_h_long);
  std::sort(spans.begin(), spans.end());
  uint32_t at = 0;
  for (const auto &sp : spans) {
    CHECK(sp.first == at, "stacks leave a gap or overlap at %u", at);
    at += sp.second;
  }
  CHECK(at == (uint32_t)n, "stacks cover %u of %d", at, n);
  if (knobs.tail_frac >= 1.0)
    for (int s = 0; s < ns_short; s++) {
      int rows = 0;
      for (uint32_t t = 0; t < R.stacks[s].count; t++) rows += (int)(K.desc[R.order[R.stacks[s].first + t]].dims & 0xffff) + 2;
      CHECK(R.stacks[s].count == 1 || rows <= knobs.tail_rows, "stack %d: the whole job is tail, %d rows", s, rows);
    }
  return 0;
}

static int check_plans(const Packed &K, int n) {
  static const int kRows[] = {0, 128, 512, 1024};  // 0: the rule
  static const struct {
    double frac;
    int rows;
  } kTail[] = {{0.0, 512}, {0.9, 64}, {1.0, 1}};
  for (int rows : kRows)
    for (const auto &tail : kTail)
      for (int roll = 0; roll < 2; roll++)
        for (int cus : {1, 256}) {
          Knobs knobs;
          knobs.stack_rows_forced = rows, knobs.tail_frac = tail.frac, knobs.tail_rows = tail.rows, knobs.roll = roll != 0;
          if (check_plan(K, n, knobs, cus)) {
            printf("  (n %d, stack rows %d, tail %.1f:%d, roll %d, cus %d)\n", n, rows, tail.frac, tail.rows, roll, cus);
            return 1;
          }
        }
  return 0;
}

// the arena as batch_reserve summed and carved it by hand before arena_layout
static int check_arena(size_t n) {
  auto up = [](size_t x) { return (x + 255) / 256 * 256; };
  const size_t sz[10] = {up(16 * n), up(4 * n), up(8 * n), up(8 * n), up(4 * n),
                         up(16 * n), up(4 * n * 8), up(n * 8), up(n), up(n)};
  size_t a = 0;
  const ArenaLayout A = arena_layout(n);
  CHECK(A.desc == a, "desc");
  a += sz[0];
  CHECK(A.rf == a, "rf");
  a += sz[1];
  CHECK(A.rd == a, "rd");
  a += sz[2];
  CHECK(A.pred == a, "pred");
  a += sz[8];
  CHECK(A.redo == a, "redo");
  a += sz[9];
  CHECK(A.out - A.rd == sz[2] + sz[8] + sz[9], "pred_bytes");
  CHECK(A.out == a, "out");
  a += sz[3];
  CHECK(A.stk_tc == a, "stk_tc");
  a += sz[4];
  CHECK(A.stacks == a, "stacks");
  a += sz[5];
  CHECK(A.units == a, "units");
  a += sz[6];
  CHECK(A.ukey == a, "ukey");
  a += sz[7];
  CHECK(A.total == a && a == sz[0] + sz[1] + sz[2] + sz[3] + sz[4] + sz[5] + sz[6] + sz[7] + sz[8] + sz[9], "total");
  return 0;
}

int main() {
  static_assert(sizeof(TcDesc) == 16 && sizeof(Stack) == 16 && kMaxF64Parts == 8, "check_arena's sizes");
  std::mt19937 rng(20261021);
  // none, one, two testcases (two: one read against two haplotypes)
  for (int n = 0; n <= 2; n++) {
    Job J;
    add_read(J, rng, 70);
    J.hap = {bases(rng, 90), bases(rng, 64)};
    for (int k = 0; k < n; k++) J.add(0, k);
    Packed P;
    if (pack(J, 1, n == 1, P) || check_decode(J, P) || check_plans(P, n)) return 1;
  }
  {  // read rows around the stripe and stack edges against haplotypes around the rolled sweep's and the LDS's
    Job J;
    for (int len : {1, 2, 62, 63, 64, 65, 66, 127, 128, 129, 1100, 2046, 2100}) add_read(J, rng, len);
    for (int len : {1, 3, 63, 64, 700, 9400, 9401}) J.hap.push_back(bases(rng, len));
    for (size_t r = 0; r < J.rs.size(); r++)
      for (size_t h = 0; h < J.hap.size(); h++) J.add((int)r, (int)h);
    const int n = (int)J.tcs.size();
    Packed P, Q;
    if (pack(J, 1, true, P) || check_decode(J, P) || check_plans(P, n)) return 1;
    if (pack(J, 1, false, Q) || check_decode(J, Q)) return 1;
  }
  {  // three chunks: reads and haplotypes shared across the chunk edges (a read's 127 testcases straddle 4096 and 8192)
    Job J;
    for (int r = 0; r < 97; r++) add_read(J, rng, 8 + (int)(rng() % 40));
    for (int h = 0; h < 127; h++) J.hap.push_back(bases(rng, 40 + (int)(rng() % 60)));
    for (int r = 0; r < 97 && J.tcs.size() < 12288; r++)
      for (int h = 0; h < 127 && J.tcs.size() < 12288; h++) J.add(r, h);
    const int n = (int)J.tcs.size();
    CHECK(n == 12288, "job size");
    Packed one, three;
    if (pack(J, 1, true, one) || check_decode(J, one) || check_plans(one, n)) return 1;
    if (pack(J, 3, true, three) || check_decode(J, three) || check_plans(three, n)) return 1;
    CHECK(one.hid == three.hid && one.cells == three.cells, "one and three threads: haplotype ids");
    CHECK(three.pool.size() > one.pool.size(), "a read shared across a chunk edge is stored once per chunk");
    for (int k = 0; k < n; k++) {  // (both decode to the inputs; the flags are the pack's own)
      const int R = J.tcs[k].rslen;
      CHECK(memcmp(one.pool.data() + one.desc[k].read_off, three.pool.data() + three.desc[k].read_off, 5 * (size_t)R + 4) == 0,
            "testcase %d: one and three threads pack another read record", k);
    }
  }
  for (size_t n : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)100000})
    if (check_arena(std::max<size_t>(n, 1))) return 1;
  printf("ok\n");
  return 0;
}
