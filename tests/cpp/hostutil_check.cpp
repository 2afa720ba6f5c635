// hostutil_check.cpp -- stand-alone host program over the host utilities of csrc/gb_common.h:
// gb::parallel, gb::thread_count, gb::thread_ws, gb::round_up, gb::env_number, gb::env_flag and
// gb::cut_chunks with gb::largest. Meant to be built with the address and undefined-behaviour sanitizers
// on the host side (`make hostutil-sanitize` builds it together with gb_common.cpp and runs it). No HIP
// call is made and no device touched. Prints "ok" and returns 0.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <random>
#include <thread>
#include <vector>

#include "../../genomicsbench_palisade_amd/csrc/gb_common.h"

static int g_fail = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                  \
    }                                                            \
  } while (0)

static const char *kWho = "hostutil_check";
static const char *kEnv = "GB_HOSTUTIL_CHECK_THREADS";

// body(t) for every t exactly once; with thrower >= 0 that body throws after it was counted
static void check_parallel(int nth, int thrower) {
  std::vector<std::atomic<int>> ran((size_t)nth);
  for (auto &r : ran) r.store(0);
  gb::set_error("none");
  const int st = gb::parallel(kWho, nth, [&](int t) {
    ran[(size_t)t].fetch_add(1);
    if (t == thrower) throw std::bad_alloc();
  });
  for (int t = 0; t < nth; ++t) CHECK(ran[(size_t)t].load() == 1);
  if (thrower < 0) {
    CHECK(st == GB_OK && !strcmp(gb::last_error(), "none"));
  } else {
    CHECK(st == GB_ERR_NOMEM);
    CHECK(!strcmp(gb::last_error(), "hostutil_check: out of host memory on the host path"));
  }
}

static void check_thread_count() {
  const int hw = (int)std::max(1u, std::thread::hardware_concurrency());
  int n = -1;
  unsetenv(kEnv);
  CHECK(gb::thread_count(kWho, kEnv, &n) == GB_OK && n == std::min(16, hw));
  setenv(kEnv, "5", 1);
  CHECK(gb::thread_count(kWho, kEnv, &n) == GB_OK && n == std::min(5, hw));
  setenv(kEnv, "1000", 1);
  CHECK(gb::thread_count(kWho, kEnv, &n) == GB_OK && n == std::min(64, hw));
  for (const char *bad : {"0", "", "abc", "5x"}) {
    setenv(kEnv, bad, 1);
    n = -1;
    CHECK(gb::thread_count(kWho, kEnv, &n) == GB_ERR_ARG && n == -1);
    CHECK(strstr(gb::last_error(), kEnv) && strstr(gb::last_error(), "is not a thread count"));
  }
  unsetenv(kEnv);
}

struct Ws {
  int dev;
};
static std::atomic<int> g_made{0};
static int make_ws(int dev, Ws **out) {
  g_made.fetch_add(1);
  *out = new Ws{dev};
  return GB_OK;
}

static void check_thread_ws() {
  Ws *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr;
  CHECK(gb::find_thread_ws<Ws>(0) == nullptr);
  CHECK(gb::thread_ws(0, &a, make_ws) == GB_OK && a && a->dev == 0 && g_made.load() == 1);
  // the same (device, slot) again, through a make of another type: one registry per workspace type
  CHECK(gb::thread_ws(0, 0, &b, [](int, Ws **) { return GB_ERR_STATE; }) == GB_OK && b == a && g_made.load() == 1);
  CHECK(gb::find_thread_ws<Ws>(0) == a);
  CHECK(gb::thread_ws(0, 1, &c, make_ws) == GB_OK && c && c != a && g_made.load() == 2);
  CHECK(gb::thread_ws(1, &d, make_ws) == GB_OK && d && d != a && d != c && d->dev == 1 && g_made.load() == 3);
  Ws *other = nullptr;
  std::thread([&] {
    CHECK(gb::find_thread_ws<Ws>(0) == nullptr);
    CHECK(gb::thread_ws(0, &other, make_ws) == GB_OK);
  }).join();
  CHECK(other && other != a && g_made.load() == 4);
  // a failing make registers nothing and is tried again
  int tries = 0;
  auto flaky = [&](int dev, Ws **out) -> int {
    if (++tries == 1) return GB_ERR_HIP;
    return make_ws(dev, out);
  };
  Ws *e = nullptr;
  CHECK(gb::thread_ws(2, &e, flaky) == GB_ERR_HIP && e == nullptr && gb::find_thread_ws<Ws>(2) == nullptr);
  CHECK(gb::thread_ws(2, &e, flaky) == GB_OK && e && tries == 2 && gb::find_thread_ws<Ws>(2) == e);
  for (Ws *w : {a, c, d, other, e}) delete w;  // the registry never frees; the program does, for the leak check
}

// gb::env_number over [lo, hi] = [10, 20] with the default 15, and over the whole of int64_t
static void check_env_number() {
  const char *name = "GB_HOSTUTIL_CHECK_NUMBER";
  auto get = [&](const char *text, int64_t lo, int64_t hi, int64_t *out) {
    if (text)
      setenv(name, text, 1);
    else
      unsetenv(name);
    *out = -7;
    gb::set_error("none");
    return gb::env_number(kWho, name, lo, hi, 15, out);
  };
  int64_t v;
  CHECK(get(nullptr, 10, 20, &v) == GB_OK && v == 15);  // unset and empty are the default
  CHECK(get("", 10, 20, &v) == GB_OK && v == 15 && !strcmp(gb::last_error(), "none"));
  CHECK(get("10", 10, 20, &v) == GB_OK && v == 10);
  CHECK(get("20", 10, 20, &v) == GB_OK && v == 20);
  CHECK(get(" 12", 10, 20, &v) == GB_OK && v == 12);  // strtoll passes over white space in front, and takes a sign
  CHECK(get("+12", 10, 20, &v) == GB_OK && v == 12);
  CHECK(get("-3", -5, 5, &v) == GB_OK && v == -3);
  CHECK(get("9223372036854775807", 1, INT64_MAX, &v) == GB_OK && v == INT64_MAX);
  // refused, named with the variable and the text, and *out left at the default
  for (const char *bad : {"9", "21", "12k", "abc", "12 ", " ", "1e3", "0x10", "12.0"}) {
    CHECK(get(bad, 10, 20, &v) == GB_ERR_ARG && v == 15);
    char want[64];
    snprintf(want, sizeof(want), "hostutil_check: %s is '%s'", name, bad);
    CHECK(strstr(gb::last_error(), want) == gb::last_error());
  }
  for (const char *bad : {"9223372036854775808", "99999999999999999999", "-9223372036854775809"})
    CHECK(get(bad, INT64_MIN, INT64_MAX, &v) == GB_ERR_ARG && v == 15);  // outside int64_t, not clamped to its ends
  unsetenv(name);
}

static void check_env_flag() {
  const char *name = "GB_HOSTUTIL_CHECK_FLAG";
  unsetenv(name);
  CHECK(!gb::env_flag(name));
  const struct {
    const char *text;
    bool on;
  } cases[] = {{"", false}, {"0", false}, {"1", true}, {"10", true}, {"true", false}, {" 1", false}, {"01", false}};
  for (const auto &c : cases) {
    setenv(name, c.text, 1);
    CHECK(gb::env_flag(name) == c.on);
  }
  unsetenv(name);
}

struct Need {  // one buffer, counted in bytes
  int64_t b;
  int64_t bytes() const { return b; }
  void operator+=(const Need &o) { b += o.b; }
  void max_with(const Need &o) { b = std::max(b, o.b); }
};
using Chunk = gb::Chunk<Need>;

static int64_t cut(const std::vector<int64_t> &sizes, int64_t budget, std::vector<Chunk> *chunks) {
  chunks->clear();
  return gb::cut_chunks((int64_t)sizes.size(), budget, [&](int64_t k) { return Need{sizes[(size_t)k]}; }, chunks);
}

static void check_cut_chunks() {
  std::vector<Chunk> ch;
  CHECK(cut({}, 100, &ch) == -1 && ch.empty());
  CHECK(gb::largest(ch).count == 0 && gb::largest(ch).bytes == 0 && gb::largest(ch).need.b == 0);
  const std::vector<int64_t> five{7, 7, 7, 7, 7};
  CHECK(cut(five, 35, &ch) == -1 && ch.size() == 1 && ch[0].first == 0 && ch[0].last == 5 && ch[0].need.b == 35);
  CHECK(cut(five, 34, &ch) == -1 && ch.size() == 2 && ch[0].last == 4 && ch[1].first == 4 && ch[1].last == 5);
  CHECK(gb::largest(ch).count == 4 && gb::largest(ch).bytes == 28 && gb::largest(ch).need.b == 28);
  CHECK(cut(five, 7, &ch) == -1 && ch.size() == 5);  // the budget is one item's need: a chunk each
  for (size_t k = 0; k < ch.size(); ++k) CHECK(ch[k].first == (int64_t)k && ch[k].last == (int64_t)k + 1 && ch[k].need.b == 7);
  CHECK(cut({3, 10, 3}, 10, &ch) == -1 && ch.size() == 3);  // exactly at the budget is accepted
  // one byte over: named by index, and still placed, alone; only the first such item is named
  CHECK(cut({3, 11, 3, 12}, 10, &ch) == 1 && ch.size() == 4 && ch[1].first == 1 && ch[1].last == 2 && ch[1].need.b == 11);
  CHECK(cut({11}, 10, &ch) == 0 && ch.size() == 1 && ch[0].need.b == 11);
  // chunks are appended: what the vector held stays
  CHECK(gb::cut_chunks(2, 100, [](int64_t) { return Need{1}; }, &ch) == -1 && ch.size() == 2 && ch[0].need.b == 11 &&
        ch[1].first == 0 && ch[1].last == 2);

  std::mt19937_64 rng(20261021);
  for (int trial = 0; trial < 200; ++trial) {
    std::vector<int64_t> sizes((size_t)(rng() % 40));
    for (auto &s : sizes) s = (int64_t)(rng() % 50);  // zero-byte items among them
    const int64_t budget = 1 + (int64_t)(rng() % 120);
    const int64_t over = cut(sizes, budget, &ch);
    int64_t want_over = -1, at = 0, big_n = 0, big_b = 0;
    for (size_t k = 0; k < sizes.size() && want_over < 0; ++k)
      if (sizes[k] > budget) want_over = (int64_t)k;
    CHECK(over == want_over);
    for (size_t c = 0; c < ch.size(); ++c) {
      CHECK(ch[c].first == at && ch[c].last > at);  // contiguous, none empty
      int64_t sum = 0;
      for (int64_t k = ch[c].first; k < ch[c].last; ++k) sum += sizes[(size_t)k];
      CHECK(ch[c].need.b == sum);
      CHECK(sum <= budget || ch[c].last - ch[c].first == 1);  // under the budget, or a single item
      if (c + 1 < ch.size()) CHECK(sum + sizes[(size_t)ch[c].last] > budget);  // greedy: the next item did not fit
      at = ch[c].last, big_n = std::max(big_n, ch[c].last - ch[c].first), big_b = std::max(big_b, sum);
    }
    CHECK(at == (int64_t)sizes.size());  // and they cover [0, n)
    const auto big = gb::largest(ch);
    CHECK(big.count == big_n && big.bytes == big_b && big.need.b == big_b);
  }
}

int main() {
  for (int nth : {1, 2, 16}) {
    check_parallel(nth, -1);
    check_parallel(nth, nth - 1);  // a worker (the caller when nth is 1)
    check_parallel(nth, 0);        // the caller
  }
  check_thread_count();
  check_thread_ws();
  check_env_number();
  check_env_flag();
  check_cut_chunks();
  for (int64_t a : {1, 4, 16, 256})
    for (int64_t k = 0; k < 5; ++k) {
      CHECK(gb::round_up<int64_t>(k * a, a) == k * a);
      CHECK(gb::round_up<int64_t>(k * a + 1, a) == (k + 1) * a);
    }
  CHECK(gb::round_up<size_t>(0, 16) == 0 && gb::round_up(17, 16) == 32 && gb::round_up<size_t>(255, 256) == 256);
  if (g_fail) return 1;
  printf("ok\n");
  return 0;
}
