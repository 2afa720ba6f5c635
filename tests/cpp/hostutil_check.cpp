// hostutil_check.cpp -- stand-alone host program over the host utilities of csrc/gb_common.h:
// gb::parallel, gb::thread_count, gb::thread_ws and gb::round_up. Meant to be built with the address
// and undefined-behaviour sanitizers on the host side (`make hostutil-sanitize` builds it together with
// gb_common.cpp and runs it). No HIP call is made and no device touched. Prints "ok" and returns 0.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
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

int main() {
  for (int nth : {1, 2, 16}) {
    check_parallel(nth, -1);
    check_parallel(nth, nth - 1);  // a worker (the caller when nth is 1)
    check_parallel(nth, 0);        // the caller
  }
  check_thread_count();
  check_thread_ws();
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
