// devbuf_check -- gb::DevBuf / gb::PinnedBuf (csrc/gb_common.h) outside the library (tests/test_devbuf.py).
//   devbuf_check            the allocation-failure path, on a machine without a device (exit 77 with one)
//   devbuf_check --device   the success path, on a device
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../../genomicsbench_palisade_amd/csrc/gb_common.h"

static int g_failed = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                \
    }                                                            \
  } while (0)

// Without a device every allocation fails, and leaves its out-parameter as it was.
template <typename B>
static void check_failure(const char *what) {
  {
    B b;
    for (int round = 0; round < 2; round++) {
      gb::set_error("%s", "");
      CHECK(b.reserve(1000) == GB_ERR_HIP);
      CHECK(b.get() == nullptr);
      CHECK(b.capacity() == 0);
      CHECK(gb_last_error()[0] != '\0');
    }
    gb::set_error("%s", "");
    CHECK(b.reserve(10, 64) == GB_ERR_HIP);
    CHECK(b.get() == nullptr && b.capacity() == 0);
    CHECK(gb_last_error()[0] != '\0');
    CHECK(b.reserve(0) == GB_OK);  // nothing asked for, nothing tried
    B moved(std::move(b));
    CHECK(moved.get() == nullptr && moved.capacity() == 0);
  }  // the destructors of failed buffers run here
  printf("%s: failure path ok (%s)\n", what, gb_last_error());
}

// Round trip of n ints through the buffer (a device buffer by hipMemcpy, a pinned one directly).
static bool round_trip(gb::DevBuf<int32_t> &b, size_t n, int32_t seed) {
  std::vector<int32_t> in(n), out(n, -1);
  for (size_t i = 0; i < n; i++) in[i] = seed + (int32_t)i;
  if (hipMemcpy(b.get(), in.data(), n * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) return false;
  if (hipMemcpy(out.data(), b.get(), n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return false;
  return in == out;
}
static bool round_trip(gb::PinnedBuf<int32_t> &b, size_t n, int32_t seed) {
  for (size_t i = 0; i < n; i++) b.get()[i] = seed + (int32_t)i;
  gb::DevBuf<int32_t> d;
  std::vector<int32_t> out(n, -1);
  if (d.reserve(n)) return false;
  if (hipMemcpy(d.get(), b.get(), n * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) return false;
  if (hipMemcpy(out.data(), d.get(), n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return false;
  return std::memcmp(out.data(), b.get(), n * sizeof(int32_t)) == 0;
}

template <typename B>
static void check_success(const char *what) {
  B b;
  CHECK(b.get() == nullptr && b.capacity() == 0);
  CHECK(b.reserve(100) == GB_OK);
  CHECK(b.get() != nullptr && b.capacity() == 100);
  if (!b.get()) return;
  CHECK(round_trip(b, 100, 7));
  int32_t *const p = b.get();
  CHECK(b.reserve(50) == GB_OK);  // small enough: untouched
  CHECK(b.get() == p && b.capacity() == 100);
  CHECK(b.reserve(200) == GB_OK);
  CHECK(b.get() != nullptr && b.capacity() == 200);
  CHECK(static_cast<int32_t *>(b) == b.get());

  B over;
  CHECK(over.reserve(10, 64) == GB_OK);  // over-allocation
  CHECK(over.get() != nullptr && over.capacity() == 64);
  CHECK(over.reserve(64, 1000) == GB_OK && over.capacity() == 64);

  // move-assignment: the target's block is freed, the source ends empty (so nothing is freed twice)
  int32_t *const q = b.get();
  over = std::move(b);
  CHECK(b.get() == nullptr && b.capacity() == 0);
  CHECK(over.get() == q && over.capacity() == 200);
  CHECK(round_trip(over, 200, 1000));
  B built(std::move(over));
  CHECK(over.get() == nullptr && over.capacity() == 0);
  CHECK(built.get() == q && built.capacity() == 200);
  built.reset();
  CHECK(built.get() == nullptr && built.capacity() == 0);
  CHECK(b.reserve(3) == GB_OK && b.capacity() == 3);  // a moved-from buffer is an empty one
  printf("%s: success path ok\n", what);
}

int main(int argc, char **argv) {
  const bool device = argc > 1 && std::strcmp(argv[1], "--device") == 0;
  int n = 0;
  const bool have = gb_device_count(&n) == GB_OK && n > 0;
  if (device) {
    if (!have) {
      fprintf(stderr, "devbuf_check --device: %s\n", gb_last_error());
      return 1;
    }
    check_success<gb::DevBuf<int32_t>>("DevBuf");
    check_success<gb::PinnedBuf<int32_t>>("PinnedBuf");
  } else {
    if (have) {
      printf("devbuf_check: %d device(s) present, allocations would succeed\n", n);
      return 77;
    }
    check_failure<gb::DevBuf<int32_t>>("DevBuf");
    check_failure<gb::PinnedBuf<int32_t>>("PinnedBuf");
  }
  return g_failed ? 1 : 0;
}
