// gb_common.h -- shared host-side plumbing for the C ABI (error state, HIP checks).
#pragma once
#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/gb.h"

namespace gb {

void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
const char *last_error();

// Returns from the enclosing int-returning function with GB_ERR_HIP on failure.
#define GB_HIP(expr)                                                                    \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) {                                                             \
      ::gb::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                      __LINE__);                                                        \
      return GB_ERR_HIP;                                                                \
    }                                                                                   \
  } while (0)

#define GB_ARG(cond, ...)          \
  do {                             \
    if (!(cond)) {                 \
      ::gb::set_error(__VA_ARGS__); \
      return GB_ERR_ARG;           \
    }                              \
  } while (0)

// Synchronous copy in pieces of at most 1 GiB, for the copies that can pass 4 GiB (index tables,
// SMEM and coordinate read-backs): no single transfer's size field reaches 32 bits.
inline hipError_t memcpy_big(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
  constexpr size_t kPiece = size_t(1) << 30;
  for (size_t o = 0; o < bytes; o += kPiece) {
    const size_t b = bytes - o < kPiece ? bytes - o : kPiece;
    const hipError_t e = hipMemcpy(static_cast<char *>(dst) + o, static_cast<const char *>(src) + o, b, kind);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// Owning grow-only buffers: DevBuf<T> is device memory, PinnedBuf<T> page-locked host memory.
// The pointer is null exactly when capacity() is 0. Growth does not keep the content. None of
// them, and no object that holds one, may have static or thread storage duration: a free at
// thread or process exit can run after the HIP runtime is torn down.
struct DeviceMem {
  static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t release(void *p) { return hipFree(p); }
  static constexpr const char *kAlloc = "hipMalloc";
};
struct PinnedMem {
  static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static hipError_t release(void *p) { return hipHostFree(p); }
  static constexpr const char *kAlloc = "hipHostMalloc";
};

template <typename T, typename Mem>
class Buf {
 public:
  Buf() = default;
  ~Buf() { reset(); }
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
  Buf(Buf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  Buf &operator=(Buf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, cap_ = o.cap_;
      o.p_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }

  // Room for n elements. A block that is too small is freed first, and the buffer is empty until
  // the new one exists: the allocators leave their out-parameter untouched when they fail.
  int reserve(size_t n) { return reserve(n, n); }
  // The same test on n, but a new block holds alloc_n >= n elements.
  int reserve(size_t n, size_t alloc_n) {
    if (n <= cap_) return GB_OK;
    reset();
    void *p = nullptr;
    const hipError_t e = Mem::alloc(&p, alloc_n * sizeof(T));
    if (e != hipSuccess) {
      set_error("%s(%zu bytes) failed: %s (%s:%d)", Mem::kAlloc, alloc_n * sizeof(T), hipGetErrorString(e), __FILE__,
                __LINE__);
      return GB_ERR_HIP;
    }
    p_ = static_cast<T *>(p);
    cap_ = alloc_n;
    return GB_OK;
  }
  void reset() {
    if (p_) (void)Mem::release(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  T *get() const { return p_; }
  operator T *() const { return p_; }
  size_t capacity() const { return cap_; }  // in elements

 private:
  T *p_ = nullptr;
  size_t cap_ = 0;
};
template <typename T>
using DevBuf = Buf<T, DeviceMem>;
template <typename T>
using PinnedBuf = Buf<T, PinnedMem>;

// roctx range around a host entry point (visible in rocprofv3 --marker-trace; a no-op otherwise)
struct Range {
  explicit Range(const char *name) { roctxRangePushA(name); }
  ~Range() { roctxRangePop(); }
  Range(const Range &) = delete;
  Range &operator=(const Range &) = delete;
};

}  // namespace gb
