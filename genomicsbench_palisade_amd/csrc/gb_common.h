// gb_common.h -- shared host-side plumbing for the C ABI: error state, HIP checks, owning buffers and
// handles, per-thread workspaces and their maker, environment numbers and switches, the chunk cutter,
// host fork-join.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>
#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

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

// Owning stream and event handles: move-only, null exactly when not created, destroyed with the
// object, and converting to the raw handle. create() returns HIP's status, so the caller words its
// own error. The storage-duration rule of the buffers above holds for them too.
template <typename H, hipError_t (*Destroy)(H)>
class Handle {
 public:
  Handle() = default;
  ~Handle() { reset(); }
  Handle(const Handle &) = delete;
  Handle &operator=(const Handle &) = delete;
  Handle(Handle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  Handle &operator=(Handle &&o) noexcept {
    if (this != &o) {
      reset();
      h_ = o.h_;
      o.h_ = nullptr;
    }
    return *this;
  }
  void reset() {
    if (h_) (void)Destroy(h_);
    h_ = nullptr;
  }
  operator H() const { return h_; }

 protected:
  H h_ = nullptr;
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {  // a non-blocking stream
  hipError_t create() {
    reset();
    return hipStreamCreateWithFlags(&h_, hipStreamNonBlocking);
  }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
  hipError_t create() {
    reset();
    return hipEventCreate(&h_);
  }
};

// The calling thread's workspace of type T for (device, slot): make(dev, &T*) builds it on first use
// and it is registered only when make returns GB_OK, so a failed make is tried again by the next
// call. One workspace per (calling thread, device, slot), never freed: a free at thread exit could
// run after the HIP runtime is torn down. The registry is keyed by T alone and holds raw pointers
// only; the workspace itself lives on the heap, so the storage-duration rule above holds.
template <typename T>
struct ThreadWs {
  int dev, slot;
  T *ws;
  static std::vector<ThreadWs> &all() {
    thread_local std::vector<ThreadWs> v;
    return v;
  }
};
template <typename T>
T *find_thread_ws(int dev, int slot = 0) {  // null before the first successful make
  for (const auto &e : ThreadWs<T>::all())
    if (e.dev == dev && e.slot == slot) return e.ws;
  return nullptr;
}
template <typename T, typename Make>
int thread_ws(int dev, int slot, T **out, Make &&make) {
  if ((*out = find_thread_ws<T>(dev, slot))) return GB_OK;
  if (const int st = make(dev, out)) return *out = nullptr, st;
  ThreadWs<T>::all().push_back({dev, slot, *out});
  return GB_OK;
}
template <typename T, typename Make>
int thread_ws(int dev, T **out, Make &&make) {
  return thread_ws<T>(dev, 0, out, make);
}

// What most legs' workspaces start with, and their maker: the calling thread's Ws (a WsBase) for dev
// through thread_ws. First use sets the device and its CU count, creates the stream and the events,
// and then runs the leg's own extra(W). extra returns a status whose error it has worded itself (a
// reserve, say), or HIP's status of more handles it created, worded here like that of the common
// ones: "<what> workspace: <hip error>", `what` naming the entry point.
template <int kEvents>
struct WsBase {
  int device = -1, num_cus = 0;  // both set by get_ws before anyone sees the workspace
  Stream stream;
  Event ev[kEvents];
};
inline int ws_status(const char *, int st) { return st; }
inline int ws_status(const char *what, hipError_t e) {
  if (e == hipSuccess) return GB_OK;
  set_error("%s workspace: %s", what, hipGetErrorString(e));
  return GB_ERR_HIP;
}
template <typename Ws, typename Extra>
int get_ws(const char *what, int dev, Ws **out, Extra &&extra) {
  return thread_ws(dev, out, [&](int dev, Ws **out) -> int {
    auto *W = new Ws();
    W->device = dev;
    hipError_t e = hipDeviceGetAttribute(&W->num_cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) e = W->stream.create();
    for (auto &ev : W->ev)
      if (e == hipSuccess) e = ev.create();
    int st = ws_status(what, e);
    if (!st) st = ws_status(what, extra(W));
    if (st) {
      delete W;
      return st;
    }
    *out = W;
    return GB_OK;
  });
}
template <typename Ws>
int get_ws(const char *what, int dev, Ws **out) {
  return get_ws(what, dev, out, [](Ws *) -> int { return GB_OK; });
}

// For the accessors (`fn`) of an entry point (`call`): the calling thread's workspace on its current
// device, or GB_ERR_STATE when call has not run there. With `ran`, a counter of the workspace such as
// &Ws::calls, a workspace whose counter is 0 has not run either.
template <typename Ws>
int ran_ws(const char *fn, const char *call, const Ws **out, int64_t Ws::*ran = nullptr) {
  int dev = 0;
  GB_HIP(hipGetDevice(&dev));
  const Ws *W = find_thread_ws<Ws>(dev);
  if (!W || (ran && !(W->*ran))) {
    set_error("%s: %s has not run on this thread and device", fn, call);
    return GB_ERR_STATE;
  }
  *out = W;
  return GB_OK;
}

// The whole decimal number in the environment variable `name`, read on every call: unset or empty is
// dflt; anything but a number in [lo, hi] (text after it, nothing at all, out of int64_t's range) is
// GB_ERR_ARG with "<who>: <name> is '<text>' ..." and leaves *out at dflt.
int env_number(const char *who, const char *name, int64_t lo, int64_t hi, int64_t dflt, int64_t *out);
// A switch such as GB_POA_HOST, read on every call: on exactly when the value begins with '1'.
bool env_flag(const char *name);

// A call cut to fit device memory. An item's need is a small struct of the leg's own: counts per
// buffer with bytes(), += and, for largest(), max_with() (the element-wise maximum). A chunk is the items
// [first, last) of the call and the sum of their needs.
template <typename Need>
struct Chunk {
  int64_t first, last;
  Need need;
};
// Appends the chunks of items 0 .. n-1, need_of(k) being item k's need: the items in order, each
// joining the current chunk unless that chunk has an item and the sum would pass the budget. An item
// that alone passes the budget is still a chunk of its own; the first such item's index is returned,
// -1 when there is none.
template <typename Need, typename F>
int64_t cut_chunks(int64_t n, int64_t budget, F &&need_of, std::vector<Chunk<Need>> *chunks) {
  int64_t over = -1;
  Chunk<Need> cur{0, 0, Need{}};
  for (int64_t k = 0; k < n; ++k) {
    const Need one = need_of(k);
    if (over < 0 && one.bytes() > budget) over = k;
    if (cur.last > cur.first && cur.need.bytes() + one.bytes() > budget) {
      chunks->push_back(cur);
      cur = Chunk<Need>{k, k, Need{}};
    }
    cur.last = k + 1, cur.need += one;
  }
  if (cur.last > cur.first) chunks->push_back(cur);
  return over;
}
// The largest any chunk asks of each buffer, the most items and the most bytes of any chunk: buffers
// reserved at these do not grow between the chunks of a call.
template <typename Need>
struct Largest {
  Need need{};
  int64_t count = 0, bytes = 0;
};
template <typename Need>
Largest<Need> largest(const std::vector<Chunk<Need>> &chunks) {
  Largest<Need> big;
  for (const Chunk<Need> &c : chunks) {
    big.need.max_with(c.need);
    big.count = std::max(big.count, c.last - c.first), big.bytes = std::max(big.bytes, c.need.bytes());
  }
  return big;
}

// Host worker threads for a call: the count in the environment variable env_name (default 16, values
// above 64 taken as 64), then at most the hardware's. Anything but a count >= 1 is GB_ERR_ARG.
int thread_count(const char *who, const char *env_name, int *n);

// Fork-join: body(t) for t in [0, nth), t == 0 on the caller. Everything that started is joined
// and no exception leaves: a body that threw, or a thread that could not start, is GB_ERR_NOMEM.
template <typename F>
int parallel(const char *who, int nth, F &&body) {
  std::atomic<bool> failed{false};
  auto guarded = [&](int t) {
    try {
      body(t);
    } catch (...) {
      failed.store(true);
    }
  };
  {
    std::vector<std::thread> th;
    try {
      for (int t = 1; t < nth; ++t) th.emplace_back(guarded, t);
    } catch (...) {
      failed.store(true);
    }
    guarded(0);
    for (auto &x : th) x.join();
  }
  if (failed.load()) {
    set_error("%s: out of host memory on the host path", who);
    return GB_ERR_NOMEM;
  }
  return GB_OK;
}

// v rounded up to a multiple of a (v >= 0, a > 0); the type is v's
template <typename T>
constexpr T round_up(T v, std::common_type_t<T> a) {
  return (v + a - 1) / a * a;
}

// roctx range around a host entry point (visible in rocprofv3 --marker-trace; a no-op otherwise)
struct Range {
  explicit Range(const char *name) { roctxRangePushA(name); }
  ~Range() { roctxRangePop(); }
  Range(const Range &) = delete;
  Range &operator=(const Range &) = delete;
};

}  // namespace gb
