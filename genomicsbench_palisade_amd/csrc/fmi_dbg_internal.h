// fmi_dbg_internal.h -- what the device path and the host path of fmi_dbg.hip share: the text views, the walk
// lengths and the fingerprint arithmetic.
#pragma once
#include <cstdint>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace gb {
namespace dbg {

struct Texts {  // the call's inputs, on the host or on the device
  const uint8_t *ref_bytes;
  const int64_t *ref_off;
  const uint8_t *seq, *qual;
  const int64_t *read_off;
};

// edges of a text of len bytes at k: the walk covers i = 0 .. len - k - 2
__host__ __device__ inline int64_t walk_edges(int64_t len, int k) { return len - k - 1 > 0 ? len - k - 1 : 0; }

constexpr uint64_t kBase = 0x9E3779B97F4A7C15ull;  // odd: the polynomial rolls modulo 2^64

__host__ __device__ inline uint64_t poly(const uint8_t *s, int k) {
  uint64_t p = 0;
  for (int j = 0; j < k; ++j) p = p * kBase + s[j];
  return p;
}
// from the k-mer that starts with `out` to the next one, which ends with `in`; top is kBase^(k - 1)
__host__ __device__ inline uint64_t roll(uint64_t p, uint8_t out, uint8_t in, uint64_t top) {
  return (p - out * top) * kBase + in;
}
__host__ __device__ inline uint64_t mix64(uint64_t x) {  // murmur3's finalizer
  x ^= x >> 33;
  x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33;
  x *= 0xC4CEB9FE1A85EC53ull;
  x ^= x >> 33;
  return x;
}
// the stored key of a k-mer: never 0, which marks an empty slot
__host__ __device__ inline uint64_t fingerprint(uint64_t p, uint64_t fp_mask) {
  const uint64_t f = mix64(p) & fp_mask;
  return f ? f : 1;
}

}  // namespace dbg
}  // namespace gb
