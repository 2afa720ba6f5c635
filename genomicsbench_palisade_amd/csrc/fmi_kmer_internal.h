// fmi_kmer_internal.h -- the bit arithmetic of the k-mer leg, one copy for the host path and the kernels.
// Reads are packed 32 bases a uint64, base j of a read in bits 63 - 2 (j % 32) and the bit below of word
// j / 32, so a k-mer's 2k-bit big-endian code is a contiguous window of at most two words. Every read starts
// at a word of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gb {
namespace kmer {

// the 2k-bit code of the k-mer at base p of a read whose words begin at w
__host__ __device__ inline uint64_t window(const uint64_t *w, int64_t p, int k) {
  const int64_t i = p >> 5;
  const int s = (int)(p & 31) * 2;
  uint64_t x = w[i] << s;
  if ((int)(p & 31) + k > 32) x |= w[i + 1] >> (64 - s);  // s >= 4 here: k <= 31
  return x >> (64 - 2 * k);
}

// reverse complement: complement every base, reverse the order of the 2-bit groups, drop the unused bits
__host__ __device__ inline uint64_t revcomp(uint64_t x, int k) {
#ifdef __HIP_DEVICE_COMPILE__
  uint64_t y = __brevll(~x);  // reverses the bits inside each group too: swap them back
  y = ((y >> 1) & 0x5555555555555555ull) | ((y & 0x5555555555555555ull) << 1);
#else
  uint64_t y = ~x;
  y = ((y >> 2) & 0x3333333333333333ull) | ((y & 0x3333333333333333ull) << 2);
  y = ((y >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((y & 0x0F0F0F0F0F0F0F0Full) << 4);
  y = __builtin_bswap64(y);
#endif
  return y >> (64 - 2 * k);
}

// the canonical code, and whether the reverse complement was strictly smaller (Kmer::standardForm)
__host__ __device__ inline uint64_t canonical(uint64_t x, int k, bool *rev) {
  const uint64_t r = revcomp(x, k);
  *rev = r < x;
  return *rev ? r : x;
}

// index of the last entry of off[0 .. n] that is <= v (off ascending, off[0] <= v < off[n])
__host__ __device__ inline int64_t owner(const int64_t *off, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}

// index of code in codes[0 .. n) ascending, or -1
__host__ __device__ inline int64_t find_code(const uint64_t *codes, int64_t n, uint64_t code) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (codes[mid] < code) lo = mid + 1; else hi = mid;
  }
  return lo < n && codes[lo] == code ? lo : -1;
}

}  // namespace kmer
}  // namespace gb
