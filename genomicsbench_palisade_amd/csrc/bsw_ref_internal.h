// bsw_ref_internal.h -- the device-resident packed reference (gb_ref) and the routine that unpacks
// it, shared by bsw_gencigar.hip (which owns gb_ref's C ABI) and bsw_chain2aln.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/gb_bsw_ref.h"
#include "gb_common.h"

// The packed reference. The host copy lives until the first device use (ensure_device).
struct gb_ref {
  int64_t l_pac = 0;
  std::mutex mu;
  std::vector<uint8_t> host;
  int device = -1;
  int64_t n_words = 0;  // 32-bit words on the device: the pac, zero-padded, plus two words of slack
  gb::DevBuf<uint32_t> d_pac;
};

namespace gbgc {

// Upload on first use; afterwards the reference belongs to that device.
int ensure_device(gb_ref *R, int dev);

// 16 bases starting at pac index b0 (which may lie outside [0, l_pac) in a slice's padding: the
// word indices are clamped, the bases there mean nothing), first base in bits 31-30
__device__ __forceinline__ uint32_t bases16(const uint32_t *pac, int64_t n_words, int64_t b0) {
  const int64_t wi = b0 >> 4;
  const int64_t i0 = min(max(wi, (int64_t)0), n_words - 1), i1 = min(max(wi + 1, (int64_t)0), n_words - 1);
  // base l sits in byte l >> 2 at shift (~l & 3) << 1: most significant first once the bytes are swapped
  const uint64_t v = (uint64_t)__builtin_bswap32(pac[i0]) << 32 | __builtin_bswap32(pac[i1]);
  return (uint32_t)((v << (2 * (int)(b0 & 15))) >> 32);
}

// One wave writes len byte codes to dst (16-byte aligned, room for len rounded up to 16): 16 bases per
// lane and one 16-byte store each. Forward: dst[k] = base src + k; backward: dst[k] = base src - k.
// cx is 0, or all ones to complement (3 - x == ~x on two bits).
__device__ __forceinline__ void fetch_bases(const uint32_t *pac, int64_t n_words, int64_t src, int32_t len, bool back,
                                            uint32_t cx, uint8_t *dst, int lane) {
  const int64_t nch = ((int64_t)len + 15) >> 4;
  for (int64_t c = lane; c < nch; c += 64) {
    const int64_t b0 = back ? src - 16 * c - 15 : src + 16 * c;
    const uint32_t v = bases16(pac, n_words, b0) ^ cx;
    uint32_t o[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      uint32_t w = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int j = 4 * d + k;
        const int sh = back ? 2 * j : 30 - 2 * j;
        w |= ((v >> sh) & 3u) << (8 * k);
      }
      o[d] = w;
    }
    *reinterpret_cast<uint4 *>(dst + 16 * c) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// The reversed copy of a query of qlen bytes, four bytes per store; dst is 4-byte aligned with room
// for qlen rounded up to 4.
__device__ __forceinline__ void reverse_query(const uint8_t *q, int32_t qlen, uint8_t *dst, int lane) {
  for (int g = lane; 4 * g < qlen; g += 64) {
    uint32_t w = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = 4 * g + b;
      if (i < qlen) w |= (uint32_t)q[qlen - 1 - i] << (8 * b);
    }
    *reinterpret_cast<uint32_t *>(dst + 4 * g) = w;
  }
}

}  // namespace gbgc
