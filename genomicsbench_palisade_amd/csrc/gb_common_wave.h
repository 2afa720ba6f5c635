// gb_common_wave.h -- wave64 DPP primitives shared by the kernels of every leg: inclusive scans, the
// one-lane shift, the wave maximum and the workgroup-wide add scan. Device only. A scan's identity
// fills the lanes a DPP step has no source for and is a template parameter: each kernel passes its
// own "minus infinity".
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gb {

// Wave-wide inclusive scans: Hillis-Steele with row_shr 1/2/4/8 inside the 16-lane rows, then
// row_bcast 15 (row mask 0b1010) and row_bcast 31 (row mask 0b1100) across them.
template <int kIdentity>
__device__ __forceinline__ int scan_max(int v) {
  v = max(v, __builtin_amdgcn_update_dpp(kIdentity, v, 0x111, 0xF, 0xF, false));  // row_shr:1
  v = max(v, __builtin_amdgcn_update_dpp(kIdentity, v, 0x112, 0xF, 0xF, false));  // row_shr:2
  v = max(v, __builtin_amdgcn_update_dpp(kIdentity, v, 0x114, 0xF, 0xF, false));  // row_shr:4
  v = max(v, __builtin_amdgcn_update_dpp(kIdentity, v, 0x118, 0xF, 0xF, false));  // row_shr:8
  v = max(v, __builtin_amdgcn_update_dpp(kIdentity, v, 0x142, 0xA, 0xF, false));  // row_bcast:15
  v = max(v, __builtin_amdgcn_update_dpp(kIdentity, v, 0x143, 0xC, 0xF, false));  // row_bcast:31
  return v;
}
template <int kIdentity>
__device__ __forceinline__ int scan_min(int v) {
  v = min(v, __builtin_amdgcn_update_dpp(kIdentity, v, 0x111, 0xF, 0xF, false));
  v = min(v, __builtin_amdgcn_update_dpp(kIdentity, v, 0x112, 0xF, 0xF, false));
  v = min(v, __builtin_amdgcn_update_dpp(kIdentity, v, 0x114, 0xF, 0xF, false));
  v = min(v, __builtin_amdgcn_update_dpp(kIdentity, v, 0x118, 0xF, 0xF, false));
  v = min(v, __builtin_amdgcn_update_dpp(kIdentity, v, 0x142, 0xA, 0xF, false));
  v = min(v, __builtin_amdgcn_update_dpp(kIdentity, v, 0x143, 0xC, 0xF, false));
  return v;
}
__device__ __forceinline__ int scan_add(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);
  return v;
}

// Lane l takes lane l-1's v and lane 0 takes lane0 (wave_shr:1; bound_ctrl is off, so lane 0 keeps
// the `old` operand).
__device__ __forceinline__ int wave_shr1(int v, int lane0) {
  return __builtin_amdgcn_update_dpp(lane0, v, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ uint64_t wave_shr1(uint64_t v, uint64_t lane0) {
  const int lo = wave_shr1((int)(uint32_t)v, (int)(uint32_t)lane0);
  const int hi = wave_shr1((int)(uint32_t)(v >> 32), (int)(uint32_t)(lane0 >> 32));
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

template <int kIdentity>
__device__ __forceinline__ int wave_max(int v) {
  return __builtin_amdgcn_readlane(scan_max<kIdentity>(v), 63);
}

// Exclusive add scan of v over the kThreads lanes of the workgroup, and the workgroup's total; lds has
// kThreads / 64 ints. Every thread of the workgroup calls it.
template <int kThreads>
__device__ __forceinline__ int block_scan_excl(int v, int *total, int *lds) {
  const int inc = scan_add(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 63) lds[threadIdx.x >> 6] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int i = 0; i < kThreads / 64; ++i) {
    const int t = lds[i];
    if (i < (int)(threadIdx.x >> 6)) base += t;
    tot += t;
  }
  *total = tot;
  return base + inc - v;
}

}  // namespace gb
