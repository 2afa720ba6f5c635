// bsw_global_internal.h -- what bsw_global.hip shares with bsw_gencigar.hip: the per-pair device
// descriptor, the per-(thread, device) workspace, and the entry that runs the fill and walk kernels
// on target / query bytes that already lie on the device.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gb_bsw.h"
#include "gb_common.h"

namespace gbbswg {

struct Pair {  // device descriptor, 40 B
  int64_t t_off, q_off;
  int64_t dir_off;  // first 16-bit word of this pair's direction matrix
  int32_t tlen, qlen, w, pad;
};

__host__ __device__ inline int cols_per_lane(int qlen) { return (qlen + 64) >> 6; }  // columns 0..qlen
__host__ __device__ inline int row_words(int qlen) {  // lanes owning a query column
  const int K = cols_per_lane(qlen);
  return (qlen + K - 1) / K;
}

struct Ws : gb::WsBase<3> {  // the calling thread's, through get_ws
  gb::DevBuf<uint8_t> d_tgt, d_qry;
  gb::DevBuf<Pair> d_pairs;
  gb::DevBuf<int32_t> d_out4;
  gb::DevBuf<uint16_t> d_dir;
  gb::DevBuf<uint32_t> d_pool;
  gb::DevBuf<unsigned int> d_ctl;  // [0] fill work counter, [1] pool operations used, [2] first clamped pair
  float fill_ms = 0.f, walk_ms = 0.f;
};

int get_ws(int dev, Ws **out);

// Work a caller adds to every chunk of run_resident. enqueue() runs after the chunk's walk kernel
// was launched on `stream` and before the chunk's one host synchronisation: d_pairs[0..m) are the
// chunk's descriptors (pairs lo .. lo+m of the call), d_out4 their {score, n_cigar, nm, pool offset}
// and d_pool the chunk's operations, all valid for work enqueued on the same stream. collect() runs
// after that synchronisation. A non-zero return ends the call with that status.
struct ChunkHook {
  virtual ~ChunkHook() = default;
  virtual int enqueue(hipStream_t stream, int64_t lo, int64_t m, const Pair *d_pairs, const int32_t *d_out4,
                      const uint32_t *d_pool) = 0;
  virtual int collect(int64_t lo, int64_t m) = 0;
};

// gb_bsw_global behind its validation and upload: pairs[p].idr / idq are offsets into d_tgt / d_qry,
// device memory that work on W->stream may read. Chunking, outputs and the capacity rule are those
// of gb_bsw_global (include/gb_bsw.h); `who` names the public entry in error texts. The kernel times
// are added to *fill_ms / *walk_ms. hook (may be null) is called once per chunk, only when cigar is
// given.
int run_resident(Ws *W, const char *who, const gb_bsw_params *params, gb_bsw_gpair *pairs, int64_t n,
                 const uint8_t *d_tgt, const uint8_t *d_qry, uint32_t *cigar, int64_t cigar_cap, int64_t *cigar_used,
                 float *fill_ms, float *walk_ms, ChunkHook *hook);

}  // namespace gbbswg
