// bsw_local_internal.h -- what bsw_local.hip shares with bsw_matesw.hip: the per-pair device
// descriptor, the per-(thread, device) workspace, and the entry that runs the local kernel on
// descriptors, target and query bytes that already lie on the device.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gb_bsw.h"
#include "gb_common.h"

namespace gbbswl {

struct Pair {  // device descriptor, 32 B
  int64_t t_off, q_off;
  int32_t tlen, qlen, xtra, pad;
};

// entries a pass over tlen rows can append: never on two adjacent rows (ksw.c:193)
__host__ __device__ inline int64_t list_entries(int tlen) { return (tlen + 1) / 2 + 1; }

struct Ws : gb::WsBase<2> {  // the calling thread's, through get_ws
  gb::DevBuf<uint8_t> d_tgt, d_qry;
  gb::DevBuf<Pair> d_pairs;
  gb::DevBuf<int32_t> d_out8;
  gb::DevBuf<uint32_t> d_list;
  gb::DevBuf<unsigned int> d_ctl;  // [0] work counter
  gb::PinnedBuf<Pair> h_pairs;
  gb::PinnedBuf<int32_t> h_out8;
  float kernel_ms = 0.f;
};

int get_ws(int dev, Ws **out);

// One launch of the local kernel behind gb_bsw_local's validation and upload, on W->stream and without
// a host synchronisation: d_pairs[0 .. m) are device descriptors whose t_off / q_off are offsets into
// d_tgt / d_qry, d_out8 receives {score, te, qe, score2, te2, tb, qb, 0} per pair, list_cap is
// list_entries() of the longest target among the pairs that carry GB_KSW_XSUBO (1 when none does).
// A descriptor with tlen == 0 runs no row and reads no target byte: score 0, te -1, qe 0, and with
// GB_KSW_XSUBO and a threshold >= 1 no start pass. e0 / e1 (may be null) are recorded around the
// launch as gb_bsw_local records them.
int run_resident(Ws *W, const gb_bsw_params *params, int max_mat, const Pair *d_pairs, int64_t m, const uint8_t *d_tgt,
                 const uint8_t *d_qry, int32_t *d_out8, int64_t list_cap, hipEvent_t e0, hipEvent_t e1);

}  // namespace gbbswl
