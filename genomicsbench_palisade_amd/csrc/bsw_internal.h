// bsw_internal.h -- what bsw.hip shares with bsw_chain2aln.hip: the entry that plans and runs the
// extension kernels on target / query bytes that already lie on the device.
#pragma once
#include <cstdint>

#include "../../include/gb_bsw.h"

namespace gbbsw {

// gb_bsw_get_scores16 behind its upload: pairs[p].idr / idq are offsets into d_tgt / d_qry, device
// memory of tgt_bytes / qry_bytes that is complete before the call (the kernels run on the streams of
// the calling thread's cached batch, which wait for no other stream). The launch plan (validation,
// kernel variant, sort key, order) is the one gb_bsw_batch_create builds. out6 receives
// {score, qle, tle, gtle, gscore, max_off} per pair once the kernels are done: the call is synchronous.
// *d_out6 (may be null) receives where the same results lie on the device, in pair order; they stay
// there until the calling thread's next extension call on this device. The kernel time is added to
// *kernel_ms (may be null). Callers that must not pay for an empty round do not call with n == 0.
int run_resident(const gb_bsw_params *params, const gb_seqpair *pairs, int64_t n, const uint8_t *d_tgt,
                 int64_t tgt_bytes, const uint8_t *d_qry, int64_t qry_bytes, int32_t *out6, const int32_t **d_out6,
                 float *kernel_ms);

}  // namespace gbbsw
