// What the files of the forward persistent recurrence share beside the protocol of rnn_persist_common.h: the two constants that
// the host-side eligibility checks (rnn_persist.hip) and the weight-stationary kernels (rnn_persist_ws.hip) both read, and one
// launcher per kernel.  A launcher starts ONE slab (<= 640 caption rows) of a prepared parameter block: uic_rnn_fwd_persist_launch
// has made the checks, taken the persist gate, set row0 / Nrows / xbase / sync and cleared the sync block.
#pragma once
#include "rnn_persist_common.h"

namespace {
constexpr int WS_NW = 4;                  // waves of a weight-stationary workgroup, each with the whole register file of its SIMD
constexpr int DEC_NJ = 5;                 // vocabulary tiles (16 columns) per wave: 32 workgroups x 4 waves x 5 x 16 = 10240 >= V1
}  // namespace

namespace rnn_persist {
int generic_f32_launch(const UicRnnFwdParams& p, hipStream_t s);   // rnn_persist_generic.hip: rnn_fwd_persist_kernel<float>
int ws_train_launch(const UicRnnFwdParams& p, hipStream_t s);      // rnn_persist_ws.hip: rnn_fwd_persist_ws_kernel (bf16)
int ws_decode_launch(const UicRnnFwdParams& p, hipStream_t s);     // rnn_persist_ws.hip: rnn_dec_persist_ws_kernel (bf16)
}  // namespace rnn_persist
