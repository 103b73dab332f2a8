// What the decoder's translation units call across file boundaries: decoder.hip (entry points, per-step kernels),
// decoder_persist.hip (plan queries, cluster kernels with LDS-resident tiles), decoder_stream.hip (cluster kernels with
// streamed tiles).  The plans and the launch path the two kernel files share are in decoder_plan.h.
#pragma once
#include "common.h"

inline size_t align_up256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- decoder_persist.hip
// What a shape gets under the current plan preference (asr_att_decoder_set_persistent) and what has to hold for either
// preference, because it can be switched between calls.  kind 0: per-step kernels, 1: LDS-resident tiles, 2: streamed tiles.
struct DecPlanInfo {
    int kind;
    int tiles, tiles_max;       // backward: tiles per utterance of the chosen plan (0: none) / the larger count of both plans
    size_t work_bytes;          // work area: the larger of both plans
};
DecPlanInfo dec_fwd_plan_info(const asr_dec_dims_t& d);
DecPlanInfo dec_bwd_plan_info(const asr_dec_dims_t& d);
// Both return ASR_OK when the whole loop was launched (resident or streamed tiles), 1 when the configuration has no
// persistent plan, negative on error.  `work`: 256-byte aligned, its first 4 KB are the status block of the launch.
int dec_fwd_persistent(const asr_dec_dims_t& d, const asr_dec_weights_t& w, const asr_dec_state_t& s, const float* enc,
                       const int64_t* enc_len, void* work, size_t work_bytes, hipStream_t st);
// What the forward did, for the backward: asr_att_decoder_fwd leaves 1 in this word of the status block of state->work when
// dec_fwd_persistent launched the loop (ASR_OK) and 0 when the per-step kernels ran (switch off, no plan, area too small, launch
// declined for residency, no teacher).  The word lies in the last 64 bytes of the block, beside the launch epoch
// (decoder_cluster.h, EPOCH_WORD = 1008), which no launcher clears.  asr_att_decoder_bwd reads it on the device
// (ctx_from_saved_att_kernel): it does not repeat the forward's decision from switches that may have changed since.
constexpr int DEC_FWD_LAUNCHED_WORD = 1009;
constexpr size_t DEC_STATUS_BYTES = 4096;
// dhs: (B,L,Dd) gradient wrt h from the output layer; wcatT: ((Dd+E+Dd) x 4Dd) fp32 transposed [W_ih | W_hh]; wqT: (Dd x A).
// *dgates_out: (B*L, 4Dd) gate pre-activation gradients inside `work`.
int dec_bwd_persistent(const asr_dec_dims_t& d, const asr_dec_weights_t& w, const asr_dec_state_t& s, const int64_t* enc_len,
                       const float* dhs, float* dxin, float* dq, float* dkey, float* slots, int slot, const float* wcatT, const float* wqT,
                       void* work, size_t work_bytes, float** dgates_out, hipStream_t st);
// the gate gradients the persistent backward of the chosen plan leaves in its work area
float* dec_bwd_dgates(const asr_dec_dims_t& d, void* work);

// ---- decoder_stream.hip (reached through the two launchers above)
int dec_fwd_streamed(const asr_dec_dims_t& d, const asr_dec_weights_t& w, const asr_dec_state_t& s, const float* enc,
                     const int64_t* enc_len, void* work, size_t work_bytes, hipStream_t st);
int dec_bwd_streamed(const asr_dec_dims_t& d, const asr_dec_weights_t& w, const asr_dec_state_t& s, const int64_t* enc_len,
                     const float* dhs, float* dxin, float* dq, float* dkey, float* slots, int slot, const float* wcatT, const float* wqT,
                     void* work, size_t work_bytes, float** dgates_out, hipStream_t st);
