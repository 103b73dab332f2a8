// Host-side plan of the encoder LSTM recurrence: which kernels run for (B, H, ND, precision) under the current
// asr_lstm_set_persistent mode and how many workspace bytes they need.  Pure host arithmetic, no device call: asr_lstm_plan,
// asr_lstm_workspace_bytes, asr_lstm16_workspace_bytes and the launches of asr_lstm_fwd / asr_lstm_bwd / asr_lstm16_* (lstm.hip)
// all ask here.  Each kernel generation contributes ONE function, defined next to its kernels; the rest is derived.
#pragma once
#include <stddef.h>
#include <hip/hip_runtime.h>

// One pass (forward / backward) of one generation.  ok: the generation has a kernel for it.  bytes: status block + exchange
// buffers of the pass, what its launcher clears and the least the workspace must hold.
struct LstmPass { bool ok; size_t bytes; };

// lstm_persist.hip (fp32 storage, either precision): plan_fwd / plan_bwd and the table of template instantiations.  `bytes` is
// also given where `ok` is false - forward: for every shape; backward: where plan_bwd has a plan but no kernel is
// instantiated - because asr_lstm_workspace_bytes has always counted those.
LstmPass lstm_gen1_pass(int B, int H, int ND, bool bf16, bool bwd);
// lstm_persist2.hip (fp32 storage): bf16 && B <= 16 && H % 16 == 0 && H <= 512; bytes 0 otherwise
LstmPass lstm_gen2_pass(int B, int H, int ND, bool bf16, bool bwd);
// lstm_persist3.hip (bf16 storage, asr_lstm16_*): lstm3_shape_ok; bytes 0 otherwise.  Whether the grid is resident beside
// `reserved_cus` is asked of the device at launch and is not part of the plan.
LstmPass lstm_gen3_pass(int B, int H, int ND, bool bwd);

// The third generation has two backward kernels: the gather form (lstm_bwd_g3: dh is exchanged, every workgroup recomputes the
// cell backward) for groups of at most 4 batch rows, the reduce-scatter form (lstm_bwd_p3) for larger ones and wherever the
// switch (ASR_LSTM3_BWD=0, lstm_gen3_set_bwd_form(0)) turns the gather form off.  lstm_gen3_pass(..., true).bytes serves both.
bool lstm_gen3_bwd_gather(int B, int H, int ND);      // the form lstm_persistent3 plans for the shape under the current switch
int lstm_gen3_set_bwd_form(int form);                 // 0 / 1 sets the switch, anything else only asks; returns the former value

// The launchers, one per generation, both passes (forward: y = h out; backward: y = dy, read-only, bias2 unused).  Generations
// 1 and 2 take a planned pass and clear its bytes of the workspace first: ASR_OK or a negative error.  Generation 3 also
// returns 1: no plan for the shape / workspace, or the grid would not be resident.
int lstm_persistent1(float* gates, const float* whh, const float* bias2, float* y, float* c, bool bwd,
                     int B, int T, int H, int ND, int prec, void* ws, hipStream_t st);
int lstm_persistent2(float* gates, const float* whh, const float* bias2, float* y, float* c, bool bwd,
                     int B, int T, int H, int ND, void* ws, hipStream_t st);
int lstm_persistent3(unsigned short* gates, const float* whh, unsigned short* y, float* c, bool bwd, int B, int T, int H, int ND,
                     void* ws, size_t ws_bytes, unsigned epoch, int reserved_cus, hipStream_t st);

// What one call can use; a query describes the ideal call.
struct LstmCall {
    bool ws_ok = true;                 // workspace given and 256-byte aligned
    size_t ws_bytes = (size_t)-1;
    bool aligned16 = true;             // gates, y and c 16-byte aligned (second generation's 16-byte accesses)
};

// Generation of one pass of the fp32-storage entry points: 0 = one launch per time step, 1, 2 = persistent kernels of that
// generation.  mode: asr_lstm_set_persistent (0 none, 1 second generation where it applies, 2 first generation only).
// The planned generation is demoted where the call cannot serve it: no usable workspace -> 0, too few bytes -> next older,
// unaligned tensors -> 1.
inline int lstm_pass_gen(int mode, int B, int H, int ND, bool bf16, bool bwd, const LstmCall& call = LstmCall()) {
    if (mode < 1 || !call.ws_ok) return 0;
    LstmPass ps = lstm_gen2_pass(B, H, ND, bf16, bwd);
    int gen = 2;
    if (mode != 1 || !call.aligned16 || !ps.ok || call.ws_bytes < ps.bytes) { ps = lstm_gen1_pass(B, H, ND, bf16, bwd); gen = 1; }
    return (ps.ok && call.ws_bytes >= ps.bytes) ? gen : 0;
}

// asr_lstm_plan: the generation of both passes of an ideal call - the second generation serves both passes or neither.
// 1 stands for the first-generation kernels WHERE THEY HAVE ONE: a pass they do not cover (lstm_gen1_pass) runs per step.
inline int lstm_plan_query(int mode, int B, int H, int ND, bool bf16) {
    if (mode < 1) return 0;
    return lstm_pass_gen(mode, B, H, ND, bf16, false) == 2 ? 2 : 1;
}

// asr_lstm_workspace_bytes: enough for either pass of any generation in either precision, the per-step backward's
// transposed W_hh + dc carry included, behind the 256-byte status block.
inline size_t lstm_workspace_bytes(int B, int H, int ND) {
    size_t n = ((size_t)ND * H * 4 * H + (size_t)ND * B * H) * sizeof(float);
    for (int k = 0; k < 4; ++k) {
        const size_t g1 = lstm_gen1_pass(B, H, ND, k & 1, k >> 1).bytes, g2 = lstm_gen2_pass(B, H, ND, k & 1, k >> 1).bytes;
        n = n > g1 ? n : g1;
        n = n > g2 ? n : g2;
    }
    return n + 256;
}
