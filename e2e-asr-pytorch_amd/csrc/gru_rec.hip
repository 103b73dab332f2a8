// Time recurrence of a single-direction nn.GRU, launch per step: the RNN language model with module 'GRU' (reference
// src/lm.py:18, nn.GRU(batch_first=True), zero initial state in training, a given state per hypothesis in beam search).
// The input projections gi = x W_ih^T + b_ih for all steps come from asr_gemm beforehand; each step adds
// gh = h_{t-1} W_hh^T + b_hh with MFMA and applies nn.GRU's cell
//     r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n), h = (1 - z) n + z h_{t-1}
// (gh_n stays separate from gi_n: r scales only the recurrent part).
//
// Tiling (both directions of the pass): a block of 4 waves owns 16 hidden units x 16 batch rows.  Batch rows are the M side
// of the 16x16 MFMA tile, hidden units the N side, the reduction is split k-step-wise across the 4 waves and summed in LDS.
// Forward: every wave keeps three accumulators (r, z, n rows of W_hh for the same 16 units), so the gate epilogue of one
// (row, unit) reads its three sums from LDS with no shuffles.  Backward: one accumulator, dgh_{t+1} (B x 3H) against the
// transposed W_hh (H, 3H), so both MFMA operands are K-contiguous.
// Any H >= 1 is handled (ragged tails go through dot_rows' clamped loads); the host refuses H above GRU_REC_MAX_H.
#include "common.h"

namespace {

constexpr int GRU_WAVES = 4;
constexpr int GRU_REC_MAX_H = 2048;

struct GruRecP {
    const float* gi;     // fwd: (B,T,3H) = x W_ih^T + b_ih
    const float* whh;    // fwd: (3H,H) weight_hh as stored;  bwd: transposed copy (H,3H)
    const float* bhh;    // fwd: (3H)
    const float* h0;     // (B,H) initial state, or null = zeros
    float* y;            // (B,T,H) h_t; fwd writes it, bwd reads h_{t-1} from it
    float* saved;        // (B,T,4H) r | z | n | gh_n (fwd: optional)
    const float* dy;     // bwd: (B,T,H) gradient wrt y
    float* dgi;          // bwd: (B,T,3H) gradient wrt gi
    float* dgh;          // bwd: (B,T,3H) gradient wrt gh (pre-activation of the recurrent part, bias included)
    float* carry;        // bwd: (B,H) dh_{t+1} z_{t+1}, the direct part of the carried gradient
    float* dh0;          // bwd: (B,H) gradient wrt h0, optional
    int B, T, H;
    int vec;             // H % 4 == 0 and every row operand 16-byte aligned: vector loads in dot_rows
};

__device__ __forceinline__ float gru_hprev(const GruRecP& p, int b, int t, int j) {
    if (t > 0) return p.y[((long)b * p.T + t - 1) * p.H + j];
    return p.h0 ? p.h0[(long)b * p.H + j] : 0.f;
}

// one step t: grid (cdiv(H,16), cdiv(B,16)), block 256
template <bool BF16>
__global__ __launch_bounds__(256) void gru_rec_fwd_step(GruRecP p, int t) {
    __shared__ float red[GRU_WAVES][3][256];
    const int H = p.H, T = p.T;
    const int j0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, q = lane >> 4;
    const bool jok = j0 + n < H;
    const int jc = jok ? j0 + n : 0;
    const float* hsrc = (t > 0) ? p.y + (long)(t - 1) * H : p.h0;
    const long hld = (t > 0) ? (long)T * H : (long)H;
    f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (hsrc) {
        const int ab = m0 + n;                       // A row = batch index
        const bool aok = ab < p.B;
        const float* hrow = hsrc + (long)(aok ? ab : 0) * hld;
#pragma unroll
        for (int g = 0; g < 3; ++g)
            acc[g] = dot_rows<BF16>(hrow, aok, p.whh + ((long)g * H + jc) * H, jok, H, wave, GRU_WAVES, p.vec != 0, acc[g]);
    }
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][g][(4 * q + r) * 16 + n] = acc[g][r];
    __syncthreads();
    const int b = m0 + (tid >> 4), j = j0 + (tid & 15);
    if (b >= p.B || j >= H) return;
    float gh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) gh[g] = p.bhh[g * H + j] + red[0][g][tid] + red[1][g][tid] + red[2][g][tid] + red[3][g][tid];
    const float* gi = p.gi + ((long)b * T + t) * 3 * H;
    const float r = sigmoidf_(gi[j] + gh[0]);
    const float z = sigmoidf_(gi[H + j] + gh[1]);
    const float nn_ = tanhf(gi[2 * H + j] + r * gh[2]);
    const float hp = gru_hprev(p, b, t, j);
    p.y[((long)b * T + t) * H + j] = (1.f - z) * nn_ + z * hp;
    if (p.saved) {
        float* sv = p.saved + ((long)b * T + t) * 4 * H;
        sv[j] = r; sv[H + j] = z; sv[2 * H + j] = nn_; sv[3 * H + j] = gh[2];
    }
}

// one step t (T-1 down to 0), then optionally t = -1, which only forms dh0.  dh_t = dy_t + carry + dgh_{t+1} W_hh.
template <bool BF16>
__global__ __launch_bounds__(256) void gru_rec_bwd_step(GruRecP p, int t) {
    __shared__ float red[GRU_WAVES][256];
    const int H = p.H, T = p.T, K = 3 * H;
    const int j0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, q = lane >> 4;
    const bool later = t < T - 1;                    // a step t+1 exists: recurrent part of dh_t
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (later) {
        const bool jok = j0 + n < H;
        const int ab = m0 + n;
        const bool aok = ab < p.B;
        const float* grow = p.dgh + ((long)(aok ? ab : 0) * T + t + 1) * K;
        acc = dot_rows<BF16>(grow, aok, p.whh + (long)(jok ? j0 + n : 0) * K, jok, K, wave, GRU_WAVES, p.vec != 0, acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][(4 * q + r) * 16 + n] = acc[r];
    __syncthreads();
    const int b = m0 + (tid >> 4), j = j0 + (tid & 15);
    if (b >= p.B || j >= H) return;
    const long bj = (long)b * H + j;
    float dh = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid] + (later ? p.carry[bj] : 0.f);
    if (t < 0) { p.dh0[bj] = dh; return; }
    dh += p.dy[((long)b * T + t) * H + j];
    const float* sv = p.saved + ((long)b * T + t) * 4 * H;
    const float r = sv[j], z = sv[H + j], nn_ = sv[2 * H + j], ghn = sv[3 * H + j];
    const float hp = gru_hprev(p, b, t, j);
    const float dpn = dh * (1.f - z) * (1.f - nn_ * nn_);
    const float dpz = dh * (hp - nn_) * z * (1.f - z);
    const float dpr = dpn * ghn * r * (1.f - r);
    const long g0 = ((long)b * T + t) * K + j;
    p.dgi[g0] = dpr; p.dgi[g0 + H] = dpz; p.dgi[g0 + 2 * H] = dpn;
    p.dgh[g0] = dpr; p.dgh[g0 + H] = dpz; p.dgh[g0 + 2 * H] = dpn * r;
    p.carry[bj] = dh * z;
}

// w (3H,H) -> wt (H,3H)
__global__ void gru_transpose_whh_kernel(const float* __restrict__ w, float* __restrict__ wt, int H) {
    const long K = 3L * H, total = K * H;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long j = i / K, k = i % K;
        wt[i] = w[k * H + j];
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

size_t carry_offset_floats(int H) { return ((size_t)3 * H * H + 63) / 64 * 64; }

}  // namespace

extern "C" size_t asr_gru_rec_workspace_bytes(int B, int H) {
    if (B <= 0 || H <= 0) return 0;
    return (carry_offset_floats(H) + (size_t)B * H) * sizeof(float);
}

extern "C" int asr_gru_rec_fwd(const float* gi, const float* whh, const float* bhh, const float* h0, int B, int T, int H, int prec,
                               float* y, float* saved, asr_stream_t stream) {
    ASR_REQUIRE(gi && whh && bhh && y, ASR_E_ARG, "asr_gru_rec_fwd: null pointer");
    ASR_REQUIRE(B > 0 && T > 0 && H > 0 && (prec == ASR_F32 || prec == ASR_BF16), ASR_E_ARG, "asr_gru_rec_fwd: bad args");
    ASR_REQUIRE(H <= GRU_REC_MAX_H, ASR_E_UNSUPPORTED, "asr_gru_rec_fwd: hidden size %d above %d", H, GRU_REC_MAX_H);
    ASR_REQUIRE(!(h0 && h0 == y), ASR_E_ARG, "asr_gru_rec_fwd: h0 must not alias y");
    GruRecP p{};
    p.gi = gi; p.whh = whh; p.bhh = bhh; p.h0 = h0; p.y = y; p.saved = saved;
    p.B = B; p.T = T; p.H = H;
    p.vec = (H % 4) == 0 && al16(whh) && al16(y) && (!h0 || al16(h0));
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(cdiv(H, 16), cdiv(B, 16)), block(256);
    for (int t = 0; t < T; ++t) {
        if (prec == ASR_BF16) hipLaunchKernelGGL(gru_rec_fwd_step<true>, grid, block, 0, st, p, t);
        else                  hipLaunchKernelGGL(gru_rec_fwd_step<false>, grid, block, 0, st, p, t);
    }
    ASR_LAUNCH_CHECK("asr_gru_rec_fwd");
    return ASR_OK;
}

extern "C" int asr_gru_rec_bwd(const float* dy, const float* y, const float* saved, const float* h0, const float* whh, int B, int T, int H,
                               int prec, float* dgi, float* dgh, float* dh0, void* workspace, size_t workspace_bytes, asr_stream_t stream) {
    ASR_REQUIRE(dy && y && saved && whh && dgi && dgh && workspace, ASR_E_ARG, "asr_gru_rec_bwd: null pointer");
    ASR_REQUIRE(B > 0 && T > 0 && H > 0 && (prec == ASR_F32 || prec == ASR_BF16), ASR_E_ARG, "asr_gru_rec_bwd: bad args");
    ASR_REQUIRE(H <= GRU_REC_MAX_H, ASR_E_UNSUPPORTED, "asr_gru_rec_bwd: hidden size %d above %d", H, GRU_REC_MAX_H);
    ASR_REQUIRE(workspace_bytes >= asr_gru_rec_workspace_bytes(B, H), ASR_E_ARG, "asr_gru_rec_bwd: workspace too small");
    ASR_REQUIRE(al16(workspace), ASR_E_ARG, "asr_gru_rec_bwd: unaligned workspace");
    hipStream_t st = (hipStream_t)stream;
    float* wt = (float*)workspace;
    GruRecP p{};
    p.whh = wt; p.h0 = h0; p.y = const_cast<float*>(y); p.saved = const_cast<float*>(saved); p.dy = dy;
    p.dgi = dgi; p.dgh = dgh; p.carry = wt + carry_offset_floats(H); p.dh0 = dh0;
    p.B = B; p.T = T; p.H = H;
    p.vec = (H % 4) == 0 && al16(dgh);
    hipLaunchKernelGGL(gru_transpose_whh_kernel, dim3(256), dim3(256), 0, st, whh, wt, H);
    dim3 grid(cdiv(H, 16), cdiv(B, 16)), block(256);
    for (int t = T - 1; t >= (dh0 ? -1 : 0); --t) {
        if (prec == ASR_BF16) hipLaunchKernelGGL(gru_rec_bwd_step<true>, grid, block, 0, st, p, t);
        else                  hipLaunchKernelGGL(gru_rec_bwd_step<false>, grid, block, 0, st, p, t);
    }
    ASR_LAUNCH_CHECK("asr_gru_rec_bwd");
    return ASR_OK;
}
