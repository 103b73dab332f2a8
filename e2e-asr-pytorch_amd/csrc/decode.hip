// Small kernels around the decoding and sampling loops (reference src/lm.py:27-37, src/asr.py:151-158); the CTC prefix scorer
// is in ctc_prefix.hip, the beam bookkeeping in beam_step.hip:
//   asr_lstm_cell        : pointwise LSTM cell on pre-computed gate sums (RNN-LM step; the two projections are asr_gemm)
//   asr_gather_rows      : row gather (embedding lookup, state re-ordering after pruning)
//   asr_masked_copy_rows : dst[r,:] = src[r,:] where mask[r] (CTC-only search: the LM rows of the slots that were extended)
//   asr_sample_tokens    : one token per row drawn from softmax(logits) (scheduled sampling)
#include "common.h"

namespace {

__global__ void lstm_cell_kernel(const float* __restrict__ pre, const float* __restrict__ bih, const float* __restrict__ bhh,
                                 const float* __restrict__ c_prev, float* __restrict__ h, float* __restrict__ c, int N, int D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * D) return;
    const int n = i / D, j = i % D;
    const float* p = pre + (long)n * 4 * D;
    const float gi = sigmoidf_(p[j] + bih[j] + bhh[j]);
    const float gf = sigmoidf_(p[D + j] + bih[D + j] + bhh[D + j]);
    const float gg = tanhf(p[2 * D + j] + bih[2 * D + j] + bhh[2 * D + j]);
    const float go = sigmoidf_(p[3 * D + j] + bih[3 * D + j] + bhh[3 * D + j]);
    const float cn = gf * (c_prev ? c_prev[i] : 0.f) + gi * gg;
    c[i] = cn;
    h[i] = go * tanhf(cn);
}

__global__ void gather_rows_kernel(const float* __restrict__ src, const int64_t* __restrict__ idx, float* __restrict__ dst,
                                   int rows, int width, long src_ld, long dst_ld, int nsrc) {
    const long total = (long)rows * width;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int r = (int)(i / width), k = (int)(i % width);
        long s = idx[r];
        s = s < 0 ? 0 : (s >= nsrc ? nsrc - 1 : s);
        dst[(long)r * dst_ld + k] = src[s * src_ld + k];
    }
}

__global__ void masked_copy_rows_kernel(const float* __restrict__ src, const int* __restrict__ mask, float* __restrict__ dst,
                                        int rows, int width, long src_ld, long dst_ld) {
    const long total = (long)rows * width;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int r = (int)(i / width), k = (int)(i % width);
        if (mask[r]) dst[(long)r * dst_ld + k] = src[(long)r * src_ld + k];
    }
}

// Scheduled sampling (reference src/asr.py:151-158): token ~ Categorical(softmax(logits)) per row, inverse-CDF with one
// Philox uniform per row (seed, row); written to out[row * out_ld] (the decoder's token table column of the next step).
__global__ __launch_bounds__(64) void sample_tokens_kernel(const float* __restrict__ logits, long ld, long long* __restrict__ out, long out_ld,
                                                           int V, uint64_t seed) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const float* x = logits + (long)row * ld;
    float m = -INFINITY;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, x[v]);
    m = wave_max(m);
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += expf(x[v] - m);
    s = wave_sum(s);
    uint32_t r[4];
    philox4x32((uint32_t)row, 0u, 0x53414d50u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const float target = ((float)(r[0] >> 8) + 0.5f) * (1.0f / 16777216.0f) * s;
    // running sum in token order: chunks of 64 tokens, inclusive scan inside the wave
    float base = 0.f;
    int pick = V - 1;
    bool found = false;
    for (int v0 = 0; v0 < V && !found; v0 += 64) {
        const int v = v0 + lane;
        float e = v < V ? expf(x[v] - m) : 0.f;
        float inc = e;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const float n = __shfl_up(inc, o); if (lane >= o) inc += n; }
        const unsigned long long hit = __ballot(v < V && base + inc >= target);
        if (hit) { pick = v0 + __builtin_ctzll(hit); found = true; }
        base += __shfl(inc, 63);
    }
    if (lane == 0) out[(long)row * out_ld] = pick;
}

}  // namespace

extern "C" int asr_lstm_cell(const float* gates_pre, const float* bias_ih, const float* bias_hh, const float* c_prev,
                             float* h, float* c, int N, int D, asr_stream_t stream) {
    ASR_REQUIRE(gates_pre && bias_ih && bias_hh && h && c && N > 0 && D > 0, ASR_E_ARG, "asr_lstm_cell: bad args");
    hipLaunchKernelGGL(lstm_cell_kernel, dim3(cdiv((long)N * D, 256)), dim3(256), 0, (hipStream_t)stream, gates_pre, bias_ih, bias_hh,
                       c_prev, h, c, N, D);
    ASR_LAUNCH_CHECK("asr_lstm_cell");
    return ASR_OK;
}

extern "C" int asr_gather_rows(const float* src, const int64_t* idx, float* dst, int rows, int width, long src_ld, long dst_ld,
                               int nsrc, asr_stream_t stream) {
    ASR_REQUIRE(src && idx && dst && rows > 0 && width > 0 && nsrc > 0, ASR_E_ARG, "asr_gather_rows: bad args");
    long g = ((long)rows * width + 255) / 256; if (g > 4096) g = 4096;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, src, idx, dst, rows, width, src_ld, dst_ld, nsrc);
    ASR_LAUNCH_CHECK("asr_gather_rows");
    return ASR_OK;
}

extern "C" int asr_masked_copy_rows(const float* src, const int* mask, float* dst, int rows, int width, long src_ld, long dst_ld,
                                    asr_stream_t stream) {
    ASR_REQUIRE(src && mask && dst, ASR_E_ARG, "asr_masked_copy_rows: null pointer");
    ASR_REQUIRE(rows > 0 && width > 0 && src_ld >= width && dst_ld >= width, ASR_E_ARG,
                "asr_masked_copy_rows: bad dims rows=%d width=%d src_ld=%ld dst_ld=%ld", rows, width, src_ld, dst_ld);
    long g = ((long)rows * width + 255) / 256; if (g > 4096) g = 4096;
    hipLaunchKernelGGL(masked_copy_rows_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, src, mask, dst, rows, width, src_ld, dst_ld);
    ASR_LAUNCH_CHECK("asr_masked_copy_rows");
    return ASR_OK;
}

extern "C" int asr_sample_tokens(const float* logits, long ld, int64_t* out, long out_ld, int rows, int V, uint64_t seed, asr_stream_t stream) {
    ASR_REQUIRE(logits && out && rows > 0 && V > 1 && ld >= V, ASR_E_ARG, "asr_sample_tokens: bad args");
    hipLaunchKernelGGL(sample_tokens_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, logits, ld, (long long*)out, out_ld, V, seed);
    ASR_LAUNCH_CHECK("asr_sample_tokens");
    return ASR_OK;
}
