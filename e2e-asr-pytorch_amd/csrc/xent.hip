// Token-level sequence losses of the attention decoder, forward + gradient in one pass:
//   mode 0: torch.nn.CrossEntropyLoss(ignore_index=0)  — mean over non-pad targets (bin/train_asr.py:134,245)
//   mode 1: LabelSmoothingLoss(classes, smoothing)     — mean over ALL rows, pad rows included, target
//           distribution 1-s on the label and s/(classes-1) elsewhere (src/util.py:11-25; the Solver
//           hard-codes classes=31, bin/train_asr.py:131)
// One wave per row (V <= a few thousand), fp32 log-softmax.
#include "common.h"

namespace {

struct XentP {
    const float* logits; const int64_t* tgt; long tgt_ld; int L;   // row r = b*L + t  ->  tgt[b*tgt_ld + t]
    float* dlogits; float* accum;   // accum[0..1] = sum of row losses as a 64-bit fixed-point integer (2^-32 units: integer
                                    // atomics commute, so the sum does not depend on the arrival order), accum[2] = counted rows
    long R; int V; int mode; int classes; float smoothing;
};

// row loss -> 64-bit fixed point; NaN / inf rows poison the float slot accum[3] instead (the result is then NaN anyway)
__device__ __forceinline__ void add_fixed(float* accum, long long& q, float v) {
    if (!(fabsf(v) < 1e9f)) { atomicAdd(&accum[3], v); return; }
    q += (long long)llrint((double)v * 4294967296.0);
}

// XROWS rows per wave, one pair of atomics per WORKGROUP: 2 x B*L atomics on two addresses were most of this kernel's time
// (56 us for 2880 rows at C2)
constexpr int XROWS = 4;
__global__ __launch_bounds__(256) void xent_rows_kernel(XentP p) {
    __shared__ long long s_loss[4];
    __shared__ float s_cnt[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    long long wloss = 0;                                // this wave's rows, each rounded to fixed point on its own: the total
    float wcnt = 0.f;                                   // is the same integer however rows are grouped into waves
    for (int i = 0; i < XROWS; ++i) {
        const long row = (blockIdx.x * 4L + wv) * XROWS + i;
        if (row >= p.R) break;
        const float* x = p.logits + row * p.V;
        float* dx = p.dlogits + row * p.V;
        long tg = p.tgt[(row / p.L) * p.tgt_ld + (row % p.L)];
        float m = -INFINITY;
        for (int v = lane; v < p.V; v += 64) m = fmaxf(m, x[v]);
        m = wave_max(m);
        float s = 0.f;
        for (int v = lane; v < p.V; v += 64) s += expf(x[v] - m);
        s = wave_sum(s);
        // log-softmax as (x - m) - log(sum): x - m is exact for the large terms, where m + log(sum) would round at ulp(|m|) and
        // carry that into every probability (1.7e-6 on the gradient at |logits| ~ 60, 26 x torch's float32 error)
        const float ls = logf(s);
        if (p.mode == 0) {
            const bool counted = (tg != 0) && tg >= 0 && tg < p.V;
            for (int v = lane; v < p.V; v += 64) dx[v] = counted ? (expf((x[v] - m) - ls) - (v == tg ? 1.f : 0.f)) : 0.f;
            if (counted) { add_fixed(p.accum, wloss, ls - (x[tg] - m)); wcnt += 1.f; }
        } else {
            const float off = p.smoothing / (float)(p.classes - 1), conf = 1.f - p.smoothing;
            float loss = 0.f;
            const float tot = conf + off * (float)(p.V - 1);
            for (int v = lane; v < p.V; v += 64) {
                const float lp = (x[v] - m) - ls;
                const float tv = (v == tg) ? conf : off;
                loss -= tv * lp;
                dx[v] = tot * expf(lp) - tv;
            }
            add_fixed(p.accum, wloss, wave_sum(loss));
            wcnt += 1.f;
        }
    }
    if (lane == 0) { s_loss[wv] = wloss; s_cnt[wv] = wcnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float c = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        if (c > 0.f) {
            const long long q = (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]);
            atomicAdd(reinterpret_cast<unsigned long long*>(p.accum), (unsigned long long)q);
            atomicAdd(&p.accum[2], c);
        }
    }
}

__global__ void xent_finish_kernel(float* dlogits, long n, const float* accum, float* loss, float gscale) {
    const float cnt = accum[2];
    // an all-pad batch has no counted row: torch returns loss = NaN (0/0) with an all-zero gradient; a NaN gradient
    // here would make the NaN guard drop the CTC part of the step too
    const float k = cnt > 0.f ? gscale / cnt : 0.f;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dlogits[i] *= k;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const long long q = (long long)*reinterpret_cast<const unsigned long long*>(accum);
        *loss = ((float)((double)q / 4294967296.0) + accum[3]) / cnt;
    }
}

}  // namespace

extern "C" int asr_xent(const float* logits, const int64_t* targets, long target_ld, float* dlogits, float* loss,
                        float* accum2, int B, int L, int V, int mode, int classes, float smoothing, float gscale,
                        asr_stream_t stream) {
    ASR_REQUIRE(logits && targets && dlogits && loss && accum2, ASR_E_ARG, "asr_xent: null pointer");
    ASR_REQUIRE(B > 0 && L > 0 && V > 1 && target_ld >= L, ASR_E_ARG, "asr_xent: bad dims");
    ASR_REQUIRE(mode == 0 || (mode == 1 && classes > 1), ASR_E_ARG, "asr_xent: bad mode");
    hipStream_t st = (hipStream_t)stream;
    const long R = (long)B * L;
    XentP p{logits, targets, target_ld, L, dlogits, accum2, R, V, mode, classes, smoothing};
    ASR_REQUIRE(((uintptr_t)accum2 & 7) == 0, ASR_E_ARG, "asr_xent: the scratch must be 8-byte aligned");
    hipMemsetAsync(accum2, 0, 4 * sizeof(float), st);
    hipLaunchKernelGGL(xent_rows_kernel, dim3(cdiv(R, 4L * XROWS)), dim3(256), 0, st, p);
    const long n = R * V;
    long g = (n + 255) / 256; if (g > 2048) g = 2048;
    hipLaunchKernelGGL(xent_finish_kernel, dim3((int)g), dim3(256), 0, st, dlogits, n, accum2, loss, gscale);
    ASR_LAUNCH_CHECK("asr_xent");
    return ASR_OK;
}
