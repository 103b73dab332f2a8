// Word-embedding regulariser and embedding-fused decoding (reference src/plugin.py::EmbeddingRegularizer), fp32:
//   asr_emb_cos_loss        nn.CosineEmbeddingLoss(target +1) between x_emb and table[label], pad rows masked, per-utterance
//                           mean then batch mean; loss, dx and (table not frozen) dy in one launch + a one-workgroup finish
//   asr_emb_fuse_fwd / _bwd out = log((1 - lam) softmax(dec) + lam softmax(relu(temp) emb) + 1e-8), optional argmax of out
//   asr_row_normalize_*     F.normalize(x, dim=-1)
// Rows are independent.  One wave per row (four rows per workgroup) up to V = 2048 - the split of the beam kernels
// (csrc/beam_step.hip) - and one workgroup of four waves per row above; lanes stride the row by 64 / 256 three times.
// The call must move two rows in and one out; that the second and third sweep are served by the caches is the expectation, not
// measured.  Every sum has a fixed order:
// xor-butterfly inside a wave, slot order across the waves of a workgroup, row order in the finish kernels.  No float atomics.
#include "common.h"
#include <limits.h>

namespace {

constexpr float FUSE_EPS = 1e-8f;     // reference src/plugin.py:84
constexpr float COS_EPS = 1e-12f;     // ATen cosine_embedding_loss: EPSILON added to both squared magnitudes
constexpr float NORM_EPS = 1e-12f;    // F.normalize default eps: x / max(||x||, eps)
constexpr int NARROW_MAX_V = 2048;

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// reductions over the 64 * WAVES threads that share a row; red: WAVES floats of LDS (WAVES = 4: every thread of the
// workgroup arrives, the workgroup holds ONE row)
template <int WAVES>
__device__ __forceinline__ float row_sum(float v, float* red) {
    v = wave_sum(v);
    if (WAVES == 1) return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = red[0];
#pragma unroll
    for (int i = 1; i < WAVES; ++i) s += red[i];
    return s;
}
// the same in double: the scalar parameter gradients are sums of N * V terms of both signs, a few hundred times their result
template <int WAVES>
__device__ __forceinline__ double row_sum_d(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (WAVES == 1) return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int i = 1; i < WAVES; ++i) s += red[i];
    return s;
}
template <int WAVES>
__device__ __forceinline__ float row_max(float v, float* red) {
    v = wave_max(v);
    if (WAVES == 1) return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = red[0];
#pragma unroll
    for (int i = 1; i < WAVES; ++i) s = fmaxf(s, red[i]);
    return s;
}

struct FuseP {
    const float* dec; long dec_ld; const float* emb;
    const float* temp; int temp_st; const float* lam; int lam_st; int lam_sig;
    float* out; float* stats; int64_t* amax; long amax_ld;
    // backward only
    const float* stats_in; const float* dout; float* ddec; float* demb; float* tterm; int tmode; float* lterm; int lmode;
    int N, V;
};

__device__ __forceinline__ float temp_at(const FuseP& p, int v) { return fmaxf(p.temp[(long)v * p.temp_st], 0.f); }
__device__ __forceinline__ float lam_at(const FuseP& p, int v) {
    const float r = p.lam[(long)v * p.lam_st];
    return p.lam_sig ? sigmoidf_(r) : r;
}

template <int WAVES>
__global__ __launch_bounds__(256) void fuse_fwd_kernel(FuseP p) {
    __shared__ float red[4];
    __shared__ int redi[4];
    constexpr int TPR = 64 * WAVES;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int tid = (WAVES == 1) ? lane : (int)threadIdx.x;
    const long row = (WAVES == 1) ? blockIdx.x * 4L + wv : (long)blockIdx.x;
    if (row >= p.N) return;                        // wave-uniform (WAVES = 1); the wide grid has exactly N workgroups
    const float* x = p.dec + row * p.dec_ld;
    const float* e = p.emb + row * (long)p.V;
    float* o = p.out + row * (long)p.V;
    float md = -INFINITY, me = -INFINITY;
    for (int v = tid; v < p.V; v += TPR) {
        md = fmaxf(md, x[v]);
        me = fmaxf(me, temp_at(p, v) * e[v]);
    }
    md = row_max<WAVES>(md, red);
    me = row_max<WAVES>(me, red);
    float sd = 0.f, se = 0.f;
    for (int v = tid; v < p.V; v += TPR) {
        sd += expf(x[v] - md);
        se += expf(temp_at(p, v) * e[v] - me);
    }
    sd = row_sum<WAVES>(sd, red);
    se = row_sum<WAVES>(se, red);
    // probabilities as exp((x - m) - log(sum)): x - m is exact for the large terms (see csrc/xent.hip)
    const float ld = logf(sd), le = logf(se);
    float best = -INFINITY;
    int bi = INT_MAX;
    for (int v = tid; v < p.V; v += TPR) {
        const float pd = expf((x[v] - md) - ld);
        const float pe = expf((temp_at(p, v) * e[v] - me) - le);
        const float l = lam_at(p, v);
        const float r = logf(((1.f - l) * pd + l * pe) + FUSE_EPS);
        o[v] = r;
        if (r > best) { best = r; bi = v; }        // ascending v per thread: the lowest index of a tie stays
    }
    if (tid == 0) { p.stats[2 * row] = md + ld; p.stats[2 * row + 1] = me + le; }
    if (p.amax) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const float ov = __shfl_xor(best, s);
            const int oi = __shfl_xor(bi, s);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        if (WAVES > 1) {
            __syncthreads();
            if (lane == 0) { red[wv] = best; redi[wv] = bi; }
            __syncthreads();
            best = red[0]; bi = redi[0];
#pragma unroll
            for (int i = 1; i < WAVES; ++i)
                if (red[i] > best || (red[i] == best && redi[i] < bi)) { best = red[i]; bi = redi[i]; }
        }
        if (tid == 0) p.amax[row * p.amax_ld] = (bi == INT_MAX) ? 0 : bi;      // a row of NaN: token 0
    }
}

// The probabilities are formed again from the logits: exp(x - lse) / sum exp(x - lse), the forward's log-sum-exp as the
// shift (x - lse rounds like x - max does; exp(x - lse) alone would carry ulp(|lse|) into every probability) and the sum,
// which is 1 up to that rounding, formed again.
template <int WAVES>
__global__ __launch_bounds__(256) void fuse_bwd_kernel(FuseP p) {
    // No contraction into fused multiply-adds here.  With a peaked p_emb (|logits| = 80) the row's largest entry has p = 1 and
    // dp - <dp, p> must cancel to exactly 0 as it does in torch; contracted, g * l - de kept the rounding error of the product
    // g * l that the dot product (formed from the ROUNDED products) does not have, and that error times the logit was 19x
    // torch's float32 error on d_temp.
#pragma clang fp contract(off)
    __shared__ float red[4];
    __shared__ double redd[4];
    constexpr int TPR = 64 * WAVES;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int tid = (WAVES == 1) ? lane : (int)threadIdx.x;
    const long row = (WAVES == 1) ? blockIdx.x * 4L + wv : (long)blockIdx.x;
    if (row >= p.N) return;
    const float* x = p.dec + row * p.dec_ld;
    const float* e = p.emb + row * (long)p.V;
    const float* go = p.dout + row * (long)p.V;
    const float cd = p.stats_in[2 * row], ce = p.stats_in[2 * row + 1];
    // the sums and the two dot products are accumulated in double and rounded once: d_emb and d_temp are p (dp - <dp, p>) times
    // logits of any size, and what the dot product loses to summation comes back multiplied by them
    double sd2 = 0.0, se2 = 0.0;
    for (int v = tid; v < p.V; v += TPR) {
        sd2 += expf(x[v] - cd);
        se2 += expf(temp_at(p, v) * e[v] - ce);
    }
    const float sd = (float)row_sum_d<WAVES>(sd2, redd);
    const float se = (float)row_sum_d<WAVES>(se2, redd);
    double dd2 = 0.0, de2 = 0.0;                   // the two softmax backward dot products
    for (int v = tid; v < p.V; v += TPR) {
        const float pd = expf(x[v] - cd) / sd;
        const float pe = expf(temp_at(p, v) * e[v] - ce) / se;
        const float l = lam_at(p, v);
        const float g = go[v] / (((1.f - l) * pd + l * pe) + FUSE_EPS);
        dd2 += g * (1.f - l) * pd;
        de2 += g * l * pe;
    }
    const float dd = (float)row_sum_d<WAVES>(dd2, redd);
    const float de = (float)row_sum_d<WAVES>(de2, redd);
    double ts = 0.0, ls = 0.0;                     // row sums of the scalar-parameter terms
    for (int v = tid; v < p.V; v += TPR) {
        const float traw = p.temp[(long)v * p.temp_st];
        const float tp = fmaxf(traw, 0.f);
        const float pd = expf(x[v] - cd) / sd;
        const float pe = expf(tp * e[v] - ce) / se;
        const float l = lam_at(p, v);
        const float g = go[v] / (((1.f - l) * pd + l * pe) + FUSE_EPS);
        p.ddec[row * (long)p.V + v] = pd * (g * (1.f - l) - dd);
        const float da = pe * (g * l - de);
        p.demb[row * (long)p.V + v] = da * tp;
        if (p.tmode) {
            const float tt = (traw > 0.f) ? da * e[v] : 0.f;
            if (p.tmode == 2) p.tterm[row * (long)p.V + v] = tt; else ts += tt;
        }
        if (p.lmode) {
            const float lt = g * (pe - pd) * (p.lam_sig ? l * (1.f - l) : 1.f);
            if (p.lmode == 2) p.lterm[row * (long)p.V + v] = lt; else ls += lt;
        }
    }
    if (p.tmode == 1) { ts = row_sum_d<WAVES>(ts, redd); if (tid == 0) p.tterm[row] = (float)ts; }
    if (p.lmode == 1) { ls = row_sum_d<WAVES>(ls, redd); if (tid == 0) p.lterm[row] = (float)ls; }
}

// out[j] = sum_i terms[i * W + j] in a fixed order: wave w of the workgroup adds rows w, w + 4, ... in ascending order, then
// (s0 + s1) + (s2 + s3); accumulated in double, rounded once
__global__ __launch_bounds__(256) void col_reduce_kernel(const float* terms, int N, int W, float* out) {
    __shared__ double s[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    double a = 0.0;
    if (j < W)
        for (long i = wv; i < N; i += 4) a += terms[i * W + j];
    s[wv][lane] = a;
    __syncthreads();
    if (wv == 0 && j < W) out[j] = (float)((s[0][lane] + s[1][lane]) + (s[2][lane] + s[3][lane]));
}

// out[0] = sum_i v[i]: thread k adds i = k, k + 256, ... in ascending order, then a fixed halving tree; in double, rounded once
__global__ __launch_bounds__(256) void vec_reduce_kernel(const float* v, long n, float* out) {
    __shared__ double s[256];
    double a = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) a += v[i];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)s[0];
}

struct CosP {
    const float* x; const float* table; const int64_t* label; long label_ld;
    float* dx; float* dy; float* rowloss;
    int B, L, E, V;
};

__global__ __launch_bounds__(256) void cos_rows_kernel(CosP p) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long row = blockIdx.x * 4L + wv;
    if (row >= (long)p.B * p.L) return;
    const int64_t* lab = p.label + (row / p.L) * p.label_ld;
    int cnt = 0;
    for (int i = lane; i < p.L; i += 64) { const int64_t l = lab[i]; cnt += (l > 0 && l < p.V) ? 1 : 0; }
    cnt = wave_sum_int(cnt);
    const int64_t tg = lab[row % p.L];
    float* dx = p.dx + row * (long)p.E;
    float* dy = p.dy ? p.dy + row * (long)p.E : nullptr;
    if (!(tg > 0 && tg < p.V)) {                   // pad (or out-of-range) label: no loss, no gradient
        for (int k = lane; k < p.E; k += 64) { dx[k] = 0.f; if (dy) dy[k] = 0.f; }
        if (lane == 0) p.rowloss[row] = 0.f;
        return;
    }
    const float* x = p.x + row * (long)p.E;
    const float* y = p.table + tg * (long)p.E;
    float pxy = 0.f, a = 0.f, b = 0.f;
    for (int k = lane; k < p.E; k += 64) { const float xv = x[k], yv = y[k]; pxy += xv * yv; a += xv * xv; b += yv * yv; }
    pxy = wave_sum(pxy);
    a = wave_sum(a) + COS_EPS;
    b = wave_sum(b) + COS_EPS;
    const float den = sqrtf(a * b), c = pxy / den;
    const float w = 1.f / ((float)p.B * (float)cnt);         // cnt >= 1: this row counts
    if (lane == 0) p.rowloss[row] = w * (1.f - c);
    for (int k = lane; k < p.E; k += 64) {
        const float xv = x[k], yv = y[k];
        dx[k] = -w * (yv / den - c * xv / a);
        if (dy) dy[k] = -w * (xv / den - c * yv / b);
    }
}

__global__ __launch_bounds__(256) void row_normalize_fwd_kernel(const float* x, float* y, long N, int E) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long row = blockIdx.x * 4L + wv;
    if (row >= N) return;
    const float* xr = x + row * E;
    float ss = 0.f;
    for (int k = lane; k < E; k += 64) ss += xr[k] * xr[k];
    const float den = fmaxf(sqrtf(wave_sum(ss)), NORM_EPS);
    for (int k = lane; k < E; k += 64) y[row * E + k] = xr[k] / den;
}

__global__ __launch_bounds__(256) void row_normalize_bwd_kernel(const float* dy, const float* x, float* dx, long N, int E) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long row = blockIdx.x * 4L + wv;
    if (row >= N) return;
    const float* xr = x + row * E;
    const float* gr = dy + row * E;
    float ss = 0.f, dot = 0.f, amax = 0.f;
    for (int k = lane; k < E; k += 64) { ss += xr[k] * xr[k]; dot += gr[k] * xr[k]; amax = fmaxf(amax, fabsf(xr[k])); }
    const float n = sqrtf(wave_sum(ss));
    dot = wave_sum(dot);
    amax = wave_max(amax);
    const float den = fmaxf(n, NORM_EPS);
    // clamp_min passes the gradient of the norm where n >= eps; below it the row is x / eps
    const float k2 = (n >= NORM_EPS) ? dot / (den * den * n) : 0.f;
    for (int k = lane; k < E; k += 64) dx[row * E + k] = (amax == 0.f) ? 0.f : gr[k] / den - xr[k] * k2;
}

}  // namespace

extern "C" int asr_emb_cos_loss(const float* x, const float* table, const int64_t* label, long label_ld, float* loss, float* dx,
                                float* dy, float* row_loss, int B, int L, int E, int V, asr_stream_t stream) {
    ASR_REQUIRE(x && table && label && loss && dx && row_loss, ASR_E_ARG, "asr_emb_cos_loss: null pointer");
    ASR_REQUIRE(B >= 1 && L >= 1 && E >= 1 && V >= 2 && V <= 65536 && label_ld >= L, ASR_E_ARG,
                "asr_emb_cos_loss: bad dims (B %d L %d E %d V %d label_ld %ld)", B, L, E, V, label_ld);
    hipStream_t st = (hipStream_t)stream;
    const long N = (long)B * L;
    CosP p{x, table, label, label_ld, dx, dy, row_loss, B, L, E, V};
    hipLaunchKernelGGL(cos_rows_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, p);
    hipLaunchKernelGGL(vec_reduce_kernel, dim3(1), dim3(256), 0, st, row_loss, N, loss);
    ASR_LAUNCH_CHECK("asr_emb_cos_loss");
    return ASR_OK;
}

static int fuse_check(const char* name, const void* dec, long dec_ld, const void* emb, const void* temp, int temp_stride,
                      const void* lam, int lam_stride, int N, int V) {
    ASR_REQUIRE(dec && emb && temp && lam, ASR_E_ARG, "%s: null pointer", name);
    ASR_REQUIRE(N >= 1 && V >= 2 && V <= 65536 && dec_ld >= V, ASR_E_ARG, "%s: bad dims (N %d V %d row stride %ld)", name, N, V, dec_ld);
    ASR_REQUIRE((temp_stride == 0 || temp_stride == 1) && (lam_stride == 0 || lam_stride == 1), ASR_E_ARG,
                "%s: temp / lam stride must be 0 (scalar) or 1 (per token)", name);
    return ASR_OK;
}

extern "C" int asr_emb_fuse_fwd(const float* dec_logit, long dec_ld, const float* emb_logit, const float* temp, int temp_stride,
                                const float* lam, int lam_stride, int lam_sigmoid, float* out, float* stats, int64_t* argmax,
                                long argmax_ld, int N, int V, asr_stream_t stream) {
    int rc = fuse_check("asr_emb_fuse_fwd", dec_logit, dec_ld, emb_logit, temp, temp_stride, lam, lam_stride, N, V);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(out && stats, ASR_E_ARG, "asr_emb_fuse_fwd: null pointer");
    ASR_REQUIRE(!argmax || argmax_ld >= 1, ASR_E_ARG, "asr_emb_fuse_fwd: argmax stride %ld < 1", argmax_ld);
    FuseP p{};
    p.dec = dec_logit; p.dec_ld = dec_ld; p.emb = emb_logit; p.temp = temp; p.temp_st = temp_stride; p.lam = lam;
    p.lam_st = lam_stride; p.lam_sig = lam_sigmoid ? 1 : 0; p.out = out; p.stats = stats; p.amax = argmax; p.amax_ld = argmax_ld;
    p.N = N; p.V = V;
    hipStream_t st = (hipStream_t)stream;
    if (V <= NARROW_MAX_V) hipLaunchKernelGGL(fuse_fwd_kernel<1>, dim3(cdiv(N, 4)), dim3(256), 0, st, p);
    else                   hipLaunchKernelGGL(fuse_fwd_kernel<4>, dim3(N), dim3(256), 0, st, p);
    ASR_LAUNCH_CHECK("asr_emb_fuse_fwd");
    return ASR_OK;
}

extern "C" int asr_emb_fuse_bwd(const float* dout, const float* dec_logit, long dec_ld, const float* emb_logit, const float* temp,
                                int temp_stride, const float* lam, int lam_stride, int lam_sigmoid, const float* stats,
                                float* d_dec_logit, float* d_emb_logit, float* d_temp, float* d_lam_raw, float* work, int N, int V,
                                asr_stream_t stream) {
    int rc = fuse_check("asr_emb_fuse_bwd", dec_logit, dec_ld, emb_logit, temp, temp_stride, lam, lam_stride, N, V);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(dout && stats && d_dec_logit && d_emb_logit, ASR_E_ARG, "asr_emb_fuse_bwd: null pointer");
    ASR_REQUIRE(work || (!d_temp && !d_lam_raw), ASR_E_ARG, "asr_emb_fuse_bwd: parameter gradients need the work area");
    FuseP p{};
    p.dec = dec_logit; p.dec_ld = dec_ld; p.emb = emb_logit; p.temp = temp; p.temp_st = temp_stride; p.lam = lam;
    p.lam_st = lam_stride; p.lam_sig = lam_sigmoid ? 1 : 0; p.stats_in = stats; p.dout = dout; p.ddec = d_dec_logit; p.demb = d_emb_logit;
    p.N = N; p.V = V;
    float* w = work;
    if (d_temp) { p.tterm = w; p.tmode = temp_stride ? 2 : 1; w += temp_stride ? (size_t)N * V : (size_t)N; }
    if (d_lam_raw) { p.lterm = w; p.lmode = lam_stride ? 2 : 1; }
    hipStream_t st = (hipStream_t)stream;
    if (V <= NARROW_MAX_V) hipLaunchKernelGGL(fuse_bwd_kernel<1>, dim3(cdiv(N, 4)), dim3(256), 0, st, p);
    else                   hipLaunchKernelGGL(fuse_bwd_kernel<4>, dim3(N), dim3(256), 0, st, p);
    if (p.tmode == 2) hipLaunchKernelGGL(col_reduce_kernel, dim3(cdiv(V, 64)), dim3(256), 0, st, p.tterm, N, V, d_temp);
    if (p.tmode == 1) hipLaunchKernelGGL(vec_reduce_kernel, dim3(1), dim3(256), 0, st, p.tterm, (long)N, d_temp);
    if (p.lmode == 2) hipLaunchKernelGGL(col_reduce_kernel, dim3(cdiv(V, 64)), dim3(256), 0, st, p.lterm, N, V, d_lam_raw);
    if (p.lmode == 1) hipLaunchKernelGGL(vec_reduce_kernel, dim3(1), dim3(256), 0, st, p.lterm, (long)N, d_lam_raw);
    ASR_LAUNCH_CHECK("asr_emb_fuse_bwd");
    return ASR_OK;
}

extern "C" int asr_row_normalize_fwd(const float* x, float* y, long N, int E, asr_stream_t stream) {
    ASR_REQUIRE(x && y, ASR_E_ARG, "asr_row_normalize_fwd: null pointer");
    ASR_REQUIRE(N >= 1 && E >= 1, ASR_E_ARG, "asr_row_normalize_fwd: bad dims (N %ld E %d)", N, E);
    hipLaunchKernelGGL(row_normalize_fwd_kernel, dim3(cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, x, y, N, E);
    ASR_LAUNCH_CHECK("asr_row_normalize_fwd");
    return ASR_OK;
}

extern "C" int asr_row_normalize_bwd(const float* dy, const float* x, float* dx, long N, int E, asr_stream_t stream) {
    ASR_REQUIRE(dy && x && dx, ASR_E_ARG, "asr_row_normalize_bwd: null pointer");
    ASR_REQUIRE(N >= 1 && E >= 1, ASR_E_ARG, "asr_row_normalize_bwd: bad dims (N %ld E %d)", N, E);
    hipLaunchKernelGGL(row_normalize_bwd_kernel, dim3(cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, dy, x, dx, N, E);
    ASR_LAUNCH_CHECK("asr_row_normalize_bwd");
    return ASR_OK;
}
