// Waveform augmentation on the GPU (data.audio.time_aug; reference src/audio.py:283-309, an audiomentations.Compose of
// AddGaussianNoise(0.001, 0.01, p=0.3), TimeStretch(0.8, 1.25, p=0.3), PitchShift(-4, 4, p=0.5) on the raw wave, train mode only).
// The recipe is DESIGN.md 4.14; tests/test_wave_aug_reference.py restates every kernel of this file in float64.
//
//   asr_wave_draws    : draws (B,6) = {noise_on, amp, stretch_on, rate, pitch_on, semitones} from Philox or from draws_in, the
//                       switches an utterance cannot take (len <= n_fft/2, a rate outside [0.5, 2]) recorded as 0, and the
//                       rates (B,2) = {stretch rate, 2^(-semitones/12)} the other kernels read, 0 = off.
//   asr_wave_noise    : x[n] += amp * z[n], z by Box-Muller on Philox uniforms keyed by (seed, utterance, n / 4).
//   asr_wave_stft     : centred, reflect-padded STFT, hop n_fft/4, periodic Hann.  A wave (64 lanes) owns two frames: frame A in
//                       the real part and frame B in the imaginary part of one complex radix-2 FFT in LDS, separated by the
//                       Hermitian symmetry on the way out.  A workgroup of 4 waves holds 8 frames; framed rows never go to HBM.
//   asr_wave_pvoc     : librosa's phase_vocoder, one thread per (utterance, bin) over the output frames.  The accumulator is a
//                       double in TURNS, reduced to [-1/2, 1/2] after every step: the expected advance phi[k] = k pi / 2 is k / 4
//                       of a turn, i.e. (k & 3) / 4 exactly, so nothing is lost however long the utterance.
//   asr_wave_istft    : inverse FFT in LDS (two frames per transform again), window, overlap-add in gather form: a workgroup
//                       transforms 8 consecutive frames and writes the 5 hop blocks that only they reach; every sample sums its
//                       at most 4 frames in ascending frame order and divides by the window envelope.  No atomics.
//   asr_wave_resample : band-limited interpolation back to len samples, one thread per output sample, Kaiser-windowed sinc with
//                       resampy's kaiser_best constants evaluated analytically in double (sinpi reduces the argument; the
//                       window by the power series of I0), accumulated in double and rounded once.
//   asr_wave_augment  : the chain over a batch from a draws array.  Never allocates, never synchronises.
#include "common.h"
#include <float.h>

#define WA_CAP_BYTES ((size_t)256 << 20)         // the sliced part of asr_wave_augment's work area stays below this
#define WA_ISTFT_BLOCKS 5                         // hop blocks a workgroup of asr_wave_istft writes (8 frames - 3 of overlap)

__device__ __forceinline__ int wa_len(const int64_t* lens, int b, int N) {
    const long l = (long)lens[b];
    return (int)min(max(l, 0L), (long)N);
}
__device__ __forceinline__ bool wa_rate_ok(float r) { return r >= 0.5f && r <= 2.0f; }             // false for NaN
__device__ __forceinline__ int wa_out_frames(int nfr, double rate) { return (int)ceil((double)nfr / rate); }
__device__ __forceinline__ long wa_out_len(int len, double rate) { return (long)rint((double)len / rate); }
// an utterance takes part in a stretch / pitch stage when its rate is legal and it can be reflect-padded
__device__ __forceinline__ bool wa_active(int len, int n_fft, float rate) { return len > n_fft / 2 && wa_rate_ok(rate); }

static int wa_log2(int n_fft) {
    for (int lg = 6; lg <= 11; ++lg)
        if (n_fft == (1 << lg)) return lg;
    return -1;
}

// ---- draws ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void wave_draws_kernel(const int64_t* __restrict__ lens, const float* __restrict__ draws_in,
                                                        float* __restrict__ draws_out, float* __restrict__ draws_out2,
                                                        float* __restrict__ rates_out, int B, int N, int n_fft, uint64_t seed) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int len = wa_len(lens, b, N);
    float d[6];
    if (draws_in) {
        for (int i = 0; i < 6; ++i) d[i] = draws_in[b * 6 + i];
    } else {
        uint32_t r[4], r2[4];
        philox4x32((uint32_t)b, 0u, 3u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
        philox4x32((uint32_t)b, 0u, 4u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r2);
        const float k = 2.3283064365386963e-10f;                                   // 2^-32
        const float u0 = (float)r[0] * k, u1 = (float)r[1] * k, u2 = (float)r[2] * k, u3 = (float)r[3] * k;
        const float u4 = (float)r2[0] * k, u5 = (float)r2[1] * k;
        d[0] = u0 < 0.3f ? 1.f : 0.f;
        d[1] = 0.001f + u1 * (0.01f - 0.001f);
        d[2] = u2 < 0.3f ? 1.f : 0.f;
        d[3] = 0.8f + u3 * (1.25f - 0.8f);
        d[4] = u4 < 0.5f ? 1.f : 0.f;
        d[5] = -4.f + u5 * (4.f - -4.f);
    }
    const float pr = (float)exp2(-(double)d[5] / 12.0);
    d[0] = d[0] != 0.f ? 1.f : 0.f;
    d[2] = (d[2] != 0.f && wa_active(len, n_fft, d[3])) ? 1.f : 0.f;
    d[4] = (d[4] != 0.f && wa_active(len, n_fft, pr)) ? 1.f : 0.f;
    for (int i = 0; i < 6; ++i) {
        if (draws_out) draws_out[b * 6 + i] = d[i];
        if (draws_out2) draws_out2[b * 6 + i] = d[i];
    }
    if (rates_out) {
        rates_out[b * 2] = d[2] != 0.f ? d[3] : 0.f;
        rates_out[b * 2 + 1] = d[4] != 0.f ? pr : 0.f;
    }
}

// ---- noise ----------------------------------------------------------------------------------------------------------------
// Philox block (n / 4, b, 5, 0) gives r[0..3]; samples 4q and 4q+1 take the pair (r0, r1), 4q+2 and 4q+3 the pair (r2, r3):
//   u1 = ((r_a >> 8) + 1) 2^-24 in (0, 1],  u2 = (r_b >> 8) 2^-24 in [0, 1)  (both exact in float32),
//   z_even = sqrt(-2 ln u1) cos(2 pi u2),  z_odd = sqrt(-2 ln u1) sin(2 pi u2).
__global__ __launch_bounds__(256) void wave_noise_kernel(float* __restrict__ wav, const int64_t* __restrict__ lens,
                                                         const float* __restrict__ draws, int B, int N, uint64_t seed) {
    const int b = blockIdx.y;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    const int len = wa_len(lens, b, N);
    if (q * 4 >= len || draws[b * 6] == 0.f) return;
    const float amp = draws[b * 6 + 1];
    uint32_t r[4];
    philox4x32((uint32_t)q, (uint32_t)b, 5u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    float z[4];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float u1 = (float)((r[2 * p] >> 8) + 1u) * 5.9604644775390625e-8f;
        const float u2 = (float)(r[2 * p + 1] >> 8) * 5.9604644775390625e-8f;
        const float rad = sqrtf(-2.f * logf(u1));
        float s, c;
        sincospif(2.f * u2, &s, &c);
        z[2 * p] = rad * c;
        z[2 * p + 1] = rad * s;
    }
    float* x = wav + (long)b * N;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long n = q * 4 + j;
        if (n < len) x[n] += amp * z[j];
    }
}

// ---- radix-2 FFT of n complex points held by one wave in LDS, input in bit-reversed order, output in natural order --------
// table: n/2 twiddles (cos, -sin)(2 pi k / n) then the n window samples.  Every wave of the workgroup calls this with the same
// n (the barriers are workgroup-wide); a wave without a frame passes act = false.
__device__ __forceinline__ void wa_fft(float2* z, const float* __restrict__ tw, int n, int lg, int lane, bool act, bool inverse) {
    for (int s = 1; s <= lg; ++s) {
        const int half = 1 << (s - 1), tstride = n >> s;
        if (act) {
            for (int i = lane; i < n / 2; i += 64) {
                const int j = i & (half - 1), a = ((i >> (s - 1)) << s) + j, c = a + half;
                const float wr = tw[2 * j * tstride], wi = inverse ? -tw[2 * j * tstride + 1] : tw[2 * j * tstride + 1];
                const float2 u = z[a], v = z[c];
                const float tr = wr * v.x - wi * v.y, ti = wr * v.y + wi * v.x;
                z[a] = make_float2(u.x + tr, u.y + ti);
                z[c] = make_float2(u.x - tr, u.y - ti);
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int wa_reflect(int i, int len) {
    if (i < 0) i = -i;
    if (i >= len) i = 2 * (len - 1) - i;
    return min(max(i, 0), len - 1);
}

extern __shared__ float2 wa_lds[];                 // 4 waves x n_fft complex: 64 KB at n_fft = 2048

// spec [B][F = 1 + N/hop][n_fft/2 + 1] complex; frames t >= 1 + len/hop of an utterance are not written
__global__ __launch_bounds__(256) void wave_stft_kernel(const float* __restrict__ wav, const int64_t* __restrict__ lens,
                                                        const float* __restrict__ rates, int rate_stride,
                                                        const float* __restrict__ table, float2* __restrict__ spec,
                                                        int B, int N, int n, int lg) {
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int len = wa_len(lens, b, N);
    if (!wa_active(len, n, rates[(long)b * rate_stride])) return;
    const int hop = n >> 2, nfr = 1 + len / hop, F = 1 + N / hop, nb = n / 2 + 1;
    if ((int)blockIdx.x * 8 >= nfr) return;
    const int f0 = ((int)blockIdx.x * 4 + wave) * 2;
    const bool act = f0 < nfr, actB = f0 + 1 < nfr;
    float2* z = wa_lds + wave * n;
    const float* win = table + n;
    const float* x = wav + (long)b * N;
    if (act) {
        for (int j = lane; j < n; j += 64) {
            const float w = win[j];
            const int ia = f0 * hop + j - n / 2;
            const float va = w * x[wa_reflect(ia, len)];
            const float vb = actB ? w * x[wa_reflect(ia + hop, len)] : 0.f;
            z[__brev((unsigned)j) >> (32 - lg)] = make_float2(va, vb);
        }
    }
    __syncthreads();
    wa_fft(z, table, n, lg, lane, act, false);
    if (act) {
        float2* oa = spec + ((long)b * F + f0) * nb;
        float2* ob = oa + nb;
        for (int k = lane; k <= n / 2; k += 64) {
            const float2 p = z[k], q = z[(n - k) & (n - 1)];
            oa[k] = make_float2(0.5f * (p.x + q.x), 0.5f * (p.y - q.y));
            if (actB) ob[k] = make_float2(0.5f * (p.y + q.y), -0.5f * (p.x - q.x));
        }
    }
}

// out [B][2F][n_fft/2 + 1] complex; frames t >= ceil(n_frames / rate) are not written
__global__ __launch_bounds__(64) void wave_pvoc_kernel(const float2* __restrict__ spec, const int64_t* __restrict__ lens,
                                                       const float* __restrict__ rates, int rate_stride,
                                                       float2* __restrict__ out, int B, int N, int n) {
    const int b = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x, nb = n / 2 + 1;
    const int len = wa_len(lens, b, N);
    const float ratef = rates[(long)b * rate_stride];
    if (k >= nb || !wa_active(len, n, ratef)) return;
    const double rate = (double)ratef, inv2pi = 0.15915494309189533577;
    const int hop = n >> 2, nfr = 1 + len / hop, F = 1 + N / hop, nout = wa_out_frames(nfr, rate);
    const float2* D = spec + (long)b * F * nb + k;
    float2* O = out + (long)b * 2 * F * nb + k;
    const float2 d0 = D[0];
    const double phi = (double)(k & 3) * 0.25;
    double acc = (double)atan2f(d0.y, d0.x) * inv2pi;
    acc -= rint(acc);
    const float2 zero = make_float2(0.f, 0.f);
    for (int t = 0; t < nout && t < 2 * F; ++t) {
        const double st = (double)t * rate;
        const int fl = (int)floor(st);
        const float a = (float)(st - (double)fl);
        const float2 c0 = fl < nfr ? D[(long)fl * nb] : zero;
        const float2 c1 = fl + 1 < nfr ? D[(long)(fl + 1) * nb] : zero;
        const float mag = (1.f - a) * hypotf(c0.x, c0.y) + a * hypotf(c1.x, c1.y);
        float s, c;
        sincospif((float)(2.0 * acc), &s, &c);
        O[(long)t * nb] = make_float2(mag * c, mag * s);
        double dp = ((double)atan2f(c1.y, c1.x) - (double)atan2f(c0.y, c0.x)) * inv2pi - phi;
        dp -= rint(dp);
        acc += phi + dp;
        acc -= rint(acc);
    }
}

// dst[b * dst_stride + m] for m < lim, lim = len (keep_len: the length-preserving stretch, zeros from M on) or M = round(len / rate)
__global__ __launch_bounds__(256) void wave_istft_kernel(const float2* __restrict__ ospec, const int64_t* __restrict__ lens,
                                                         const float* __restrict__ rates, int rate_stride,
                                                         const float* __restrict__ table, float* __restrict__ dst, long dst_stride,
                                                         int keep_len, int B, int N, int n, int lg) {
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int len = wa_len(lens, b, N);
    const float ratef = rates[(long)b * rate_stride];
    if (!wa_active(len, n, ratef)) return;
    const double rate = (double)ratef;
    const int hop = n >> 2, nfr = 1 + len / hop, F = 1 + N / hop, nb = n / 2 + 1;
    const int nout = min(wa_out_frames(nfr, rate), 2 * F);
    const long M = min(wa_out_len(len, rate), 2L * N);
    const long lim = keep_len ? (long)len : M;
    const long q0 = (long)blockIdx.x * WA_ISTFT_BLOCKS;              // first hop block (padded coordinates) this workgroup writes
    if (q0 * hop - n / 2 >= lim) return;
    const long ffirst = q0 - 3, fa = ffirst + 2 * wave, fb = fa + 1;
    const bool actA = fa >= 0 && fa < nout, actB = fb >= 0 && fb < nout, act = actA || actB;
    float2* z = wa_lds + wave * n;
    const float* win = table + n;
    if (act) {
        const float2* pa = ospec + ((long)b * 2 * F + fa) * nb;
        const float2* pb = pa + nb;
        const float2 zero = make_float2(0.f, 0.f);
        for (int k = lane; k <= n / 2; k += 64) {
            const float2 A = actA ? pa[k] : zero, Bv = actB ? pb[k] : zero;
            if (k == 0 || k == n / 2) {
                z[__brev((unsigned)k) >> (32 - lg)] = make_float2(A.x, Bv.x);
            } else {
                z[__brev((unsigned)k) >> (32 - lg)] = make_float2(A.x - Bv.y, A.y + Bv.x);
                z[__brev((unsigned)(n - k)) >> (32 - lg)] = make_float2(A.x + Bv.y, Bv.x - A.y);
            }
        }
    }
    __syncthreads();
    wa_fft(z, table, n, lg, lane, act, true);
    const float inv_n = 1.f / (float)n;
    float* y = dst + (long)b * dst_stride;
    for (int idx = tid; idx < WA_ISTFT_BLOCKS * hop; idx += 256) {
        const long p = q0 * hop + idx, m = p - n / 2;
        if (m < 0 || m >= lim) continue;
        float v = 0.f;
        if (m < M) {
            const long q = p / hop;
            float sum = 0.f, env = 0.f;
            for (long f = q - 3; f <= q; ++f) {
                if (f < 0 || f >= nout) continue;
                const int j = (int)(p - f * hop), li = (int)(f - ffirst);
                const float2 e = wa_lds[(li >> 1) * n + j];
                const float w = win[j];
                sum += w * ((li & 1) ? e.y : e.x);
                env += w * w;
            }
            v = env > FLT_MIN ? (sum * inv_n) / env : 0.f;
        }
        y[m] = v;
    }
}

#define WA_KAISER_BETA 14.769656459379492
#define WA_ROLLOFF 0.9475937167399596
#define WA_ZEROS 64.0
#define WA_I0_TERMS 32

// kaiser(u) = I0(beta sqrt(1 - u^2)) / I0(beta) as the power series of I0 in s2 = 1 - u^2:
//   I0(beta sqrt(s2)) = sum_k (beta^2 / 4)^k s2^k / (k!)^2,
// coefficients divided by I0(beta) and built at compile time.  All of them are positive and s2 is in [0, 1], so Horner's scheme
// loses a few double ulps and needs no square root; the first dropped term is 2e-21 of the sum at s2 = 1.
struct WaKaiser {
    double c[WA_I0_TERMS];
    constexpr WaKaiser() : c() {
        const double q = 0.25 * WA_KAISER_BETA * WA_KAISER_BETA;
        double t = 1.0, sum = 0.0;
        for (int k = 0; k < WA_I0_TERMS; ++k) {
            c[k] = t;
            sum += t;
            t = t * q / ((double)(k + 1) * (double)(k + 1));
        }
        for (int k = 0; k < WA_I0_TERMS; ++k) c[k] /= sum;
    }
};
__constant__ WaKaiser wa_kaiser = WaKaiser();

__device__ __forceinline__ double wa_kaiser_window(double s2) {
    double p = wa_kaiser.c[WA_I0_TERMS - 1];
#pragma unroll
    for (int k = WA_I0_TERMS - 2; k >= 0; --k) p = fma(p, s2, wa_kaiser.c[k]);
    return p;
}

// wav[b][i] for i < len: the band-limited interpolation of src[b][0 .. M) at i / rate
__global__ __launch_bounds__(256) void wave_resample_kernel(const float* __restrict__ src, long src_stride,
                                                            const int64_t* __restrict__ lens, const float* __restrict__ rates,
                                                            int rate_stride, float* __restrict__ wav, int B, int N, int n_fft) {
    const int b = blockIdx.y;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int len = wa_len(lens, b, N);
    const float ratef = rates[(long)b * rate_stride];
    if (i >= len || !wa_active(len, n_fft, ratef)) return;
    const double rate = (double)ratef, mn = fmin(1.0, rate), c = WA_ROLLOFF * mn, W = WA_ZEROS / mn, invW = mn / WA_ZEROS;
    const long M = min(wa_out_len(len, rate), 2L * N);
    const double pos = (double)i / rate;
    const long jlo = max((long)ceil(pos - W), 0L), jhi = min((long)floor(pos + W), M - 1);
    const float* y = src + (long)b * src_stride;
    double acc = 0.0;
    for (long j = jlo; j <= jhi; ++j) {
        const double t = pos - (double)j, u = t * invW, s2 = 1.0 - u * u;
        if (s2 < 0.0) continue;
        const double ct = c * t;
        const double sinc = ct == 0.0 ? 1.0 : sinpi(ct) / (3.14159265358979323846 * ct);
        acc += (double)y[j] * (c * sinc * wa_kaiser_window(s2));
    }
    wav[(long)b * N + i] = (float)acc;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
#define WA_COMMON_REQUIRE(name)                                                                                          \
    do {                                                                                                                 \
        ASR_REQUIRE(B > 0 && N > 0, ASR_E_ARG, name ": B and N must be positive");                                       \
        ASR_REQUIRE(B <= 65535, ASR_E_ARG, name ": B = %d is beyond one grid axis", B);                                  \
        ASR_REQUIRE(N <= (1 << 28), ASR_E_ARG, name ": N = %d is beyond 2^28 samples", N);                               \
    } while (0)
#define WA_FFT_REQUIRE(name)                                                                                             \
    const int lg = wa_log2(n_fft);                                                                                       \
    ASR_REQUIRE(lg > 0, ASR_E_ARG, name ": n_fft = %d is not a power of two in 64..2048", n_fft)

static size_t wa_align(size_t v) { return (v + 255) & ~(size_t)255; }
static size_t wa_spec_bytes(int N, int n_fft) { return (size_t)(1 + N / (n_fft / 4)) * (size_t)(n_fft / 2 + 1) * sizeof(float2); }

static void wa_launch_stft(const float* wav, const int64_t* lens, const float* rates, int rs, const float* table, float* spec,
                           int B, int N, int n_fft, int lg, hipStream_t st) {
    const int F = 1 + N / (n_fft / 4);
    hipLaunchKernelGGL(wave_stft_kernel, dim3(cdiv(F, 8), B), dim3(256), (size_t)4 * n_fft * sizeof(float2), st, wav, lens, rates, rs,
                       table, (float2*)spec, B, N, n_fft, lg);
}
static void wa_launch_pvoc(const float* spec, const int64_t* lens, const float* rates, int rs, float* out, int B, int N, int n_fft,
                           hipStream_t st) {
    hipLaunchKernelGGL(wave_pvoc_kernel, dim3(cdiv(n_fft / 2 + 1, 64), B), dim3(64), 0, st, (const float2*)spec, lens, rates, rs,
                       (float2*)out, B, N, n_fft);
}
static void wa_launch_istft(const float* ospec, const int64_t* lens, const float* rates, int rs, const float* table, float* dst,
                            long dst_stride, int keep_len, int B, int N, int n_fft, int lg, hipStream_t st) {
    const int hop = n_fft / 4;
    const long maxlim = keep_len ? (long)N : 2L * N, qmax = (maxlim - 1 + n_fft / 2) / hop;
    hipLaunchKernelGGL(wave_istft_kernel, dim3((unsigned)(qmax / WA_ISTFT_BLOCKS + 1), B), dim3(256), (size_t)4 * n_fft * sizeof(float2),
                       st, (const float2*)ospec, lens, rates, rs, table, dst, dst_stride, keep_len, B, N, n_fft, lg);
}
static void wa_launch_resample(const float* src, long src_stride, const int64_t* lens, const float* rates, int rs, float* wav, int B,
                               int N, int n_fft, hipStream_t st) {
    hipLaunchKernelGGL(wave_resample_kernel, dim3(cdiv(N, 256), B), dim3(256), 0, st, src, src_stride, lens, rates, rs, wav, B, N, n_fft);
}

extern "C" int asr_wave_draws(const int64_t* wav_len, const float* draws_in, float* draws_out, float* rates_out, int B, int N, int n_fft,
                              uint64_t seed, void* stream) {
    ASR_REQUIRE(wav_len && draws_out, ASR_E_ARG, "asr_wave_draws: null pointer");
    WA_COMMON_REQUIRE("asr_wave_draws");
    WA_FFT_REQUIRE("asr_wave_draws");
    (void)lg;
    hipLaunchKernelGGL(wave_draws_kernel, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, wav_len, draws_in, draws_out, (float*)nullptr,
                       rates_out, B, N, n_fft, seed);
    ASR_LAUNCH_CHECK("asr_wave_draws");
    return ASR_OK;
}

extern "C" int asr_wave_noise(float* wav, const int64_t* wav_len, const float* draws, int B, int N, uint64_t seed, void* stream) {
    ASR_REQUIRE(wav && wav_len && draws, ASR_E_ARG, "asr_wave_noise: null pointer");
    WA_COMMON_REQUIRE("asr_wave_noise");
    hipLaunchKernelGGL(wave_noise_kernel, dim3(cdiv(cdiv(N, 4), 256), B), dim3(256), 0, (hipStream_t)stream, wav, wav_len, draws, B, N, seed);
    ASR_LAUNCH_CHECK("asr_wave_noise");
    return ASR_OK;
}

extern "C" int asr_wave_stft(const float* wav, const int64_t* wav_len, const float* rates, int rate_stride, const float* table, float* spec,
                             int B, int N, int n_fft, void* stream) {
    ASR_REQUIRE(wav && wav_len && rates && table && spec, ASR_E_ARG, "asr_wave_stft: null pointer");
    ASR_REQUIRE(rate_stride > 0, ASR_E_ARG, "asr_wave_stft: rate_stride must be positive");
    WA_COMMON_REQUIRE("asr_wave_stft");
    WA_FFT_REQUIRE("asr_wave_stft");
    wa_launch_stft(wav, wav_len, rates, rate_stride, table, spec, B, N, n_fft, lg, (hipStream_t)stream);
    ASR_LAUNCH_CHECK("asr_wave_stft");
    return ASR_OK;
}

extern "C" int asr_wave_pvoc(const float* spec, const int64_t* wav_len, const float* rates, int rate_stride, float* out, int B, int N,
                             int n_fft, void* stream) {
    ASR_REQUIRE(spec && wav_len && rates && out, ASR_E_ARG, "asr_wave_pvoc: null pointer");
    ASR_REQUIRE(rate_stride > 0, ASR_E_ARG, "asr_wave_pvoc: rate_stride must be positive");
    WA_COMMON_REQUIRE("asr_wave_pvoc");
    WA_FFT_REQUIRE("asr_wave_pvoc");
    (void)lg;
    wa_launch_pvoc(spec, wav_len, rates, rate_stride, out, B, N, n_fft, (hipStream_t)stream);
    ASR_LAUNCH_CHECK("asr_wave_pvoc");
    return ASR_OK;
}

extern "C" int asr_wave_istft(const float* out_spec, const int64_t* wav_len, const float* rates, int rate_stride, const float* table,
                              float* dst, long dst_stride, int keep_len, int B, int N, int n_fft, void* stream) {
    ASR_REQUIRE(out_spec && wav_len && rates && table && dst, ASR_E_ARG, "asr_wave_istft: null pointer");
    ASR_REQUIRE(rate_stride > 0, ASR_E_ARG, "asr_wave_istft: rate_stride must be positive");
    WA_COMMON_REQUIRE("asr_wave_istft");
    WA_FFT_REQUIRE("asr_wave_istft");
    ASR_REQUIRE(keep_len == 0 || keep_len == 1, ASR_E_ARG, "asr_wave_istft: keep_len must be 0 or 1");
    ASR_REQUIRE(dst_stride >= (keep_len ? (long)N : 2L * N), ASR_E_ARG, "asr_wave_istft: dst_stride = %ld is below %ld", dst_stride,
                keep_len ? (long)N : 2L * N);
    wa_launch_istft(out_spec, wav_len, rates, rate_stride, table, dst, dst_stride, keep_len, B, N, n_fft, lg, (hipStream_t)stream);
    ASR_LAUNCH_CHECK("asr_wave_istft");
    return ASR_OK;
}

extern "C" int asr_wave_resample(const float* src, long src_stride, const int64_t* wav_len, const float* rates, int rate_stride, float* wav,
                                 int B, int N, int n_fft, void* stream) {
    ASR_REQUIRE(src && wav_len && rates && wav, ASR_E_ARG, "asr_wave_resample: null pointer");
    ASR_REQUIRE(rate_stride > 0, ASR_E_ARG, "asr_wave_resample: rate_stride must be positive");
    WA_COMMON_REQUIRE("asr_wave_resample");
    WA_FFT_REQUIRE("asr_wave_resample");
    (void)lg;
    ASR_REQUIRE(src_stride >= 2L * N, ASR_E_ARG, "asr_wave_resample: src_stride = %ld is below 2 N = %ld", src_stride, 2L * N);
    wa_launch_resample(src, src_stride, wav_len, rates, rate_stride, wav, B, N, n_fft, (hipStream_t)stream);
    ASR_LAUNCH_CHECK("asr_wave_resample");
    return ASR_OK;
}

// work area: draws (B,6) and rates (B,2), then for a slice of S utterances the spectrogram (F frames), the stretched one (2F
// frames: the worst legal rate, 0.5) and the stretched wave of the pitch stage (2N samples).  S is the largest count whose
// three areas stay below WA_CAP_BYTES (at least 1).
static int wa_slice(int B, int N, int n_fft) {
    const size_t per = 3 * wa_spec_bytes(N, n_fft) + (size_t)2 * N * sizeof(float);
    const size_t s = WA_CAP_BYTES / per;
    return (int)(s < 1 ? 1 : (s > (size_t)B ? (size_t)B : s));
}

extern "C" size_t asr_wave_augment_workspace_bytes(int B, int N, int n_fft) {
    if (B <= 0 || N <= 0 || N > (1 << 28) || wa_log2(n_fft) < 0) return 0;
    const size_t S = (size_t)wa_slice(B, N, n_fft), sp = wa_spec_bytes(N, n_fft);
    return wa_align((size_t)B * 8 * sizeof(float)) + wa_align(S * sp) + wa_align(S * 2 * sp) + wa_align(S * 2 * N * sizeof(float));
}

extern "C" int asr_wave_augment(float* wav, const int64_t* wav_len, const float* draws_in, float* draws_out, const float* table, int B,
                                int N, int n_fft, uint64_t seed, void* workspace, size_t workspace_bytes, void* stream) {
    ASR_REQUIRE(wav && wav_len && table && workspace, ASR_E_ARG, "asr_wave_augment: null pointer");
    WA_COMMON_REQUIRE("asr_wave_augment");
    WA_FFT_REQUIRE("asr_wave_augment");
    ASR_REQUIRE(workspace_bytes >= asr_wave_augment_workspace_bytes(B, N, n_fft) && ((uintptr_t)workspace & 15) == 0, ASR_E_ARG,
                "asr_wave_augment: workspace too small (%zu bytes needed) or not 16-byte aligned", asr_wave_augment_workspace_bytes(B, N, n_fft));
    hipStream_t st = (hipStream_t)stream;
    const int S = wa_slice(B, N, n_fft);
    const size_t sp = wa_spec_bytes(N, n_fft);
    char* base = (char*)workspace;
    float* draws = (float*)base;
    float* rates = draws + (size_t)B * 6;
    base += wa_align((size_t)B * 8 * sizeof(float));
    float* spec = (float*)base;
    base += wa_align((size_t)S * sp);
    float* ospec = (float*)base;
    base += wa_align((size_t)S * 2 * sp);
    float* work = (float*)base;
    hipLaunchKernelGGL(wave_draws_kernel, dim3(cdiv(B, 64)), dim3(64), 0, st, wav_len, draws_in, draws, draws_out, rates, B, N, n_fft,
                       seed);
    hipLaunchKernelGGL(wave_noise_kernel, dim3(cdiv(cdiv(N, 4), 256), B), dim3(256), 0, st, wav, wav_len, (const float*)draws, B, N, seed);
    for (int stage = 0; stage < 2; ++stage) {
        for (int s0 = 0; s0 < B; s0 += S) {
            const int sb = min(S, B - s0);
            float* w = wav + (size_t)s0 * N;
            const int64_t* l = wav_len + s0;
            const float* r = rates + (size_t)s0 * 2 + stage;
            wa_launch_stft(w, l, r, 2, table, spec, sb, N, n_fft, lg, st);
            wa_launch_pvoc(spec, l, r, 2, ospec, sb, N, n_fft, st);
            if (stage == 0) {
                wa_launch_istft(ospec, l, r, 2, table, w, (long)N, 1, sb, N, n_fft, lg, st);
            } else {
                wa_launch_istft(ospec, l, r, 2, table, work, 2L * N, 0, sb, N, n_fft, lg, st);
                wa_launch_resample(work, 2L * N, l, r, 2, w, sb, N, n_fft, st);
            }
        }
    }
    ASR_LAUNCH_CHECK("asr_wave_augment");
    return ASR_OK;
}
