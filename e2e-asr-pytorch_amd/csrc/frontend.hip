// Acoustic front-end on the GPU, batched over utterances (the reference runs it per file on CPU workers):
//   asr_fbank       : ExtractAudioFeature.forward (src/audio.py:158-171,231-244): pre-emphasis -> STFT
//                     (n_fft 1025, hann 400 centred, hop 160, center + reflect pad) -> |.| -> mel (80 x 513)
//                     -> 20 log10(max(x,1e-5)) - ref_db -> clamp((x - min_db) / -min_db, 0, 1)
//                     The DFT is a contraction of the 400 windowed samples of each frame with a (1026 x 400)
//                     cos/-sin table (exact fp32 MFMA), the mel projection a second contraction.
//   asr_delta_stack : Delta (src/audio.py:59-93) + Postprocess (:108-121): cross-correlation along time with
//                     the order-k delta filters, zero padding at the utterance ends, channel-major stacking.
//   asr_specaug     : Augment (src/audio.py:364-406): one time mask and one frequency mask per utterance,
//                     filled with the mean (recomputed after the time mask), in place on the padded batch.
//   asr_cmvn        : CMVN.forward (src/audio.py:31-34) between Delta and Augment: every column of an utterance minus its mean
//                     over the valid frames, over (eps + unbiased standard deviation), in place on the padded batch.
// Every length is taken as min(length, padded extent).  An utterance shorter than the time-mask width, or a feature axis
// narrower than the frequency-mask width, draws its mask width below its own extent (specaug_draws); the reference raises there.
#include "common.h"
#include "gemm_plan.h"

namespace {

// frames[(b*T + k), m] = hann[m] * y_b[reflect(k*hop + (n_fft-win)/2 + m - n_fft/2)],  y = pre-emphasised wave
__global__ void frame_kernel(const float* __restrict__ wav, const int64_t* __restrict__ wav_len, float* __restrict__ frames,
                             const float* __restrict__ window, int B, int N, int T, int win, int hop, int n_fft, float preemph) {
    const long total = (long)B * T * win;
    const int off = (n_fft - win) / 2 - n_fft / 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int m = (int)(i % win);
        const int k = (int)((i / win) % T);
        const int b = (int)(i / ((long)win * T));
        const int n = (int)min(wav_len[b], (int64_t)N);
        float v = 0.f;
        if (n > 1 && k < 1 + (n - 1) / hop) {   // center padding n_fft/2 each side with odd n_fft: 1 + (n-1)/hop frames
            int p = k * hop + off + m;
            if (p < 0) p = -p;
            if (p >= n) p = 2 * (n - 1) - p;
            p = max(0, min(p, n - 1));
            const float* x = wav + (long)b * N;
            const float y = (p == 0) ? x[0] : x[p] - preemph * x[p - 1];
            v = window[m] * y;
        }
        frames[i] = v;
    }
}

__global__ void magnitude_kernel(const float* __restrict__ spec, float* __restrict__ mag, long rows, int nbins) {
    // spec: (rows, 2*nbins) = [re | im]
    const long total = rows * nbins;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / nbins;
        const int f = (int)(i % nbins);
        const float re = spec[r * 2 * nbins + f], im = spec[r * 2 * nbins + nbins + f];
        mag[i] = sqrtf(re * re + im * im);
    }
}

__global__ void logmel_kernel(float* __restrict__ mel, const int64_t* __restrict__ wav_len, long rows, int N, int T, int nmel, int hop,
                              float ref_db, float min_db) {
    const long total = rows * nmel;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / nmel;
        const int b = (int)(r / T), k = (int)(r % T);
        float v = 0.f;
        if (k < 1 + ((int)min(wav_len[b], (int64_t)N) - 1) / hop) {
            const float db = 20.f * log10f(fmaxf(mel[i], 1e-5f)) - ref_db;
            v = fminf(fmaxf((db - min_db) / -min_db, 0.f), 1.f);
        }
        mel[i] = v;   // frames beyond the utterance are zero padding
    }
}

// out[b,t,c*F+f] = sum_j filt[c][j] * x[b, t + j - pad, f], zero outside [0, len_b)
__global__ void delta_stack_kernel(const float* __restrict__ x, const int64_t* __restrict__ lens, float* __restrict__ out,
                                   const float* __restrict__ filt, int B, int T, int F, int C, int taps) {
    const long total = (long)B * T * C * F;
    const int pad = (taps - 1) / 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int f = (int)(i % F);
        const int c = (int)((i / F) % C);
        const int t = (int)((i / ((long)F * C)) % T);
        const int b = (int)(i / ((long)F * C * T));
        const int len = (int)min(lens[b], (int64_t)T);
        float acc = 0.f;
        if (t < len) {
            for (int j = 0; j < taps; ++j) {
                const int tt = t + j - pad;
                if (tt >= 0 && tt < len) acc += filt[c * taps + j] * x[((long)b * T + tt) * F + f];
            }
        }
        out[i] = acc;
    }
}

// SpecAugment draws of utterance b, stated once for the three kernels: dr = {t, t0, tend, f, f0, fend} (reference draw order),
// 0 <= t0 <= tend <= len and 0 <= f0 <= fend <= D on return; t == 0 / f == 0 is an empty band (tend = t0 / fend = f0).
//   device draws: t = r0 % min(Tmask, max(len, 1)), t0 = r1 % max(len - t, 1), tend = t0 + r2 % t; f = r3 % min(Fmask, D),
//                 f0 = r4 % (D - f), fend = f0 + r5 % f - the reference's draws wherever it has any (len >= Tmask, D >= Fmask);
//   draws_in    : t and f as given, the bands clamped into the utterance.
__device__ __forceinline__ void specaug_draws(int b, int len, int D, int Tmask, int Fmask, uint64_t seed, const int* draws_in, int (&dr)[6]) {
    len = max(len, 0);
    if (draws_in) {
        for (int i = 0; i < 6; ++i) dr[i] = draws_in[b * 6 + i];
        dr[1] = min(max(dr[1], 0), len);
        dr[2] = (dr[0] > 0) ? min(max(dr[2], dr[1]), len) : dr[1];
        dr[4] = min(max(dr[4], 0), D);
        dr[5] = (dr[3] > 0) ? min(max(dr[5], dr[4]), D) : dr[4];
    } else {
        uint32_t r[4], r2[4];
        philox4x32((uint32_t)b, 0u, 1u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
        philox4x32((uint32_t)b, 0u, 2u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r2);
        const int t = (int)(r[0] % (uint32_t)min(Tmask, max(len, 1)));
        const int t0 = (int)(r[1] % (uint32_t)max(len - t, 1));
        const int tend = (t > 0) ? t0 + (int)(r[2] % (uint32_t)t) : t0;
        const int f = (int)(r[3] % (uint32_t)min(Fmask, D));
        const int f0 = (int)(r2[0] % (uint32_t)(D - f));
        const int fend = (f > 0) ? f0 + (int)(r2[1] % (uint32_t)f) : f0;
        dr[0] = t; dr[1] = t0; dr[2] = tend; dr[3] = f; dr[4] = f0; dr[5] = fend;
    }
}

// SpecAugment: one workgroup per utterance.  draws[b] = {t, t0, tend, f, f0, fend} (reference draw order).
__global__ __launch_bounds__(1024) void specaug_kernel(float* __restrict__ x, const int64_t* __restrict__ lens,
                                                       const int* __restrict__ draws_in, int* __restrict__ draws_out,
                                                       int B, int T, int D, int Tmask, int Fmask, uint64_t seed) {
    __shared__ double s_red[16];
    __shared__ int s_draw[6];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int len = min((int)lens[b], T);
    float* xb = x + (long)b * T * D;
    if (tid == 0) {
        int dr[6];
        specaug_draws(b, len, D, Tmask, Fmask, seed, draws_in, dr);
        for (int i = 0; i < 6; ++i) { s_draw[i] = dr[i]; if (draws_out) draws_out[b * 6 + i] = dr[i]; }
    }
    __syncthreads();
    const int t0 = s_draw[1], tend = s_draw[2], f0 = s_draw[4], fend = s_draw[5];
    if (len <= 0) return;
    // sums over the valid region and over the rows of the time mask
    double sum = 0.0, srow = 0.0;
    const long n = (long)len * D;
    for (long i = tid; i < n; i += 1024) {
        const float v = xb[i];
        sum += v;
        const int t = (int)(i / D);
        if (t >= t0 && t < tend) srow += v;
    }
    for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o); srow += __shfl_xor(srow, o); }
    if ((tid & 63) == 0) s_red[tid >> 6] = sum;
    __syncthreads();
    double tot = 0.0;
    for (int i = 0; i < 16; ++i) tot += s_red[i];
    __syncthreads();
    if ((tid & 63) == 0) s_red[tid >> 6] = srow;
    __syncthreads();
    double rowtot = 0.0;
    for (int i = 0; i < 16; ++i) rowtot += s_red[i];
    const float mean1 = (float)(tot / (double)n);
    const double nrow = (double)(tend - t0) * D;
    const float mean2 = (float)((tot - rowtot + (double)mean1 * nrow) / (double)n);   // mean after the time mask
    for (long i = tid; i < n; i += 1024) {
        const int t = (int)(i / D), f = (int)(i % D);
        if (f >= f0 && f < fend) xb[i] = mean2;
        else if (t >= t0 && t < tend) xb[i] = mean1;
    }
}

// ---- the same in two launches over many workgroups (asr_specaug_ws): one workgroup per utterance reads 0.77 MB alone (114 us at
// C2); here SA_SPLIT workgroups per utterance form partial sums (fixed slots, summed in fixed order: deterministic), then only the
// masked rows / columns are written.
constexpr int SA_SPLIT = 16;

__global__ __launch_bounds__(256) void specaug_sum_kernel(const float* __restrict__ x, const int64_t* __restrict__ lens,
                                                          const int* __restrict__ draws_in, int* __restrict__ draws_out,
                                                          double* __restrict__ part, int B, int T, int D, int Tmask, int Fmask, uint64_t seed) {
    __shared__ double s_red[2][4];
    const int b = blockIdx.y, sp = blockIdx.x, tid = threadIdx.x;
    const int len = min((int)lens[b], T);
    int dr[6];
    specaug_draws(b, len, D, Tmask, Fmask, seed, draws_in, dr);          // every workgroup derives the same draws
    if (sp == 0 && tid == 0 && draws_out) for (int i = 0; i < 6; ++i) draws_out[b * 6 + i] = dr[i];
    const int t0 = dr[1], tend = dr[2];
    const float* xb = x + (long)b * T * D;
    const long n = (long)max(len, 0) * D;
    const long per = (n + SA_SPLIT - 1) / SA_SPLIT, i0 = sp * per, i1 = min(n, i0 + per);
    double sum = 0.0, srow = 0.0;
    for (long i = i0 + tid; i < i1; i += 256) {
        const float v = xb[i];
        sum += v;
        const int t = (int)(i / D);
        if (t >= t0 && t < tend) srow += v;
    }
    for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o); srow += __shfl_xor(srow, o); }
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = sum; s_red[1][tid >> 6] = srow; }
    __syncthreads();
    if (tid == 0) {
        part[((long)b * SA_SPLIT + sp) * 2] = (s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3]);
        part[((long)b * SA_SPLIT + sp) * 2 + 1] = (s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]);
    }
}

__global__ __launch_bounds__(256) void specaug_apply_kernel(float* __restrict__ x, const int64_t* __restrict__ lens,
                                                            const int* __restrict__ draws_in, const double* __restrict__ part,
                                                            int B, int T, int D, int Tmask, int Fmask, uint64_t seed) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int len = min((int)lens[b], T);
    if (len <= 0) return;
    int dr[6];
    specaug_draws(b, len, D, Tmask, Fmask, seed, draws_in, dr);
    const int t0 = dr[1], tend = dr[2], f0 = dr[4], fend = dr[5];
    double tot = 0.0, rowtot = 0.0;
    for (int i = 0; i < SA_SPLIT; ++i) { tot += part[((long)b * SA_SPLIT + i) * 2]; rowtot += part[((long)b * SA_SPLIT + i) * 2 + 1]; }
    const long n = (long)len * D;
    const float mean1 = (float)(tot / (double)n);
    const double nrow = (double)(tend - t0) * D;
    const float mean2 = (float)((tot - rowtot + (double)mean1 * nrow) / (double)n);   // mean after the time mask
    float* xb = x + (long)b * T * D;
    const int fw = fend - f0, tw = tend - t0;
    // frequency band: columns f0..fend of every valid row; time band: rows t0..tend outside that band
    const long nf = (long)len * fw, nt = (long)tw * D;
    for (long i = blockIdx.x * 256L + tid; i < nf + nt; i += (long)gridDim.x * 256) {
        if (i < nf) {
            const int t = (int)(i / fw), f = f0 + (int)(i - (long)t * fw);
            xb[(long)t * D + f] = mean2;
        } else {
            const long k = i - nf;
            const int t = t0 + (int)(k / D), f = (int)(k % D);
            if (!(f >= f0 && f < fend)) xb[(long)t * D + f] = mean1;
        }
    }
}

// ---- CMVN (asr_cmvn): per utterance and column, over the len valid frames, y = (x - mean) / (eps + unbiased std).  Two launches
// over CM_SPLIT x ceil(D / CM_COLS) workgroups per utterance.  Partial sp owns rows [sp R, min((sp + 1) R, len)), R = ceil(T /
// CM_SPLIT); a thread owns one column (a wave reads 64 neighbouring floats of a row) and every CM_LANES-th row of the range.
//   moments: float64 Welford (count, mean, M2) per thread, the CM_LANES states of a column merged in lane order (Chan), the
//            partial's (mean, M2) stored at its fixed slot part[((b CM_SPLIT + sp) 2 + {0,1}) D + d]; its count follows from len.
//   apply  : every workgroup merges the non-empty partials of its columns in sp order and normalises its own rows in place.
// No sum of squares is ever formed: M2 is a sum of non-negative terms w (difference)^2, so nothing cancels.  No atomics, fixed
// merge order: two calls on one input give the same bits.  Rows >= len are neither read nor written.
constexpr int CM_SPLIT = 16;
constexpr int CM_COLS = 64;
constexpr int CM_LANES = 4;
constexpr int CM_BATCH = 8;      // rows a thread loads before it uses them: one memory round trip per batch, not per row

// (na, ma, Ma) <- (na, ma, Ma) + (nb, mb, Mb); an empty side leaves the other as it is
__device__ __forceinline__ void cmvn_merge(int& na, double& ma, double& Ma, int nb, double mb, double Mb) {
    if (nb == 0) return;
    if (na == 0) { na = nb; ma = mb; Ma = Mb; return; }
    const double f = (double)nb / (double)(na + nb), d = mb - ma;       // the one division: counts only, off the data's chain
    ma += d * f;
    Ma += Mb + d * d * (double)na * f;
    na += nb;
}

// rows lane w of a partial with `rows` rows owns: w, w + CM_LANES, ...
__device__ __forceinline__ int cmvn_lane_rows(int rows, int w) { return rows > w ? (rows - w + CM_LANES - 1) / CM_LANES : 0; }

__global__ __launch_bounds__(CM_COLS * CM_LANES) void cmvn_moments_kernel(const float* __restrict__ x, const int64_t* __restrict__ lens,
                                                                           double* __restrict__ part, int B, int T, int D) {
    __shared__ double s_mean[CM_LANES][CM_COLS], s_m2[CM_LANES][CM_COLS];
    const int ntile = (D + CM_COLS - 1) / CM_COLS;
    const int sp = blockIdx.x / ntile, b = blockIdx.y, c = threadIdx.x % CM_COLS, w = threadIdx.x / CM_COLS;
    const int d = (blockIdx.x % ntile) * CM_COLS + c;
    const int len = (int)max(min(lens[b], (int64_t)T), (int64_t)0);
    const int R = (T + CM_SPLIT - 1) / CM_SPLIT;
    const int r0 = sp * R, r1 = min(len, r0 + R);
    if (r0 >= r1) return;                                       // an empty partial: its slot is never read
    int n = 0;
    double mean = 0.0, m2 = 0.0;
    if (d < D) {
        const float* xc = x + (long)b * T * D + d;
        for (int t = r0 + w; t < r1; t += CM_LANES * CM_BATCH) {
            float v[CM_BATCH];
#pragma unroll
            for (int j = 0; j < CM_BATCH; ++j) v[j] = (t + j * CM_LANES < r1) ? xc[(long)(t + j * CM_LANES) * D] : 0.f;
#pragma unroll
            for (int j = 0; j < CM_BATCH; ++j) {
                if (t + j * CM_LANES < r1) {
                    const double dl = (double)v[j] - mean;
                    mean += dl / (double)(++n);
                    m2 += dl * ((double)v[j] - mean);
                }
            }
        }
    }
    s_mean[w][c] = mean;
    s_m2[w][c] = m2;
    __syncthreads();
    if (w == 0 && d < D) {
        for (int k = 1; k < CM_LANES; ++k) cmvn_merge(n, mean, m2, cmvn_lane_rows(r1 - r0, k), s_mean[k][c], s_m2[k][c]);
        double* p = part + ((long)b * CM_SPLIT + sp) * 2 * D + d;
        p[0] = mean;
        p[D] = m2;
    }
}

__global__ __launch_bounds__(CM_COLS * CM_LANES) void cmvn_apply_kernel(float* __restrict__ x, const int64_t* __restrict__ lens,
                                                                         const double* __restrict__ part, float* __restrict__ stats,
                                                                         int B, int T, int D, float eps) {
    const int ntile = (D + CM_COLS - 1) / CM_COLS;
    const int sp = blockIdx.x / ntile, b = blockIdx.y, c = threadIdx.x % CM_COLS, w = threadIdx.x / CM_COLS;
    const int d = (blockIdx.x % ntile) * CM_COLS + c;
    if (d >= D) return;
    const int len = (int)max(min(lens[b], (int64_t)T), (int64_t)0);
    const int R = (T + CM_SPLIT - 1) / CM_SPLIT;
    const int r0 = sp * R, r1 = min(len, r0 + R);
    const bool writes_stats = stats && sp == 0 && w == 0;
    if (len <= 0) {
        if (writes_stats) { stats[(long)b * 2 * D + d] = 0.f; stats[((long)b * 2 + 1) * D + d] = 0.f; }
        return;
    }
    if (r0 >= r1) return;
    int n = 0;
    double mean = 0.0, m2 = 0.0;
    double pm[CM_SPLIT], pq[CM_SPLIT];
#pragma unroll
    for (int q = 0; q < CM_SPLIT; ++q) {                       // every load first, then the merges in range order
        const double* p = part + ((long)b * CM_SPLIT + q) * 2 * D + d;
        pm[q] = (q * R < len) ? p[0] : 0.0;
        pq[q] = (q * R < len) ? p[D] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < CM_SPLIT; ++q) cmvn_merge(n, mean, m2, max(min(len, (q + 1) * R) - q * R, 0), pm[q], pq[q]);
    const double sd = sqrt(m2 / (double)(len - 1));            // len == 1: 0 / 0, NaN as torch.std gives it
    if (writes_stats) { stats[(long)b * 2 * D + d] = (float)mean; stats[((long)b * 2 + 1) * D + d] = (float)sd; }
    const double den = (double)eps + sd;
    float* xc = x + (long)b * T * D + d;
    for (int t = r0 + w; t < r1; t += CM_LANES * CM_BATCH) {
        float v[CM_BATCH];
#pragma unroll
        for (int j = 0; j < CM_BATCH; ++j) v[j] = (t + j * CM_LANES < r1) ? xc[(long)(t + j * CM_LANES) * D] : 0.f;
#pragma unroll
        for (int j = 0; j < CM_BATCH; ++j)
            if (t + j * CM_LANES < r1) xc[(long)(t + j * CM_LANES) * D] = (float)(((double)v[j] - mean) / den);
    }
}

inline int grid_for(long n) { long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g)); }

}  // namespace

extern "C" size_t asr_fbank_workspace_bytes(int B, int T, int win, int n_fft) {
    const size_t rows = (size_t)B * T, nb = n_fft / 2 + 1;
    return (rows * win + rows * 2 * nb + rows * nb) * sizeof(float) + 1024;
}

extern "C" int asr_fbank(const float* wav, const int64_t* wav_len, float* out, const float* dft_table, const float* mel_fb,
                         const float* window, int B, int N, int T, int win, int hop, int n_fft, int nmel,
                         float preemph, float ref_db, float min_db,
                         void* workspace, size_t workspace_bytes, asr_stream_t stream) {
    ASR_REQUIRE(wav && wav_len && out && dft_table && mel_fb && window && workspace, ASR_E_ARG, "asr_fbank: null pointer");
    ASR_REQUIRE(B > 0 && N > 0 && T > 0 && win > 0 && hop > 0 && n_fft >= win && nmel > 0, ASR_E_ARG, "asr_fbank: bad dims");
    ASR_REQUIRE(n_fft & 1, ASR_E_ARG, "asr_fbank: n_fft %d is even (the frame count 1 + (n-1)/hop holds for odd n_fft)", n_fft);
    ASR_REQUIRE(workspace_bytes >= asr_fbank_workspace_bytes(B, T, win, n_fft), ASR_E_ARG, "asr_fbank: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const long rows = (long)B * T;
    const int nb = n_fft / 2 + 1;
    float* frames = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float* spec = frames + rows * win;
    float* mag = spec + rows * 2 * nb;
    hipLaunchKernelGGL(frame_kernel, dim3(grid_for(rows * win)), dim3(256), 0, st, wav, wav_len, frames, window, B, N, T, win, hop, n_fft, preemph);
    // spec (rows, 2*nb) = frames (rows, win) x table^T, table (2*nb, win): exact fp32 MFMA
    GemmCall dft{frames, dft_table, spec, nullptr, (int)rows, 2 * nb, win, win, win, 2 * nb};
    dft.prec = ASR_F32;
    int rc = gemm_run(dft, st);
    if (rc != ASR_OK) return rc;
    hipLaunchKernelGGL(magnitude_kernel, dim3(grid_for(rows * nb)), dim3(256), 0, st, spec, mag, rows, nb);
    GemmCall mel{mag, mel_fb, out, nullptr, (int)rows, nmel, nb, nb, nb, nmel};
    mel.prec = ASR_F32;
    rc = gemm_run(mel, st);
    if (rc != ASR_OK) return rc;
    hipLaunchKernelGGL(logmel_kernel, dim3(grid_for(rows * nmel)), dim3(256), 0, st, out, wav_len, rows, N, T, nmel, hop, ref_db, min_db);
    ASR_LAUNCH_CHECK("asr_fbank");
    return ASR_OK;
}

extern "C" int asr_delta_stack(const float* x, const int64_t* lens, float* out, const float* filters,
                               int B, int T, int F, int channels, int taps, asr_stream_t stream) {
    ASR_REQUIRE(x && lens && out && filters && B > 0 && T > 0 && F > 0 && channels > 0 && taps > 0 && (taps & 1), ASR_E_ARG,
                "asr_delta_stack: bad args");
    hipLaunchKernelGGL(delta_stack_kernel, dim3(grid_for((long)B * T * channels * F)), dim3(256), 0, (hipStream_t)stream, x, lens, out,
                       filters, B, T, F, channels, taps);
    ASR_LAUNCH_CHECK("asr_delta_stack");
    return ASR_OK;
}

extern "C" int asr_specaug(float* x, const int64_t* lens, const int* draws_in, int* draws_out, int B, int T, int D,
                           int time_width, int freq_width, uint64_t seed, asr_stream_t stream) {
    ASR_REQUIRE(x && lens && B > 0 && T > 0 && D > 0 && time_width > 0 && freq_width > 0, ASR_E_ARG, "asr_specaug: bad args");
    hipLaunchKernelGGL(specaug_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, x, lens, draws_in, draws_out, B, T, D,
                       time_width, freq_width, seed);
    ASR_LAUNCH_CHECK("asr_specaug");
    return ASR_OK;
}


extern "C" size_t asr_specaug_workspace_bytes(int B) { return (size_t)(B > 0 ? B : 0) * SA_SPLIT * 2 * sizeof(double); }

// asr_specaug with its reductions spread over SA_SPLIT workgroups per utterance (same arithmetic, same draws)
extern "C" int asr_specaug_ws(float* x, const int64_t* lens, const int* draws_in, int* draws_out, int B, int T, int D,
                              int time_width, int freq_width, uint64_t seed, void* workspace, size_t workspace_bytes, asr_stream_t stream) {
    ASR_REQUIRE(x && lens && workspace && B > 0 && T > 0 && D > 0 && time_width > 0 && freq_width > 0, ASR_E_ARG, "asr_specaug_ws: bad args");
    ASR_REQUIRE(workspace_bytes >= asr_specaug_workspace_bytes(B) && ((uintptr_t)workspace & 7) == 0, ASR_E_ARG, "asr_specaug_ws: workspace too small or unaligned");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(specaug_sum_kernel, dim3(SA_SPLIT, B), dim3(256), 0, st, x, lens, draws_in, draws_out, (double*)workspace, B, T, D,
                       time_width, freq_width, seed);
    hipLaunchKernelGGL(specaug_apply_kernel, dim3(8, B), dim3(256), 0, st, x, lens, draws_in, (const double*)workspace, B, T, D,
                       time_width, freq_width, seed);
    ASR_LAUNCH_CHECK("asr_specaug_ws");
    return ASR_OK;
}

extern "C" size_t asr_cmvn_workspace_bytes(int B, int D) {
    return (size_t)(B > 0 ? B : 0) * CM_SPLIT * 2 * (size_t)(D > 0 ? D : 0) * sizeof(double);
}

extern "C" int asr_cmvn(float* x, const int64_t* lens, float* stats_out, int B, int T, int D, float eps,
                        void* workspace, size_t workspace_bytes, asr_stream_t stream) {
    ASR_REQUIRE(x && lens && workspace && B > 0 && T > 0 && D > 0, ASR_E_ARG, "asr_cmvn: bad args");
    ASR_REQUIRE(B <= 65535, ASR_E_ARG, "asr_cmvn: B = %d is beyond one grid axis", B);
    ASR_REQUIRE(workspace_bytes >= asr_cmvn_workspace_bytes(B, D) && ((uintptr_t)workspace & 7) == 0, ASR_E_ARG,
                "asr_cmvn: workspace too small or unaligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(CM_SPLIT * ((D + CM_COLS - 1) / CM_COLS), B), block(CM_COLS * CM_LANES);
    hipLaunchKernelGGL(cmvn_moments_kernel, grid, block, 0, st, x, lens, (double*)workspace, B, T, D);
    hipLaunchKernelGGL(cmvn_apply_kernel, grid, block, 0, st, x, lens, (const double*)workspace, stats_out, B, T, D, eps);
    ASR_LAUNCH_CHECK("asr_cmvn");
    return ASR_OK;
}
