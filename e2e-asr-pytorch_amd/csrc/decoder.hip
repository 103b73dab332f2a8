// Location-aware attention + LSTM decoder ("speller") of the joint CTC-attention model: the whole
// decode loop of ASR.forward (reference src/asr.py:123-175) and its backward as two C-ABI calls.
//   per step t:  query = tanh(W_q hcat_{t-1} + b_q)                                     (src/asr.py:337)
//                loc   = tanh(W_proj conv1d(prev_att))                                  (src/module.py:1163)
//                e     = w_g . tanh(key + query + loc) + b_g ; /temperature ; mask ; softmax
//                ctx   = attn . enc                                                     (src/module.py:1110-1117,1168)
//                (h,c) = LSTM([emb(prev token), ctx])  per decoder layer                (src/asr.py:141-143,259-266)
// after the loop: logits = W_c h_top + b_c for all steps at once (same arithmetic as the per-step
// char_trans, src/asr.py:265).  Greedy mode (teacher == NULL) also evaluates logits/argmax per step.
//
// Step kernels are bandwidth/latency bound: key (B,T',A) and enc (B,T',E) are re-read every step and
// stay resident in the 256 MB Infinity Cache between steps; one launch covers the whole batch.
#include "common.h"
#include "gemm_plan.h"
#include "decoder_internal.h"
#include <stdlib.h>
#include <initializer_list>
#include <type_traits>

namespace {

// Run-time switches that pick a template instantiation: f receives them as std::integral_constant arguments.
template <typename F> void with_bool(bool v, F&& f) { if (v) f(std::true_type{}); else f(std::false_type{}); }
// (Kn, h16) -> (KNMAX, H16) of the energy kernels, forward and backward: the location filters a thread holds in registers
template <typename F> void with_knmax_h16(int Kn, bool h16, F&& f) {
    with_bool(h16, [&](auto h) {
        if (Kn <= 4) f(std::integral_constant<int, 4>{}, h);
        else if (Kn <= 10) f(std::integral_constant<int, 10>{}, h);
        else f(std::integral_constant<int, 16>{}, h);
    });
}

// Tap ranges the location convolution of a tile (att_energy_kernel) and its transpose (att_bwd_conv_body) are split into, for
// nout = Kn * tile / 4 outputs per range over 512 threads.  Each range has a partial-sum tile in LDS: kernels and host sizes ask here.
__host__ __device__ inline int conv_parts(int nout) { const int p = 512 / nout; return p < 1 ? 1 : (p > 8 ? 8 : p); }

// tanh via one v_exp and one v_rcp: 1 - 2/(1+e^{2x}); absolute error ~2e-7 (the energy kernels evaluate ~6 M of these per step)
__device__ __forceinline__ float tanh_fast(float x) { return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * x)); }

// A batch of U strided global reads per thread whose values are consumed LATER (usually stored to LDS): the loads are
// unconditional from clamped indices, so several batches can be put in flight back to back and cost one round trip in
// all.  (A plain `for (i = tid; i < n; i += nthr) lds[i] = g[i];` costs one serialized round trip per iteration: the
// compiler branches around each bounds-checked load and waits for it.)  Elements beyond U*nthr: `rest`.
template <int U> struct Stage {
    float v[U];
    template <typename L> __device__ __forceinline__ void load(int n, int tid, int nthr, L ld) {
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = ld(max(min(tid + u * nthr, n - 1), 0));
    }
    template <typename S> __device__ __forceinline__ void store(int n, int tid, int nthr, S st) const {
#pragma unroll
        for (int u = 0; u < U; ++u) if (tid + u * nthr < n) st(tid + u * nthr, v[u]);
    }
    template <typename L, typename S> __device__ __forceinline__ void rest(int n, int tid, int nthr, L ld, S st) const {
        for (int i = tid + U * nthr; i < n; i += nthr) st(i, ld(i));
    }
};

__device__ __forceinline__ float bf2f(unsigned short x) { return __uint_as_float((unsigned)x << 16); }
// four consecutive bf16 (8 bytes, 8-byte aligned) -> float4
__device__ __forceinline__ float4 ld4_bf16(const unsigned short* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
}
__global__ void cast_bf16_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, long n) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dst[i] = f2bf_bits(src[i]);
}

// i / n for 0 <= i < 2^22, n <= 2^10 through a float reciprocal (a runtime integer division costs ~40 VALU instructions;
// the index maps of the staging loops do a dozen of them per thread per launch)
__device__ __forceinline__ int fdiv(int i, int n, float inv) {
    int q = (int)((float)i * inv);
    const int r = i - q * n;
    q += (r >= n) - (r < 0);
    return q;
}

struct DecP {
    asr_dec_dims_t d;
    asr_dec_weights_t w;
    asr_dec_state_t s;
    const float* enc;
    const int64_t* enc_len;
};

// ------------------------------------------------------------------------------------------------
// token embedding rows:  xin[b,t,0:Dd] = emb[tokens[b,t]]
// ------------------------------------------------------------------------------------------------
__global__ void shift_tokens_kernel(const int64_t* __restrict__ teacher, int64_t* __restrict__ tokens, int B, int L, int Lt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * L) return;
    const int b = i / L, t = i % L;
    tokens[i] = (t == 0) ? 0 : teacher[(long)b * Lt + (t - 1)];
}

__global__ void embed_kernel(const float* __restrict__ emb, const int64_t* __restrict__ tokens, float* __restrict__ xin,
                             int B, int L, int Dd, int XW, int t0, int nt, int V) {
    // rows (b, t) for t in [t0, t0+nt)
    const long total = (long)B * nt * Dd;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % Dd);
        const int t = t0 + (int)((i / Dd) % nt);
        const int b = (int)(i / ((long)Dd * nt));
        long tok = tokens[(long)b * L + t];
        tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
        xin[((long)b * L + t) * XW + k] = emb[tok * Dd + k];
    }
}

// ------------------------------------------------------------------------------------------------
// K1: query projection  q[b,t,:] = tanh(W_q hcat_{t-1}[b] + b_q);  one wave per 16 output columns
// ------------------------------------------------------------------------------------------------
template <bool BF16>
__global__ __launch_bounds__(256) void dec_query_kernel(DecP p, int t) {
    __shared__ float red[4][256];
    const asr_dec_dims_t& d = p.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, q = lane >> 4;
    const int a = blockIdx.x * 16 + n;
    const bool aok = a < d.A;
    const float* wrow = p.w.Wq + (long)(aok ? a : 0) * d.Q;
    const bool vec = (d.Q % 4) == 0;
    for (int m0 = 0; m0 < d.B; m0 += 16) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (t > 0) {
            const int ab = m0 + n;
            const bool rok = ab < d.B;
            const float* hrow = p.s.hs + ((long)(rok ? ab : 0) * d.L + (t - 1)) * d.Q;
            acc = dot_rows<BF16>(hrow, rok, wrow, aok, d.Q, wave, 4, vec, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][(4 * q + r) * 16 + n] = acc[r];
        __syncthreads();
        const int row = tid >> 4, col = tid & 15;
        const int b = m0 + row, ac = blockIdx.x * 16 + col;
        if (b < d.B && ac < d.A)
            p.s.q[((long)b * d.L + t) * d.A + ac] = tanhf(red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid] + p.w.bq[ac]);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// K2: energies.  grid (ceil(T'/TE), B), TE = 8 waves x TPW frames; wave w owns frames w*TPW.., lanes sweep the
// attention dimension.  TPW is chosen by the host so that the whole batch is ONE round of workgroups (<= 1 per CU):
// the kernel is a chain of dependent round trips (window -> conv -> keys -> reduce), not bandwidth, so a second
// round of workgroups doubles its time.  Every global operand of the sweep is requested before the location
// convolution is computed; the convolution itself is spread over all 512 threads (tap ranges x 4-frame groups).
// conv (B,L,Kn,T') is kept for the backward pass when state.conv != NULL.
// ------------------------------------------------------------------------------------------------
// Floats of the kernel's dynamic LDS regions, in order: previous attention window [win], location filters [Kn*taps], conv output
// of the tile [Kn*TE], W_proj transposed [Kn][A], partial conv sums [parts][Kn*TE].  The kernel chains its pointers over them and
// energy_plan sums them (lds_bytes); the *_regions functions of the backward kernels below serve the same two readers.
__host__ __device__ inline void energy_regions(int TE, int Kn, int Ks, int A, int n[4]) {      // the partial sums close the carve
    n[0] = (TE + 2 * Ks + 3) & ~3; n[1] = (Kn * (2 * Ks + 1) + 3) & ~3; n[2] = Kn * TE; n[3] = (Kn * A + 3) & ~3;
}
inline size_t lds_bytes(const int* n, int count) { size_t f = 0; for (int i = 0; i < count; ++i) f += n[i]; return sizeof(float) * f; }

template <int KNMAX, int TPW, bool H16>
__global__ __launch_bounds__(512) void att_energy_kernel(DecP p, int t) {
    constexpr int TE = 8 * TPW, NA = 5;                 // NA: attention columns per lane held in flight
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const asr_dec_dims_t& d = p.d;
    const int b = blockIdx.y, tau0 = blockIdx.x * TE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int taps = 2 * d.Ks + 1, win = TE + 2 * d.Ks;
    const int len = min((int)p.enc_len[b], d.Tp);
    int n[4];
    energy_regions(TE, d.Kn, d.Ks, d.A, n);
    float *s_pa = smem_f, *s_wc = s_pa + n[0], *s_conv = s_wc + n[1], *s_wp = s_conv + n[2], *s_part = s_wp + n[3];
    // ---- stage 0: every global read that does not depend on the convolution, all in flight together
    const float* prev = (t > 0) ? p.s.att + ((long)b * d.L + (t - 1)) * d.Tp : nullptr;
    const float uni = 1.f / (float)max(len, 1);
    auto ld_pa = [&](int i) { return prev[min(max(tau0 + i - d.Ks, 0), d.Tp - 1)]; };
    auto st_pa = [&](int i, float v) {
        const int tau = tau0 + i - d.Ks;
        s_pa[i] = (tau >= 0 && tau < d.Tp) ? (prev ? v : (tau < len ? uni : 0.f)) : 0.f;
    };
    auto ld_wc = [&](int i) { return p.w.Wconv[i]; };
    auto st_wc = [&](int i, float v) { s_wc[i] = v; };
    auto ld_wp = [&](int i) { return p.w.Wproj[i]; };
    const float inv_kn = 1.f / (float)d.Kn;
    auto st_wp = [&](int i, float v) { const int a = fdiv(i, d.Kn, inv_kn), k = i - a * d.Kn; s_wp[k * d.A + a] = v; };
    Stage<2> g_pa; Stage<4> g_wc; Stage<6> g_wp;
    g_pa.v[0] = g_pa.v[1] = 0.f;
    if (prev) g_pa.load(win, tid, 512, ld_pa);
    g_wc.load(d.Kn * taps, tid, 512, ld_wc);
    g_wp.load(d.Kn * d.A, tid, 512, ld_wp);
    const float* qrow = p.s.q + ((long)b * d.L + t) * d.A;
    const int tmax = max(len - 1, 0);
    float kv[NA][TPW], qa[NA], wga[NA];
    auto load_cols = [&](int a0) {
#pragma unroll
        for (int c = 0; c < NA; ++c) {
            const int a = min(a0 + 64 * c + lane, d.A - 1);
            qa[c] = qrow[a]; wga[c] = p.w.wg[a];
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const long ki = ((long)b * d.Tp + min(tau0 + wave * TPW + i, tmax)) * d.A + a;
                kv[c][i] = H16 ? bf2f(reinterpret_cast<const unsigned short*>(p.s.key16)[ki]) : p.s.key[ki];
            }
        }
    };
    load_cols(0);
    g_pa.store(win, tid, 512, st_pa);
    g_wc.store(d.Kn * taps, tid, 512, st_wc);
    g_wp.store(d.Kn * d.A, tid, 512, st_wp);
    g_pa.rest(win, tid, 512, [&](int i) { return prev ? ld_pa(i) : 0.f; }, st_pa);
    g_wc.rest(d.Kn * taps, tid, 512, ld_wc, st_wc);
    g_wp.rest(d.Kn * d.A, tid, 512, ld_wp, st_wp);
    __syncthreads();
    // ---- stage 1: conv[k][i] = sum_j Wconv[k][j] * pa[i + j];  item = (tap range, k, group of 4 frames)
    {
        const int ngrp = TE / 4, nout = d.Kn * ngrp;
        const int parts = conv_parts(nout);
        const int tp = (taps + parts - 1) / parts;
        const float inv_nout = 1.f / (float)nout;
        for (int it = tid; it < parts * nout; it += 512) {
            const int pz = fdiv(it, nout, inv_nout), o = it - pz * nout, k = o / ngrp, ig = o - k * ngrp;   // ngrp is a constant
            const int j0 = pz * tp, j1 = min(taps, j0 + tp);
            const float* wk = s_wc + k * taps;
            const float* pa = s_pa + 4 * ig;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            float p0 = pa[j0], p1 = pa[j0 + 1], p2 = pa[j0 + 2];
            for (int j = j0; j < j1; ++j) {
                const float w = wk[j], p3 = pa[j + 3];
                a0 += w * p0; a1 += w * p1; a2 += w * p2; a3 += w * p3;
                p0 = p1; p1 = p2; p2 = p3;
            }
            float* o4 = s_part + (long)pz * d.Kn * TE + k * TE + 4 * ig;
            o4[0] = a0; o4[1] = a1; o4[2] = a2; o4[3] = a3;
        }
        __syncthreads();
        for (int o = tid; o < d.Kn * TE; o += 512) {
            float v = 0.f;
            for (int pz = 0; pz < parts; ++pz) v += s_part[(long)pz * d.Kn * TE + o];
            s_conv[o] = v;
            const int k = o / TE, tau = tau0 + (o - k * TE);
            if (p.s.conv && tau < d.Tp) p.s.conv[(((long)b * d.L + t) * d.Kn + k) * d.Tp + tau] = v;
        }
        __syncthreads();
    }
    // ---- stage 2: sweep.  The wave's conv values are the same for every lane: keep them in registers.
    float cv[KNMAX][TPW];
#pragma unroll
    for (int k = 0; k < KNMAX; ++k)
#pragma unroll
        for (int i = 0; i < TPW; ++i) cv[k][i] = (k < d.Kn) ? s_conv[k * TE + wave * TPW + i] : 0.f;
    float e[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) e[i] = 0.f;
    for (int a0 = 0; a0 < d.A; a0 += 64 * NA) {
        if (a0 > 0) load_cols(a0);
#pragma unroll
        for (int c = 0; c < NA; ++c) {
            const int a = a0 + 64 * c + lane;
            const bool aok = a < d.A;
            const int ac = aok ? a : d.A - 1;
            float wp[KNMAX];
#pragma unroll
            for (int k = 0; k < KNMAX; ++k) wp[k] = (k < d.Kn) ? s_wp[k * d.A + ac] : 0.f;
            const float wg_ = aok ? wga[c] : 0.f;
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                float lp = 0.f;
#pragma unroll
                for (int k = 0; k < KNMAX; ++k) lp += wp[k] * cv[k][i];
                e[i] += wg_ * tanh_fast(kv[c][i] + qa[c] + tanh_fast(lp));
            }
        }
    }
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const float s = wave_sum(e[i]);
        const int tau = tau0 + wave * TPW + i;
        if (lane == 0 && tau < d.Tp)
            p.s.energy[(long)b * d.Tp + tau] = (tau < len) ? (s + p.w.bg[0]) / d.temperature : -INFINITY;
    }
}

// block-wide reductions over 256 threads (4 waves)
__device__ __forceinline__ float block_max(float v, float* s4) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(s4[0], s4[1]), fmaxf(s4[2], s4[3]));
}
__device__ __forceinline__ float block_sum(float v, float* s4) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return s4[0] + s4[1] + s4[2] + s4[3];
}

// ------------------------------------------------------------------------------------------------
// K3: softmax over T' + context.  grid (ceil(E/64), B); every block redoes the (cheap) softmax of its
// utterance and owns 64 columns of the context vector; block x == 0 also stores the attention row.
// ------------------------------------------------------------------------------------------------
template <bool H16>
__global__ __launch_bounds__(256) void att_softmax_ctx_kernel(DecP p, int t) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    __shared__ float s4[4];
    __shared__ float red[4][64];
    const asr_dec_dims_t& d = p.d;
    const int b = blockIdx.y, e0 = blockIdx.x * 64;
    const int len = min((int)p.enc_len[b], d.Tp);
    float* s_att = smem_f;  // [Tp]
    const float* en = p.s.energy + (long)b * d.Tp;
    float m = -INFINITY;
    {
        Stage<4> g_en;                     // the whole energy row in one round trip (T' <= 1024; the rest in a plain loop)
        g_en.load(d.Tp, threadIdx.x, 256, [&](int i) { return en[i]; });
        g_en.store(d.Tp, threadIdx.x, 256, [&](int i, float v) { s_att[i] = v; m = fmaxf(m, v); });
        g_en.rest(d.Tp, threadIdx.x, 256, [&](int i) { return en[i]; }, [&](int i, float v) { s_att[i] = v; m = fmaxf(m, v); });
    }
    m = block_max(m, s4);
    float sum = 0.f;
    for (int i = threadIdx.x; i < d.Tp; i += 256) { const float v = expf(s_att[i] - m); s_att[i] = v; sum += v; }
    sum = block_sum(sum, s4);
    const float inv = 1.f / sum;
    for (int i = threadIdx.x; i < d.Tp; i += 256) {
        const float a = s_att[i] * inv;
        s_att[i] = a;
        if (blockIdx.x == 0) p.s.att[((long)b * d.L + t) * d.Tp + i] = a;
    }
    __syncthreads();
    float* xrow = p.s.xin + ((long)b * d.L + t) * (d.Dd + d.E) + d.Dd;
    if ((d.E & 3) == 0) {
        // 16 lanes x float4 cover the block's 64 columns; 16 frame groups, 4 independent loads in flight each
        const int c4 = threadIdx.x & 15, grp = threadIdx.x >> 4;
        const int ecol = e0 + 4 * c4;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ecol < d.E) {
            const float* ep = p.enc + (long)b * d.Tp * d.E + ecol;
            const unsigned short* ep16 = reinterpret_cast<const unsigned short*>(p.s.enc16) + (long)b * d.Tp * d.E + ecol;
            // 16 frame groups x 16 float4 columns; each thread walks frames grp, grp+16, ... ten at a time in flight
            // (clamped addresses, weights of frames >= len are read as 0 from the padded attention row)
            for (int tau = grp; tau < len; tau += 160) {
                float4 v[10];
#pragma unroll
                for (int u = 0; u < 10; ++u) {
                    const long off = (long)min(tau + 16 * u, len - 1) * d.E;
                    v[u] = H16 ? ld4_bf16(ep16 + off) : *reinterpret_cast<const float4*>(ep + off);
                }
#pragma unroll
                for (int u = 0; u < 10; ++u) {
                    const float a = (tau + 16 * u < len) ? s_att[tau + 16 * u] : 0.f;
                    acc.x += a * v[u].x; acc.y += a * v[u].y; acc.z += a * v[u].z; acc.w += a * v[u].w;
                }
            }
        }
        __shared__ float4 red4[16][16];
        red4[grp][c4] = acc;
        __syncthreads();
        if (threadIdx.x < 16 && e0 + 4 * threadIdx.x < d.E) {
            float4 r = red4[0][threadIdx.x];
#pragma unroll
            for (int g = 1; g < 16; ++g) { const float4 v = red4[g][threadIdx.x]; r.x += v.x; r.y += v.y; r.z += v.z; r.w += v.w; }
            float* o = xrow + e0 + 4 * threadIdx.x;
            o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
        }
    } else {
        const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
        const int ecol = e0 + col;
        float acc = 0.f;
        if (ecol < d.E) {
            const float* ep = p.enc + (long)b * d.Tp * d.E + ecol;
            for (int tau = grp; tau < len; tau += 4) acc += s_att[tau] * ep[(long)tau * d.E];
        }
        red[grp][col] = acc;
        __syncthreads();
        if (grp == 0 && ecol < d.E) xrow[ecol] = red[0][col] + red[1][col] + red[2][col] + red[3][col];
    }
}

// ------------------------------------------------------------------------------------------------
// K4: one decoder LSTM layer, one step.  Same wave layout as the encoder step: column n of the tile is
// gate n>>2 of hidden unit 4*blockIdx.x + (n&3).
// ------------------------------------------------------------------------------------------------
template <bool BF16>
__global__ __launch_bounds__(256) void dec_cell_fwd_kernel(DecP p, int t, int l) {
    // block = 4 hidden units x 4 gates (16 columns); the K = Kx + Dd reduction is split over the 4 waves
    // (interleaved k-steps) and summed through LDS, so one memory round trip per wave covers ~K/4.
    __shared__ float red[4][256];
    const asr_dec_dims_t& d = p.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, q = lane >> 4;
    const int g = n >> 2;
    const int j = blockIdx.x * 4 + (n & 3);
    const bool jok = j < d.Dd;
    const int XW = d.Dd + d.E;
    const int Kx = (l == 0) ? XW : d.Dd;
    const float* wih = p.w.Wih[l] + ((long)g * d.Dd + (jok ? j : 0)) * Kx;
    const float* whh = p.w.Whh[l] + ((long)g * d.Dd + (jok ? j : 0)) * d.Dd;
    const long SW = (long)d.NL * d.Dd;  // row width of hs/cs
    for (int m0 = 0; m0 < d.B; m0 += 16) {
        const int ab = m0 + n;
        const bool rok = ab < d.B;
        const long rowi = (long)(rok ? ab : 0) * d.L + t;
        const float* xrow = (l == 0) ? p.s.xin + rowi * XW : p.s.hs + rowi * SW + (long)(l - 1) * d.Dd;
        const float* hrow = p.s.hs + (rowi - (t > 0 ? 1 : 0)) * SW + (long)l * d.Dd;
        // the epilogue's operands (biases, previous cell state) are requested together with the contraction's
        const int erow = tid >> 2, ejj = tid & 3;
        const int eb = m0 + erow, eju = blockIdx.x * 4 + ejj;
        const bool eok = tid < 64 && eb < d.B && eju < d.Dd;
        const long eri = (long)(eok ? eb : 0) * d.L + t;
        float bsum[4] = {0.f, 0.f, 0.f, 0.f}, cp = 0.f;
        if (eok) {
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) bsum[gg] = p.w.bih[l][gg * d.Dd + eju] + p.w.bhh[l][gg * d.Dd + eju];
            if (t > 0) cp = p.s.cs[(eri - 1) * SW + (long)l * d.Dd + eju];
        }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = dot_rows_cat<BF16, 10>(xrow, wih, Kx, (Kx % 4) == 0 && (d.Dd % 4) == 0, hrow, whh, (t > 0) ? d.Dd : 0, (d.Dd % 4) == 0,
                                     rok, jok, wave, 4, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][(4 * q + r) * 16 + n] = acc[r];
        __syncthreads();
        if (eok) {
            // thread (row, unit): gathers its four gate columns
            float pre[4];
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                const int c = erow * 16 + gg * 4 + ejj;
                pre[gg] = red[0][c] + red[1][c] + red[2][c] + red[3][c] + bsum[gg];
            }
            const float ai = sigmoidf_(pre[0]), af = sigmoidf_(pre[1]), ag = tanhf(pre[2]), ao = sigmoidf_(pre[3]);
            float* go = p.s.gates + (eri * d.NL + l) * 4 * d.Dd;
            go[eju] = ai; go[d.Dd + eju] = af; go[2 * d.Dd + eju] = ag; go[3 * d.Dd + eju] = ao;
            const float cn = af * cp + ai * ag;
            p.s.cs[eri * SW + (long)l * d.Dd + eju] = cn;
            p.s.hs[eri * SW + (long)l * d.Dd + eju] = ao * tanhf(cn);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// K5 (greedy decoding only): logits of step t, argmax, next input token.  One block per utterance.
// ------------------------------------------------------------------------------------------------
// The arg-max is the LOWEST index among equal logits (torch.argmax on the reference's side): every wave keeps a running
// (value, index) over the entries it computes - ascending v, strict `>` - and the four waves meet in eight LDS words, so the
// kernel's LDS does not grow with V.
__global__ __launch_bounds__(256) void dec_greedy_kernel(DecP p, int t) {
    __shared__ float s_val[4];
    __shared__ int s_idx[4];
    const asr_dec_dims_t& d = p.d;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* h = p.s.hs + (((long)b * d.L + t) * d.NL + (d.NL - 1)) * d.Dd;
    float bv = -INFINITY;
    int bi = -1;                         // -1: the wave owns no entry (V < 4)
    for (int v = wave; v < d.V; v += 4) {
        float acc = 0.f;
        for (int k = lane; k < d.Dd; k += 64) acc += h[k] * p.w.Wc[(long)v * d.Dd + k];
        acc = wave_sum(acc);             // every lane holds the sum
        acc += p.w.bc[v];
        if (lane == 0) p.s.logits[((long)b * d.L + t) * d.V + v] = acc;
        if (bi < 0 || acc > bv) { bv = acc; bi = v; }
    }
    if (lane == 0) { s_val[wave] = bv; s_idx[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0 && t + 1 < d.L) {
        float best_v = s_val[0];         // wave 0 owns entry 0
        int best = s_idx[0];
        for (int w = 1; w < 4; ++w) {
            const float v = s_val[w];
            const int i = s_idx[w];
            if (i >= 0 && (v > best_v || (v == best_v && i < best))) { best_v = v; best = i; }
        }
        p.s.tokens[(long)b * d.L + t + 1] = best;
    }
}

// The decode step's vocabulary projection, one workgroup per hypothesis row: every row walks all of Wc, which is the cheaper
// way only while Wc is small.  Above this V asr_att_decoder_step computes the projection as one contraction over all rows.
constexpr int DEC_LOGITS_ROW_MAX_V = 2048;
__global__ __launch_bounds__(256) void dec_logits_kernel(DecP p, int t) {
    const asr_dec_dims_t& d = p.d;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* h = p.s.hs + (((long)b * d.L + t) * d.NL + (d.NL - 1)) * d.Dd;
    for (int v = wave; v < d.V; v += 4) {
        float acc = 0.f;
        for (int k = lane; k < d.Dd; k += 64) acc += h[k] * p.w.Wc[(long)v * d.Dd + k];
        acc = wave_sum(acc);
        if (lane == 0) p.s.logits[((long)b * d.L + t) * d.V + v] = acc + p.w.bc[v];
    }
}

// =================================================================================================
// backward
// =================================================================================================
struct DecB {
    DecP f;
    asr_dec_grads_t g;
    float* dhs;        // (B,L,NL,Dd)   gradient wrt every h (accumulated in place)
    float* dxin;       // (B,L,Dd+E)
    float* dq;         // (B,L,A)       gradient wrt the query pre-activation (per-tile partials added atomically)
    float* dkey;       // (B,T',A)
    float* datt_next;  // (B,T')        gradient flowing into attn_t from step t+1's location conv
    float* dcf;        // (NL,B,Dd)
    float* wcatT[ASR_MAX_DEC_LAYERS];  // ((Kx+Dd) x 4Dd) transposed [W_ih ; W_hh]
    float* wqT;        // (Q x A)
    float* slots;      // (B*nte, slot) per-workgroup partial sums of d w_g, d W_proj ([k][a]), d b_g
    int nte, slot;     // energy-backward tiles per utterance, floats per slot
};

// cell backward, elementwise part: dgates (in place over the activated gates) and the dc*f carry
__global__ void dec_cell_bwd_elem_kernel(DecB p, int t, int l, int last) {
    const asr_dec_dims_t& d = p.f.d;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.B * d.Dd) return;
    const int b = i / d.Dd, j = i % d.Dd;
    const long ri = (long)b * d.L + t;
    const long SW = (long)d.NL * d.Dd;
    float* g = p.f.s.gates + (ri * d.NL + l) * 4 * d.Dd;
    const float gi = g[j], gf = g[d.Dd + j], gg = g[2 * d.Dd + j], go = g[3 * d.Dd + j];
    const float ct = p.f.s.cs[ri * SW + (long)l * d.Dd + j];
    const float cp = (t > 0) ? p.f.s.cs[(ri - 1) * SW + (long)l * d.Dd + j] : 0.f;
    const float dh = p.dhs[ri * SW + (long)l * d.Dd + j];
    const long ci = ((long)l * d.B + b) * d.Dd + j;
    const float carry = last ? 0.f : p.dcf[ci];
    const float tc = tanhf(ct);
    const float dc = dh * go * (1.f - tc * tc) + carry;
    g[j] = dc * gg * gi * (1.f - gi);
    g[d.Dd + j] = dc * cp * gf * (1.f - gf);
    g[2 * d.Dd + j] = dc * gi * (1.f - gg * gg);
    g[3 * d.Dd + j] = dh * tc * go * (1.f - go);
    p.dcf[ci] = dc * gf;
}

// cell backward, contraction part: [d_input | d_h_prev] = dgates (B x 4Dd) * [W_ih | W_hh]
// block = 4 waves (split over the 4Dd reduction) x 16 output columns of the concatenated width Kx+Dd.
template <bool BF16>
__global__ __launch_bounds__(256) void dec_cell_bwd_mm_kernel(DecB p, int t, int l) {
    __shared__ float red[4][256];
    const asr_dec_dims_t& d = p.f.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, q = lane >> 4;
    const int XW = d.Dd + d.E;
    const int Kx = (l == 0) ? XW : d.Dd;
    const int K = 4 * d.Dd;
    const int c0 = blockIdx.x * 16;
    const bool cok = (c0 + n) < Kx + d.Dd;
    const float* wrow = p.wcatT[l] + (long)(cok ? c0 + n : 0) * K;
    const long SW = (long)d.NL * d.Dd;
    for (int m0 = 0; m0 < d.B; m0 += 16) {
        const int ab = m0 + n;
        const bool rok = ab < d.B;
        const float* grow = p.f.s.gates + ((((long)(rok ? ab : 0) * d.L + t) * d.NL) + l) * K;
        // accumulate targets are read before the contraction (one round trip for everything)
        const int row = tid >> 4, col = tid & 15;
        const int b = m0 + row, c = c0 + col;
        const bool ook = b < d.B && c < Kx + d.Dd;
        const long ri = (long)(ook ? b : 0) * d.L + t;
        float* dst = nullptr;
        bool add = false;
        if (ook) {
            if (c < Kx) {
                if (l == 0) dst = p.dxin + ri * XW + c;
                else { dst = p.dhs + ri * SW + (long)(l - 1) * d.Dd + c; add = true; }
            } else if (t > 0) {
                dst = p.dhs + (ri - 1) * SW + (long)l * d.Dd + (c - Kx); add = true;
            }
        }
        const float oldv = (dst && add) ? *dst : 0.f;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = dot_rows<BF16, 10>(grow, rok, wrow, cok, K, wave, 4, true, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][(4 * q + r) * 16 + n] = acc[r];
        __syncthreads();
        if (dst) *dst = oldv + red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
        __syncthreads();
    }
}

// B2: attention backward of one (utterance, TE-frame tile) in ONE kernel:
//   dattn[tau] = dctx . enc[tau] + datt_next[tau]                      (context + next step's location path)
//   softmax backward: de = attn * (dattn - dot) / temperature, with dot = sum_tau attn*dattn over the WHOLE utterance
//     = dctx . ctx + sum_tau attn*datt_next   (ctx = sum attn*enc is the saved context), so no workgroup needs another
//     tile's dattn and the former separate dattn kernel + buffer are gone;
//   energy backward: recompute loc/u from the saved conv, accumulate dkey (RMW), per-workgroup partial sums of
//     d w_g / d W_proj / d b_g in private slots, d query (x (1-q^2), atomically into dq[b,t,:]) and
//     dconv[tau,k] = sum_a dl[tau,a] W_proj[a,k], written over the saved conv of this step.
// Threads: NG frame groups x ceil(A/64) waves; wave (g, wa) owns attention dims a = 64*wa + lane for the frames of
// group g, so the per-a sums have one writer per group and meet in LDS.  TE is chosen by the host so that the batch is
// one round of workgroups; all global operands are requested before the first barrier.
// LDS regions: conv of the tile [TE][KP] (KP: the kernel's KNMAX rounded up to 4), de [TE], dattn [TE], dctx [E], W_proj transposed
// [Kn][AP], dl [TE][AP], the groups' sums [NG][Kn+2][A].  Returns AP / 4.
__host__ __device__ inline int bwd_energy_regions(int TE, int KP, int NG, int A, int E, int Kn, int n[7]) {
    int ap4 = (A + 3) >> 2; if ((ap4 & 1) == 0) ++ap4;
    const int AP = 4 * ap4;                             // row stride of the [frame][a] / [k][a] tiles: 16B rows, odd in float4 units
    n[0] = TE * KP; n[1] = n[2] = TE; n[3] = (E + 3) & ~3; n[4] = Kn * AP; n[5] = TE * AP; n[6] = NG * (Kn + 2) * A;
    return ap4;
}
constexpr int BWD_ENERGY_KP_HOST = 16;      // bwd_layout's KP, the widest instantiation's: TE and the bytes do not depend on the dispatch

template <int KNMAX, bool H16>
__global__ __launch_bounds__(640) void att_bwd_energy_kernel(DecB p, int t, int TE, int NG, int last) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    __shared__ float s_red[16];
    constexpr int KP = (KNMAX + 3) & ~3, CHK = 10;
    const asr_dec_dims_t& d = p.f.d;
    const int b = blockIdx.y, tau0 = blockIdx.x * TE;
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int nwa = (d.A + 63) >> 6, g = wave / nwa, wa = wave - g * nwa;
    const int FG = TE / NG;                              // frames per group
    int n[7];
    const int ap4 = bwd_energy_regions(TE, KP, NG, d.A, d.E, d.Kn, n), AP = 4 * ap4;
    const int XW = d.Dd + d.E;
    float *s_cv = smem_f, *s_de = s_cv + n[0], *s_dat = s_de + n[1], *s_dctx = s_dat + n[2], *s_wpT = s_dctx + n[3];
    float *s_dl = s_wpT + n[4], *s_acc = s_dl + n[5];
    const int len = min((int)p.f.enc_len[b], d.Tp);
    const int tmax = max(len - 1, 0);
    const long row = (long)b * d.L + t;
    float* convrow = p.f.s.conv + row * d.Kn * d.Tp;     // conv in, dconv out
    const float* att = p.f.s.att + row * d.Tp;
    const float* dnext = p.datt_next + (long)b * d.Tp;

    // ---- stage 0: all global reads, in flight together (consumed after the key/dkey chunk has been requested too)
    auto ld_dc = [&](int e) { return p.dxin[row * XW + d.Dd + e]; };
    auto ld_cx = [&](int e) { return p.f.s.xin[row * XW + d.Dd + e]; };
    auto ld_at = [&](int i) { return att[i]; };
    auto ld_dn = [&](int i) { return dnext[i]; };
    const float inv_te = 1.f / (float)TE, inv_kn = 1.f / (float)d.Kn;
    auto ld_cv = [&](int i) { const int k = fdiv(i, TE, inv_te), ti = i - k * TE; return convrow[(long)k * d.Tp + min(tau0 + ti, d.Tp - 1)]; };
    auto st_cv = [&](int i, float v) { const int k = fdiv(i, TE, inv_te), ti = i - k * TE; s_cv[ti * KP + k] = (tau0 + ti < d.Tp) ? v : 0.f; };
    auto ld_wp = [&](int i) { return p.f.w.Wproj[i]; };
    auto st_wp = [&](int i, float v) { const int a_ = fdiv(i, d.Kn, inv_kn), k = i - a_ * d.Kn; s_wpT[k * AP + a_] = v; };
    Stage<2> g_dc, g_cx, g_at, g_dn, g_cv; Stage<6> g_wp;
    g_dc.load(d.E, tid, nthr, ld_dc);
    g_cx.load(d.E, tid, nthr, ld_cx);
    g_at.load(max(len, 1), tid, nthr, ld_at);
    g_dn.load(max(len, 1), tid, nthr, ld_dn);
    g_cv.load(d.Kn * TE, tid, nthr, ld_cv);
    g_wp.load(d.Kn * d.A, tid, nthr, ld_wp);
    const int a = 64 * wa + lane;
    const bool aok = a < d.A;
    const int ac = aok ? a : d.A - 1;
    const float qa = p.f.s.q[row * d.A + ac], wga = p.f.w.wg[ac];
    float* slot = p.slots + ((long)b * p.nte + blockIdx.x) * p.slot;
    float old[KNMAX + 1];
    if (g == 0) {
        old[KNMAX] = slot[ac];
#pragma unroll
        for (int k = 0; k < KNMAX; ++k) old[k] = (k < d.Kn) ? slot[d.A + k * d.A + ac] : 0.f;
    }
    float kv[CHK], dk[CHK];
    const int f_beg = g * FG, f_end = f_beg + FG;
    auto load_chunk = [&](int f0) {
#pragma unroll
        for (int i = 0; i < CHK; ++i) {
            const long ki = ((long)b * d.Tp + min(tau0 + f0 + i, tmax)) * d.A + ac;
            kv[i] = H16 ? bf2f(reinterpret_cast<const unsigned short*>(p.f.s.key16)[ki]) : p.f.s.key[ki];
            dk[i] = p.dkey[ki];
        }
    };
    load_chunk(f_beg);
    float dot = 0.f;
    {
        g_dc.store(d.E, tid, nthr, [&](int e, float v) { s_dctx[e] = v; });
#pragma unroll
        for (int u = 0; u < 2; ++u) if (tid + u * nthr < d.E) dot += g_dc.v[u] * g_cx.v[u];
        for (int e = tid + 2 * nthr; e < d.E; e += nthr) { const float dc = ld_dc(e); s_dctx[e] = dc; dot += dc * ld_cx(e); }
        if (!last) {
#pragma unroll
            for (int u = 0; u < 2; ++u) if (tid + u * nthr < len) dot += g_at.v[u] * g_dn.v[u];
            for (int i = tid + 2 * nthr; i < len; i += nthr) dot += att[i] * dnext[i];
        }
        g_cv.store(d.Kn * TE, tid, nthr, st_cv);
        g_cv.rest(d.Kn * TE, tid, nthr, ld_cv, st_cv);
        g_wp.store(d.Kn * d.A, tid, nthr, st_wp);
        g_wp.rest(d.Kn * d.A, tid, nthr, ld_wp, st_wp);
        for (int i = tid; i < d.Kn * (AP - d.A); i += nthr) { const int k = i / (AP - d.A); s_wpT[k * AP + d.A + (i - k * (AP - d.A))] = 0.f; }
        // pad columns Kn..KP-1 of the conv tile: the KNMAX-wide sweep multiplies them by zero weights, and 0 * (stale LDS) can be NaN
        for (int i = tid; i < TE * (KP - d.Kn); i += nthr) { const int ti = i / (KP - d.Kn); s_cv[ti * KP + d.Kn + (i - ti * (KP - d.Kn))] = 0.f; }
    }
    __syncthreads();
    // ---- stage 1: dattn of the tile (16 lanes per frame, float4 over E), block-wide dot, de
    {
        const int part = tid & 15;
        const bool vec = (d.E & 3) == 0;
        for (int f = tid >> 4; f < TE; f += nthr >> 4) {
            const int tau = tau0 + f;
            const float* er = p.f.enc + ((long)b * d.Tp + min(tau, tmax)) * d.E;
            const unsigned short* er16 = reinterpret_cast<const unsigned short*>(p.f.s.enc16) + ((long)b * d.Tp + min(tau, tmax)) * d.E;
            float v = 0.f;
            if (vec) {
                // E/64 float4 per lane, ten at a time in flight (clamped address, contribution zeroed by the LDS operand)
                for (int e0 = 4 * part; e0 < d.E; e0 += 640) {
                    float4 x[10];
#pragma unroll
                    for (int u = 0; u < 10; ++u) x[u] = H16 ? ld4_bf16(er16 + min(e0 + 64 * u, d.E - 4)) : *reinterpret_cast<const float4*>(er + min(e0 + 64 * u, d.E - 4));
#pragma unroll
                    for (int u = 0; u < 10; ++u) {
                        if (e0 + 64 * u < d.E) {
                            const float4 c = *reinterpret_cast<const float4*>(s_dctx + e0 + 64 * u);
                            v += x[u].x * c.x + x[u].y * c.y + x[u].z * c.z + x[u].w * c.w;
                        }
                    }
                }
            } else {
                for (int e = part; e < d.E; e += 16) v += er[e] * s_dctx[e];
            }
            v += __shfl_xor(v, 8); v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
            if (part == 0) s_dat[f] = (tau < len) ? v + (last ? 0.f : dnext[tau]) : 0.f;
        }
        dot = wave_sum(dot);
        if (lane == 0) s_red[wave] = dot;
    }
    __syncthreads();
    dot = 0.f;
    for (int w = 0; w < (nthr >> 6); ++w) dot += s_red[w];
    for (int f = tid; f < TE; f += nthr) {
        const int tau = tau0 + f;
        s_de[f] = (tau < len) ? att[tau] * (s_dat[f] - dot) / d.temperature : 0.f;
    }
    __syncthreads();
    // ---- stage 2: sweep over the group's frames
    float wp[KNMAX], dwp[KNMAX];
#pragma unroll
    for (int k = 0; k < KNMAX; ++k) { wp[k] = (k < d.Kn) ? s_wpT[k * AP + ac] : 0.f; dwp[k] = 0.f; }
    float dwg = 0.f, dqa = 0.f;
    for (int f0 = f_beg; f0 < f_end; f0 += CHK) {
        float kc[CHK], dc_[CHK];
#pragma unroll
        for (int i = 0; i < CHK; ++i) { kc[i] = kv[i]; dc_[i] = dk[i]; }
        if (f0 + CHK < f_end) load_chunk(f0 + CHK);          // next chunk in flight during this one
#pragma unroll
        for (int i = 0; i < CHK; ++i) {
            const int f = f0 + i, tau = tau0 + f;
            if (f < f_end) {
                float cvv[KP];
#pragma unroll
                for (int k4 = 0; k4 < KP; k4 += 4) {
                    const float4 c4 = *reinterpret_cast<const float4*>(s_cv + f * KP + k4);
                    cvv[k4] = c4.x; cvv[k4 + 1] = c4.y; cvv[k4 + 2] = c4.z; cvv[k4 + 3] = c4.w;
                }
                float lp = 0.f;
#pragma unroll
                for (int k = 0; k < KNMAX; ++k) lp += wp[k] * cvv[k];
                const float loc = tanh_fast(lp);
                const float u = tanh_fast(kc[i] + qa + loc);
                const float de = s_de[f];                        // 0 for tau >= len
                const float du = de * wga * (1.f - u * u);
                const float dl = du * (1.f - loc * loc);
                dwg += de * u;
                dqa += du;
#pragma unroll
                for (int k = 0; k < KNMAX; ++k) dwp[k] += dl * cvv[k];
                if (aok && tau < len) p.dkey[((long)b * d.Tp + tau) * d.A + a] = dc_[i] + du;
                if (aok) s_dl[f * AP + a] = dl;
            }
        }
    }
    if (wa == nwa - 1) {                                     // zero the pad columns of the dl tile (read as float4 below)
        for (int f = f_beg; f < f_end; ++f)
            for (int x = d.A + lane; x < AP; x += 64) s_dl[f * AP + x] = 0.f;
    }
    if (NG > 1 && aok) {
        float* acc = s_acc + (long)g * (d.Kn + 2) * d.A;
        acc[a] = dwg; acc[d.A + a] = dqa;
#pragma unroll
        for (int k = 0; k < KNMAX; ++k) if (k < d.Kn) acc[(2 + k) * d.A + a] = dwp[k];
    }
    __syncthreads();
    if (g == 0 && aok) {
        for (int gg = 1; gg < NG; ++gg) {
            const float* acc = s_acc + (long)gg * (d.Kn + 2) * d.A;
            dwg += acc[a]; dqa += acc[d.A + a];
#pragma unroll
            for (int k = 0; k < KNMAX; ++k) if (k < d.Kn) dwp[k] += acc[(2 + k) * d.A + a];
        }
        slot[a] = old[KNMAX] + dwg;
#pragma unroll
        for (int k = 0; k < KNMAX; ++k) if (k < d.Kn) slot[d.A + k * d.A + a] = old[k] + dwp[k];
        atomicAdd(&p.dq[row * d.A + a], dqa * (1.f - qa * qa));
    }
    if (tid == 0) {
        float sde = 0.f;
        for (int f = 0; f < TE; ++f) sde += s_de[f];
        slot[d.A * (1 + d.Kn)] += sde;
    }
    // ---- stage 3: dconv[tau,k] = sum_a dl[tau,a] * W_proj[a,k]  (thread per (frame, k), float4 over a)
    for (int o = tid; o < TE * d.Kn; o += nthr) {
        const int k = fdiv(o, TE, inv_te), f = o - k * TE;
        const float4* dl4 = reinterpret_cast<const float4*>(s_dl + f * AP);
        const float4* w4 = reinterpret_cast<const float4*>(s_wpT + k * AP);
        float v0 = 0.f, v1 = 0.f;
        int x = 0;
        for (; x + 1 < ap4; x += 2) {
            const float4 d0 = dl4[x], w0 = w4[x], d1 = dl4[x + 1], w1 = w4[x + 1];
            v0 += d0.x * w0.x + d0.y * w0.y + d0.z * w0.z + d0.w * w0.w;
            v1 += d1.x * w1.x + d1.y * w1.y + d1.z * w1.z + d1.w * w1.w;
        }
        if (x < ap4) { const float4 d0 = dl4[x], w0 = w4[x]; v0 += d0.x * w0.x + d0.y * w0.y + d0.z * w0.z + d0.w * w0.w; }
        const int tau = tau0 + f;
        if (tau < d.Tp) convrow[(long)k * d.Tp + tau] = (tau < len) ? v0 + v1 : 0.f;
    }
}

// B3: gradient through the location convolution wrt attn_{t-1}:
//   datt_next[tau'] = sum_k sum_j W[k][j] * dconv[k][tau' - j + Ks]      (dconv = this step's rows of state.conv)
// grid (ceil(T'/TC), B), 512 threads; item = (tap range, k, group of 4 outputs) with a sliding register window.
// (d W_conv needs no place in the sequential chain: wconv_grad_kernel after the loop.)
// LDS regions: filters [Kn*taps], dconv window tau0-Ks .. tau0+TC+Ks [Kn][winp], partial sums [parts*Kn][TC].  Returns winp.
__host__ __device__ inline int bwd_conv_regions(int TC, int Kn, int Ks, int n[3]) {
    const int winp = TC + 2 * Ks + 4;
    n[0] = (Kn * (2 * Ks + 1) + 3) & ~3; n[1] = Kn * winp; n[2] = conv_parts(Kn * (TC / 4)) * Kn * TC;
    return winp;
}

__device__ __forceinline__ void att_bwd_conv_body(const DecB& p, int t, int TC, int bx, int by) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const asr_dec_dims_t& d = p.f.d;
    const int b = by, tau0 = bx * TC, tid = threadIdx.x;
    const int taps = 2 * d.Ks + 1, win = TC + 2 * d.Ks;
    int n[3];
    const int winp = bwd_conv_regions(TC, d.Kn, d.Ks, n);
    float *s_wc = smem_f, *s_dc = s_wc + n[0], *s_part = s_dc + n[1];
    const float* dconv = p.f.s.conv + ((long)b * d.L + t) * d.Kn * d.Tp;
    for (int i = tid; i < d.Kn * taps; i += 512) s_wc[i] = p.f.w.Wconv[i];
    for (int i = tid; i < d.Kn * winp; i += 512) {
        const int k = i / winp, x = i - k * winp, tau = tau0 + x - d.Ks;
        s_dc[i] = (x < win && tau >= 0 && tau < d.Tp) ? dconv[(long)k * d.Tp + tau] : 0.f;
    }
    __syncthreads();
    const int ngrp = TC / 4, nout = d.Kn * ngrp;
    const int parts = conv_parts(nout);
    const int tp = (taps + parts - 1) / parts;
    for (int it = tid; it < parts * nout; it += 512) {
        const int pz = it / nout, o = it - pz * nout, k = o / ngrp, ig = o - k * ngrp;
        const int j0 = pz * tp, j1 = min(taps, j0 + tp);
        const float* wk = s_wc + k * taps;
        const float* dc = s_dc + k * winp + 4 * ig + 2 * d.Ks;      // dc[i - j] for output i of the group
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        float p1 = 0.f, p2 = 0.f, p3 = 0.f;
        if (j0 < j1) { p1 = dc[1 - j0]; p2 = dc[2 - j0]; p3 = dc[3 - j0]; }
        for (int j = j0; j < j1; ++j) {
            const float w = wk[j], p0 = dc[-j];
            a0 += w * p0; a1 += w * p1; a2 += w * p2; a3 += w * p3;
            p3 = p2; p2 = p1; p1 = p0;
        }
        float* o4 = s_part + (long)(pz * d.Kn + k) * TC + 4 * ig;
        o4[0] = a0; o4[1] = a1; o4[2] = a2; o4[3] = a3;
    }
    __syncthreads();
    for (int i = tid; i < TC; i += 512) {
        float v = 0.f;
        for (int r = 0; r < parts * d.Kn; ++r) v += s_part[(long)r * TC + i];
        if (tau0 + i < d.Tp) p.datt_next[(long)b * d.Tp + tau0 + i] = v;
    }
}

// d W_conv[k][j] += sum_{l,b} sum_tau dconv_l[b,k,tau] * prev_att_l[b, tau + j - Ks]   after the loop, all steps at once.
// grid (NCH, B): workgroup (c, b) walks the steps l = c, c+NCH, ...; thread (k, group of 4 taps) slides over tau.
// Partial sums per workgroup land in `out` (gridDim.x*gridDim.y, Kn*taps) and are reduced by slot_reduce_kernel.
// LDS regions: zero-padded previous attention [wpa = Tp + 2Ks + 8], dconv [Kn][Tp].  Returns wpa.
__host__ __device__ inline int wconv_regions(int Tp, int Kn, int Ks, int n[2]) {
    const int wpa = Tp + 2 * Ks + 8;
    n[0] = (wpa + 3) & ~3; n[1] = Kn * Tp;
    return wpa;
}

__global__ __launch_bounds__(512) void wconv_grad_kernel(DecP p, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const asr_dec_dims_t& d = p.d;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int taps = 2 * d.Ks + 1;
    const int tg = (taps + 3) / 4, nitem = d.Kn * tg;
    const int len = min((int)p.enc_len[b], d.Tp);
    int n[2];
    const int wpa = wconv_regions(d.Tp, d.Kn, d.Ks, n);
    float *s_pa = smem_f, *s_dc = s_pa + n[0];
    float acc[4][4];                                     // up to 4 items per thread
#pragma unroll
    for (int u = 0; u < 4; ++u) { acc[u][0] = acc[u][1] = acc[u][2] = acc[u][3] = 0.f; }
    for (int l = blockIdx.x; l < d.L; l += gridDim.x) {
        __syncthreads();
        const float* prev = (l > 0) ? p.s.att + ((long)b * d.L + (l - 1)) * d.Tp : nullptr;
        const float uni = 1.f / (float)max(len, 1);
        for (int i = tid; i < wpa; i += 512) {
            const int tau = i - d.Ks;
            float v = 0.f;
            if (tau >= 0 && tau < d.Tp) v = prev ? prev[tau] : (tau < len ? uni : 0.f);
            s_pa[i] = v;
        }
        const float* dconv = p.s.conv + ((long)b * d.L + l) * d.Kn * d.Tp;
        for (int i = tid; i < d.Kn * d.Tp; i += 512) s_dc[i] = dconv[i];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int it = tid + 512 * u;
            if (it < nitem) {
                const int k = it / tg, j0 = 4 * (it - k * tg);
                const float* dc = s_dc + k * d.Tp;
                const float* pa = s_pa + j0;                 // pa[tau + jj] = prev_att[tau + j0 + jj - Ks]
                float q0 = pa[0], q1 = pa[1], q2 = pa[2];
                float a0 = acc[u][0], a1 = acc[u][1], a2 = acc[u][2], a3 = acc[u][3];
                for (int tau = 0; tau < len; ++tau) {
                    const float w = dc[tau], q3 = pa[tau + 3];
                    a0 += w * q0; a1 += w * q1; a2 += w * q2; a3 += w * q3;
                    q0 = q1; q1 = q2; q2 = q3;
                }
                acc[u][0] = a0; acc[u][1] = a1; acc[u][2] = a2; acc[u][3] = a3;
            }
        }
    }
    float* o = out + ((long)blockIdx.y * gridDim.x + blockIdx.x) * d.Kn * taps;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int it = tid + 512 * u;
        if (it < nitem) {
            const int k = it / tg, j0 = 4 * (it - k * tg);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) if (j0 + jj < taps) o[k * taps + j0 + jj] = acc[u][jj];
        }
    }
}

// The same gradient on the matrix cores (bf16 mode, Kn <= 16): per (b, l) the product  dconv (Kn x T')  x  Toeplitz(prev_att)
// (T' x taps),  D[k][j] += sum_tau dconv[k][tau] * pa[tau + j]  with pa the zero-padded previous attention.  A tile = the
// dconv rows of a 32-frame chunk (loaded once per chunk), B tile = 32 x 16 window of pa for taps j0..j0+15 (eight LDS words
// per lane); 16-tap tiles are dealt round-robin to the 4 waves, whose accumulators run over all frames and all steps of
// the workgroup.  Same grid, slots and reduction as wconv_grad_kernel.
// LDS regions: zero-padded previous attention s_pa[i] = att[seg + i - Ks] [wpa = SEG + 16*ntile + 16], dconv rows of the segment,
// zero beyond Kn / len [16][SEG].  Returns wpa.
__host__ __device__ inline int wconv_mfma_regions(int Tp, int Ks, int n[2], int* ntile, int* SEG) {
    *ntile = (2 * Ks + 1 + 15) >> 4;                     // 16-tap output tiles
    // frames are walked in segments of <= 768 (one LDS image of the dconv rows and of the attention window per segment), so any
    // T' is covered (round 2 took this kernel only up to T' = 768 and fell back to the VALU kernel beyond: 14 ms at config 5)
    const int TpP = 32 * ((Tp + 31) >> 5);
    *SEG = TpP < 768 ? TpP : 768;
    const int wpa = *SEG + 16 * *ntile + 16;
    n[0] = (wpa + 3) & ~3; n[1] = 16 * *SEG;
    return wpa;
}
// The shapes the kernel takes: bf16 mode, the Kn rows in one 16-row A tile, 16 tap tiles over its 4 waves x MAXT accumulators,
// and an attention window its four 256-thread staging batches cover.  Returns the launch's dynamic LDS bytes, 0 for any other shape.
inline size_t wconv_mfma_lds(const asr_dec_dims_t& d, bool bf) {
    int n[2], ntile, SEG;
    const int wpa = wconv_mfma_regions(d.Tp, d.Ks, n, &ntile, &SEG);
    return (bf && d.Kn <= 16 && ntile <= 16 && lds_bytes(n, 2) <= 150 * 1024 && wpa <= 1024) ? lds_bytes(n, 2) : 0;
}

__global__ __launch_bounds__(256) void wconv_grad_mfma_kernel(DecP p, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const asr_dec_dims_t& d = p.d;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int taps = 2 * d.Ks + 1;
    const int len = min((int)p.enc_len[b], d.Tp);
    int n[2], ntile, SEG;
    const int wpa = wconv_mfma_regions(d.Tp, d.Ks, n, &ntile, &SEG);
    float *s_pa = smem_f, *s_dc = s_pa + n[0];
    constexpr int MAXT = 4;                              // tiles per wave (taps <= 256)
    f32x4 acc[MAXT];
#pragma unroll
    for (int u = 0; u < MAXT; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int m = lane & 15, q = lane >> 4;
    for (int l = blockIdx.x; l < d.L; l += gridDim.x) {
        const float* prev = (l > 0) ? p.s.att + ((long)b * d.L + (l - 1)) * d.Tp : nullptr;
        const float uni = 1.f / (float)max(len, 1);
        const float* dconv = p.s.conv + ((long)b * d.L + l) * d.Kn * d.Tp;
        for (int seg = 0; seg < len; seg += SEG) {
            __syncthreads();
            // staging with all loads of a batch in flight (clamped addresses, zeroing by selects): SEG <= 768, wpa <= 1024
            {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int tau = seg + tid + 256 * j - d.Ks;
                    v[j] = prev ? prev[min(max(tau, 0), d.Tp - 1)] : uni;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = tid + 256 * j, tau = seg + i - d.Ks;
                    if (i < wpa) s_pa[i] = (tau >= 0 && tau < (prev ? d.Tp : len)) ? v[j] : 0.f;
                }
            }
#pragma unroll 1
            for (int k0 = 0; k0 < 16; k0 += 4) {
                float v[4][3];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        v[kk][j] = dconv[(long)min(k0 + kk, d.Kn - 1) * d.Tp + min(seg + tid + 256 * j, d.Tp - 1)];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const int ti = tid + 256 * j;
                        if (ti < SEG) s_dc[(k0 + kk) * SEG + ti] = (k0 + kk < d.Kn && seg + ti < len) ? v[kk][j] : 0.f;
                    }
            }
            __syncthreads();
            const int nchunk = (min(len - seg, SEG) + 31) >> 5;
            for (int c = 0; c < nchunk; ++c) {
                const float* ar = s_dc + m * SEG + 32 * c + 8 * q;
                const float4 a0 = *reinterpret_cast<const float4*>(ar), a1 = *reinterpret_cast<const float4*>(ar + 4);
                bf16x8 av;
                av[0] = (__bf16)a0.x; av[1] = (__bf16)a0.y; av[2] = (__bf16)a0.z; av[3] = (__bf16)a0.w;
                av[4] = (__bf16)a1.x; av[5] = (__bf16)a1.y; av[6] = (__bf16)a1.z; av[7] = (__bf16)a1.w;
#pragma unroll
                for (int u = 0; u < MAXT; ++u) {
                    const int tile = wave + 4 * u;
                    if (tile < ntile) {
                        const float* br = s_pa + 32 * c + 8 * q + 16 * tile + m;      // pa[tau + j], tau = seg + 32c + 8q + e, j = 16*tile + m
                        bf16x8 bv;
#pragma unroll
                        for (int e = 0; e < 8; ++e) bv[e] = (__bf16)br[e];
                        acc[u] = mma16(av, bv, acc[u]);
                    }
                }
            }
        }
    }
    // D[row = 4q + r = k][col = m = tap within the tile]
    float* o = out + ((long)blockIdx.y * gridDim.x + blockIdx.x) * d.Kn * taps;
#pragma unroll
    for (int u = 0; u < MAXT; ++u) {
        const int tile = wave + 4 * u, j = 16 * tile + m;
        if (tile < ntile && j < taps) {
#pragma unroll
            for (int r = 0; r < 4; ++r) if (4 * q + r < d.Kn) o[(4 * q + r) * taps + j] = acc[u][r];
        }
    }
}

// B4: query backward.  dq[b,t,:] already holds the gradient wrt the query pre-activation;  dhs[b,t-1,:] += dq * W_q.
template <bool BF16>
__device__ __forceinline__ void dec_query_bwd_body(const DecB& p, int t, int fuse_elem, int qblock) {
    // fuse_elem (single-layer decoders): dhs[b,t-1,:] is complete once this kernel has added its part, so the same
    // thread goes on with the cell backward of step t-1 for its (row, unit) - the elementwise kernel of that step and
    // its launch boundary are saved.  Operands of that epilogue are requested before the contraction.
    __shared__ float red[4][256];
    const asr_dec_dims_t& d = p.f.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, q = lane >> 4;
    const int c = qblock * 16 + n;
    const bool cok = c < d.Q;
    const float* wrow = p.wqT + (long)(cok ? c : 0) * d.A;
    for (int m0 = 0; m0 < d.B; m0 += 16) {
        const int ab = m0 + n;
        const bool rok = ab < d.B;
        const float* drow = p.dq + ((long)(rok ? ab : 0) * d.L + t) * d.A;
        const int row = tid >> 4, col = tid & 15;
        const int b = m0 + row, cc = qblock * 16 + col;
        const bool ook = b < d.B && cc < d.Q;
        const long ri = (long)(ook ? b : 0) * d.L + (t - 1);
        float* dh = p.dhs + ri * d.Q + (ook ? cc : 0);
        const float dh_old = *dh;
        float gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f, ct = 0.f, cp = 0.f, carry = 0.f;
        float* g = p.f.s.gates + ri * 4 * d.Dd + (ook ? cc : 0);          // NL == 1 when fuse_elem
        const long ci = (long)(ook ? b : 0) * d.Dd + (ook ? cc : 0);
        if (fuse_elem) {
            gi = g[0]; gf = g[d.Dd]; gg = g[2 * d.Dd]; go = g[3 * d.Dd];
            ct = p.f.s.cs[ri * d.Dd + (ook ? cc : 0)];
            cp = p.f.s.cs[(ri - (t > 1 ? 1 : 0)) * d.Dd + (ook ? cc : 0)];
            if (t <= 1) cp = 0.f;
            carry = p.dcf[ci];
        }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = dot_rows<BF16>(drow, rok, wrow, cok, d.A, wave, 4, (d.A % 4) == 0, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][(4 * q + r) * 16 + n] = acc[r];
        __syncthreads();
        if (ook) {
            const float dhv = dh_old + red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
            *dh = dhv;
            if (fuse_elem) {
                const float tc = tanhf(ct);
                const float dc = dhv * go * (1.f - tc * tc) + carry;
                g[0] = dc * gg * gi * (1.f - gi);
                g[d.Dd] = dc * cp * gf * (1.f - gf);
                g[2 * d.Dd] = dc * gi * (1.f - gg * gg);
                g[3 * d.Dd] = dhv * tc * go * (1.f - go);
                p.dcf[ci] = dc * gf;
            }
        }
        __syncthreads();
    }
}

// B3 + B4 in one launch: the location-conv gradient and the query backward both consume the attention backward's outputs
// and do not depend on each other, so their workgroups share a launch (one dependent kernel boundary per step less; the
// launch lasts as long as the longer of the two).  blockIdx.x < nconv: conv tile (bx, by); else query block.
template <bool BF16>
__global__ __launch_bounds__(512) void att_bwd_tail_kernel(DecB p, int t, int TC, int gx, int nconv, int fuse_elem) {
    if ((int)blockIdx.x < nconv) {
        att_bwd_conv_body(p, t, TC, blockIdx.x % gx, blockIdx.x / gx);
    } else {
        if (threadIdx.x >= 256) return;                 // the matvec body is written for 4 waves
        dec_query_bwd_body<BF16>(p, t, fuse_elem, blockIdx.x - nconv);
    }
}

__global__ void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int R, int C, long ld_dst, long col0) {
    // src (R x C) -> dst[(c + 0) * ld_dst + col0 + r]
    const long total = (long)R * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int r = (int)(i / C), c = (int)(i % C);
        dst[(long)c * ld_dst + col0 + r] = src[i];
    }
}

// reduce the per-workgroup slots into the parameter gradients: one wave per output element
__global__ __launch_bounds__(256) void slot_reduce_kernel(const float* __restrict__ slots, int nslots, int slot, float* __restrict__ out,
                                                          int off, int n, int tr_rows, int tr_cols) {
    // tr_rows > 0: the slot holds this block transposed ([col][row]) and `out` is [row][col]
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const int src = tr_rows > 0 ? (i % tr_cols) * tr_rows + (i / tr_cols) : i;
    float acc = 0.f;
    for (int s = lane; s < nslots; s += 64) acc += slots[(long)s * slot + off + src];
    acc = wave_sum(acc);
    if (lane == 0) out[i] += acc;
}

// embedding gradient: dE[v,:] += sum over (b,t) with tokens[b,t] == v of dxin[b,t,0:Dd]   (deterministic)
// grid (V, ceil(Dd/64)); wave g owns the positions i = g (mod 4): it first compacts the matching ones, in order, into an LDS
// list (coalesced token scan, ballot + prefix count), then sums those rows with independent loads; lanes over 64 columns
constexpr int EMB_LIST_MAX = 3584;          // positions per wave list and chunk (4 lists of 14 KB in LDS)
__global__ __launch_bounds__(256) void embed_bwd_kernel(const float* __restrict__ dxin, const int64_t* __restrict__ tokens,
                                                        float* __restrict__ demb, int B, int L, int Dd, int XW, int V) {
    extern __shared__ int s_rows[];                       // 4 lists of `cper` positions, rebuilt per chunk of 4*cper positions
    __shared__ float red[4][64];
    const int v = blockIdx.x, lane = threadIdx.x & 63, k = blockIdx.y * 64 + lane, grp = threadIdx.x >> 6;
    const int BL = B * L, per = (BL + 3) / 4;
    const int cper = min(per, EMB_LIST_MAX);
    int* list = s_rows + grp * cper;
    float acc = 0.f;
    const int kc = min(k, Dd - 1);
    for (int p0 = 0; p0 < per; p0 += cper) {             // positions 4*(p0 + j) + grp, j < cper: ascending per wave, so the sum order is fixed
        int n = 0;
        const int pend = min(per, p0 + cper);
        for (int base = p0; base < pend; base += 64) {
            const int i = 4 * (base + lane) + grp;
            const bool m = (base + lane < pend) && i < BL && tokens[min(i, BL - 1)] == v;
            const unsigned long long bal = __ballot(m);
            const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
            if (m) list[n + before] = i;
            n += __popcll(bal);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");     // the list is read by the wave that wrote it
        int q = 0;
        for (; q + 4 <= n; q += 4) {
            const float x0 = dxin[(long)list[q] * XW + kc], x1 = dxin[(long)list[q + 1] * XW + kc];
            const float x2 = dxin[(long)list[q + 2] * XW + kc], x3 = dxin[(long)list[q + 3] * XW + kc];
            acc += x0; acc += x1; acc += x2; acc += x3;
        }
        for (; q < n; ++q) acc += dxin[(long)list[q] * XW + kc];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");     // the list is rewritten by the next chunk
    }
    red[grp][lane] = acc;
    __syncthreads();
    if (grp == 0 && k < Dd) demb[(long)v * Dd + k] += red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
}

struct BwdLayout {
    size_t dhs, dxin, dq, dkey, datt_next, dcf, wq_t, slots, wslots, dkeypre, wcat[ASR_MAX_DEC_LAYERS], pwork, pwork_bytes, total;
    int ntp, ntp_max;       // tiles per utterance of the persistent backward under the current plan preference (0: no plan) / the larger of its two plans
    int nte, slot;          // energy-backward tiles per utterance, floats per slot
    int TE, NG;             // frames per energy-backward workgroup, frame groups
    int TC;                 // outputs per conv-backward workgroup
    int nch;                // step chunks of the W_conv gradient kernel
    size_t lds_e, lds_c, lds_w;
};
BwdLayout bwd_layout(const asr_dec_dims_t& d) {
    BwdLayout o;
    size_t off = 0;
    auto take = [&](size_t nfloat) { size_t r = off; off += align_up256(nfloat * sizeof(float)); return r; };
    const int XW = d.Dd + d.E;
    const int taps = 2 * d.Ks + 1;
    // energy backward: NG frame groups x ceil(A/64) waves (<= 640 threads); the smallest tile that keeps the batch in
    // one round of workgroups and fits the LDS budget
    const int nwa = cdiv(d.A, 64);
    o.NG = nwa <= 2 ? 4 : (nwa <= 5 ? 2 : 1);
    int n[7];
    auto lds_of = [&](int te) { bwd_energy_regions(te, BWD_ENERGY_KP_HOST, o.NG, d.A, d.E, d.Kn, n); return lds_bytes(n, 7); };
    const int te_cand[] = {8, 16, 24, 32, 40, 48, 64};
    o.TE = 8;
    for (int i = 0; i < 7; ++i) {
        const int te = te_cand[i];
        if (lds_of(te) > 150 * 1024) break;
        o.TE = te;
        if ((long)d.B * cdiv(d.Tp, te) <= 256) break;
    }
    o.lds_e = lds_of(o.TE);
    o.nte = cdiv(d.Tp, o.TE);
    o.slot = d.A * (1 + d.Kn) + 1;
    // conv backward
    const int tc_cand[] = {8, 16, 24, 32, 40, 48, 64};
    o.TC = 64;
    for (int i = 0; i < 7; ++i) if ((long)d.B * cdiv(d.Tp, tc_cand[i]) <= 256) { o.TC = tc_cand[i]; break; }
    bwd_conv_regions(o.TC, d.Kn, d.Ks, n);
    o.lds_c = lds_bytes(n, 3);
    // W_conv gradient
    o.nch = (int)(256 / d.B > 0 ? 256 / d.B : 1);
    if (o.nch > d.L) o.nch = d.L;
    wconv_regions(d.Tp, d.Kn, d.Ks, n);
    o.lds_w = lds_bytes(n, 2);
    // the zero-initialised accumulators first and back to back, the persistent launch's status block right behind them: ONE fill
    // from `dhs` to `pwork + 256` at the start of a call (five separate fills before)
    o.dhs = take((size_t)d.B * d.L * d.NL * d.Dd);
    o.dq = take((size_t)d.B * d.L * d.A);
    o.dkey = take((size_t)d.B * d.Tp * d.A);
    const DecPlanInfo pi = dec_bwd_plan_info(d);
    o.ntp = pi.tiles;
    o.ntp_max = pi.tiles_max;
    o.slots = take((size_t)d.B * (o.nte > o.ntp_max ? o.nte : o.ntp_max) * o.slot);
    o.pwork_bytes = pi.work_bytes;
    o.pwork = take(o.pwork_bytes / sizeof(float) + 64);
    o.dxin = take((size_t)d.B * d.L * XW);
    o.dkeypre = take((size_t)d.B * d.Tp * d.A);
    o.datt_next = take((size_t)d.B * d.Tp);
    o.dcf = take((size_t)d.NL * d.B * d.Dd);
    o.wq_t = take((size_t)d.Q * d.A);
    o.wslots = take((size_t)d.B * o.nch * d.Kn * taps);
    for (int l = 0; l < d.NL; ++l) o.wcat[l] = take((size_t)((l == 0 ? XW : d.Dd) + d.Dd) * 4 * d.Dd);
    o.total = off;
    return o;
}

int check_dims(const asr_dec_dims_t& d, const char* who) {
    ASR_REQUIRE(d.B > 0 && d.Tp > 0 && d.E > 0 && d.A > 0 && d.Dd > 0 && d.V > 1 && d.L > 0, ASR_E_ARG, "%s: bad dims", who);
    ASR_REQUIRE(d.NL >= 1 && d.NL <= ASR_MAX_DEC_LAYERS, ASR_E_UNSUPPORTED, "%s: %d decoder layers (max %d)", who, d.NL, ASR_MAX_DEC_LAYERS);
    ASR_REQUIRE(d.Q == d.Dd * d.NL, ASR_E_ARG, "%s: Q must equal Dd*NL", who);
    ASR_REQUIRE(d.Kn >= 1 && d.Kn <= 16, ASR_E_UNSUPPORTED, "%s: loc_kernel_num %d not in [1,16]", who, d.Kn);
    ASR_REQUIRE(d.Ks >= 0 && d.Ks <= 512, ASR_E_UNSUPPORTED, "%s: loc_kernel_size %d too large", who, d.Ks);
    ASR_REQUIRE(d.temperature > 0.f, ASR_E_ARG, "%s: temperature must be > 0", who);
    ASR_REQUIRE(d.Tp <= 12000, ASR_E_UNSUPPORTED, "%s: T'=%d exceeds the LDS row budget", who, d.Tp);
    return ASR_OK;
}

// Launch geometry of the forward energy kernel: the smallest frames-per-wave count that puts the whole batch in one
// round of workgroups (<= 256), within the register budget of the (KNMAX, TPW) instantiations.
struct EnergyPlan { int tpw; dim3 grid; size_t lds; };
EnergyPlan energy_plan(const asr_dec_dims_t& d) {
    const int cand_small[] = {2, 4, 5, 8}, cand_big[] = {2, 4, 5};
    const int* cand = (d.Kn <= 4) ? cand_small : cand_big;
    const int nc = (d.Kn <= 4) ? 4 : (d.Kn <= 10 ? 3 : 2);
    int tpw = cand[nc - 1];
    for (int i = 0; i < nc; ++i)
        if ((long)d.B * cdiv(d.Tp, 8 * cand[i]) <= 256) { tpw = cand[i]; break; }
    EnergyPlan pl;
    pl.tpw = tpw;
    const int TE = 8 * tpw;
    pl.grid = dim3(cdiv(d.Tp, TE), d.B);
    int n[5];
    energy_regions(TE, d.Kn, d.Ks, d.A, n);
    n[4] = conv_parts(d.Kn * (TE / 4)) * d.Kn * TE;     // (a division the kernel does not need before its stage 1)
    pl.lds = lds_bytes(n, 5);
    return pl;
}
void launch_energy(const DecP& p, int t, const EnergyPlan& pl, hipStream_t st) {
    // the if constexpr guards keep (KNMAX, TPW) pairs beyond the register budget from being instantiated (energy_plan never picks them)
    with_knmax_h16(p.d.Kn, p.s.key16 != nullptr, [&](auto kn, auto h) {
        constexpr int KNMAX = decltype(kn)::value;
        constexpr bool H16 = decltype(h)::value;
        switch (pl.tpw) {
            case 2: hipLaunchKernelGGL((att_energy_kernel<KNMAX, 2, H16>), pl.grid, dim3(512), pl.lds, st, p, t); break;
            case 4: hipLaunchKernelGGL((att_energy_kernel<KNMAX, 4, H16>), pl.grid, dim3(512), pl.lds, st, p, t); break;
            case 5: if constexpr (KNMAX <= 10) { hipLaunchKernelGGL((att_energy_kernel<KNMAX, 5, H16>), pl.grid, dim3(512), pl.lds, st, p, t); } break;
            default: if constexpr (KNMAX <= 4) { hipLaunchKernelGGL((att_energy_kernel<KNMAX, 8, H16>), pl.grid, dim3(512), pl.lds, st, p, t); } break;
        }
    });
}

// One decoder step on the per-step kernels: the token's embedding row (unless the whole table was embedded), query, energies, softmax +
// context, one cell per layer.  Context and energy pick their half copies apart (enc16 / key16): a caller may pass one without the other.
void launch_step(const DecP& p, int t, bool bf, const EnergyPlan& epl, bool embed, hipStream_t st) {
    const asr_dec_dims_t& d = p.d;
    if (embed)
        hipLaunchKernelGGL(embed_kernel, dim3(cdiv((long)d.B * d.Dd, 256)), dim3(256), 0, st, p.w.emb, p.s.tokens, p.s.xin, d.B, d.L, d.Dd,
                           d.Dd + d.E, t, 1, d.V);
    with_bool(bf, [&](auto b) { hipLaunchKernelGGL(dec_query_kernel<decltype(b)::value>, dim3(cdiv(d.A, 16)), dim3(256), 0, st, p, t); });
    launch_energy(p, t, epl, st);
    if (p.s.enc16 && (d.E & 3) == 0) hipLaunchKernelGGL(att_softmax_ctx_kernel<true>, dim3(cdiv(d.E, 64), d.B), dim3(256), sizeof(float) * d.Tp, st, p, t);
    else hipLaunchKernelGGL(att_softmax_ctx_kernel<false>, dim3(cdiv(d.E, 64), d.B), dim3(256), sizeof(float) * d.Tp, st, p, t);
    for (int l = 0; l < d.NL; ++l)
        with_bool(bf, [&](auto b) { hipLaunchKernelGGL(dec_cell_fwd_kernel<decltype(b)::value>, dim3(cdiv(d.Dd, 4)), dim3(256), 0, st, p, t, l); });
}

// key = tanh(enc W_k^T + b_k), once per batch (src/asr.py:345)
GemmCall key_call(const asr_dec_dims_t& d, const asr_dec_weights_t& w, const float* enc, float* key, int prec) {
    GemmCall c{enc, w.Wk, key, w.bk, d.B * d.Tp, d.A, d.E, d.E, d.E, d.A};
    c.act = ASR_ACT_TANH; c.prec = prec;
    return c;
}

}  // namespace

extern "C" size_t asr_att_decoder_fwd_work_bytes(const asr_dec_dims_t* dims) {
    return dims ? dec_fwd_plan_info(*dims).work_bytes : 0;
}
extern "C" int asr_att_decoder_fwd_plan(const asr_dec_dims_t* dims) { return dims ? dec_fwd_plan_info(*dims).kind : 0; }
extern "C" int asr_att_decoder_bwd_plan(const asr_dec_dims_t* dims) { return dims ? dec_bwd_plan_info(*dims).kind : 0; }
// the (KNMAX, TPW) pair launch_energy picks for this shape
extern "C" int asr_att_decoder_energy_plan(const asr_dec_dims_t* dims, int* knmax, int* tpw) {
    ASR_REQUIRE(dims && knmax && tpw, ASR_E_ARG, "asr_att_decoder_energy_plan: null pointer");
    const int rc = check_dims(*dims, "asr_att_decoder_energy_plan");
    if (rc != ASR_OK) return rc;
    with_knmax_h16(dims->Kn, false, [&](auto kn, auto) { *knmax = decltype(kn)::value; });      // the dispatch's own thresholds
    *tpw = energy_plan(*dims).tpw;
    return ASR_OK;
}

// first 256 bytes of a work area (the abort word leads them) = 0, and the forward's launch record where the area has a status block
static __global__ void dec_fwd_begin_kernel(unsigned* status, int has_block) {
    status[threadIdx.x] = 0u;
    if (has_block && threadIdx.x == 0) status[DEC_FWD_LAUNCHED_WORD] = 0u;
}

extern "C" int asr_att_decoder_fwd(const asr_dec_dims_t* dims, const asr_dec_weights_t* weights,
                                   const float* enc, const int64_t* enc_len, const int64_t* teacher, int teacher_ld,
                                   const asr_dec_state_t* state, int prec, asr_stream_t stream) {
    ASR_REQUIRE(dims && weights && enc && enc_len && state, ASR_E_ARG, "asr_att_decoder_fwd: null pointer");
    const asr_dec_dims_t& d = *dims;
    int rc = check_dims(d, "asr_att_decoder_fwd");
    if (rc != ASR_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    DecP p{d, *weights, *state, enc, enc_len};
    const bool bf = (prec == ASR_BF16);
    // the abort word (first word of `work`) is defined after EVERY call, whichever kernels run: callers fold it into
    // their status word without knowing whether the persistent launch was taken
    // and so is the word that tells the backward what this forward did (DEC_FWD_LAUNCHED_WORD: 0 here, 1 behind a single launch)
    if (state->work && state->work_bytes >= 256)
        hipLaunchKernelGGL(dec_fwd_begin_kernel, dim3(1), dim3(64), 0, st, (unsigned*)state->work, state->work_bytes >= DEC_STATUS_BYTES ? 1 : 0);

    rc = gemm_run(key_call(d, *weights, enc, state->key, prec), st);
    if (rc != ASR_OK) return rc;
    // bf16 working copies of the two tensors every step re-reads (bf16 contraction mode only; the caller provides the
    // buffers): they halve the loop's HBM traffic and bring its per-XCD working set under the 4 MB L2
    if (state->key16) hipLaunchKernelGGL(cast_bf16_kernel, dim3(1024), dim3(256), 0, st, state->key, (unsigned short*)state->key16, (long)d.B * d.Tp * d.A);
    if (state->enc16) hipLaunchKernelGGL(cast_bf16_kernel, dim3(1024), dim3(256), 0, st, enc, (unsigned short*)state->enc16, (long)d.B * d.Tp * d.E);

    if (teacher) {
        hipLaunchKernelGGL(shift_tokens_kernel, dim3(cdiv(d.B * d.L, 256)), dim3(256), 0, st, teacher, state->tokens, d.B, d.L, teacher_ld);
        hipLaunchKernelGGL(embed_kernel, dim3(cdiv((long)d.B * d.L * d.Dd, 256)), dim3(256), 0, st, weights->emb, state->tokens,
                           state->xin, d.B, d.L, d.Dd, d.Dd + d.E, 0, d.L, d.V);
    } else {
        hipMemsetAsync(state->tokens, 0, sizeof(int64_t) * d.B * d.L, st);
    }

    const EnergyPlan epl = energy_plan(d);
    ASR_REQUIRE(epl.lds <= 64 * 1024, ASR_E_UNSUPPORTED, "asr_att_decoder_fwd: energy tile needs %zu B of LDS", epl.lds);
    int t_begin = 0;
    if (teacher && bf && state->work) {
        // the whole teacher-forced loop as one persistent launch (decoder_persist.hip) when the shape has a plan
        rc = dec_fwd_persistent(d, *weights, *state, enc, enc_len, state->work, state->work_bytes, st);
        if (rc < 0) return rc;
        if (rc == ASR_OK) t_begin = d.L;
    }
    for (int t = t_begin; t < d.L; ++t) {
        launch_step(p, t, bf, epl, !teacher, st);      // the teacher's tokens were embedded above, all steps at once
        if (!teacher) hipLaunchKernelGGL(dec_greedy_kernel, dim3(d.B), dim3(256), 0, st, p, t);
    }
    ASR_LAUNCH_CHECK("asr_att_decoder_fwd");
    if (teacher) {
        // logits[b,t,:] = W_c h_top[b,t] + b_c for all steps in one contraction
        GemmCall logits{state->hs + (size_t)(d.NL - 1) * d.Dd, weights->Wc, state->logits, weights->bc, d.B * d.L, d.V, d.Dd,
                        (long)d.NL * d.Dd, d.Dd, d.V};
        logits.prec = prec;
        rc = gemm_run(logits, st);
        if (rc != ASR_OK) return rc;
    }
    return ASR_OK;
}

// One decode step t for every row of the state (beam search: rows = live hypotheses, all at the same step).
// The caller has set state->tokens[:, t] (input token of the step) and, for t > 0, the step t-1 entries of
// hs / cs / att of every row (parents' values after pruning).  Produces att[:, t], xin[:, t], gates/cs/hs[:, t]
// and logits[:, t].  (state->key must hold tanh(proj_k(enc)) — asr_att_decoder_keys.)
extern "C" int asr_att_decoder_keys(const asr_dec_dims_t* dims, const asr_dec_weights_t* weights, const float* enc,
                                    float* key, int prec, asr_stream_t stream) {
    ASR_REQUIRE(dims && weights && enc && key, ASR_E_ARG, "asr_att_decoder_keys: null pointer");
    return gemm_run(key_call(*dims, *weights, enc, key, prec), (hipStream_t)stream);
}

extern "C" int asr_att_decoder_step(const asr_dec_dims_t* dims, const asr_dec_weights_t* weights,
                                    const float* enc, const int64_t* enc_len, const asr_dec_state_t* state, int t,
                                    int prec, asr_stream_t stream) {
    ASR_REQUIRE(dims && weights && enc && enc_len && state, ASR_E_ARG, "asr_att_decoder_step: null pointer");
    const asr_dec_dims_t& d = *dims;
    int rc = check_dims(d, "asr_att_decoder_step");
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(t >= 0 && t < d.L, ASR_E_ARG, "asr_att_decoder_step: step %d outside [0,%d)", t, d.L);
    hipStream_t st = (hipStream_t)stream;
    DecP p{d, *weights, *state, enc, enc_len};
    const EnergyPlan epl = energy_plan(d);
    ASR_REQUIRE(epl.lds <= 64 * 1024, ASR_E_UNSUPPORTED, "asr_att_decoder_step: energy tile needs %zu B of LDS", epl.lds);
    launch_step(p, t, prec == ASR_BF16, epl, true, st);
    ASR_LAUNCH_CHECK("asr_att_decoder_step");
    if (d.V > DEC_LOGITS_ROW_MAX_V) {
        // word and subword vocabularies: logits[:, t] = hs_top[:, t] Wc^T + bc as ONE contraction over all rows, which reads Wc
        // once per row tile; the per-row kernel below reads it once per row
        GemmCall logits{state->hs + ((size_t)t * d.NL + (d.NL - 1)) * d.Dd, weights->Wc, state->logits + (size_t)t * d.V, weights->bc,
                        d.B, d.V, d.Dd, (long)d.L * d.NL * d.Dd, d.Dd, (long)d.L * d.V};
        logits.prec = prec;
        return gemm_run(logits, st);
    }
    hipLaunchKernelGGL(dec_logits_kernel, dim3(d.B), dim3(256), 0, st, p, t);
    ASR_LAUNCH_CHECK("asr_att_decoder_step");
    return ASR_OK;
}

// offset of the persistent backward's status block inside the workspace: it opens the launch's work area (decoder_plan.h::bwd_work;
// diagnostics: tools/diag_dec.py)
extern "C" size_t asr_att_decoder_bwd_status_offset(const asr_dec_dims_t* dims) {
    if (!dims) return 0;
    return bwd_layout(*dims).pwork;
}

// tiles per utterance of the persistent backward launch (0: the shape has no plan and the per-step kernels run)
extern "C" int asr_att_decoder_bwd_persistent_tiles(const asr_dec_dims_t* dims) {
    if (!dims) return 0;
    return bwd_layout(*dims).ntp;
}

extern "C" size_t asr_att_decoder_bwd_workspace_bytes(const asr_dec_dims_t* dims) {
    if (!dims) return 0;
    return bwd_layout(*dims).total;
}

// reduction slices of a weight-gradient contraction (out_rows x out_cols, reduction over `depth` rows): these outputs are a
// handful of 128x128 tiles with a reduction thousands of rows deep, i.e. a few workgroups walking ~100 dependent k-steps;
// slices of >= 256 rows spread them over about one round of workgroups (fp32 atomics into the gradient)
static int wgrad_slices(int out_rows, int out_cols, int depth) {
    const int tiles = cdiv(out_rows, 128) * cdiv(out_cols, 128);
    int s = 768 / tiles;
    if (s > depth / 256) s = depth / 256;
    return s < 1 ? 1 : (s > 64 ? 64 : s);
}

// What both halves of the backward start with: argument checks under the name of the entry point called, the workspace
// layout, and the kernels' argument block over that workspace (every pointer, whichever half reads it).
static int bwd_begin(const char* who, const asr_dec_dims_t* dims, const asr_dec_weights_t* weights, const asr_dec_grads_t* grads,
                     const float* enc, const int64_t* enc_len, const asr_dec_state_t* state, const float* dlogits,
                     void* workspace, size_t workspace_bytes, BwdLayout* lay, DecB* p) {
    ASR_REQUIRE(dims && weights && grads && enc && enc_len && state && dlogits && workspace, ASR_E_ARG, "%s: null pointer", who);
    const asr_dec_dims_t& d = *dims;
    const int rc = check_dims(d, who);
    if (rc != ASR_OK) return rc;
    *lay = bwd_layout(d);
    ASR_REQUIRE(workspace_bytes >= lay->total, ASR_E_ARG, "%s: workspace %zu < %zu", who, workspace_bytes, lay->total);
    auto at = [&](size_t off) { return (float*)((char*)workspace + off); };
    p->f = DecP{d, *weights, *state, enc, enc_len};
    p->g = *grads;
    p->dhs = at(lay->dhs); p->dxin = at(lay->dxin); p->dq = at(lay->dq);
    p->dkey = at(lay->dkey); p->datt_next = at(lay->datt_next);
    p->dcf = at(lay->dcf); p->wqT = at(lay->wq_t);
    p->slots = at(lay->slots); p->nte = lay->nte; p->slot = lay->slot;
    for (int l = 0; l < ASR_MAX_DEC_LAYERS; ++l) p->wcatT[l] = (l < d.NL) ? at(lay->wcat[l]) : nullptr;
    return ASR_OK;
}

// dst[r * dst_ld + c] += src[r * width + c]: an outside gradient on the top layer's h_t joins dh_top (asr_att_decoder_bwd_hs)
static __global__ __launch_bounds__(256) void add_rows_kernel(float* dst, long dst_ld, const float* src, long rows, int width) {
    const long n = rows * width;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[(i / width) * dst_ld + i % width] += src[i];
}

// Both backward loops take the dot of the softmax backward from the SAVED context (att_bwd_energy_kernel and the persistent launch:
// dot = dctx . ctx), which is exact only when ctx = sum_tau attn[tau] * enc[tau] over the operands the backward itself reads: the fp32
// attention row and the bf16 copy of enc, as att_softmax_ctx_kernel<true> forms it.  The single-launch forward rounds its context
// operands differently (coherently for a flat attention row: 0.5 % of ctx measured), which leaves sum_tau de[tau] != 0 and biases
// every gradient of the energy path (gradient cosine 0.974 against float64 at A = 24).  Behind such a forward the context columns
// of xin are restated from the saved attention before the loop.  grid (ceil(E/256), B, ceil(L/32)): a block owns 256 columns of 32
// decoder steps of one utterance; the attention rows pass through LDS 64 frames at a time and each frame of enc is read once
// for all of them (thread = four columns x 8 steps: one 8-byte load and 8 LDS broadcasts per 32 products).  E % 4 == 0.
// The kernel OVERWRITES the saved xin: asr_att_decoder_bwd_params then takes dW_ih from the restated context, not from the value the
// forward's gates saw (they differ by the same 0.5 %; the restated one is the exact sum).  Whether the forward took the single launch
// is not decided again here: the plan switches can change between the two passes and a launch can be declined for residency.  The
// forward records what it did in the status block of state->work (DEC_FWD_LAUNCHED_WORD, decoder_internal.h), the backward launches
// this kernel whenever the state carries such a block, and the kernel returns at once where the word is 0 (per-step loop, greedy or
// sampled forward handed a work area: att_softmax_ctx_kernel<true> formed this very sum).  The record is as old as the last forward
// on that work area: a second forward of the same area before the first one's backward replaces it.  An utterance with
// enc_len <= 0 keeps the forward's context.
static __global__ __launch_bounds__(256) void ctx_from_saved_att_kernel(DecP p) {
    __shared__ float s_att[32 * 64];                      // [step][frame]
    const asr_dec_dims_t& d = p.d;
    const int b = blockIdx.y, c4 = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int e = blockIdx.x * 256 + 4 * c4, lb = blockIdx.z * 32;
    const int len = min((int)p.enc_len[b], d.Tp);
    if (len <= 0) return;                                 // the whole block
    if (reinterpret_cast<const unsigned*>(p.s.work)[DEC_FWD_LAUNCHED_WORD] == 0u) return;    // the per-step loop ran: its context is this sum
    const unsigned short* ep = reinterpret_cast<const unsigned short*>(p.s.enc16) + (long)b * d.Tp * d.E + min(e, d.E - 4);
    float4 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int tau0 = 0; tau0 < len; tau0 += 64) {
        __syncthreads();
        for (int i = threadIdx.x; i < 32 * 64; i += 256) {
            const int r = i >> 6, tau = tau0 + (i & 63);
            s_att[i] = (tau < len && lb + r < d.L) ? p.s.att[((long)b * d.L + lb + r) * d.Tp + tau] : 0.f;
        }
        __syncthreads();
        // sixteen frames of enc in flight per thread (clamped addresses: frames past len meet a zero attention weight in LDS)
        for (int t0 = 0; t0 < 64 && tau0 + t0 < len; t0 += 16) {
            float4 x[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) x[u] = ld4_bf16(ep + (long)min(tau0 + t0 + u, len - 1) * d.E);
#pragma unroll
            for (int u = 0; u < 16; ++u) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float a = s_att[(rg * 8 + j) * 64 + t0 + u];
                    acc[j].x += a * x[u].x; acc[j].y += a * x[u].y; acc[j].z += a * x[u].z; acc[j].w += a * x[u].w;
                }
            }
        }
    }
    if (e < d.E) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int l = lb + rg * 8 + j;
            if (l < d.L) {                                // Dd need not be a multiple of 4: scalar stores
                float* o = p.s.xin + ((long)b * d.L + l) * (d.Dd + d.E) + d.Dd + e;
                o[0] = acc[j].x; o[1] = acc[j].y; o[2] = acc[j].z; o[3] = acc[j].w;
            }
        }
    }
}

extern "C" int asr_att_decoder_bwd_ex(const asr_dec_dims_t* dims, const asr_dec_weights_t* weights, const asr_dec_grads_t* grads,
                                      const float* enc, const int64_t* enc_len, const asr_dec_state_t* state,
                                      const float* dlogits, float* denc,
                                      void* workspace, size_t workspace_bytes, int prec, int defer_params, int* looped_out,
                                      asr_stream_t stream) {
    return asr_att_decoder_bwd_hs(dims, weights, grads, enc, enc_len, state, dlogits, nullptr, denc, workspace, workspace_bytes, prec,
                                  defer_params, looped_out, stream);
}

extern "C" int asr_att_decoder_bwd_hs(const asr_dec_dims_t* dims, const asr_dec_weights_t* weights, const asr_dec_grads_t* grads,
                                      const float* enc, const int64_t* enc_len, const asr_dec_state_t* state,
                                      const float* dlogits, const float* dhs_ext, float* denc,
                                      void* workspace, size_t workspace_bytes, int prec, int defer_params, int* looped_out,
                                      asr_stream_t stream) {
    ASR_REQUIRE(denc, ASR_E_ARG, "asr_att_decoder_bwd: null pointer");
    BwdLayout lay;
    DecB p;
    int rc = bwd_begin("asr_att_decoder_bwd", dims, weights, grads, enc, enc_len, state, dlogits, workspace, workspace_bytes, &lay, &p);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(((uintptr_t)workspace & 255) == 0, ASR_E_ARG, "asr_att_decoder_bwd: workspace must be 256B aligned");
    const asr_dec_dims_t& d = *dims;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int XW = d.Dd + d.E;
    const bool bf = (prec == ASR_BF16);
    const long SW = (long)d.NL * d.Dd;
    const int BL = d.B * d.L;
    float* dkeypre = (float*)(ws + lay.dkeypre);

    // zero-initialised accumulators dhs, dq, dkey, slots (dxin is fully written by the loop) and the abort word of the persistent
    // launch's status block (defined, 0, after every call - see asr_att_decoder_fwd): contiguous in the layout, one fill
    hipMemsetAsync(ws + lay.dhs, 0, lay.pwork + 256 - lay.dhs, st);

    // transposed weights so that every per-step contraction is K-contiguous
    for (int l = 0; l < d.NL; ++l) {
        const int Kx = (l == 0) ? XW : d.Dd;
        hipLaunchKernelGGL(transpose_kernel, dim3(256), dim3(256), 0, st, weights->Wih[l], p.wcatT[l], 4 * d.Dd, Kx, (long)4 * d.Dd, 0L);
        // rows Kx.. of wcatT hold W_hh^T
        hipLaunchKernelGGL(transpose_kernel, dim3(256), dim3(256), 0, st, weights->Whh[l], p.wcatT[l] + (size_t)Kx * 4 * d.Dd, 4 * d.Dd, d.Dd,
                           (long)4 * d.Dd, 0L);
    }
    hipLaunchKernelGGL(transpose_kernel, dim3(256), dim3(256), 0, st, weights->Wq, p.wqT, d.A, d.Q, (long)d.A, 0L);

    // output layer: dh_top = dlogits W_c ; dW_c += dlogits^T h_top ; db_c += colsum(dlogits)
    GemmCall dh_top{dlogits, weights->Wc, p.dhs + (size_t)(d.NL - 1) * d.Dd, nullptr, BL, d.Dd, d.V, d.V, d.Dd, SW};
    dh_top.b_kc = 0; dh_top.prec = prec;
    rc = gemm_run(dh_top, st);
    if (rc != ASR_OK) return rc;
    if (dhs_ext) {
        const long n = (long)BL * d.Dd;
        hipLaunchKernelGGL(add_rows_kernel, dim3((unsigned)((n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256)), dim3(256), 0, st,
                           p.dhs + (size_t)(d.NL - 1) * d.Dd, SW, dhs_ext, (long)BL, d.Dd);
    }

    const int taps = 2 * d.Ks + 1;
    const int nw_e = cdiv(d.A, 64);
    ASR_REQUIRE(state->conv, ASR_E_ARG, "asr_att_decoder_bwd: state->conv (saved location convolution) is NULL");
    ASR_REQUIRE(nw_e * lay.NG <= 10, ASR_E_UNSUPPORTED, "asr_att_decoder_bwd: attention dim %d > 640", d.A);
    ASR_REQUIRE(d.Kn * ((taps + 3) / 4) <= 2048, ASR_E_UNSUPPORTED, "asr_att_decoder_bwd: location filter bank %d x %d too large", d.Kn, taps);
    ASR_REQUIRE(lay.lds_e <= 150 * 1024 && lay.lds_c <= 148 * 1024 && lay.lds_w <= 150 * 1024, ASR_E_UNSUPPORTED,
                "asr_att_decoder_bwd: shape needs %zu / %zu / %zu B of LDS", lay.lds_e, lay.lds_c, lay.lds_w);
    static bool attr_set = false;
    if (!attr_set) {
        for (int kn : {4, 10, 16})                      // one Kn per arm of with_knmax_h16: all six instantiations
            for (bool h : {false, true})
                with_knmax_h16(kn, h, [](auto k, auto hh) {
                    hipFuncSetAttribute((const void*)att_bwd_energy_kernel<decltype(k)::value, decltype(hh)::value>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024);
                });
        // (4 KB of static LDS of the query part count against the 160 KB)
        hipFuncSetAttribute((const void*)att_bwd_tail_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 8192);
        hipFuncSetAttribute((const void*)att_bwd_tail_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 8192);
        hipFuncSetAttribute((const void*)wconv_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024);
        attr_set = true;
    }
    bool looped = false;
    float* pdg = nullptr;         // gate gradients of the persistent backward (it leaves the saved gates intact)
    const bool h16 = state->key16 != nullptr && state->enc16 != nullptr && (d.E & 3) == 0;
    if (bf && h16 && state->work && state->work_bytes >= DEC_STATUS_BYTES)
        hipLaunchKernelGGL(ctx_from_saved_att_kernel, dim3(cdiv(d.E, 256), d.B, cdiv(d.L, 32)), dim3(256), 0, st, p.f);
    if (bf && lay.ntp > 0 && state->enc16 && d.NL == 1) {
        // the whole loop as one persistent, cluster-per-utterance launch (decoder_persist.hip)
        rc = dec_bwd_persistent(d, *weights, *state, enc_len, p.dhs, p.dxin, p.dq, p.dkey, p.slots, lay.slot, p.wcatT[0], p.wqT,
                                ws + lay.pwork, lay.pwork_bytes, &pdg, st);
        if (rc < 0) return rc;
        if (rc == ASR_OK) {
            looped = true;
            // (the kernel wrote the context part of dxin; the embedding part is only read by the embedding gradient and is
            // computed with it, asr_att_decoder_bwd_params)
        }
    }
    const dim3 grid_e(lay.nte, d.B), block_e(64 * nw_e * lay.NG);
    const dim3 grid_c(cdiv(d.Tp, lay.TC), d.B);
    for (int t = looped ? -1 : d.L - 1; t >= 0; --t) {
        const int last = (t == d.L - 1);
        const int fuse = (d.NL == 1) ? 1 : 0;    // the cell backward's elementwise part rides on the previous query backward
        for (int l = d.NL - 1; l >= 0; --l) {
            if (!fuse || last)
                hipLaunchKernelGGL(dec_cell_bwd_elem_kernel, dim3(cdiv(d.B * d.Dd, 256)), dim3(256), 0, st, p, t, l, last);
            const int width = ((l == 0) ? XW : d.Dd) + d.Dd;
            with_bool(bf, [&](auto b) { hipLaunchKernelGGL(dec_cell_bwd_mm_kernel<decltype(b)::value>, dim3(cdiv(width, 16)), dim3(256), 0, st, p, t, l); });
        }
        with_knmax_h16(d.Kn, h16, [&](auto kn, auto h) {
            hipLaunchKernelGGL((att_bwd_energy_kernel<decltype(kn)::value, decltype(h)::value>), grid_e, block_e, lay.lds_e, st, p, t, lay.TE, lay.NG, last);
        });
        if (t > 0) {
            // the location path reaches attn_{t-1}; step 0 convolves the constant initial attention
            const int nconv = (int)(grid_c.x * grid_c.y), nq = cdiv(d.Q, 16);
            if (bf) hipLaunchKernelGGL(att_bwd_tail_kernel<true>, dim3(nconv + nq), dim3(512), lay.lds_c, st, p, t, lay.TC, (int)grid_c.x, nconv, fuse);
            else    hipLaunchKernelGGL(att_bwd_tail_kernel<false>, dim3(nconv + nq), dim3(512), lay.lds_c, st, p, t, lay.TC, (int)grid_c.x, nconv, fuse);
        }
    }
    ASR_LAUNCH_CHECK("asr_att_decoder_bwd");

    // ---- the rest of the critical path: gradient wrt the encoder output ----------------------------------------
    // context: denc[b] += attn[b]^T (T' x L) dctx[b] (L x E)
    GemmCall dctx = gemm_wgrad_call(state->att, p.dxin + d.Dd, denc, d.Tp, d.E, d.L, d.Tp, XW, d.E, 1);
    dctx.batch = d.B; dctx.sA = (long)d.L * d.Tp; dctx.sB = (long)d.L * XW; dctx.sC = (long)d.Tp * d.E;
    dctx.prec = prec;
    rc = gemm_run(dctx, st);
    if (rc != ASR_OK) return rc;
    // key projection backward
    rc = asr_act_bwd(p.dkey, state->key, dkeypre, (long)d.B * d.Tp * d.A, ASR_ACT_TANH, stream);
    if (rc != ASR_OK) return rc;
    GemmCall dkey{dkeypre, weights->Wk, denc, nullptr, d.B * d.Tp, d.E, d.A, d.A, d.E, d.E};
    dkey.b_kc = 0; dkey.accum = 1; dkey.prec = prec;
    rc = gemm_run(dkey, st);
    if (rc != ASR_OK) return rc;
    ASR_LAUNCH_CHECK("asr_att_decoder_bwd(tail)");
    if (looped_out) *looped_out = looped ? 1 : 0;
    if (defer_params) return ASR_OK;
    return asr_att_decoder_bwd_params(dims, weights, grads, enc, enc_len, state, dlogits, workspace, workspace_bytes, looped ? 1 : 0, prec, stream);
}

extern "C" int asr_att_decoder_bwd(const asr_dec_dims_t* dims, const asr_dec_weights_t* weights, const asr_dec_grads_t* grads,
                                   const float* enc, const int64_t* enc_len, const asr_dec_state_t* state,
                                   const float* dlogits, float* denc,
                                   void* workspace, size_t workspace_bytes, int prec, asr_stream_t stream) {
    return asr_att_decoder_bwd_ex(dims, weights, grads, enc, enc_len, state, dlogits, denc, workspace, workspace_bytes, prec, 0, nullptr, stream);
}

// Parameter gradients of the decoder from what asr_att_decoder_bwd_ex left in the workspace and the saved state: nothing on
// the path to the encoder gradient depends on them, so the caller may run this on another stream beside the encoder's BPTT.
extern "C" int asr_att_decoder_bwd_params(const asr_dec_dims_t* dims, const asr_dec_weights_t* weights, const asr_dec_grads_t* grads,
                                          const float* enc, const int64_t* enc_len, const asr_dec_state_t* state, const float* dlogits,
                                          void* workspace, size_t workspace_bytes, int looped, int prec, asr_stream_t stream) {
    BwdLayout lay;
    DecB p;
    int rc = bwd_begin("asr_att_decoder_bwd_params", dims, weights, grads, enc, enc_len, state, dlogits, workspace, workspace_bytes, &lay, &p);
    if (rc != ASR_OK) return rc;
    const asr_dec_dims_t& d = *dims;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int XW = d.Dd + d.E;
    const bool bf = (prec == ASR_BF16);
    const long SW = (long)d.NL * d.Dd;
    const int BL = d.B * d.L;
    const int taps = 2 * d.Ks + 1;
    float* wslots = (float*)(ws + lay.wslots);
    float* dkeypre = (float*)(ws + lay.dkeypre);
    const float* pdg = looped ? dec_bwd_dgates(d, ws + lay.pwork) : nullptr;
    const int nslots_used = d.B * (looped ? lay.ntp : lay.nte);
    // output layer: dW_c += dlogits^T h_top ; db_c += colsum(dlogits)
    GemmCall gWc = gemm_wgrad_call(dlogits, state->hs + (size_t)(d.NL - 1) * d.Dd, grads->Wc, d.V, d.Dd, BL, d.V, SW, d.Dd, wgrad_slices(d.V, d.Dd, BL));
    gWc.prec = prec;
    rc = gemm_run(gWc, st);
    if (rc != ASR_OK) return rc;
    rc = asr_colsum(dlogits, d.V, BL, d.V, grads->bc, stream);
    if (rc != ASR_OK) return rc;
    // ---- batched parameter gradients -----------------------------------------------------------
    for (int l = 0; l < d.NL; ++l) {
        const float* dg = looped ? pdg : state->gates + (size_t)l * 4 * d.Dd;   // rows (b,t), stride NL*4Dd
        const long ldg = (long)d.NL * 4 * d.Dd;
        const int Kx = (l == 0) ? XW : d.Dd;
        const float* xl = (l == 0) ? state->xin : state->hs + (size_t)(l - 1) * d.Dd;
        const long ldx = (l == 0) ? XW : SW;
        GemmCall gWih = gemm_wgrad_call(dg, xl, grads->Wih[l], 4 * d.Dd, Kx, BL, ldg, ldx, Kx, wgrad_slices(4 * d.Dd, Kx, BL));
        gWih.prec = prec;
        rc = gemm_run(gWih, st);
        if (rc != ASR_OK) return rc;
        // against h_{t-1}: row (b,t) of hs is read at (b, t - 1), zero at t = 0
        GemmCall gWhh = gemm_wgrad_call(dg, state->hs + (size_t)l * d.Dd, grads->Whh[l], 4 * d.Dd, d.Dd, BL, ldg, SW, d.Dd, wgrad_slices(4 * d.Dd, d.Dd, BL));
        gWhh.seqT = d.L; gWhh.bshift = -1; gWhh.prec = prec;
        rc = gemm_run(gWhh, st);
        if (rc != ASR_OK) return rc;
        rc = asr_colsum2(dg, ldg, BL, 4 * d.Dd, grads->bih[l], grads->bhh[l], stream);
        if (rc != ASR_OK) return rc;
    }
    // query projection: dW_q += dqpre^T hcat_{t-1}, db_q += colsum(dqpre)
    GemmCall gWq = gemm_wgrad_call(p.dq, state->hs, grads->Wq, d.A, d.Q, BL, d.A, d.Q, d.Q, wgrad_slices(d.A, d.Q, BL));
    gWq.seqT = d.L; gWq.bshift = -1; gWq.prec = prec;
    rc = gemm_run(gWq, st);
    if (rc != ASR_OK) return rc;
    rc = asr_colsum(p.dq, d.A, BL, d.A, grads->bq, stream);
    if (rc != ASR_OK) return rc;
    // embedding.  After the persistent backward the embedding part of dxin is still to be formed:
    // dgates (B*L x 4Dd) . W_ih[:, :Dd]
    if (looped) {
        GemmCall demb{pdg, weights->Wih[0], p.dxin, nullptr, BL, d.Dd, 4 * d.Dd, 4 * d.Dd, XW, XW};
        demb.b_kc = 0; demb.prec = prec;
        rc = gemm_run(demb, st);
        if (rc != ASR_OK) return rc;
    }
    hipLaunchKernelGGL(embed_bwd_kernel, dim3(d.V, cdiv(d.Dd, 64)), dim3(256), (size_t)4 * std::min(cdiv(BL, 4), EMB_LIST_MAX) * sizeof(int), st,
                       p.dxin, state->tokens, grads->emb, d.B, d.L, d.Dd, XW, d.V);
    // key projection
    const int M = d.B * d.Tp;
    const int splits = wgrad_slices(d.A, d.E, M);
    GemmCall gWk = gemm_wgrad_call(dkeypre, enc, grads->Wk, d.A, d.E, M, d.A, d.E, d.E, splits);
    gWk.prec = prec;
    rc = gemm_run(gWk, st);
    if (rc != ASR_OK) return rc;
    rc = asr_colsum(dkeypre, d.A, M, d.A, grads->bk, stream);
    if (rc != ASR_OK) return rc;
    // slot partials -> d w_g, d W_proj, d b_g;  d W_conv from the saved dconv of every step
    const int nslots = nslots_used;
    hipLaunchKernelGGL(slot_reduce_kernel, dim3(cdiv(d.A, 4)), dim3(256), 0, st, p.slots, nslots, lay.slot, grads->wg, 0, d.A, 0, 0);
    hipLaunchKernelGGL(slot_reduce_kernel, dim3(cdiv(d.A * d.Kn, 4)), dim3(256), 0, st, p.slots, nslots, lay.slot, grads->Wproj, d.A, d.A * d.Kn, d.A, d.Kn);
    hipLaunchKernelGGL(slot_reduce_kernel, dim3(1), dim3(256), 0, st, p.slots, nslots, lay.slot, grads->bg, d.A * (1 + d.Kn), 1, 0, 0);
    {
        if (const size_t lds_m = wconv_mfma_lds(d, bf)) {
            static bool attr_m = false;
            if (!attr_m) { hipFuncSetAttribute((const void*)wconv_grad_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024); attr_m = true; }
            hipLaunchKernelGGL(wconv_grad_mfma_kernel, dim3(lay.nch, d.B), dim3(256), lds_m, st, p.f, wslots);
        } else {
            hipLaunchKernelGGL(wconv_grad_kernel, dim3(lay.nch, d.B), dim3(512), lay.lds_w, st, p.f, wslots);
        }
    }
    hipLaunchKernelGGL(slot_reduce_kernel, dim3(cdiv(d.Kn * taps, 4)), dim3(256), 0, st, wslots, d.B * lay.nch, d.Kn * taps, grads->Wconv,
                       0, d.Kn * taps, 0, 0);
    ASR_LAUNCH_CHECK("asr_att_decoder_bwd_params");
    return ASR_OK;
}


// ---- embedding gradient as a stand-alone entry (RNN-LM training, src/lm.py) ----------------------------------------
// demb[v, :] += sum over rows r with idx[r] == v of dy[r, :width]   (deterministic: fixed summation order per row)
extern "C" int asr_embedding_bwd(const float* dy, long dy_ld, const int64_t* idx, float* demb, int rows, int width, int V, asr_stream_t stream) {
    ASR_REQUIRE(dy && idx && demb && rows > 0 && width > 0 && V > 0 && dy_ld >= width && dy_ld <= 0x7fffffffL, ASR_E_ARG, "asr_embedding_bwd: bad args");
    hipLaunchKernelGGL(embed_bwd_kernel, dim3(V, cdiv(width, 64)), dim3(256), (size_t)4 * std::min(cdiv(rows, 4), EMB_LIST_MAX) * sizeof(int),
                       (hipStream_t)stream, dy, idx, demb, rows, 1, width, (int)dy_ld, V);
    ASR_LAUNCH_CHECK("asr_embedding_bwd");
    return ASR_OK;
}
