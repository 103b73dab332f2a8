// CTC loss (blank = 0, reduction 'mean', zero_infinity = False) forward + gradient in one launch —
// stands in for torch.nn.CTCLoss as the reference calls it (bin/train_asr.py:135,237).
//
// Two launches.  (1) ctc_sweep_kernel, grid (B, 2): workgroup (b, 0) runs the alpha recursion forward in time, workgroup
// (b, 1) the beta recursion backward, concurrently; one thread per state of the extended label sequence, the previous
// frame's lattice column in an LDS double buffer, ONE barrier per frame, the log-probabilities of a chunk of frames
// staged in LDS so that no global read sits on the per-frame critical path; both lattices are spilled to the workspace
// (2 x (B,T,2L+1) fp32).  (2) ctc_grad_kernel, grid (ceil(T/FCH), B): gradient of every frame from alpha + beta,
// fully parallel over frames.  All fp32 log-space (log-sum-exp), whatever `prec` the model runs in.
//
// Gradient convention = the one torch returns for log-softmax inputs: for t < input_len
//   g[b,t,v] = gscale / (B * max(target_len_b,1)) * ( exp(lp[b,t,v]) - sum_{s: ext_s = v} exp(alpha+beta-lp+nll) )
// and exactly 0 for t >= input_len.  An infeasible alignment gives nll = +inf and NaN gradients.
#include "common.h"

namespace {

struct CtcP {
    const float* lp;        // (B,T,V) log-probs
    const int64_t* tgt;     // (B,L) padded with 0
    const int64_t* in_len;  // (B)
    const int64_t* tgt_len; // (B)
    float* nll;             // (B)
    float* loss;            // scalar, += nll_b / (max(tl,1) * B)
    float* grad;            // (B,T,V)
    float* alpha;           // workspace (B,T,Smax)
    float* beta;            // workspace (B,T,Smax)
    int B, T, V, L, Smax;
    float gscale;
};

// log(exp(a) + exp(b)) with one v_exp and one v_log; tolerates -inf on either side
__device__ __forceinline__ float lse2(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + __logf(1.f + __expf(-fabsf(a - b)));
}

// three-way form for the label states (same state, one back, skip): the largest term is exp(0) = 1, so two v_exp and one
// v_log instead of the two + two of a pair of lse2 - the sweeps are bound by the transcendental issue rate
__device__ __forceinline__ float lse3(float a, float b, float c) {
    const float m = fmaxf(fmaxf(a, b), c);
    if (m == -INFINITY) return -INFINITY;
    const float md = __builtin_amdgcn_fmed3f(a, b, c), mn = fminf(fminf(a, b), c);
    return m + __logf(1.f + __expf(md - m) + __expf(mn - m));
}

constexpr int CTC_FCH = 8;        // frames per workgroup of the gradient kernel (halved until the class sums fit in LDS)
constexpr size_t CTC_GRAD_LDS = 60 * 1024;   // dynamic LDS budget of the gradient kernel, the sweep's (64 KiB is what a launch gets at most)

__global__ __launch_bounds__(1024) void ctc_sweep_kernel(CtcP p, int CF) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x, back = blockIdx.y;
    const int tid = threadIdx.x, NTH = blockDim.x;
    const int V = p.V, T = p.T;
    int tl = (int)p.tgt_len[b];
    tl = max(0, min(tl, p.L));
    const int S = 2 * tl + 1;
    int Tin = (int)p.in_len[b];
    Tin = max(0, min(Tin, T));
    int* ext = reinterpret_cast<int*>(smem);                     // [Smax + 2]
    float* buf0 = reinterpret_cast<float*>(ext + p.Smax + 2) + 2;  // [-2 .. Smax+2) padded with -inf on both sides
    float* buf1 = buf0 + p.Smax + 6;
    float* s_lp = buf1 + p.Smax + 4;                              // [CF][V] chunk of log-probs
    const float* lp = p.lp + (long)b * T * V;
    float* lat = (back ? p.beta : p.alpha) + (long)b * T * p.Smax;

    for (int s = tid; s < p.Smax + 2; s += NTH) ext[s] = (s < S && (s & 1)) ? (int)p.tgt[(long)b * p.L + (s >> 1)] : 0;
    for (int s = tid - 2; s < p.Smax + 2; s += NTH) { buf0[s] = -INFINITY; buf1[s] = -INFINITY; }
    __syncthreads();
    if (Tin == 0) {
        if (!back && tid == 0) {                 // no frames: only the empty target is feasible
            const float n = (tl == 0) ? 0.f : INFINITY;
            p.nll[b] = n;
        }
        return;
    }
    // per-state constants: label, and whether the skip transition (s-2 -> s forward, s+2 -> s backward) is allowed.
    // Blank states (even s, never a skip) sit in the first `nwb` waves, label states in the others: a blank wave issues one
    // exp + one log per frame, a label wave two + one, and the round-robin wave -> SIMD placement pairs a blank wave with a
    // label wave (mixed waves would execute the label form in every lane).
    const int nwb = (p.L + 1 + 63) >> 6;
    const bool label = (tid >> 6) >= nwb;           // wave-uniform
    const int s = label ? 2 * (tid - 64 * nwb) + 1 : 2 * tid;
    const bool sok = s < S;
    const int sr = sok ? s : 0;                     // threads past the last state read state 0's neighbourhood (results unused)
    const int e = sok ? ext[s] : 0;
    bool skip = false;
    if (sok && !back) skip = (s >= 2) && e != 0 && e != ext[s - 2];
    if (sok && back) skip = (s + 2 < S) && ext[s + 2] != 0 && ext[s + 2] != e;
    float* prev = buf0;
    float* cur = buf1;
    for (int c0 = 0; c0 < Tin; c0 += CF) {
        // frames of this chunk in processing order: forward t = c0 + i, backward t = Tin-1 - (c0 + i)
        const int nf = min(CF, Tin - c0);
        const int tlo = back ? Tin - c0 - nf : c0;
        __syncthreads();
        for (int i = tid; i < nf * V; i += NTH) s_lp[i] = lp[(long)tlo * V + i];
        __syncthreads();
        for (int i = 0; i < nf; ++i) {
            const int t = back ? Tin - 1 - (c0 + i) : c0 + i;
            const float lpe = s_lp[(t - tlo) * V + e];
            float a;
            if (c0 + i == 0) {
                if (!back) a = (s == 0 || s == 1) ? lpe : -INFINITY;          // alpha_0: states 0 and 1 (ext[1] read is safe: ext is padded)
                else       a = (s == S - 1 || s == S - 2) ? lpe : -INFINITY;  // beta_{Tin-1}
            } else {
                const int d1 = back ? 1 : -1;
                if (label) a = lse3(prev[sr], prev[sr + d1], skip ? prev[sr + 2 * d1] : -INFINITY);
                else       a = lse2(prev[sr], prev[sr + d1]);
                a += lpe;
            }
            if (sok) { cur[s] = a; lat[(long)t * p.Smax + s] = a; }
            __syncthreads();
            float* tmp = prev; prev = cur; cur = tmp;
        }
    }
    if (!back && tid == 0) {
        float ll = prev[S - 1];
        if (S > 1) ll = lse2(ll, prev[S - 2]);
        p.nll[b] = -ll;
    }
}

// gradient of FCH frames of one utterance: one thread per state, class sums through LDS (labels by atomics with the
// multiplicity of the label in the target as contention, blank by a wave reduction)
template <int FCH>
__global__ __launch_bounds__(1024) void ctc_grad_kernel(CtcP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.y, t0 = blockIdx.x * FCH;
    const int tid = threadIdx.x, NTH = blockDim.x, lane = tid & 63, wave = tid >> 6, nwave = NTH >> 6;
    const int V = p.V, T = p.T;
    int tl = (int)p.tgt_len[b];
    tl = max(0, min(tl, p.L));
    const int S = 2 * tl + 1;
    int Tin = (int)p.in_len[b];
    Tin = max(0, min(Tin, T));
    float* acc = reinterpret_cast<float*>(smem);          // [FCH][V]
    float* blk = acc + FCH * V;                       // [FCH][nwave] blank partial sums
    const float* lp = p.lp + (long)b * T * V;
    float* grad = p.grad + (long)b * T * V;
    for (int i = tid; i < FCH * V; i += NTH) acc[i] = 0.f;
    const int s = tid;
    const bool sok = s < S;
    const int e = (sok && (s & 1)) ? (int)p.tgt[(long)b * p.L + (s >> 1)] : 0;
    const float nll = p.nll[b];
    const float scale = p.gscale / (float)(max(tl, 1) * p.B);
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
        // loss = mean_b nll_b / max(target_len_b, 1), summed in utterance order (bitwise repeatable; the sweeps of all
        // utterances have finished before this launch started)
        float sum = 0.f;
        for (int bb = 0; bb < p.B; ++bb) {
            int l = (int)p.tgt_len[bb];
            l = max(1, min(l, p.L));
            sum += p.nll[bb] / (float)(l * p.B);
        }
        *p.loss = sum;
    }
    float occ[FCH];
#pragma unroll
    for (int f = 0; f < FCH; ++f) {
        const int t = t0 + f;
        occ[f] = 0.f;
        if (sok && t < Tin) {
            const long li = ((long)b * T + t) * p.Smax + s;
            // occupancy: exp(alpha + beta - lp + nll); NaN when nll = +inf (infeasible), as in the reference
            occ[f] = expf(p.alpha[li] + p.beta[li] - lp[(long)t * V + e] + nll);
        }
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < FCH; ++f) {
        if (sok && (s & 1) && t0 + f < Tin) atomicAdd(&acc[f * V + e], occ[f]);
        const float bsum = wave_sum((sok && !(s & 1)) ? occ[f] : 0.f);
        if (lane == 0) blk[f * nwave + wave] = bsum;
    }
    __syncthreads();
    for (int i = tid; i < FCH * V; i += NTH) {
        const int f = i / V, v = i - f * V, t = t0 + f;
        if (t >= T) continue;
        float g = 0.f;
        if (t < Tin) {
            float a = acc[i];
            if (v == 0) for (int w = 0; w < nwave; ++w) a += blk[f * nwave + w];
            // a class without a lattice state has posterior exp(-inf + nll): NaN for an infeasible alignment like every
            // other class of the row (torch), not the plain softmax term
            if (!(nll < INFINITY)) a = NAN;
            g = scale * (expf(lp[(long)t * V + v]) - a);
        }
        grad[(long)t * V + v] = g;
    }
}

}  // namespace

extern "C" size_t asr_ctc_loss_workspace_bytes(int B, int T, int L) {
    return 2 * (size_t)B * T * (2 * (size_t)L + 1) * sizeof(float);
}

extern "C" int asr_ctc_loss(const float* logp, const int64_t* targets, const int64_t* input_len, const int64_t* target_len,
                            float* nll, float* loss, float* grad, int B, int T, int V, int L, float gscale,
                            void* workspace, size_t workspace_bytes, asr_stream_t stream) {
    ASR_REQUIRE(logp && targets && input_len && target_len && nll && loss && grad && workspace, ASR_E_ARG, "asr_ctc_loss: null pointer");
    ASR_REQUIRE(B > 0 && T > 0 && V > 1 && L > 0, ASR_E_ARG, "asr_ctc_loss: bad dims");
    ASR_REQUIRE(workspace_bytes >= asr_ctc_loss_workspace_bytes(B, T, L), ASR_E_ARG, "asr_ctc_loss: workspace too small");
    const int Smax = 2 * L + 1;
    float* wsf = (float*)workspace;
    CtcP p{logp, targets, input_len, target_len, nll, loss, grad, wsf, wsf + (size_t)B * T * Smax, B, T, V, L, Smax, gscale};
    ASR_REQUIRE(Smax <= 1024, ASR_E_UNSUPPORTED, "asr_ctc_loss: 2L+1=%d states exceed one workgroup", Smax);
    const int nthr = 64 * ((L + 1 + 63) / 64 + (L + 63) / 64);        // blank waves + label waves (ctc_sweep_kernel)
    // frames of log-probs staged per chunk: as many as fit beside the lattice buffers in 60 KB
    const size_t fixed = (size_t)(Smax + 2) * 4 + 2 * (size_t)(Smax + 6) * 4 + 16;
    int CF = (int)((60 * 1024 - fixed) / ((size_t)V * 4));
    ASR_REQUIRE(CF >= 1, ASR_E_UNSUPPORTED, "asr_ctc_loss: V=%d classes exceed the LDS budget: at most V=%d with 2L+1=%d states "
                "(one frame of log-probs beside the lattice buffers in 60 KB)", V, (int)((60 * 1024 - fixed) / 4), Smax);
    if (CF > T) CF = T;
    const size_t lds_s = fixed + (size_t)CF * V * 4;
    // gradient kernel: CTC_FCH frames of class sums per workgroup, fewer for a vocabulary whose sums would pass the launch limit
    // (V > ~1900; one frame always fits: it is smaller than the sweep's one staged frame + lattice buffers)
    const size_t lds_g1 = (size_t)(V + nthr / 64) * 4;
    ASR_REQUIRE(lds_g1 <= CTC_GRAD_LDS, ASR_E_UNSUPPORTED, "asr_ctc_loss: V=%d classes exceed the %zu bytes of LDS of the gradient kernel",
                V, CTC_GRAD_LDS);
    int fch = CTC_FCH;
    while ((size_t)fch * lds_g1 > CTC_GRAD_LDS) fch >>= 1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ctc_sweep_kernel, dim3(B, 2), dim3(nthr), lds_s, st, p, CF);
    const dim3 gg(cdiv(T, fch), B);
    switch (fch) {
        case 8: hipLaunchKernelGGL(ctc_grad_kernel<8>, gg, dim3(nthr), 8 * lds_g1, st, p); break;
        case 4: hipLaunchKernelGGL(ctc_grad_kernel<4>, gg, dim3(nthr), 4 * lds_g1, st, p); break;
        case 2: hipLaunchKernelGGL(ctc_grad_kernel<2>, gg, dim3(nthr), 2 * lds_g1, st, p); break;
        default: hipLaunchKernelGGL(ctc_grad_kernel<1>, gg, dim3(nthr), lds_g1, st, p); break;
    }
    ASR_LAUNCH_CHECK("asr_ctc_loss");
    return ASR_OK;
}
