// The CTC prefix scorer of the joint beam search (reference src/ctc.py:68-107), batched over live hypotheses:
//   asr_ctc_prefix_init[_batched]  : CTCPrefixScore.init_state (running blank-only path)
//   asr_ctc_prefix_score[_batched] : CTCPrefixScore.cheap_compute for N hypotheses x C candidate tokens in one launch
// Row n belongs to utterance n / rows_per_utt, whose log-probs are logp[utt] (Tmax,V) with tlen[utt] valid frames.  The
// single-utterance entries are the same kernels on one utterance that owns every row and has no tlen: all Tmax frames valid.
#include "common.h"

namespace {

constexpr float LOGZERO = -100000000.0f;   // src/ctc.py:12

// numpy float32 logaddexp (finite "log zero", no -inf handling needed)
__device__ __forceinline__ float lae(float a, float b) {
    const float m = fmaxf(a, b);
    return m + log1pf(expf(-fabsf(a - b)));
}

// the valid frames of utterance utt
__device__ __forceinline__ int ctc_frames(const int* tlen, int utt, int Tmax) { return tlen ? min(max(tlen[utt], 1), Tmax) : Tmax; }

// r (Tmax,2) of one row: r[:,0] = logzero ; r[t,1] = cumulative blank log-prob over the T valid frames, log zero behind them
__device__ __forceinline__ void ctc_prefix_init_row(const float* __restrict__ x, float* __restrict__ r, int T, int Tmax, int V) {
    float acc = 0.f;
    for (int t = 0; t < Tmax; ++t) {
        if (t < T) acc = (t == 0) ? x[0] : acc + x[(long)t * V];
        r[2 * t] = LOGZERO;
        r[2 * t + 1] = t < T ? acc : LOGZERO;
    }
}

// One (hypothesis, candidate `tok`) pair over the T valid frames of x: rp (Tmax,2) the hypothesis' state, ro (Tmax,2) the
// state with tok appended -> psi.  The frames T..Tmax-1 of ro stay unwritten.
__device__ __forceinline__ float ctc_prefix_score_row(const float* __restrict__ x, const float* __restrict__ rp, float* __restrict__ ro,
                                                      int tok, int plen, int last, int T, int V) {
    const int start = max(1, plen);
    for (int t = 0; t < start && t < T; ++t) { ro[2 * t] = LOGZERO; ro[2 * t + 1] = LOGZERO; }
    if (plen == 0) ro[0] = x[tok];
    float r0 = ro[2 * (min(start, T) - 1)], r1 = ro[2 * (min(start, T) - 1) + 1];   // plen > T: stay inside the row
    float psi = r0;
    const bool same = (plen > 0 && tok == last);
    for (int t = start; t < T; ++t) {
        const float p0 = rp[2 * (t - 1)], p1 = rp[2 * (t - 1) + 1];
        const float phi = same ? p1 : lae(p0, p1);
        const float xt = x[(long)t * V + tok];
        const float n0 = lae(r0, phi) + xt;
        const float n1 = lae(r1, r0) + x[(long)t * V];
        psi = lae(psi, phi + xt);
        r0 = n0; r1 = n1;
        ro[2 * t] = r0; ro[2 * t + 1] = r1;
    }
    if (tok == 1) {                                                   // <eos>: probability of the prefix itself
        psi = lae(rp[2 * (T - 1)], rp[2 * (T - 1) + 1]);
        // With no frame left to sweep (plen >= T, or T == 1) the reference's psi is still a view of r[start-1, 0, :], so
        // its assignment lands in the state as well (src/ctc.py:85, 107); the next step reads it back through r_prev[T-1].
        if (start >= T) ro[2 * (T - 1)] = psi;
    }
    return psi;
}

// r (R, Tmax, 2): one workgroup per row, its first thread walks the frames
__global__ void ctc_prefix_init_kernel(const float* __restrict__ x, const int* __restrict__ tlen, float* __restrict__ r, int Tmax, int V, int rpu) {
    if (threadIdx.x != 0) return;
    const int row = blockIdx.x, utt = row / rpu;
    ctc_prefix_init_row(x + (long)utt * Tmax * V, r + (long)row * Tmax * 2, ctc_frames(tlen, utt, Tmax), Tmax, V);
}

// one thread per (hypothesis n, candidate c)
__global__ void ctc_prefix_score_kernel(const float* __restrict__ x, const int* __restrict__ tlen, const float* __restrict__ r_prev,
                                        const int* __restrict__ cand, const int* __restrict__ prefix_len, const int* __restrict__ last_tok,
                                        float* __restrict__ psi_out, float* __restrict__ r_out, int N, int C, int Tmax, int V, int rpu) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * C) return;
    const int n = i / C, utt = n / rpu;
    psi_out[i] = ctc_prefix_score_row(x + (long)utt * Tmax * V, r_prev + (long)n * Tmax * 2, r_out + (long)i * Tmax * 2, cand[i], prefix_len[n],
                                      last_tok[n], ctc_frames(tlen, utt, Tmax), V);
}

int prefix_init(const char* who, const float* logp, const int* tlen, float* r, int rows, int rpu, int Tmax, int V, asr_stream_t stream) {
    hipLaunchKernelGGL(ctc_prefix_init_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, logp, tlen, r, Tmax, V, rpu);
    ASR_LAUNCH_CHECK(who);
    return ASR_OK;
}

int prefix_score(const char* who, const float* logp, const int* tlen, const float* r_prev, const int* cand, const int* prefix_len,
                 const int* last_tok, float* psi, float* r_out, int N, int C, int Tmax, int V, int rpu, asr_stream_t stream) {
    hipLaunchKernelGGL(ctc_prefix_score_kernel, dim3(cdiv((long)N * C, 64)), dim3(64), 0, (hipStream_t)stream, logp, tlen, r_prev, cand,
                       prefix_len, last_tok, psi, r_out, N, C, Tmax, V, rpu);
    ASR_LAUNCH_CHECK(who);
    return ASR_OK;
}

}  // namespace

extern "C" int asr_ctc_prefix_init(const float* logp, float* r, int T, int V, asr_stream_t stream) {
    ASR_REQUIRE(logp && r && T > 0 && V > 1, ASR_E_ARG, "asr_ctc_prefix_init: bad args");
    return prefix_init("asr_ctc_prefix_init", logp, nullptr, r, 1, 1, T, V, stream);
}

extern "C" int asr_ctc_prefix_score(const float* logp, const float* r_prev, const int* candidates, const int* prefix_len,
                                    const int* last_token, float* psi, float* r_out, int N, int C, int T, int V,
                                    asr_stream_t stream) {
    ASR_REQUIRE(logp && r_prev && candidates && prefix_len && last_token && psi && r_out, ASR_E_ARG, "asr_ctc_prefix_score: null pointer");
    ASR_REQUIRE(N > 0 && C > 0 && T > 0 && V > 1, ASR_E_ARG, "asr_ctc_prefix_score: bad dims");
    return prefix_score("asr_ctc_prefix_score", logp, nullptr, r_prev, candidates, prefix_len, last_token, psi, r_out, N, C, T, V, N, stream);
}

extern "C" int asr_ctc_prefix_init_batched(const float* logp, const int* tlen, float* r, int rows, int rows_per_utt, int Tmax, int V,
                                           asr_stream_t stream) {
    ASR_REQUIRE(logp && tlen && r && rows > 0 && rows_per_utt > 0 && Tmax > 0 && V > 1, ASR_E_ARG, "asr_ctc_prefix_init_batched: bad args");
    return prefix_init("asr_ctc_prefix_init_batched", logp, tlen, r, rows, rows_per_utt, Tmax, V, stream);
}

extern "C" int asr_ctc_prefix_score_batched(const float* logp, const int* tlen, const float* r_prev, const int* candidates,
                                            const int* prefix_len, const int* last_token, float* psi, float* r_out,
                                            int N, int C, int Tmax, int V, int rows_per_utt, asr_stream_t stream) {
    ASR_REQUIRE(logp && tlen && r_prev && candidates && prefix_len && last_token && psi && r_out, ASR_E_ARG, "asr_ctc_prefix_score_batched: null pointer");
    ASR_REQUIRE(N > 0 && C > 0 && Tmax > 0 && V > 1 && rows_per_utt > 0, ASR_E_ARG, "asr_ctc_prefix_score_batched: bad dims");
    return prefix_score("asr_ctc_prefix_score_batched", logp, tlen, r_prev, candidates, prefix_len, last_token, psi, r_out, N, C, Tmax, V,
                        rows_per_utt, stream);
}
