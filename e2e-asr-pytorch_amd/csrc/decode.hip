// Kernels of the beam-search inference path (reference src/decode.py:65-183, src/ctc.py:68-107, src/lm.py:27-37),
// batched over live hypotheses:
//   asr_ctc_prefix_score : CTCPrefixScore.cheap_compute for N hypotheses x C candidate tokens in one launch
//   asr_ctc_prefix_init  : CTCPrefixScore.init_state (running blank-only path)
//   asr_lstm_cell        : pointwise LSTM cell on pre-computed gate sums (RNN-LM step; the two projections are asr_gemm)
//   asr_gather_rows      : row gather (embedding lookup, state re-ordering after pruning)
//   asr_masked_copy_rows : dst[r,:] = src[r,:] where mask[r] (CTC-only search: the LM rows of the slots that were extended)
#include <algorithm>
#include "common.h"

namespace {

constexpr float LOGZERO = -100000000.0f;   // src/ctc.py:12

// numpy float32 logaddexp (finite "log zero", no -inf handling needed)
__device__ __forceinline__ float lae(float a, float b) {
    const float m = fmaxf(a, b);
    return m + log1pf(expf(-fabsf(a - b)));
}

__global__ void ctc_prefix_init_kernel(const float* __restrict__ x, float* __restrict__ r, int T, int V) {
    // r (T,2): r[:,0] = logzero ; r[t,1] = cumulative blank log-prob
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float acc = 0.f;
        for (int t = 0; t < T; ++t) {
            acc = (t == 0) ? x[0] : acc + x[(long)t * V];
            r[2 * t] = LOGZERO;
            r[2 * t + 1] = acc;
        }
    }
}

// one thread per (hypothesis n, candidate c)
__global__ void ctc_prefix_score_kernel(const float* __restrict__ x, const float* __restrict__ r_prev, const int* __restrict__ cand,
                                        const int* __restrict__ prefix_len, const int* __restrict__ last_tok,
                                        float* __restrict__ psi_out, float* __restrict__ r_out, int N, int C, int T, int V) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * C) return;
    const int n = i / C;
    const int tok = cand[i];
    const int plen = prefix_len[n], last = last_tok[n];
    const float* rp = r_prev + (long)n * T * 2;
    float* ro = r_out + (long)i * T * 2;
    const int start = max(1, plen);
    for (int t = 0; t < start && t < T; ++t) { ro[2 * t] = LOGZERO; ro[2 * t + 1] = LOGZERO; }
    if (plen == 0) ro[0] = x[tok];
    float r0 = ro[2 * (min(start, T) - 1)], r1 = ro[2 * (min(start, T) - 1) + 1];   // plen > T: stay inside the row, as the batched kernel does
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
    psi_out[i] = psi;
}

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

}  // namespace

extern "C" int asr_ctc_prefix_init(const float* logp, float* r, int T, int V, asr_stream_t stream) {
    ASR_REQUIRE(logp && r && T > 0 && V > 1, ASR_E_ARG, "asr_ctc_prefix_init: bad args");
    hipLaunchKernelGGL(ctc_prefix_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, logp, r, T, V);
    ASR_LAUNCH_CHECK("asr_ctc_prefix_init");
    return ASR_OK;
}

extern "C" int asr_ctc_prefix_score(const float* logp, const float* r_prev, const int* candidates, const int* prefix_len,
                                    const int* last_token, float* psi, float* r_out, int N, int C, int T, int V,
                                    asr_stream_t stream) {
    ASR_REQUIRE(logp && r_prev && candidates && prefix_len && last_token && psi && r_out, ASR_E_ARG, "asr_ctc_prefix_score: null pointer");
    ASR_REQUIRE(N > 0 && C > 0 && T > 0 && V > 1, ASR_E_ARG, "asr_ctc_prefix_score: bad dims");
    hipLaunchKernelGGL(ctc_prefix_score_kernel, dim3(cdiv((long)N * C, 64)), dim3(64), 0, (hipStream_t)stream, logp, r_prev, candidates,
                       prefix_len, last_token, psi, r_out, N, C, T, V);
    ASR_LAUNCH_CHECK("asr_ctc_prefix_score");
    return ASR_OK;
}

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

// =================================================================================================================
// Device-side beam bookkeeping: one decoding step of BeamDecoder.forward (reference src/decode.py:104-177) for U
// utterances x `beam` hypothesis rows WITHOUT a device-to-host copy: candidate selection for the CTC scorer
// (`att_prob.topk(ctc_beam_size)`, :129), score fusion (:131-152), per-hypothesis top-k + the <eos> threshold rule
// (Hypothesis.addTopk :214-263), pruning by average score (:175-177), the `finals` list, and the parent / token indices
// the state gathers of the next step need.  One wave per utterance; vocabularies up to 2048 (lane owns tokens lane + 64k).
// =================================================================================================================
namespace {

constexpr float BEAM_LOG_ZERO = -10000000.0f;      // src/decode.py:11
constexpr int BEAM_MAX = 16, VPL = 32;             // hypotheses per utterance; tokens per lane

// top-C tokens of every row of att (rows, V), descending (ties: lower token first)
__global__ __launch_bounds__(64) void beam_candidates_kernel(const float* __restrict__ att, int* __restrict__ cand, int V, int C) {
    const int row = blockIdx.x, lane = threadIdx.x;
    float v[VPL];
    unsigned taken = 0u;
#pragma unroll
    for (int k = 0; k < VPL; ++k) { const int t = lane + 64 * k; v[k] = t < V ? att[(long)row * V + t] : -INFINITY; }
    for (int c = 0; c < C; ++c) {
        float best = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < VPL; ++k) if (!((taken >> k) & 1u) && lane + 64 * k < V && (v[k] > best)) { best = v[k]; bi = lane + 64 * k; }
        float wb = best; int wi = bi;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(wb, o); const int oi = __shfl_xor(wi, o);
            if (ob > wb || (ob == wb && oi < wi)) { wb = ob; wi = oi; }
        }
        if (wi != 0x7fffffff && (wi & 63) == lane) taken |= 1u << (wi >> 6);
        if (lane == 0) cand[(long)row * C + c] = (wi == 0x7fffffff) ? 0 : wi;
    }
}

struct BeamP {
    // per row (R = U * beam)
    const float* att; const float* lm; const float* psi; const int* cand;        // (R,V), (R,V)|null, (R,C)|null, (R,C)|null
    const int* alive_in; const float* sum_in; const float* ctcp_in; const int* len_in; const int* seq_in; const float* sc_in;
    int* alive_out; float* sum_out; float* ctcp_out; int* len_out; int* seq_out; float* sc_out;
    int* last_tok;                 // (R) last token of each new row (for the CTC scorer)
    long long* parent; long long* ctcidx;   // (R) gather indices for the state of the next step
    long long* tokens; long tok_ld; // decoder token table (R, tok_ld): column t+1 receives the new rows' tokens
    // per utterance
    const int* min_len; const int* max_len; int* done;
    int* fin_n; int* fin_len; float* fin_avg; int* fin_seq; float* fin_sc;          // best `beam` finished hypotheses, sorted
    int U, beam, V, C, Lmax, t;
    float ctc_w, lm_w, eos_thr;
};

__device__ __forceinline__ void final_insert(const BeamP& p, int u, int lane, const int* seq, const float* sc, int len, int last_tok,
                                             float last_sc, bool append, float avg) {
    // stable descending insert into the utterance's finals (new entry behind equal ones); keeps the best `beam`
    const int nf = p.fin_n[u];
    int pos = 0;
    for (int i = 0; i < nf; ++i) if (p.fin_avg[(long)u * p.beam + i] >= avg) pos = i + 1;
    if (pos >= p.beam) return;
    const int newn = min(nf + 1, p.beam);
    const int W = p.Lmax + 1;
    for (int i = newn - 1; i > pos; --i) {
        const long d = ((long)u * p.beam + i), s = d - 1;
        for (int k = lane; k < W; k += 64) { p.fin_seq[d * W + k] = p.fin_seq[s * W + k]; p.fin_sc[d * W + k] = p.fin_sc[s * W + k]; }
        if (lane == 0) { p.fin_avg[d] = p.fin_avg[s]; p.fin_len[d] = p.fin_len[s]; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    }
    const long d = (long)u * p.beam + pos;
    for (int k = lane; k < len; k += 64) { p.fin_seq[d * W + k] = seq[k]; p.fin_sc[d * W + k] = sc[k]; }
    if (lane == 0) {
        int l = len;
        if (append) { p.fin_seq[d * W + len] = last_tok; p.fin_sc[d * W + len] = last_sc; l = len + 1; }
        p.fin_avg[d] = avg; p.fin_len[d] = l; p.fin_n[u] = newn;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
}

// the children of one utterance before pruning: at most beam x beam entries, in LDS
struct BeamPool {
    float avg[BEAM_MAX * BEAM_MAX], sum[BEAM_MAX * BEAM_MAX], topv[BEAM_MAX * BEAM_MAX], ctcp[BEAM_MAX * BEAM_MAX];
    int par[BEAM_MAX * BEAM_MAX], tok[BEAM_MAX * BEAM_MAX], ci[BEAM_MAX * BEAM_MAX], rank[BEAM_MAX * BEAM_MAX];
};

// rows first..beam-1 of the utterance at r0 are dead after this step
__device__ __forceinline__ void beam_kill_rows(const BeamP& p, int r0, int first, int lane) {
    for (int i = first + lane; i < p.beam; i += 64) {
        p.alive_out[r0 + i] = 0; p.parent[r0 + i] = r0 + i; p.ctcidx[r0 + i] = (long long)(r0 + i) * max(p.C, 1);
        p.last_tok[r0 + i] = 0; p.sum_out[r0 + i] = 0.f; p.ctcp_out[r0 + i] = 0.f; p.len_out[r0 + i] = 0;
        p.tokens[(long)(r0 + i) * p.tok_ld + min(p.t + 1, (int)p.tok_ld - 1)] = 0;
    }
}

// lane 0: token wi with fused score wb, picked by hypothesis i of the utterance (row `row`), joins the pool at `slot`
__device__ __forceinline__ void beam_pool_push(const BeamP& p, BeamPool& s, int slot, int i, int row, int wi, float wb, float sum_i, int len_i) {
    s.par[slot] = i; s.tok[slot] = wi; s.topv[slot] = wb; s.sum[slot] = sum_i + wb;
    s.avg[slot] = (sum_i + wb) / (float)(len_i + 1);
    int ci = 0; float cp = 0.f;
    if (p.cand) {
        for (int cc = 0; cc < p.C; ++cc) if (p.cand[(long)row * p.C + cc] == wi) { ci = cc; cp = p.psi[(long)row * p.C + cc]; break; }
    }
    s.ci[slot] = ci; s.ctcp[slot] = cp;
}

// What follows the per-hypothesis picks, for one wave per utterance (asr_beam_step and phase B of asr_beam_step_wide): pruning of
// the pool to the `beam` best by average in stable order, the new rows, the dead rows, the last-step flush into the finals
__device__ __forceinline__ void beam_step_tail(const BeamP& p, BeamPool& s, int u, int lane, int pool, bool stop) {
    const int beam = p.beam, r0 = u * beam, t = p.t;
    __syncthreads();
    if (stop) { beam_kill_rows(p, r0, 0, lane); if (lane == 0) p.done[u] = 1; return; }
    // prune: stable descending order by average score, keep `beam`
    for (int e = lane; e < pool; e += 64) {
        int rank = 0;
        const float a = s.avg[e];
        for (int o = 0; o < pool; ++o) rank += (s.avg[o] > a || (s.avg[o] == a && o < e)) ? 1 : 0;
        s.rank[e] = rank;
    }
    __syncthreads();
    const int kept = min(pool, beam);
    const bool last_step = (t + 1 >= p.max_len[u]);
    for (int e = 0; e < pool; ++e) {
        const int rk = s.rank[e];
        if (rk >= beam) continue;                                        // uniform
        const int src = r0 + s.par[e], dst = r0 + rk;
        const int len_i = p.len_in[src];
        for (int k = lane; k < len_i; k += 64) { p.seq_out[(long)dst * p.Lmax + k] = p.seq_in[(long)src * p.Lmax + k]; p.sc_out[(long)dst * p.Lmax + k] = p.sc_in[(long)src * p.Lmax + k]; }
        if (lane == 0) {
            if (len_i < p.Lmax) { p.seq_out[(long)dst * p.Lmax + len_i] = s.tok[e]; p.sc_out[(long)dst * p.Lmax + len_i] = s.topv[e]; }
            p.alive_out[dst] = 1; p.sum_out[dst] = s.sum[e]; p.ctcp_out[dst] = s.ctcp[e]; p.len_out[dst] = len_i + 1;
            p.last_tok[dst] = s.tok[e]; p.parent[dst] = src; p.ctcidx[dst] = (long long)src * max(p.C, 1) + s.ci[e];
            p.tokens[(long)dst * p.tok_ld + min(t + 1, (int)p.tok_ld - 1)] = s.tok[e];
        }
    }
    beam_kill_rows(p, r0, kept, lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (kept == 0) { if (lane == 0) p.done[u] = 1; return; }
    if (last_step) {
        // the loop of the reference ends here: the surviving hypotheses join the finals in their order (src/decode.py:179-181)
        for (int rk = 0; rk < kept; ++rk) {
            const int row = r0 + rk;
            const int l = p.len_out[row];
            final_insert(p, u, lane, p.seq_out + (long)row * p.Lmax, p.sc_out + (long)row * p.Lmax, min(l, p.Lmax), 0, 0.f, false,
                         p.sum_out[row] / (float)max(l, 1));
        }
        if (lane == 0) p.done[u] = 1;
    }
}

__global__ __launch_bounds__(64) void beam_step_kernel(BeamP p) {
    __shared__ BeamPool s;
    const int u = blockIdx.x, lane = threadIdx.x;
    const int beam = p.beam, V = p.V, r0 = u * beam;
    const int t = p.t;
    if (p.done[u] || t >= p.max_len[u]) { beam_kill_rows(p, r0, 0, lane); if (lane == 0) p.done[u] = 1; return; }
    int pool = 0;
    bool stop = false;
    for (int i = 0; i < beam; ++i) {
        const int row = r0 + i;
        if (!p.alive_in[row]) continue;                                  // uniform
        float att[VPL], cur[VPL];
        const float sum_i = p.sum_in[row], ctcp_i = p.ctcp_in[row];
        const int len_i = p.len_in[row];
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
            const int v = lane + 64 * k;
            att[k] = v < V ? p.att[(long)row * V + v] : -INFINITY;
            float c = att[k];
            if (p.cand) {
                float hack = BEAM_LOG_ZERO;
                for (int cc = 0; cc < p.C; ++cc) if (p.cand[(long)row * p.C + cc] == v) hack = p.psi[(long)row * p.C + cc] - ctcp_i;
                c = (1.f - p.ctc_w) * c + p.ctc_w * hack;
                if (v == 0) c = BEAM_LOG_ZERO;
            }
            if (p.lm && v < V) c += p.lm_w * p.lm[(long)row * V + v];
            cur[k] = v < V ? c : -INFINITY;
        }
        // <eos> rule operands: the attention log-probs, not the fused scores (src/decode.py:235-242)
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < VPL; ++k) { const int v = lane + 64 * k; if (v >= 2 && v < V) mx = fmaxf(mx, att[k]); }
        mx = wave_max(mx);
        const float att_eos = __shfl(att[0], 1);
        unsigned taken = 0u;
        bool term = false; float term_score = 0.f;
        for (int k2 = 0; k2 < beam; ++k2) {
            float best = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
            for (int k = 0; k < VPL; ++k) if (!((taken >> k) & 1u) && lane + 64 * k < V && cur[k] > best) { best = cur[k]; bi = lane + 64 * k; }
            float wb = best; int wi = bi;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ob = __shfl_xor(wb, o); const int oi = __shfl_xor(wi, o);
                if (ob > wb || (ob == wb && oi < wi)) { wb = ob; wi = oi; }
            }
            if (wi == 0x7fffffff) break;
            if ((wi & 63) == lane) taken |= 1u << (wi >> 6);
            if (wi == 1 && att_eos > p.eos_thr * mx) { term = true; term_score = wb; continue; }
            if (lane == 0) beam_pool_push(p, s, pool, i, row, wi, wb, sum_i, len_i);
            ++pool;
        }
        if (term && t >= p.min_len[u]) {
            final_insert(p, u, lane, p.seq_in + (long)row * p.Lmax, p.sc_in + (long)row * p.Lmax, len_i, 1, term_score, true,
                         (sum_i + term_score) / (float)(len_i + 1));
            if (beam == 1) { stop = true; break; }
        }
    }
    beam_step_tail(p, s, u, lane, pool, stop);
}

// =================================================================================================================
// The same bookkeeping for vocabularies of word and subword size (V <= WIDE_VMAX): a row no longer fits one wave's
// registers, so a multi-wave workgroup owns a ROW and its threads stride over V.
//   wide_topk : the K best of a row in the narrow kernels' order (value descending, lower token first among equals).  A
//       thread keeps the best token of its own stride that has not been picked; per pick the workgroup reduces these to one
//       winner (one barrier) and only the winner's thread scans its stride again, for the best entry BEHIND the pick in that
//       order - no mask of taken tokens, and the row is read about once, not K times.
//   asr_beam_candidates_wide : wide_topk on the attention log-probs.
//   asr_beam_step_wide, phase A : per live row the fused score on the fly (the C candidates are marked in a V-bit map in LDS,
//       8 KB at the most, so a token costs one LDS word and the C-entry list is walked for candidates only), wide_topk with
//       K = beam, att[1] and max(att[2:]) -> the row's shortlist in the workspace.
//   phase B : one wave per utterance walks the shortlists of its rows in the order of the narrow kernel's picks and shares
//       everything behind a pick with it (beam_pool_push, final_insert, beam_step_tail).
// Nothing in LDS scales with V beyond the bit map; rows are read from global memory (L2 on the re-scans).
// =================================================================================================================
constexpr int WIDE_NT = 512;             // largest workgroup: __launch_bounds__ of the row kernels, checked on the host; the stride over V
constexpr int WIDE_NW = WIDE_NT / WAVE;
constexpr int WIDE_VMAX = 65536, WIDE_CMAX = 32;
constexpr int WIDE_BITS = 32;            // tokens per word of the candidate bit map
constexpr int WIDE_NONE = 0x7fffffff;

struct WideShort {                       // one row's shortlist: n picks in their order, and the <eos> rule's operands
    float val[BEAM_MAX]; int tok[BEAM_MAX];
    float att1, mx; int n, pad;
};

struct WideRed { float v[2][WIDE_NW]; int i[2][WIDE_NW]; };

// whole waves, one thread per four tokens up to the launch bound
static int wide_threads(int V) { return WAVE * (int)std::min((long)WIDE_NW, (long)cdiv(V, 4 * WAVE)); }

// the best (value, token) over the workgroup; every thread returns it.  `par` alternates between consecutive calls
__device__ __forceinline__ void wide_block_best(float& wb, int& wi, WideRed& red, int par) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(wb, o); const int oi = __shfl_xor(wi, o);
        if (ob > wb || (ob == wb && oi < wi)) { wb = ob; wi = oi; }
    }
    if (lane == 0) { red.v[par][wave] = wb; red.i[par][wave] = wi; }
    __syncthreads();
    wb = red.v[par][0]; wi = red.i[par][0];
    for (int w = 1; w < nw; ++w) {
        const float ob = red.v[par][w]; const int oi = red.i[par][w];
        if (ob > wb || (ob == wb && oi < wi)) { wb = ob; wi = oi; }
    }
}

// the best entry above -inf of this thread's stride that lies behind (pv, pi) in the order
template <class Score> __device__ __forceinline__ void wide_scan(const Score& sc, int V, float pv, int pi, float& bv, int& bi) {
    bv = -INFINITY; bi = WIDE_NONE;
    for (int v = threadIdx.x; v < V; v += blockDim.x) {
        const float x = sc(v);
        if ((x < pv || (x == pv && v > pi)) && x > bv) { bv = x; bi = v; }
    }
}

// -> the number of picks n <= K; thread 0 writes pick k to out_tok[k] (and out_val[k])
template <class Score> __device__ __forceinline__ int wide_topk(const Score& sc, int V, int K, int* out_tok, float* out_val, WideRed& red) {
    float bv; int bi;
    wide_scan(sc, V, INFINITY, -1, bv, bi);
    int n = 0;
    for (; n < K; ++n) {
        float wb = bv; int wi = bi;
        wide_block_best(wb, wi, red, n & 1);
        if (wi == WIDE_NONE) break;                                      // uniform
        if (threadIdx.x == 0) { out_tok[n] = wi; if (out_val) out_val[n] = wb; }
        if (bi == wi) wide_scan(sc, V, wb, wi, bv, bi);
    }
    return n;
}

struct WideAtt {
    const float* att;
    __device__ __forceinline__ float operator()(int v) const { return att[v]; }
};

__global__ __launch_bounds__(WIDE_NT) void beam_candidates_wide_kernel(const float* __restrict__ att, int* __restrict__ cand, int V, int C) {
    __shared__ WideRed red;
    const int row = blockIdx.x;
    const WideAtt sc{att + (long)row * V};
    const int n = wide_topk(sc, V, C, cand + (long)row * C, nullptr, red);
    for (int c = n + threadIdx.x; c < C; c += blockDim.x) cand[(long)row * C + c] = 0;
}

// the fused score of asr_beam_step, in its operation order and without contraction: bit for bit the float32 transcription
struct WideFused {
    const float* att; const float* lm; const unsigned* bits; const int* cand; const float* hack;
    int C; bool ctc; float ctc_w, lm_w;
    __device__ __forceinline__ float operator()(int v) const {
#pragma clang fp contract(off)
        float c = att[v];
        if (ctc) {
            float h = BEAM_LOG_ZERO;
            if ((bits[v / WIDE_BITS] >> (v % WIDE_BITS)) & 1u)
                for (int cc = 0; cc < C; ++cc) if (cand[cc] == v) h = hack[cc];
            c = (1.f - ctc_w) * c + ctc_w * h;
            if (v == 0) c = BEAM_LOG_ZERO;
        }
        if (lm) c += lm_w * lm[v];
        return c;
    }
};

__global__ __launch_bounds__(WIDE_NT) void beam_step_wide_rows_kernel(BeamP p, WideShort* __restrict__ ws) {
    __shared__ WideRed red;
    __shared__ unsigned s_bits[WIDE_VMAX / WIDE_BITS];
    __shared__ int s_cand[WIDE_CMAX];
    __shared__ float s_hack[WIDE_CMAX], s_mx[WIDE_NW];
    const int row = blockIdx.x, u = row / p.beam, tid = threadIdx.x, V = p.V;
    if (p.done[u] || p.t >= p.max_len[u] || !p.alive_in[row]) return;    // uniform: phase B reads no shortlist of such a row
    const float* att = p.att + (long)row * V;
    const bool ctc = p.cand != nullptr;
    if (ctc) {
        const float ctcp_i = p.ctcp_in[row];
        for (int w = tid; w < (V + WIDE_BITS - 1) / WIDE_BITS; w += blockDim.x) s_bits[w] = 0u;
        __syncthreads();
        if (tid < p.C) {
            const int tok = p.cand[(long)row * p.C + tid];
            s_cand[tid] = tok; s_hack[tid] = p.psi[(long)row * p.C + tid] - ctcp_i;
            if (tok >= 0 && tok < V) atomicOr(&s_bits[tok / WIDE_BITS], 1u << (tok % WIDE_BITS));
        }
    }
    // <eos> rule operands: the attention log-probs, not the fused scores (src/decode.py:235-242)
    float mx = -INFINITY;
    for (int v = 2 + tid; v < V; v += blockDim.x) mx = fmaxf(mx, att[v]);
    mx = wave_max(mx);
    if ((tid & 63) == 0) s_mx[tid >> 6] = mx;
    __syncthreads();
    const WideFused sc{att, p.lm ? p.lm + (long)row * V : nullptr, s_bits, s_cand, s_hack, p.C, ctc, p.ctc_w, p.lm_w};
    WideShort& out = ws[row];
    const int n = wide_topk(sc, V, p.beam, out.tok, out.val, red);
    if (tid == 0) {
        mx = s_mx[0];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) mx = fmaxf(mx, s_mx[w]);
        out.att1 = att[1]; out.mx = mx; out.n = n;
    }
}

__global__ __launch_bounds__(64) void beam_step_wide_pool_kernel(BeamP p, const WideShort* __restrict__ ws) {
    __shared__ BeamPool s;
    const int u = blockIdx.x, lane = threadIdx.x;
    const int beam = p.beam, r0 = u * beam, t = p.t;
    if (p.done[u] || t >= p.max_len[u]) { beam_kill_rows(p, r0, 0, lane); if (lane == 0) p.done[u] = 1; return; }
    int pool = 0;
    bool stop = false;
    for (int i = 0; i < beam; ++i) {
        const int row = r0 + i;
        if (!p.alive_in[row]) continue;                                  // uniform
        const WideShort& sl = ws[row];
        const float sum_i = p.sum_in[row];
        const int len_i = p.len_in[row], n = min(sl.n, beam);
        bool term = false; float term_score = 0.f;
        for (int k2 = 0; k2 < n; ++k2) {
            const float wb = sl.val[k2]; const int wi = sl.tok[k2];
            if (wi == 1 && sl.att1 > p.eos_thr * sl.mx) { term = true; term_score = wb; continue; }
            if (lane == 0) beam_pool_push(p, s, pool, i, row, wi, wb, sum_i, len_i);
            ++pool;
        }
        if (term && t >= p.min_len[u]) {
            final_insert(p, u, lane, p.seq_in + (long)row * p.Lmax, p.sc_in + (long)row * p.Lmax, len_i, 1, term_score, true,
                         (sum_i + term_score) / (float)(len_i + 1));
            if (beam == 1) { stop = true; break; }
        }
    }
    beam_step_tail(p, s, u, lane, pool, stop);
}

// CTCPrefixScore.cheap_compute for N hypothesis rows x C candidates over a BATCH of utterances: row n belongs to utterance
// n / rows_per_utt, whose log-probs are logp[utt] (Tmax,V) with tlen[utt] valid frames
__global__ void ctc_prefix_score_batched_kernel(const float* __restrict__ x, const int* __restrict__ tlen, const float* __restrict__ r_prev,
                                                const int* __restrict__ cand, const int* __restrict__ prefix_len, const int* __restrict__ last_tok,
                                                float* __restrict__ psi_out, float* __restrict__ r_out, int N, int C, int Tmax, int V, int rpu) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * C) return;
    const int n = i / C, utt = n / rpu;
    const int T = min(max(tlen[utt], 1), Tmax);
    const float* xu = x + (long)utt * Tmax * V;
    const int tok = cand[i];
    const int plen = prefix_len[n], last = last_tok[n];
    const float* rp = r_prev + (long)n * Tmax * 2;
    float* ro = r_out + (long)i * Tmax * 2;
    const int start = max(1, plen);
    for (int t = 0; t < start && t < T; ++t) { ro[2 * t] = LOGZERO; ro[2 * t + 1] = LOGZERO; }
    if (plen == 0) ro[0] = xu[tok];
    float r0 = ro[2 * (min(start, T) - 1)], r1 = ro[2 * (min(start, T) - 1) + 1];
    float psi = r0;
    const bool same = (plen > 0 && tok == last);
    for (int t = start; t < T; ++t) {
        const float p0 = rp[2 * (t - 1)], p1 = rp[2 * (t - 1) + 1];
        const float phi = same ? p1 : lae(p0, p1);
        const float xt = xu[(long)t * V + tok];
        const float n0 = lae(r0, phi) + xt;
        const float n1 = lae(r1, r0) + xu[(long)t * V];
        psi = lae(psi, phi + xt);
        r0 = n0; r1 = n1;
        ro[2 * t] = r0; ro[2 * t + 1] = r1;
    }
    if (tok == 1) {
        psi = lae(rp[2 * (T - 1)], rp[2 * (T - 1) + 1]);
        if (start >= T) ro[2 * (T - 1)] = psi;                           // as in ctc_prefix_score_kernel
    }
    psi_out[i] = psi;
}

__global__ void ctc_prefix_init_batched_kernel(const float* __restrict__ x, const int* __restrict__ tlen, float* __restrict__ r, int Tmax, int V, int rpu) {
    // r (R, Tmax, 2) for row = blockIdx.x of utterance row / rpu
    if (threadIdx.x != 0) return;
    const int row = blockIdx.x, utt = row / rpu;
    const int T = min(max(tlen[utt], 1), Tmax);
    const float* xu = x + (long)utt * Tmax * V;
    float* rr = r + (long)row * Tmax * 2;
    float acc = 0.f;
    for (int t = 0; t < Tmax; ++t) {
        if (t < T) acc = (t == 0) ? xu[0] : acc + xu[(long)t * V];
        rr[2 * t] = LOGZERO;
        rr[2 * t + 1] = t < T ? acc : LOGZERO;
    }
}

}  // namespace

extern "C" int asr_beam_candidates(const float* att_logp, int* candidates, int rows, int V, int C, asr_stream_t stream) {
    ASR_REQUIRE(att_logp && candidates && rows > 0 && V > 1 && C > 0 && C <= V, ASR_E_ARG, "asr_beam_candidates: bad args");
    ASR_REQUIRE(V <= 64 * VPL, ASR_E_UNSUPPORTED, "asr_beam_candidates: vocabulary %d > %d", V, 64 * VPL);
    hipLaunchKernelGGL(beam_candidates_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, att_logp, candidates, V, C);
    ASR_LAUNCH_CHECK("asr_beam_candidates");
    return ASR_OK;
}

extern "C" int asr_beam_step(const asr_beam_step_t* a, asr_stream_t stream) {
    // ctcp_in / ctcp_out are read and written in every mode (0 without CTC), so they are required in every mode
    ASR_REQUIRE(a && a->att_logp && a->alive_in && a->sum_in && a->ctcp_in && a->len_in && a->seq_in && a->score_in && a->alive_out && a->sum_out && a->ctcp_out &&
                a->len_out && a->seq_out && a->score_out && a->last_token && a->parent && a->ctc_index && a->tokens && a->min_len &&
                a->max_len && a->done && a->fin_n && a->fin_len && a->fin_avg && a->fin_seq && a->fin_score, ASR_E_ARG, "asr_beam_step: null pointer");
    ASR_REQUIRE(a->U > 0 && a->beam > 0 && a->beam <= BEAM_MAX && a->V > 1 && a->V <= 64 * VPL && a->Lmax > 0 && a->t >= 0, ASR_E_ARG,
                "asr_beam_step: bad dims (beam <= %d, V <= %d)", BEAM_MAX, 64 * VPL);
    ASR_REQUIRE((a->psi == nullptr) == (a->candidates == nullptr) && (!a->candidates || a->C > 0), ASR_E_ARG,
                "asr_beam_step: CTC operands come together");
    BeamP p{a->att_logp, a->lm_logp, a->psi, a->candidates, a->alive_in, a->sum_in, a->ctcp_in, a->len_in, a->seq_in, a->score_in,
            a->alive_out, a->sum_out, a->ctcp_out, a->len_out, a->seq_out, a->score_out, a->last_token, (long long*)a->parent,
            (long long*)a->ctc_index, (long long*)a->tokens, a->tokens_ld, a->min_len, a->max_len, a->done, a->fin_n, a->fin_len, a->fin_avg,
            a->fin_seq, a->fin_score, a->U, a->beam, a->V, a->candidates ? a->C : 0, a->Lmax, a->t, a->ctc_weight, a->lm_weight, a->eos_threshold};
    hipLaunchKernelGGL(beam_step_kernel, dim3(a->U), dim3(64), 0, (hipStream_t)stream, p);
    ASR_LAUNCH_CHECK("asr_beam_step");
    return ASR_OK;
}

extern "C" int asr_beam_candidates_wide(const float* att_logp, int* candidates, int rows, int V, int C, asr_stream_t stream) {
    ASR_REQUIRE(att_logp && candidates, ASR_E_ARG, "asr_beam_candidates_wide: null pointer");
    ASR_REQUIRE(rows > 0 && V > 1 && C > 0 && C <= V && C <= WIDE_CMAX, ASR_E_ARG,
                "asr_beam_candidates_wide: bad dims rows=%d V=%d C=%d (1 <= C <= min(V, %d))", rows, V, C, WIDE_CMAX);
    ASR_REQUIRE(V <= WIDE_VMAX, ASR_E_UNSUPPORTED, "asr_beam_candidates_wide: vocabulary %d > %d", V, WIDE_VMAX);
    const int nthr = wide_threads(V);
    ASR_REQUIRE(nthr >= WAVE && nthr <= WIDE_NT, ASR_E_ARG, "asr_beam_candidates_wide: %d threads outside the kernel's launch bounds (%d)", nthr, WIDE_NT);
    hipLaunchKernelGGL(beam_candidates_wide_kernel, dim3(rows), dim3(nthr), 0, (hipStream_t)stream, att_logp, candidates, V, C);
    ASR_LAUNCH_CHECK("asr_beam_candidates_wide");
    return ASR_OK;
}

extern "C" size_t asr_beam_step_wide_workspace_bytes(int U, int beam) {
    if (U <= 0 || beam <= 0 || beam > BEAM_MAX) return 0;
    return (size_t)U * beam * sizeof(WideShort);
}

extern "C" int asr_beam_step_wide(const asr_beam_step_t* a, void* workspace, size_t workspace_bytes, asr_stream_t stream) {
    ASR_REQUIRE(a && a->att_logp && a->alive_in && a->sum_in && a->ctcp_in && a->len_in && a->seq_in && a->score_in && a->alive_out && a->sum_out && a->ctcp_out &&
                a->len_out && a->seq_out && a->score_out && a->last_token && a->parent && a->ctc_index && a->tokens && a->min_len &&
                a->max_len && a->done && a->fin_n && a->fin_len && a->fin_avg && a->fin_seq && a->fin_score && workspace, ASR_E_ARG,
                "asr_beam_step_wide: null pointer");
    ASR_REQUIRE(a->U > 0 && a->beam > 0 && a->beam <= BEAM_MAX && a->V > 1 && a->Lmax > 0 && a->t >= 0, ASR_E_ARG,
                "asr_beam_step_wide: bad dims (beam <= %d)", BEAM_MAX);
    ASR_REQUIRE(a->V <= WIDE_VMAX, ASR_E_UNSUPPORTED, "asr_beam_step_wide: vocabulary %d > %d", a->V, WIDE_VMAX);
    ASR_REQUIRE((a->psi == nullptr) == (a->candidates == nullptr) && (!a->candidates || (a->C > 0 && a->C <= WIDE_CMAX)), ASR_E_ARG,
                "asr_beam_step_wide: CTC operands come together, 1 <= C <= %d", WIDE_CMAX);
    ASR_REQUIRE(workspace_bytes >= asr_beam_step_wide_workspace_bytes(a->U, a->beam), ASR_E_ARG, "asr_beam_step_wide: workspace too small");
    const int nthr = wide_threads(a->V);
    ASR_REQUIRE(nthr >= WAVE && nthr <= WIDE_NT, ASR_E_ARG, "asr_beam_step_wide: %d threads outside the kernel's launch bounds (%d)", nthr, WIDE_NT);
    BeamP p{a->att_logp, a->lm_logp, a->psi, a->candidates, a->alive_in, a->sum_in, a->ctcp_in, a->len_in, a->seq_in, a->score_in,
            a->alive_out, a->sum_out, a->ctcp_out, a->len_out, a->seq_out, a->score_out, a->last_token, (long long*)a->parent,
            (long long*)a->ctc_index, (long long*)a->tokens, a->tokens_ld, a->min_len, a->max_len, a->done, a->fin_n, a->fin_len, a->fin_avg,
            a->fin_seq, a->fin_score, a->U, a->beam, a->V, a->candidates ? a->C : 0, a->Lmax, a->t, a->ctc_weight, a->lm_weight, a->eos_threshold};
    hipLaunchKernelGGL(beam_step_wide_rows_kernel, dim3(a->U * a->beam), dim3(nthr), 0, (hipStream_t)stream, p, (WideShort*)workspace);
    hipLaunchKernelGGL(beam_step_wide_pool_kernel, dim3(a->U), dim3(64), 0, (hipStream_t)stream, p, (const WideShort*)workspace);
    ASR_LAUNCH_CHECK("asr_beam_step_wide");
    return ASR_OK;
}

extern "C" int asr_ctc_prefix_init_batched(const float* logp, const int* tlen, float* r, int rows, int rows_per_utt, int Tmax, int V,
                                           asr_stream_t stream) {
    ASR_REQUIRE(logp && tlen && r && rows > 0 && rows_per_utt > 0 && Tmax > 0 && V > 1, ASR_E_ARG, "asr_ctc_prefix_init_batched: bad args");
    hipLaunchKernelGGL(ctc_prefix_init_batched_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, logp, tlen, r, Tmax, V, rows_per_utt);
    ASR_LAUNCH_CHECK("asr_ctc_prefix_init_batched");
    return ASR_OK;
}

extern "C" int asr_ctc_prefix_score_batched(const float* logp, const int* tlen, const float* r_prev, const int* candidates,
                                            const int* prefix_len, const int* last_token, float* psi, float* r_out,
                                            int N, int C, int Tmax, int V, int rows_per_utt, asr_stream_t stream) {
    ASR_REQUIRE(logp && tlen && r_prev && candidates && prefix_len && last_token && psi && r_out, ASR_E_ARG, "asr_ctc_prefix_score_batched: null pointer");
    ASR_REQUIRE(N > 0 && C > 0 && Tmax > 0 && V > 1 && rows_per_utt > 0, ASR_E_ARG, "asr_ctc_prefix_score_batched: bad dims");
    hipLaunchKernelGGL(ctc_prefix_score_batched_kernel, dim3(cdiv((long)N * C, 64)), dim3(64), 0, (hipStream_t)stream, logp, tlen, r_prev,
                       candidates, prefix_len, last_token, psi, r_out, N, C, Tmax, V, rows_per_utt);
    ASR_LAUNCH_CHECK("asr_ctc_prefix_score_batched");
    return ASR_OK;
}

// Scheduled sampling (reference src/asr.py:151-158): token ~ Categorical(softmax(logits)) per row, inverse-CDF with one
// Philox uniform per row (seed, row); written to out[row * out_ld] (the decoder's token table column of the next step).
namespace {
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

extern "C" int asr_sample_tokens(const float* logits, long ld, int64_t* out, long out_ld, int rows, int V, uint64_t seed, asr_stream_t stream) {
    ASR_REQUIRE(logits && out && rows > 0 && V > 1 && ld >= V, ASR_E_ARG, "asr_sample_tokens: bad args");
    hipLaunchKernelGGL(sample_tokens_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, logits, ld, (long long*)out, out_ld, V, seed);
    ASR_LAUNCH_CHECK("asr_sample_tokens");
    return ASR_OK;
}
