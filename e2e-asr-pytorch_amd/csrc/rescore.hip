// Two-pass decoding of a joint CTC/attention model: the n-best list of the CTC prefix beam search (ctc_decode.hip) is scored by
// the attention decoder, teacher-forced in one batched pass (the decoder kernels, unchanged), and re-ranked.  The two kernels
// here are what that needs around the decoder pass; the reference has no counterpart (its only mode is the joint search of
// src/decode.py:65-183).  Row r = u*K + i is beam slot i of utterance u.
//
// asr_rescore_pack: the first pass's (tokens, len, n) -> the teacher table of the decoder pass, the per-row lengths and the
// indices that expand the encoder output to one row per hypothesis.  One workgroup per utterance; the largest tgt_len (the
// decoder's step count, the one value the host reads before the pass) is found by workgroup 0 from len and n alone, so no
// workgroup waits for another and nothing has to be cleared beforehand.
//
// asr_rescore_nbest: per hypothesis sum_t log_softmax(logits[r,t,:])[teacher[r,t]], mixed with the first pass's scores and
// ranked.  One workgroup per utterance, wave i walks hypothesis i over t: lanes stride over V, one max and one sum reduction
// per position (RS_UNROLL positions in flight together - the chain per position is load, 6 shuffles, exp, 6 shuffles, log, and
// at V = 31 a position is a single load per lane), the log-probabilities added in order of t.  A hypothesis is one wave's work
// whatever K, U and the grid are, so its score does not depend on them.  The rank is a count over the K totals in LDS.  The
// work is the read of the logit block, K*L*V*4 bytes per utterance - small next to the decoder pass that wrote it.
#include <algorithm>
#include "common.h"

namespace {

constexpr int RS_KMAX = ASR_CTC_BEAM_MAX;
constexpr int RS_PACK_NT = 256;
constexpr int RS_UNROLL = 4;

struct RsPackP {
    const int* tokens;          // (U,K,Lcap)
    const int* len;             // (U,K)
    const int* n;               // (U)
    const long long* enc_len;   // (U)
    long long* teacher;         // (R,Lr)
    int* tgt_len;               // (R)
    long long* row_utt;         // (R)
    long long* row_enc_len;     // (R)
    int* max_len;               // (1)
    int U, K, Lcap, Lr, eos;
};

// tokens to score of slot i of utterance u (0: unused slot); hyp_len = the tokens of the hypothesis itself
__device__ __forceinline__ int rs_tgt_len(const RsPackP& p, int u, int i, int& hyp_len) {
    hyp_len = 0;
    if (i >= p.n[u]) return 0;
    const long r = (long)u * p.K + i;
    const int l = max(0, min(p.len[r], p.Lcap));
    hyp_len = l;
    const int last = l > 0 ? p.tokens[r * p.Lcap + l - 1] : -1;
    return l + (last != p.eos ? 1 : 0);
}

__global__ __launch_bounds__(RS_PACK_NT) void rescore_pack_kernel(RsPackP p) {
    __shared__ int s_len[RS_KMAX], s_tgt[RS_KMAX];
    __shared__ int red[RS_PACK_NT / WAVE];
    const int u = blockIdx.x, tid = threadIdx.x, K = p.K;
    if (tid < K) {
        int l;
        const int tg = rs_tgt_len(p, u, tid, l);
        const long r = (long)u * K + tid;
        s_len[tid] = l; s_tgt[tid] = tg;
        p.tgt_len[r] = tg;
        p.row_utt[r] = u;
        p.row_enc_len[r] = p.enc_len[u];
    }
    if (u == 0) {                                   // uniform in the workgroup
        int m = 0;
        for (long r = tid; r < (long)p.U * K; r += RS_PACK_NT) {
            int l;
            m = max(m, rs_tgt_len(p, (int)(r / K), (int)(r % K), l));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
        if ((tid & 63) == 0) red[tid >> 6] = m;
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < RS_PACK_NT / WAVE; ++k) m = max(m, red[k]);
            p.max_len[0] = m;
        }
    }
    __syncthreads();
    const int Lr = p.Lr;
    const int* tok_u = p.tokens + (long)u * K * p.Lcap;
    long long* tea_u = p.teacher + (long)u * K * Lr;
    for (long idx = tid; idx < (long)K * Lr; idx += RS_PACK_NT) {
        const int i = (int)(idx / Lr), t = (int)(idx - (long)i * Lr);
        long long v = 0;
        if (t < s_len[i]) v = tok_u[(long)i * p.Lcap + t];
        else if (t < s_tgt[i]) v = p.eos;
        tea_u[idx] = v;
    }
}

struct RsP {
    const float* logits;
    long row_stride, pos_stride;
    const long long* teacher;
    long teacher_ld;
    const int* tgt_len;
    const float* ctc;
    const float* first;
    const int* n;
    float* att;
    float* total;
    int* order;
    int K, L, V;
    float w;
};

// sum over t < tl of log_softmax(base[t*pos_stride + .])[teach[t]] by ONE wave, the same value in every lane.  A block of
// RS_UNROLL positions is reduced together; behind the last position the block re-reads position tl - 1 (never one at or past
// tl) and drops the result.
__device__ __forceinline__ float rs_hyp_score(const float* base, long pos_stride, const long long* teach, int tl, int V) {
    const int lane = threadIdx.x & 63;
    float att = 0.f;
    for (int t0 = 0; t0 < tl; t0 += RS_UNROLL) {
        const float* row[RS_UNROLL];
        float m[RS_UNROLL], s[RS_UNROLL];
#pragma unroll
        for (int j = 0; j < RS_UNROLL; ++j) {
            row[j] = base + (long)min(t0 + j, tl - 1) * pos_stride;
            m[j] = -INFINITY; s[j] = 0.f;
        }
        for (int c = lane; c < V; c += WAVE) {
#pragma unroll
            for (int j = 0; j < RS_UNROLL; ++j) m[j] = fmaxf(m[j], row[j][c]);
        }
#pragma unroll
        for (int j = 0; j < RS_UNROLL; ++j) {
            m[j] = wave_max(m[j]);
            if (m[j] == -INFINITY) m[j] = 0.f;      // a position with every logit at -inf: the sum below is 0, its log -inf
        }
        for (int c = lane; c < V; c += WAVE) {
#pragma unroll
            for (int j = 0; j < RS_UNROLL; ++j) s[j] += expf(row[j][c] - m[j]);
        }
#pragma unroll
        for (int j = 0; j < RS_UNROLL; ++j) s[j] = wave_sum(s[j]);
#pragma unroll
        for (int j = 0; j < RS_UNROLL; ++j) {
            if (t0 + j < tl) {
                const long long tok = teach[t0 + j];
                const float x = (tok >= 0 && tok < V) ? row[j][tok] : -INFINITY;
                att += x == -INFINITY ? -INFINITY : (x - m[j]) - logf(s[j]);
            }
        }
    }
    return att;
}

__global__ __launch_bounds__(RS_KMAX * WAVE) void rescore_nbest_kernel(RsP p) {
    __shared__ float s_total[RS_KMAX];
    const int u = blockIdx.x, tid = threadIdx.x, K = p.K;
    const int i = tid >> 6;                         // blockDim.x = K * WAVE: wave i scores slot i
    const long r = (long)u * K + i;
    float att = -INFINITY, tot = -INFINITY;
    if (i < p.n[u]) {
        const int tl = max(0, min(p.tgt_len[r], p.L));
        att = rs_hyp_score(p.logits + r * p.row_stride, p.pos_stride, p.teacher + r * p.teacher_ld, tl, p.V);
        // a hypothesis with an impossible token stays impossible whatever the weights (0 * -inf would be NaN at ctc_weight = 1)
        if (att > -INFINITY) tot = (1.f - p.w) * att + p.w * p.ctc[r] + (p.first[r] - p.ctc[r]);
    }
    if ((tid & 63) == 0) {
        p.att[r] = att; p.total[r] = tot;
        s_total[i] = tot;
    }
    __syncthreads();
    if (tid < K) {                                  // rank of slot tid: the slots ahead of it, ties to the lower slot
        const float mine = s_total[tid];
        int rank = 0;
        for (int j = 0; j < K; ++j) {
            const float o = s_total[j];
            rank += (o > mine || (o == mine && j < tid)) ? 1 : 0;
        }
        p.order[(long)u * K + rank] = tid;
    }
}

}  // namespace

extern "C" int asr_rescore_pack(const int* tokens, const int* len, const int* n, const int64_t* enc_len, int U, int K, int Lcap, int Lr,
                                int eos, int64_t* teacher, int* tgt_len, int64_t* row_utt, int64_t* row_enc_len, int* max_len,
                                asr_stream_t stream) {
    ASR_REQUIRE(tokens && len && n && enc_len && teacher && tgt_len && row_utt && row_enc_len && max_len, ASR_E_ARG,
                "asr_rescore_pack: null pointer");
    ASR_REQUIRE(U > 0 && Lcap > 0 && eos >= 0, ASR_E_ARG, "asr_rescore_pack: bad dims U=%d Lcap=%d eos=%d", U, Lcap, eos);
    ASR_REQUIRE(K >= 1 && K <= RS_KMAX, ASR_E_ARG, "asr_rescore_pack: beam %d outside 1..%d", K, RS_KMAX);
    ASR_REQUIRE(Lr >= Lcap + 1, ASR_E_ARG, "asr_rescore_pack: Lr=%d below Lcap+1=%d (a hypothesis of Lcap tokens and its <eos>)", Lr, Lcap + 1);
    RsPackP p{tokens, len, n, (const long long*)enc_len, (long long*)teacher, tgt_len, (long long*)row_utt, (long long*)row_enc_len,
              max_len, U, K, Lcap, Lr, eos};
    hipLaunchKernelGGL(rescore_pack_kernel, dim3(U), dim3(RS_PACK_NT), 0, (hipStream_t)stream, p);
    ASR_LAUNCH_CHECK("asr_rescore_pack");
    return ASR_OK;
}

extern "C" int asr_rescore_nbest(const float* logits, long row_stride, long pos_stride, const int64_t* teacher, long teacher_ld,
                                 const int* tgt_len, const float* ctc_score, const float* first_score, const int* n, int U, int K,
                                 int L, int V, float ctc_weight, float* att_score, float* total, int* order, asr_stream_t stream) {
    ASR_REQUIRE(logits && teacher && tgt_len && ctc_score && first_score && n && att_score && total && order, ASR_E_ARG,
                "asr_rescore_nbest: null pointer");
    ASR_REQUIRE(U > 0 && L >= 1 && V > 1, ASR_E_ARG, "asr_rescore_nbest: bad dims U=%d L=%d V=%d", U, L, V);
    ASR_REQUIRE(K >= 1 && K <= RS_KMAX, ASR_E_ARG, "asr_rescore_nbest: beam %d outside 1..%d", K, RS_KMAX);
    ASR_REQUIRE(row_stride >= V && pos_stride >= V, ASR_E_ARG, "asr_rescore_nbest: stride below V=%d (row %ld, position %ld)", V,
                row_stride, pos_stride);
    ASR_REQUIRE(teacher_ld >= L, ASR_E_ARG, "asr_rescore_nbest: teacher_ld=%ld below L=%d", teacher_ld, L);
    RsP p{logits, row_stride, pos_stride, (const long long*)teacher, teacher_ld, tgt_len, ctc_score, first_score, n, att_score, total,
          order, K, L, V, ctc_weight};
    hipLaunchKernelGGL(rescore_nbest_kernel, dim3(U), dim3(K * WAVE), 0, (hipStream_t)stream, p);
    ASR_LAUNCH_CHECK("asr_rescore_nbest");
    return ASR_OK;
}

// ---- the RNN-LM in the second pass ---------------------------------------------------------------------------------------------
// The LM scores the same n-best list teacher-forced: asr_rescore_lm_input shifts the teacher table into the LM's input, the LM's
// full-sequence forward writes logits (R,L,V), asr_rescore_token_logp reduces every (row, position) to the log-probability of its
// target, asr_rescore_rank_lm sums them per hypothesis, mixes and ranks.  V goes up to 65 536 here, so a position is one wave's
// work (not a hypothesis, as above) and the grid covers R*L positions: the launch is bound by ONE read of the logit block.  A wave
// takes its row in blocks of TL_BLOCK_V columns that sit in registers (TL_REG per lane) between the block's max and its sum, and
// carries a running max m and the sum s of exp(x - m) from block to block: a block whose max exceeds m scales s by exp(m - max)
// first.  So no logit is loaded twice, whatever the caches hold - swept twice, a row of V = 65 536 came from HBM twice: every wave
// resident on an XCD holds another 256 KiB row and the 4 MiB L2 keeps none of them (measured).  Up to TL_BLOCK_V
// columns there is one block and no scaling: max, then sum, as in rs_hyp_score.  m is uniform in the wave and lane c adds the
// columns c, c + 64, .. in ascending order, so a value depends on the row alone, not on R, on the chunk or on the grid.
namespace {

constexpr int TL_WAVES = 4;                         // positions per workgroup
constexpr int TL_REG = 16;                          // logits of a block a lane holds
constexpr int TL_BLOCK_V = TL_REG * WAVE;           // 1024 columns per block
constexpr int LMIN_NT = 256;

// the per-position arithmetic of rs_hyp_score, for a single position
__device__ __forceinline__ float tl_logp(float x, float m, float s) { return x == -INFINITY ? -INFINITY : (x - m) - logf(s); }

struct TlP {
    const float* logits;
    long row_stride, pos_stride;
    const long long* target;
    long target_ld;
    const int* len;
    float* out;
    long out_ld;
    long R;
    int L, V;
};

__global__ __launch_bounds__(TL_WAVES * WAVE) void rescore_token_logp_kernel(TlP p) {
    const int lane = threadIdx.x & 63;
    const long pos = (long)blockIdx.x * TL_WAVES + (threadIdx.x >> 6);          // uniform in the wave
    if (pos >= p.R * p.L) return;
    const long r = pos / p.L;
    const int t = (int)(pos - r * p.L), V = p.V;
    float* dst = p.out + r * p.out_ld + t;
    if (t >= max(0, min(p.len[r], p.L))) {          // behind the hypothesis: nothing is read
        if (lane == 0) *dst = 0.f;
        return;
    }
    const float* row = p.logits + r * p.row_stride + (long)t * p.pos_stride;
    float m = -INFINITY, s = 0.f;                   // m: the max so far, uniform in the wave; s: this lane's sum of exp(x - m)
    for (int c0 = 0; c0 < V; c0 += TL_BLOCK_V) {
        float x[TL_REG];
#pragma unroll
        for (int j = 0; j < TL_REG; ++j) {          // every load unconditional, from a clamped column
            const int c = c0 + lane + j * WAVE;
            const float v = row[min(c, V - 1)];
            x[j] = c < V ? v : -INFINITY;
        }
        float bm = -INFINITY;
#pragma unroll
        for (int j = 0; j < TL_REG; ++j) bm = fmaxf(bm, x[j]);
        bm = wave_max(bm);
        if (bm > m) {                               // uniform; from m = -inf: s = 0 stays 0
            s *= expf(m - bm);
            m = bm;
        }
        const float mm = m == -INFINITY ? 0.f : m;  // every logit so far at -inf: the terms below are exp(-inf) = 0
#pragma unroll
        for (int j = 0; j < TL_REG; ++j) s += expf(x[j] - mm);                  // 0 behind V
    }
    if (m == -INFINITY) m = 0.f;                    // every logit at -inf: the sum is 0, its log -inf
    s = wave_sum(s);
    if (lane == 0) {
        const long long tok = p.target[r * p.target_ld + t];
        const float x = (tok >= 0 && tok < V) ? row[tok] : -INFINITY;
        *dst = tl_logp(x, m, s);
    }
}

__global__ __launch_bounds__(LMIN_NT) void rescore_lm_input_kernel(const long long* teacher, long teacher_ld, long R, int L, long long sos,
                                                                   long long* lm_in) {
    const long total = R * L;
    for (long idx = (long)blockIdx.x * LMIN_NT + threadIdx.x; idx < total; idx += (long)gridDim.x * LMIN_NT) {
        const long r = idx / L;
        const int t = (int)(idx - r * L);
        lm_in[idx] = t == 0 ? sos : teacher[r * teacher_ld + t - 1];
    }
}

struct RkP {
    const float* att;
    const float* ctc;
    const float* tok_logp;
    long tok_ld;
    const int* len;
    const int* n;
    float* lm_score;
    float* total;
    int* order;
    int K, L;
    float w, lm_w, bonus;
};

__global__ __launch_bounds__(RS_KMAX * WAVE) void rescore_rank_lm_kernel(RkP p) {
    __shared__ float s_total[RS_KMAX];
    const int u = blockIdx.x, tid = threadIdx.x, K = p.K, lane = tid & 63;
    const int i = tid >> 6;                         // blockDim.x = K * WAVE: wave i sums slot i
    const long r = (long)u * K + i;
    float lm = -INFINITY, tot = -INFINITY;
    if (i < p.n[u]) {
        const int nl = max(0, min(p.len[r], p.L));
        const float* tl = p.tok_logp + r * p.tok_ld;
        float a = 0.f;
        for (int t = lane; t < nl; t += WAVE) a += tl[t];                        // lane c: positions c, c + 64, .. in order, then the butterfly
        lm = wave_sum(a);
        const float att = p.att[r], ctc = p.ctc[r];
        // an impossible hypothesis stays impossible whatever the weights (0 * -inf would be NaN); lm_weight = 0 leaves the LM out
        if (att > -INFINITY && ctc > -INFINITY && (p.lm_w == 0.f || lm > -INFINITY)) {
            tot = (1.f - p.w) * att + p.w * ctc;
            if (p.lm_w != 0.f) tot += p.lm_w * lm;
            tot += p.bonus * (float)nl;
        }
    }
    if (lane == 0) {
        p.lm_score[r] = lm; p.total[r] = tot;
        s_total[i] = tot;
    }
    __syncthreads();
    if (tid < K) {                                  // rank of slot tid: the slots ahead of it, ties to the lower slot
        const float mine = s_total[tid];
        int rank = 0;
        for (int j = 0; j < K; ++j) {
            const float o = s_total[j];
            rank += (o > mine || (o == mine && j < tid)) ? 1 : 0;
        }
        p.order[(long)u * K + rank] = tid;
    }
}

}  // namespace

extern "C" int asr_rescore_lm_input(const int64_t* teacher, long teacher_ld, int R, int L, int64_t sos, int64_t* lm_in,
                                    asr_stream_t stream) {
    ASR_REQUIRE(teacher && lm_in, ASR_E_ARG, "asr_rescore_lm_input: null pointer");
    ASR_REQUIRE(R > 0 && L >= 1 && sos >= 0, ASR_E_ARG, "asr_rescore_lm_input: bad dims R=%d L=%d sos=%ld", R, L, (long)sos);
    ASR_REQUIRE(teacher_ld >= L, ASR_E_ARG, "asr_rescore_lm_input: teacher_ld=%ld below L=%d", teacher_ld, L);
    const int grid = (int)std::min<long>(2048, ((long)R * L + LMIN_NT - 1) / LMIN_NT);
    hipLaunchKernelGGL(rescore_lm_input_kernel, dim3(grid), dim3(LMIN_NT), 0, (hipStream_t)stream, (const long long*)teacher, teacher_ld,
                       (long)R, L, (long long)sos, (long long*)lm_in);
    ASR_LAUNCH_CHECK("asr_rescore_lm_input");
    return ASR_OK;
}

extern "C" int asr_rescore_token_logp(const float* logits, long row_stride, long pos_stride, const int64_t* target, long target_ld,
                                      const int* len, int R, int L, int V, float* out, long out_ld, asr_stream_t stream) {
    ASR_REQUIRE(logits && target && len && out, ASR_E_ARG, "asr_rescore_token_logp: null pointer");
    ASR_REQUIRE(R > 0 && L >= 1 && V > 1 && V <= (1 << 30), ASR_E_ARG, "asr_rescore_token_logp: bad dims R=%d L=%d V=%d", R, L, V);
    const long blocks = ((long)R * L + TL_WAVES - 1) / TL_WAVES;
    ASR_REQUIRE(blocks <= 0x7fffffffL, ASR_E_ARG, "asr_rescore_token_logp: R*L=%ld positions exceed one grid", (long)R * L);
    ASR_REQUIRE(pos_stride >= V && row_stride >= V, ASR_E_ARG, "asr_rescore_token_logp: stride below V=%d (row %ld, position %ld)", V,
                row_stride, pos_stride);
    ASR_REQUIRE(target_ld >= L && out_ld >= L, ASR_E_ARG, "asr_rescore_token_logp: target_ld=%ld or out_ld=%ld below L=%d", target_ld,
                out_ld, L);
    TlP p{logits, row_stride, pos_stride, (const long long*)target, target_ld, len, out, out_ld, R, L, V};
    hipLaunchKernelGGL(rescore_token_logp_kernel, dim3((unsigned)blocks), dim3(TL_WAVES * WAVE), 0,
                       (hipStream_t)stream, p);
    ASR_LAUNCH_CHECK("asr_rescore_token_logp");
    return ASR_OK;
}

extern "C" int asr_rescore_rank_lm(const float* att_score, const float* ctc_score, const float* tok_logp, long tok_ld, const int* len,
                                   const int* n, int U, int K, int L, float ctc_weight, float lm_weight, float len_bonus,
                                   float* lm_score, float* total, int* order, asr_stream_t stream) {
    ASR_REQUIRE(att_score && ctc_score && tok_logp && len && n && lm_score && total && order, ASR_E_ARG,
                "asr_rescore_rank_lm: null pointer");
    ASR_REQUIRE(U > 0 && L >= 1, ASR_E_ARG, "asr_rescore_rank_lm: bad dims U=%d L=%d", U, L);
    ASR_REQUIRE(K >= 1 && K <= RS_KMAX, ASR_E_ARG, "asr_rescore_rank_lm: beam %d outside 1..%d", K, RS_KMAX);
    ASR_REQUIRE(tok_ld >= L, ASR_E_ARG, "asr_rescore_rank_lm: tok_ld=%ld below L=%d", tok_ld, L);
    ASR_REQUIRE(lm_weight >= 0.f, ASR_E_ARG, "asr_rescore_rank_lm: lm_weight %g below 0", (double)lm_weight);
    RkP p{att_score, ctc_score, tok_logp, tok_ld, len, n, lm_score, total, order, K, L, ctc_weight, lm_weight, len_bonus};
    hipLaunchKernelGGL(rescore_rank_lm_kernel, dim3(U), dim3(K * WAVE), 0, (hipStream_t)stream, p);
    ASR_LAUNCH_CHECK("asr_rescore_rank_lm");
    return ASR_OK;
}
