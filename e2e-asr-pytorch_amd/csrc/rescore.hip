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
