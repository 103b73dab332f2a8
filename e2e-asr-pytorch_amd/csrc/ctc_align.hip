// CTC forced alignment: the most probable alignment of a KNOWN transcript to the CTC posteriors (Viterbi), the fourth
// member of the CTC kernel family beside the loss (ctc.hip), the prefix scorer (ctc_prefix.hip) and the prefix beam search
// (ctc_decode.hip).  No reference counterpart: the reference never aligns.
//
// Lattice of the loss: l' = (0, y1, 0, y2, ..., yL, 0), S = 2L+1 states, blank = 0.  Max-plus recursion
//   d[t][s] = lp[t][l'_s] + max(d[t-1][s], d[t-1][s-1], d[t-1][s-2])       (s-2 only when l'_s != 0 and l'_s != l'_{s-2})
// from d[0][0], d[0][1], ending at the better of d[Tb-1][S-1] and d[Tb-1][S-2].  Ties are decided by strict `>` in a fixed
// order, so the result is deterministic: among predecessors stay, then s-1, then s-2 (the smaller move wins a tie); at the
// end S-1 wins a tie; -inf is never greater than anything, so it never wins over a finite value.
//
// ONE launch, one workgroup per utterance, one thread per state (at most 1024, the limit of asr_ctc_loss).
//   forward   : d double-buffered in LDS, ONE barrier per frame; every thread gathers the log-prob of its own label from
//               global memory a group of frames ahead (issued before the barriers of the group in flight, so the round trip
//               of a gather is off the frame chain); the move (0, 1, 2) of every (t, s) goes to the workspace as 2 bits: a
//               thread collects 16 frames in a register and stores one word.
//   back-trace: a dependent chain of Tb steps.  The moves of a chunk of frames are staged into LDS by all threads (coalesced
//               dwords), one thread walks the chunk there (an LDS round trip per frame instead of a global one) and leaves the
//               chunk's states in LDS, all threads write frame_token / frame_pos of the chunk.
//   spans     : one thread per frame marks first / last frame of its token, one thread per token sums its frames' log-probs
//               in frame order.
// Latency-bound by construction: Tb x (one barrier + one LDS round trip); the device is nearly empty (B workgroups).
#include "common.h"

namespace {

constexpr int CA_SMAX = 1024;            // states = threads of a workgroup at most
constexpr int CA_G = 4;                  // frames per group of the forward pass (even): the gathers run one group ahead
constexpr int CA_STAGE = 8 * 1024;       // words of moves staged per chunk of the back-trace (32 KiB: >= 8 blocks of 16 frames)
constexpr int CA_CHMAX = 1024;           // frames per chunk at most (the chunk's states, 2 bytes each)

struct CaP {
    const float* lp;          // (B,T,V)
    const int64_t* tgt;       // (B,L)
    const int64_t* in_len;    // (B)
    const int64_t* tgt_len;   // (B)
    int* frame_token;         // (B,T)
    int* frame_pos;           // (B,T)
    int* tok_start;           // (B,L)
    int* tok_end;             // (B,L)
    float* tok_score;         // (B,L)
    float* score;             // (B)
    int* ok;                  // (B)
    uint32_t* moves;          // workspace (B, ceil(T/16), SP): word (k, s) = the moves of state s at frames 16k .. 16k+15, 2 bits each
    int T, V, L, SP;          // SP = 2L+1
};

__host__ __device__ __forceinline__ int cdiv16(int t) { return (t + 15) >> 4; }
__device__ __forceinline__ int clamp_len(int64_t v, int hi) { return (int)(v < 0 ? 0 : (v > hi ? hi : v)); }

__global__ __launch_bounds__(CA_SMAX) void ctc_align_kernel(CaP p) {
    __shared__ float s_d[2][CA_SMAX + 2];                                   // [-2 .. S): two cells of -inf in front
    __shared__ int s_ext[CA_SMAX];                                          // l'
    __shared__ uint32_t s_mv[CA_STAGE];
    __shared__ short s_path[CA_CHMAX];
    __shared__ int s_flag, s_state;

    const int b = blockIdx.x, tid = threadIdx.x, NTH = blockDim.x;
    const int T = p.T, V = p.V, L = p.L, SP = p.SP;
    const int tl = clamp_len(p.tgt_len[b], L);
    const int Tb = clamp_len(p.in_len[b], T);
    const int S = 2 * tl + 1;
    const float* lp = p.lp + (long)b * T * V;
    int* ftok = p.frame_token + (long)b * T;
    int* fpos = p.frame_pos + (long)b * T;
    int* tstart = p.tok_start + (long)b * L;
    int* tend = p.tok_end + (long)b * L;
    float* tscore = p.tok_score + (long)b * L;

    const int s = tid;
    const bool sok = s < S;
    if (tid == 0) s_flag = 0;
    for (int i = tid; i < 2 * (CA_SMAX + 2); i += NTH) (&s_d[0][0])[i] = -INFINITY;
    __syncthreads();
    // a token outside 1..V-1 has no column to gather from (and 0 is the blank): the row is not aligned
    int e = 0;
    if (sok && (s & 1)) {
        const int64_t y = p.tgt[(long)b * L + (s >> 1)];
        if (y < 1 || y >= V) s_flag = 1;
        else e = (int)y;
    }
    s_ext[s] = e;
    __syncthreads();
    const bool bad = s_flag != 0;
    const bool skip = sok && (s & 1) && s >= 3 && e != s_ext[s - 2];
    __syncthreads();                                     // s_flag is written again below

    // ---- forward.  Frame t reads column d[(t & 1) ^ 1] and writes d[t & 1]; the column "before frame 0" holds 0 in state 0 and
    // -inf elsewhere, which makes frame 0 the general step (d[0][0] = lp, d[0][1] = lp, the rest -inf).  Frames go in groups of
    // CA_G: the gathers of the NEXT group are issued before the first barrier of this one and consumed a whole group later, so
    // no frame waits for global memory.  A thread keeps its moves of 16 frames in a register and stores the word at the start
    // of the following group (behind no wait: the store is older than the gathers that the group's end waits for).
    if (!bad && Tb > 0) {
        if (tid == 0) s_d[1][2] = 0.f;
        __syncthreads();
        uint32_t* words = p.moves + (size_t)b * cdiv16(T) * SP;
        uint32_t word = 0;
        float xc[CA_G], xn[CA_G];
#pragma unroll
        for (int k = 0; k < CA_G; ++k) xc[k] = (sok && k < Tb) ? lp[(long)k * V + e] : 0.f;
        for (int t0 = 0; t0 < Tb; t0 += CA_G) {
            if ((t0 & 15) == 0 && t0 > 0) {
                if (sok) words[(size_t)((t0 >> 4) - 1) * SP + s] = word;
                word = 0;
            }
#pragma unroll
            for (int k = 0; k < CA_G; ++k) xn[k] = (sok && t0 + CA_G + k < Tb) ? lp[(long)(t0 + CA_G + k) * V + e] : 0.f;
#pragma unroll
            for (int k = 0; k < CA_G; ++k) {
                const int t = t0 + k;
                if (t >= Tb) break;                          // the same in every thread
                const float* prev = &s_d[(k & 1) ^ 1][2];    // CA_G is even: the parity of t is the parity of k
                float* cur = &s_d[k & 1][2];
                if (sok) {
                    float best = prev[s];
                    uint32_t mv = 0;
                    const float b1 = prev[s - 1];
                    if (b1 > best) { best = b1; mv = 1; }
                    if (skip) {
                        const float b2 = prev[s - 2];
                        if (b2 > best) { best = b2; mv = 2; }
                    }
                    cur[s] = best + xc[k];
                    word |= mv << (2 * (t & 15));
                }
                __syncthreads();
            }
#pragma unroll
            for (int k = 0; k < CA_G; ++k) xc[k] = xn[k];
        }
        if (sok) words[(size_t)((Tb - 1) >> 4) * SP + s] = word;
    }
    const float* last = &s_d[(Tb - 1) & 1][2];
    if (tid == 0) {
        float sc = -INFINITY;
        int se = S - 1;
        if (!bad && Tb > 0) {
            sc = last[S - 1];
            const float v2 = S > 1 ? last[S - 2] : -INFINITY;
            if (v2 > sc) { sc = v2; se = S - 2; }
        } else if (!bad && tl == 0) {
            sc = 0.f;                                    // no frames, empty target: the empty alignment
        }
        const int okv = sc > -INFINITY ? 1 : 0;
        p.score[b] = okv ? sc : -INFINITY;
        p.ok[b] = okv;
        s_flag = okv;
        s_state = se;
    }
    __syncthreads();
    const bool ok = s_flag != 0;

    // ---- everything outside the alignment
    for (int t = tid + (ok ? Tb : 0); t < T; t += NTH) { ftok[t] = -1; fpos[t] = -1; }
    for (int j = tid + (ok ? tl : 0); j < L; j += NTH) { tstart[j] = -1; tend[j] = -1; tscore[j] = 0.f; }
    if (!ok) return;

    // ---- back-trace, a chunk of 16-frame blocks at a time, last chunk first
    const uint32_t* words = p.moves + (size_t)b * cdiv16(T) * SP;
    const int NB = min(CA_CHMAX / 16, CA_STAGE / SP);    // blocks per chunk
    for (int b1 = cdiv16(Tb); b1 > 0; b1 -= NB) {
        const int b0 = max(0, b1 - NB), c0 = 16 * b0, n = min(Tb, 16 * b1) - c0;
        const uint32_t* src = words + (size_t)b0 * SP;
        for (int i = tid; i < (b1 - b0) * SP; i += NTH) s_mv[i] = src[i];
        __syncthreads();
        if (tid == 0) {
            int st = s_state;
            for (int i = n - 1; i >= 0; --i) {
                s_path[i] = (short)st;
                st = max(0, st - (int)((s_mv[(i >> 4) * SP + st] >> (2 * (i & 15))) & 3u));
            }
            s_state = st;
        }
        __syncthreads();
        for (int i = tid; i < n; i += NTH) {
            const int st = s_path[i];
            ftok[c0 + i] = s_ext[st];
            fpos[c0 + i] = (st & 1) ? (st >> 1) : -1;
        }
    }
    __syncthreads();                                     // the path is in global memory, visible to the workgroup

    // ---- spans and per-token scores from the finished path
    for (int t = tid; t < Tb; t += NTH) {
        const int pos = fpos[t];
        if (pos < 0) continue;
        if (t == 0 || fpos[t - 1] != pos) tstart[pos] = t;
        if (t == Tb - 1 || fpos[t + 1] != pos) tend[pos] = t;
    }
    __syncthreads();
    for (int j = tid; j < tl; j += NTH) {
        const int y = s_ext[2 * j + 1], t0 = tstart[j], t1 = tend[j];
        float sum = 0.f;
        for (int t = t0; t <= t1; ++t) sum += lp[(long)t * V + y];
        tscore[j] = sum;
    }
}

}  // namespace

extern "C" size_t asr_ctc_align_workspace_bytes(int B, int T, int L) {
    if (B <= 0 || T <= 0 || L < 0) return 0;
    return (size_t)B * cdiv16(T) * (2 * (size_t)L + 1) * sizeof(uint32_t);
}

extern "C" int asr_ctc_align(const float* logp, const int64_t* targets, const int64_t* input_len, const int64_t* target_len,
                             int B, int T, int V, int L, int* frame_token, int* frame_pos, int* tok_start, int* tok_end,
                             float* tok_score, float* score, int* ok, void* workspace, size_t workspace_bytes, asr_stream_t stream) {
    ASR_REQUIRE(logp && input_len && target_len && frame_token && frame_pos && score && ok && workspace, ASR_E_ARG,
                "asr_ctc_align: null pointer");
    ASR_REQUIRE(B > 0 && T > 0 && V > 1 && L >= 0, ASR_E_ARG, "asr_ctc_align: bad dims B=%d T=%d V=%d L=%d", B, T, V, L);
    ASR_REQUIRE(L == 0 || (targets && tok_start && tok_end && tok_score), ASR_E_ARG, "asr_ctc_align: null pointer");
    ASR_REQUIRE(2 * (long)L + 1 <= CA_SMAX, ASR_E_UNSUPPORTED, "asr_ctc_align: 2L+1=%ld states exceed one workgroup (%d)",
                2 * (long)L + 1, CA_SMAX);
    ASR_REQUIRE(workspace_bytes >= asr_ctc_align_workspace_bytes(B, T, L), ASR_E_ARG, "asr_ctc_align: workspace too small");
    ASR_REQUIRE(((uintptr_t)workspace & 3) == 0, ASR_E_ARG, "asr_ctc_align: workspace is not 4-byte aligned");
    CaP p{logp, targets, input_len, target_len, frame_token, frame_pos, tok_start, tok_end, tok_score, score, ok,
          (uint32_t*)workspace, T, V, L, 2 * L + 1};
    const int nthr = WAVE * cdiv(2 * L + 1, WAVE);
    hipLaunchKernelGGL(ctc_align_kernel, dim3(B), dim3(nthr), 0, (hipStream_t)stream, p);
    ASR_LAUNCH_CHECK("asr_ctc_align");
    return ASR_OK;
}
