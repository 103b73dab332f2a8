// CTC prefix beam search of a CTC-only model (ctc_weight = 1, no attention decoder) - stands in for the reference's
// missing decoder (`# ToDo : implement pure ctc decode`, src/decode.py:26) behind the BeamDecoder.forward contract.
//
// ONE launch for all utterances and all frames: workgroup u runs the whole frame loop of utterance u, the beam (at most
// K <= ASR_CTC_BEAM_MAX prefixes: pb, pnb, last token, length, trie node, parent node) stays in LDS, double buffered.
// Blank = 0 as in ctc.hip.  Frame t, beam slot i with last token e and p = pb (+) pnb:
//   stay    l    : pb' (+)= p + lp[t,0];  pnb' (+)= pnb + lp[t,e] when l is not empty
//   extend  l+c  : pnb' (+)= (pb if c == e else p) + lp[t,c]     for every allowed token c != 0
// An extension that is a beam member itself (same parent node, same token) goes into that member's entry with the
// member's stay terms, never into an entry of its own.  Allowed tokens: all (cand = 0) or the `cand` largest lp[t,.] of
// the frame, ties to the lower index, found as a threshold by `cand` workgroup arg-max rounds.  The K best entries by
// pb' (+) pnb' survive, found by K workgroup arg-max rounds over the K stay entries and the K x allowed extensions
// (nothing is materialised: a round re-derives each thread's candidates, one add each); ties go to the smaller
// (parent slot, token) with a stay entry counting as (slot, 0); entries at -inf are never kept, so an empty slot never
// survives.  The survivors' order is the slot order of the next frame and the rank order of the result.
//
// Prefix trie in the workspace, per utterance 1 + K*Tmax nodes of four ints (parent, token, first child, next sibling).
// A prefix has exactly one node: a survivor that is new looks its (parent, token) up in the parent's child list (all
// survivors in parallel) and only if it is not there one thread appends it - at most K per frame - so "same parent node
// and same token" is the same prefix however often a prefix left the beam and came back.
#include <limits.h>
#include <algorithm>
#include "common.h"

namespace {

constexpr int CB_KMAX = ASR_CTC_BEAM_MAX;
constexpr int CB_NT = 256;           // largest workgroup: __launch_bounds__ of the kernel, checked on the host
constexpr int CB_NW = CB_NT / WAVE;

struct CbP {
    const float* lp;       // (U,Tmax,V)
    const int* tlen;       // (U)
    int* trie;             // (U, 1 + K*Tmax, 4)
    int* out_tok;          // (U,K,Lcap)
    int* out_len;          // (U,K)
    float* out_score;      // (U,K)
    int* out_n;            // (U)
    int Tmax, V, K, cand, Lcap;
};

struct Best { float s; long long id; };

// total order of the candidates: larger score first, then smaller id
__device__ __forceinline__ bool better(float s1, long long i1, float s2, long long i2) { return s1 > s2 || (s1 == s2 && i1 < i2); }
// strictly behind the pick (ps, pid) of the previous round in that order
__device__ __forceinline__ bool behind(float s, long long id, float ps, long long pid) { return s < ps || (s == ps && id > pid); }

// the workgroup's best candidate, in every thread; `red` holds two rows of per-wave results used in turn (`round` counts
// every call of the launch), so one barrier per call is enough
__device__ __forceinline__ Best wg_best(Best b, Best* red, int round) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float s2 = __shfl_xor(b.s, o);
        const long long i2 = __shfl_xor(b.id, o);
        if (better(s2, i2, b.s, b.id)) { b.s = s2; b.id = i2; }
    }
    const int nw = blockDim.x >> 6;
    Best* r = red + (round & 1) * CB_NW;
    if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = b;
    __syncthreads();
    Best w = r[0];
    for (int k = 1; k < nw; ++k)
        if (better(r[k].s, r[k].id, w.s, w.id)) w = r[k];
    return w;
}

__global__ __launch_bounds__(CB_NT) void ctc_beam_kernel(CbP p) {
    __shared__ float s_pb[2][CB_KMAX], s_pnb[2][CB_KMAX];
    __shared__ int s_tok[2][CB_KMAX], s_len[2][CB_KMAX], s_node[2][CB_KMAX], s_par[2][CB_KMAX];
    __shared__ float s_p[CB_KMAX], s_spb[CB_KMAX], s_spnb[CB_KMAX], s_stot[CB_KMAX];   // p of a slot; its stay entry
    __shared__ int s_ms[CB_KMAX];                 // slot of the beam member that is this member's parent prefix, or -1
    __shared__ float s_sel_s[CB_KMAX];
    __shared__ long long s_sel_id[CB_KMAX];
    __shared__ Best s_red[2 * CB_NW];
    __shared__ int s_nnodes;

    const int u = blockIdx.x, tid = threadIdx.x, NTH = blockDim.x;
    const int V = p.V, K = p.K;
    const int T = max(0, min(p.tlen[u], p.Tmax));
    const float* lpu = p.lp + (long)u * p.Tmax * V;
    int* trie = p.trie + (long)u * (1 + (long)K * p.Tmax) * 4;
    const bool prune = p.cand > 0 && p.cand < V - 1;

    if (tid < CB_KMAX) {
        s_pb[0][tid] = tid == 0 ? 0.f : -INFINITY;
        s_pnb[0][tid] = -INFINITY;
        s_tok[0][tid] = 0; s_len[0][tid] = 0; s_node[0][tid] = 0; s_par[0][tid] = -1;
    }
    if (tid == 0) {
        trie[0] = -1; trie[1] = 0; trie[2] = -1; trie[3] = -1;       // root = the empty prefix
        s_nnodes = 1;
    }
    int nlive = 1, cur = 0, round = 0;
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const float* row = lpu + (long)t * V;
        // the arg-max rounds below walk this thread's tokens again and again: its first token's log-prob (its only one while
        // V - 1 <= blockDim.x) is read once per frame, not once per round
        const int c0 = 1 + tid;
        const float l0 = c0 < V ? row[c0] : -INFINITY;
        // ---- allowed tokens: (lp, index) of the cand-th largest non-blank log-prob of the frame
        float thv = -INFINITY;
        int thi = INT_MAX;
        if (prune) {
            float pv = INFINITY;
            long long pi = -1;
            for (int r = 0; r < p.cand; ++r) {
                Best b{-INFINITY, LLONG_MAX};
                for (int c = c0; c < V; c += NTH) {
                    const float l = c == c0 ? l0 : row[c];
                    if (behind(l, c, pv, pi) && better(l, c, b.s, b.id)) { b.s = l; b.id = c; }
                }
                const Best w = wg_best(b, s_red, round++);
                pv = w.s; pi = w.id;
            }
            thv = pv;
            thi = (int)min(pi, (long long)INT_MAX);
        }
#define CB_ALLOWED(c, l) ((l) > thv || ((l) == thv && (c) <= thi))
        // ---- stay entries
        if (tid < nlive) s_p[tid] = logaddexpf_(s_pb[cur][tid], s_pnb[cur][tid]);
        __syncthreads();
        if (tid < nlive) {
            const int j = tid, tj = s_tok[cur][j];
            int ms = -1;
            if (s_len[cur][j] > 0)
                for (int i = 0; i < nlive; ++i)
                    if (s_node[cur][i] == s_par[cur][j]) ms = i;
            const float lj = row[tj];
            const float spb = s_p[j] + row[0];
            float spnb = s_len[cur][j] > 0 ? s_pnb[cur][j] + lj : -INFINITY;
            if (ms >= 0 && CB_ALLOWED(tj, lj))
                spnb = logaddexpf_(spnb, (tj == s_tok[cur][ms] ? s_pb[cur][ms] : s_p[ms]) + lj);
            s_ms[j] = ms;
            s_spb[j] = spb; s_spnb[j] = spnb; s_stot[j] = logaddexpf_(spb, spnb);
        }
        __syncthreads();
        // ---- the K best entries, one per round
        float ps = INFINITY;
        long long pid = -1;
        int nsel = 0;
        for (int r = 0; r < K; ++r) {
            Best b{-INFINITY, LLONG_MAX};
            if (tid < nlive) {
                const float s = s_stot[tid];
                const long long id = (long long)tid * V;
                if (behind(s, id, ps, pid) && better(s, id, b.s, b.id)) { b.s = s; b.id = id; }
            }
            for (int c = c0; c < V; c += NTH) {
                const float l = c == c0 ? l0 : row[c];
                if (!CB_ALLOWED(c, l)) continue;
                unsigned merged = 0;                       // slots whose extension by c is a beam member's entry
                for (int j = 0; j < nlive; ++j)
                    if (s_ms[j] >= 0 && s_tok[cur][j] == c) merged |= 1u << s_ms[j];
                for (int i = 0; i < nlive; ++i) {
                    if ((merged >> i) & 1u) continue;
                    const float s = (c == s_tok[cur][i] ? s_pb[cur][i] : s_p[i]) + l;
                    const long long id = (long long)i * V + c;
                    if (behind(s, id, ps, pid) && better(s, id, b.s, b.id)) { b.s = s; b.id = id; }
                }
            }
            const Best w = wg_best(b, s_red, round++);
            if (!(w.s > -INFINITY)) break;                 // nothing live is left (the same in every thread)
            if (tid == 0) { s_sel_s[r] = w.s; s_sel_id[r] = w.id; }
            ps = w.s; pid = w.id; nsel = r + 1;
        }
#undef CB_ALLOWED
        __syncthreads();
        // ---- the next beam; a new prefix looks for its node among its parent's children
        const int nxt = cur ^ 1;
        if (tid < nsel) {
            const int r = tid;
            const int i = (int)(s_sel_id[r] / V), c = (int)(s_sel_id[r] - (long long)i * V);
            if (c == 0) {
                s_pb[nxt][r] = s_spb[i]; s_pnb[nxt][r] = s_spnb[i];
                s_tok[nxt][r] = s_tok[cur][i]; s_len[nxt][r] = s_len[cur][i];
                s_node[nxt][r] = s_node[cur][i]; s_par[nxt][r] = s_par[cur][i];
            } else {
                const int parent = s_node[cur][i];
                int n = trie[4 * (long)parent + 2];
                while (n >= 0 && trie[4 * (long)n + 1] != c) n = trie[4 * (long)n + 3];
                s_pb[nxt][r] = -INFINITY; s_pnb[nxt][r] = s_sel_s[r];
                s_tok[nxt][r] = c; s_len[nxt][r] = s_len[cur][i] + 1;
                s_node[nxt][r] = n;                        // -1: not in the trie yet
                s_par[nxt][r] = parent;
            }
        }
        __syncthreads();
        if (tid == 0) {
            for (int r = 0; r < nsel; ++r) {
                if (s_node[nxt][r] >= 0) continue;
                const int parent = s_par[nxt][r], n = s_nnodes++;
                int* nd = trie + 4 * (long)n;
                nd[0] = parent; nd[1] = s_tok[nxt][r]; nd[2] = -1; nd[3] = trie[4 * (long)parent + 2];
                trie[4 * (long)parent + 2] = n;
                s_node[nxt][r] = n;
            }
        }
        nlive = nsel;
        cur = nxt;
        __syncthreads();
    }

    // ---- read-out: the beam is in rank order; a hypothesis is the path from its node to the root
    int* otok = p.out_tok + (long)u * K * p.Lcap;
    if (tid == 0) p.out_n[u] = nlive;
    for (int r = tid; r < K; r += NTH) {
        const bool live = r < nlive;
        const int len = live ? s_len[cur][r] : 0;
        p.out_len[(long)u * K + r] = len;
        p.out_score[(long)u * K + r] = live ? logaddexpf_(s_pb[cur][r], s_pnb[cur][r]) : -INFINITY;
        int n = live ? s_node[cur][r] : 0;
        for (int pos = len - 1; pos >= 0; --pos) {
            otok[(long)r * p.Lcap + pos] = trie[4 * (long)n + 1];
            n = trie[4 * (long)n];
        }
    }
    for (long idx = tid; idx < (long)K * p.Lcap; idx += NTH) {
        const int r = (int)(idx / p.Lcap), pos = (int)(idx - (long)r * p.Lcap);
        if (pos >= (r < nlive ? s_len[cur][r] : 0)) otok[idx] = 0;
    }
}

}  // namespace

extern "C" size_t asr_ctc_beam_search_workspace_bytes(int U, int Tmax, int K) {
    if (U <= 0 || Tmax <= 0 || K <= 0) return 0;
    return (size_t)U * (1 + (size_t)K * Tmax) * 4 * sizeof(int);
}

extern "C" int asr_ctc_beam_search(const float* logp, const int* tlen, int U, int Tmax, int V, int K, int cand, int Lcap,
                                   int* out_tokens, int* out_len, float* out_score, int* out_n,
                                   void* workspace, size_t workspace_bytes, asr_stream_t stream) {
    ASR_REQUIRE(logp && tlen && out_tokens && out_len && out_score && out_n && workspace, ASR_E_ARG, "asr_ctc_beam_search: null pointer");
    ASR_REQUIRE(U > 0 && Tmax > 0 && V > 1, ASR_E_ARG, "asr_ctc_beam_search: bad dims U=%d Tmax=%d V=%d", U, Tmax, V);
    ASR_REQUIRE(K >= 1 && K <= CB_KMAX, ASR_E_ARG, "asr_ctc_beam_search: beam %d outside 1..%d", K, CB_KMAX);
    ASR_REQUIRE(cand >= 0, ASR_E_ARG, "asr_ctc_beam_search: cand=%d is negative", cand);
    ASR_REQUIRE(Lcap >= Tmax, ASR_E_ARG, "asr_ctc_beam_search: Lcap=%d below Tmax=%d (a hypothesis can have one token per frame)", Lcap, Tmax);
    ASR_REQUIRE(1 + (size_t)K * Tmax <= (size_t)INT_MAX, ASR_E_ARG, "asr_ctc_beam_search: K*Tmax=%zu trie nodes exceed the node index",
                (size_t)K * Tmax);
    ASR_REQUIRE(workspace_bytes >= asr_ctc_beam_search_workspace_bytes(U, Tmax, K), ASR_E_ARG, "asr_ctc_beam_search: workspace too small");
    // one thread per non-blank token up to the launch bound; whole waves, at least one thread per beam slot
    const int nthr = WAVE * std::min(CB_NW, cdiv(std::max(V - 1, K), WAVE));
    ASR_REQUIRE(nthr >= K && nthr <= CB_NT, ASR_E_ARG, "asr_ctc_beam_search: %d threads outside the kernel's launch bounds (%d)", nthr, CB_NT);
    CbP p{logp, tlen, (int*)workspace, out_tokens, out_len, out_score, out_n, Tmax, V, K, cand, Lcap};
    hipLaunchKernelGGL(ctc_beam_kernel, dim3(U), dim3(nthr), 0, (hipStream_t)stream, p);
    ASR_LAUNCH_CHECK("asr_ctc_beam_search");
    return ASR_OK;
}
