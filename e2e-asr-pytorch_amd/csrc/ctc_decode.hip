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
//
// RNN-LM shallow fusion (asr_ctc_beam_lm_init / _advance / _readout): the same frame (cb_frame<true>) ranks an entry by
// p + its LM part - inherited by a stay, lms_i + lm_weight * lm_logp[row_i, c] + len_bonus for the extension of slot i by c -
// while pb / pnb stay pure CTC.  A new prefix needs an LM step (GEMMs) before it can be extended, so that search is RESUMABLE:
// the beam lives in the workspace between launches, and a launch runs frames until the first frame whose survivors include
// an extension, then tells the host which LM rows to gather (stays permute the slots) and which to step.
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

// ---- LDS of a search workgroup -----------------------------------------------------------------------------------------
struct CbBeam {
    float pb[CB_KMAX], pnb[CB_KMAX];
    int tok[CB_KMAX], len[CB_KMAX], node[CB_KMAX], par[CB_KMAX];
};

struct CbS {
    CbBeam b[2];                                   // the beam, double buffered
    float p[CB_KMAX], spb[CB_KMAX], spnb[CB_KMAX], stot[CB_KMAX];   // p of a slot; its stay entry
    int ms[CB_KMAX];                               // slot of the beam member that is this member's parent prefix, or -1
    float sel_s[CB_KMAX];
    long long sel_id[CB_KMAX];
    Best red[2 * CB_NW];
    int nnodes;
};

// what the search with a language model holds on top: per slot the LM part of the score and the row of the launch's LM
// table its distribution sits in; of the last frame run, whether a slot is an extension and whether any is
struct CbLmS {
    float lms[2][CB_KMAX];
    int row[2][CB_KMAX];
    int need[CB_KMAX];
    int ext;
};

struct CbLm {
    const float* lp;       // (K,V) of this utterance: row r = log P_lm(. | prefix of the slot whose row is r)
    float w, bonus;
};

// LM part of the extension of slot i by token c
__device__ __forceinline__ float cb_ext_lms(const CbLm& lm, const CbLmS* L, int cur, int i, int c, int V) {
    return fmaf(lm.w, lm.lp[(long)L->row[cur][i] * V + c], L->lms[cur][i]) + lm.bonus;
}

// ONE frame of the search, for the one-launch kernel (LM = false: L, lm unused) and the resumable one (LM = true): `row` =
// the frame's V log-probs.  S.b[cur] is the beam with nlive slots; on return cur is flipped and nlive updated.  With LM the
// entries are ranked by p_ctc + LM part, pb / pnb stay pure CTC.
template <bool LM>
__device__ __forceinline__ void cb_frame(CbS& S, CbLmS* L, const CbLm& lm, const float* row, int* trie, int V, int K, int cand,
                                         bool prune, int& nlive, int& cur, int& round) {
    const int tid = threadIdx.x, NTH = blockDim.x;
    const CbBeam& B = S.b[cur];
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
        for (int r = 0; r < cand; ++r) {
            Best b{-INFINITY, LLONG_MAX};
            for (int c = c0; c < V; c += NTH) {
                const float l = c == c0 ? l0 : row[c];
                if (behind(l, c, pv, pi) && better(l, c, b.s, b.id)) { b.s = l; b.id = c; }
            }
            const Best w = wg_best(b, S.red, round++);
            pv = w.s; pi = w.id;
        }
        thv = pv;
        thi = (int)min(pi, (long long)INT_MAX);
    }
#define CB_ALLOWED(c, l) ((l) > thv || ((l) == thv && (c) <= thi))
    // ---- stay entries
    if (tid < nlive) S.p[tid] = logaddexpf_(B.pb[tid], B.pnb[tid]);
    __syncthreads();
    if (tid < nlive) {
        const int j = tid, tj = B.tok[j];
        int ms = -1;
        if (B.len[j] > 0)
            for (int i = 0; i < nlive; ++i)
                if (B.node[i] == B.par[j]) ms = i;
        const float lj = row[tj];
        const float spb = S.p[j] + row[0];
        float spnb = B.len[j] > 0 ? B.pnb[j] + lj : -INFINITY;
        if (ms >= 0 && CB_ALLOWED(tj, lj))
            spnb = logaddexpf_(spnb, (tj == B.tok[ms] ? B.pb[ms] : S.p[ms]) + lj);
        S.ms[j] = ms;
        S.spb[j] = spb; S.spnb[j] = spnb; S.stot[j] = logaddexpf_(spb, spnb);
    }
    __syncthreads();
    // ---- the K best entries, one per round
    float ps = INFINITY;
    long long pid = -1;
    int nsel = 0;
    for (int r = 0; r < K; ++r) {
        Best b{-INFINITY, LLONG_MAX};
        if (tid < nlive) {
            float s = S.stot[tid];
            if constexpr (LM) s += L->lms[cur][tid];
            const long long id = (long long)tid * V;
            if (behind(s, id, ps, pid) && better(s, id, b.s, b.id)) { b.s = s; b.id = id; }
        }
        for (int c = c0; c < V; c += NTH) {
            const float l = c == c0 ? l0 : row[c];
            if (!CB_ALLOWED(c, l)) continue;
            unsigned merged = 0;                       // slots whose extension by c is a beam member's entry
            for (int j = 0; j < nlive; ++j)
                if (S.ms[j] >= 0 && B.tok[j] == c) merged |= 1u << S.ms[j];
            for (int i = 0; i < nlive; ++i) {
                if ((merged >> i) & 1u) continue;
                float s = (c == B.tok[i] ? B.pb[i] : S.p[i]) + l;
                if constexpr (LM) s += cb_ext_lms(lm, L, cur, i, c, V);
                const long long id = (long long)i * V + c;
                if (behind(s, id, ps, pid) && better(s, id, b.s, b.id)) { b.s = s; b.id = id; }
            }
        }
        const Best w = wg_best(b, S.red, round++);
        if (!(w.s > -INFINITY)) break;                 // nothing live is left (the same in every thread)
        if (tid == 0) { S.sel_s[r] = w.s; S.sel_id[r] = w.id; }
        ps = w.s; pid = w.id; nsel = r + 1;
    }
#undef CB_ALLOWED
    __syncthreads();
    // ---- the next beam; a new prefix looks for its node among its parent's children
    const int nxt = cur ^ 1;
    CbBeam& N = S.b[nxt];
    if (tid < nsel) {
        const int r = tid;
        const int i = (int)(S.sel_id[r] / V), c = (int)(S.sel_id[r] - (long long)i * V);
        if (c == 0) {
            N.pb[r] = S.spb[i]; N.pnb[r] = S.spnb[i];
            N.tok[r] = B.tok[i]; N.len[r] = B.len[i];
            N.node[r] = B.node[i]; N.par[r] = B.par[i];
            if constexpr (LM) L->lms[nxt][r] = L->lms[cur][i];
        } else {
            const int parent = B.node[i];
            int n = trie[4 * (long)parent + 2];
            while (n >= 0 && trie[4 * (long)n + 1] != c) n = trie[4 * (long)n + 3];
            N.pb[r] = -INFINITY;
            if constexpr (LM) {                        // sel_s is the fused score: the CTC part again
                N.pnb[r] = (c == B.tok[i] ? B.pb[i] : S.p[i]) + row[c];
                L->lms[nxt][r] = cb_ext_lms(lm, L, cur, i, c, V);
                L->ext = 1;
            } else {
                N.pnb[r] = S.sel_s[r];
            }
            N.tok[r] = c; N.len[r] = B.len[i] + 1;
            N.node[r] = n;                             // -1: not in the trie yet
            N.par[r] = parent;
        }
        if constexpr (LM) { L->row[nxt][r] = L->row[cur][i]; L->need[r] = c != 0; }
    }
    __syncthreads();
    if (tid == 0) {
        for (int r = 0; r < nsel; ++r) {
            if (N.node[r] >= 0) continue;
            const int parent = N.par[r], n = S.nnodes++;
            int* nd = trie + 4 * (long)n;
            nd[0] = parent; nd[1] = N.tok[r]; nd[2] = -1; nd[3] = trie[4 * (long)parent + 2];
            trie[4 * (long)parent + 2] = n;
            N.node[r] = n;
        }
    }
    nlive = nsel;
    cur = nxt;
    __syncthreads();
}

// read-out of utterance u: the beam is in rank order; a hypothesis is the path from its node to the root.  With LM
// out_score is the fused score and out_ctc the CTC part.
template <bool LM>
__device__ __forceinline__ void cb_readout(const CbBeam& B, const float* lms, int nlive, const int* trie, int u, int K, int Lcap,
                                           int* out_tok, int* out_len, float* out_score, float* out_ctc, int* out_n) {
    const int tid = threadIdx.x, NTH = blockDim.x;
    int* otok = out_tok + (long)u * K * Lcap;
    if (tid == 0) out_n[u] = nlive;
    for (int r = tid; r < K; r += NTH) {
        const bool live = r < nlive;
        const int len = live ? B.len[r] : 0;
        out_len[(long)u * K + r] = len;
        const float ctc = live ? logaddexpf_(B.pb[r], B.pnb[r]) : -INFINITY;
        if constexpr (LM) {
            out_ctc[(long)u * K + r] = ctc;
            out_score[(long)u * K + r] = live ? ctc + lms[r] : -INFINITY;
        } else {
            out_score[(long)u * K + r] = ctc;
        }
        int n = live ? B.node[r] : 0;
        for (int pos = len - 1; pos >= 0; --pos) {
            otok[(long)r * Lcap + pos] = trie[4 * (long)n + 1];
            n = trie[4 * (long)n];
        }
    }
    for (long idx = tid; idx < (long)K * Lcap; idx += NTH) {
        const int r = (int)(idx / Lcap), pos = (int)(idx - (long)r * Lcap);
        if (pos >= (r < nlive ? B.len[r] : 0)) otok[idx] = 0;
    }
}

__global__ __launch_bounds__(CB_NT) void ctc_beam_kernel(CbP p) {
    __shared__ CbS S;

    const int u = blockIdx.x, tid = threadIdx.x;
    const int V = p.V, K = p.K;
    const int T = max(0, min(p.tlen[u], p.Tmax));
    const float* lpu = p.lp + (long)u * p.Tmax * V;
    int* trie = p.trie + (long)u * (1 + (long)K * p.Tmax) * 4;
    const bool prune = p.cand > 0 && p.cand < V - 1;

    if (tid < CB_KMAX) {
        CbBeam& B = S.b[0];
        B.pb[tid] = tid == 0 ? 0.f : -INFINITY;
        B.pnb[tid] = -INFINITY;
        B.tok[tid] = 0; B.len[tid] = 0; B.node[tid] = 0; B.par[tid] = -1;
    }
    if (tid == 0) {
        trie[0] = -1; trie[1] = 0; trie[2] = -1; trie[3] = -1;       // root = the empty prefix
        S.nnodes = 1;
    }
    int nlive = 1, cur = 0, round = 0;
    __syncthreads();

    for (int t = 0; t < T; ++t)
        cb_frame<false>(S, nullptr, CbLm{}, lpu + (long)t * V, trie, V, K, p.cand, prune, nlive, cur, round);

    cb_readout<false>(S.b[cur], nullptr, nlive, trie, u, K, p.Lcap, p.out_tok, p.out_len, p.out_score, nullptr, p.out_n);
}

// ---- the resumable search (RNN-LM shallow fusion): the beam lives in the workspace between launches ------------------------
// workspace = the tries of all utterances (as above), then per utterance cbl_words(K) 4-byte words:
//   pb[K] pnb[K] lms[K] (float)  tok[K] len[K] node[K] par[K] (int)  nlive nnodes frame done magic (int)
// magic = the tag _init leaves for (Tmax, K): a workspace without it holds no beam, and its node indices are never followed
constexpr int CBL_TAIL = 5;
__host__ __device__ constexpr long cbl_words(int K) { return 7L * K + CBL_TAIL; }
__host__ __device__ inline int cbl_magic(int Tmax, int K) { return (int)(0x43420000u ^ ((unsigned)Tmax << 5) ^ (unsigned)K); }

struct CblP {
    const float* lp;       // (U,Tmax,V)
    const int* tlen;       // (U)
    const float* lm_lp;    // (U*K,V)
    int* trie;             // (U, 1 + K*Tmax, 4)
    int* state;            // (U, cbl_words(K))
    long long* src_row;    // (U*K)
    long long* step_tok;   // (U*K)
    int* need;             // (U*K)
    int* frame;            // (U)
    int* done;             // (U)
    int Tmax, V, K, cand, max_frames;
    float lm_w, bonus;
};

__global__ __launch_bounds__(CB_NT) void ctc_beam_lm_init_kernel(int* trie_all, int* state_all, int Tmax, int K) {
    const int u = blockIdx.x, tid = threadIdx.x;
    int* trie = trie_all + (long)u * (1 + (long)K * Tmax) * 4;
    int* st = state_all + (long)u * cbl_words(K);
    float* stf = (float*)st;
    if (tid < K) {
        stf[tid] = tid == 0 ? 0.f : -INFINITY;     // pb
        stf[K + tid] = -INFINITY;                  // pnb
        stf[2 * K + tid] = 0.f;                    // lms
        st[3 * K + tid] = 0; st[4 * K + tid] = 0; st[5 * K + tid] = 0; st[6 * K + tid] = -1;
    }
    if (tid == 0) {
        trie[0] = -1; trie[1] = 0; trie[2] = -1; trie[3] = -1;
        int* tail = st + 7 * K;
        tail[0] = 1; tail[1] = 1; tail[2] = 0; tail[3] = 0; tail[4] = cbl_magic(Tmax, K);
    }
}

// loads utterance u's beam into B (and lms); returns false when the workspace was not initialised for (Tmax, K)
__device__ __forceinline__ bool cbl_load(const int* st, int Tmax, int K, CbBeam& B, float* lms, int& nlive, int& nnodes, int& frame, int& done) {
    const int tid = threadIdx.x;
    const float* stf = (const float*)st;
    const int* tail = st + 7 * K;
    if (tail[4] != cbl_magic(Tmax, K)) return false;
    if (tid < K) {
        B.pb[tid] = stf[tid]; B.pnb[tid] = stf[K + tid]; lms[tid] = stf[2 * K + tid];
        B.tok[tid] = st[3 * K + tid]; B.len[tid] = st[4 * K + tid]; B.node[tid] = st[5 * K + tid]; B.par[tid] = st[6 * K + tid];
    }
    nlive = max(0, min(tail[0], K)); nnodes = tail[1]; frame = tail[2]; done = tail[3];
    return true;
}

__global__ __launch_bounds__(CB_NT) void ctc_beam_lm_advance_kernel(CblP p) {
    __shared__ CbS S;
    __shared__ CbLmS L;

    const int u = blockIdx.x, tid = threadIdx.x;
    const int V = p.V, K = p.K;
    const int T = max(0, min(p.tlen[u], p.Tmax));
    const float* lpu = p.lp + (long)u * p.Tmax * V;
    int* trie = p.trie + (long)u * (1 + (long)K * p.Tmax) * 4;
    int* st = p.state + (long)u * cbl_words(K);
    const bool prune = p.cand > 0 && p.cand < V - 1;
    const CbLm lm{p.lm_lp + (long)u * K * V, p.lm_w, p.bonus};

    int nlive = 0, nnodes = 0, frame = 0, done = 1, cur = 0, round = 0;
    const bool ok = cbl_load(st, p.Tmax, K, S.b[0], L.lms[0], nlive, nnodes, frame, done);
    if (tid < CB_KMAX) { L.row[0][tid] = tid; L.need[tid] = 0; }
    if (tid == 0) { S.nnodes = nnodes; L.ext = 0; }
    __syncthreads();

    const bool run = ok && !done && frame < T;
    if (run) {
        int nrun = 0;
        while (frame < T) {
            cb_frame<true>(S, &L, lm, lpu + (long)frame * V, trie, V, K, p.cand, prune, nlive, cur, round);
            ++frame; ++nrun;
            if (L.ext || (p.max_frames > 0 && nrun >= p.max_frames)) break;
        }
        const CbBeam& B = S.b[cur];
        float* stf = (float*)st;
        if (tid < K) {
            stf[tid] = B.pb[tid]; stf[K + tid] = B.pnb[tid]; stf[2 * K + tid] = L.lms[cur][tid];
            st[3 * K + tid] = B.tok[tid]; st[4 * K + tid] = B.len[tid]; st[5 * K + tid] = B.node[tid]; st[6 * K + tid] = B.par[tid];
        }
        if (tid == 0) {
            int* tail = st + 7 * K;
            tail[0] = nlive; tail[1] = S.nnodes; tail[2] = frame; tail[3] = frame >= T;
        }
    }
    // what the glue does with the LM rows: a finished utterance and a dead slot keep theirs
    if (tid < K) {
        const bool live = run && tid < nlive;
        const long g = (long)u * K + tid;
        p.src_row[g] = (long)u * K + (live ? L.row[cur][tid] : tid);
        p.step_tok[g] = live ? S.b[cur].tok[tid] : 0;
        p.need[g] = live ? L.need[tid] : 0;
    }
    if (tid == 0) {
        p.frame[u] = ok ? frame : 0;
        p.done[u] = !ok || done || frame >= T;
    }
}

struct CblOut {
    const int* trie; const int* state;
    int* out_tok; int* out_len; float* out_score; float* out_ctc; int* out_n;
    int Tmax, K, Lcap;
};

__global__ __launch_bounds__(CB_NT) void ctc_beam_lm_readout_kernel(CblOut p) {
    __shared__ CbBeam B;
    __shared__ float lms[CB_KMAX];
    const int u = blockIdx.x, K = p.K;
    const int* trie = p.trie + (long)u * (1 + (long)K * p.Tmax) * 4;
    int nlive = 0, nnodes, frame, done;
    if (!cbl_load(p.state + (long)u * cbl_words(K), p.Tmax, K, B, lms, nlive, nnodes, frame, done)) nlive = 0;
    __syncthreads();
    cb_readout<true>(B, lms, nlive, trie, u, K, p.Lcap, p.out_tok, p.out_len, p.out_score, p.out_ctc, p.out_n);
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

// ---- the resumable search with RNN-LM shallow fusion -------------------------------------------------------------------------
static size_t cbl_trie_bytes(int U, int Tmax, int K) { return (size_t)U * (1 + (size_t)K * Tmax) * 4 * sizeof(int); }

extern "C" size_t asr_ctc_beam_lm_workspace_bytes(int U, int Tmax, int K) {
    if (U <= 0 || Tmax <= 0 || K <= 0) return 0;
    return cbl_trie_bytes(U, Tmax, K) + (size_t)U * cbl_words(K) * sizeof(int);
}

// the checks the three entry points share
static int cbl_check(const char* who, int U, int Tmax, int K, const void* workspace, size_t workspace_bytes) {
    ASR_REQUIRE(workspace, ASR_E_ARG, "%s: null pointer", who);
    ASR_REQUIRE(U > 0 && Tmax > 0, ASR_E_ARG, "%s: bad dims U=%d Tmax=%d", who, U, Tmax);
    ASR_REQUIRE(K >= 1 && K <= CB_KMAX, ASR_E_ARG, "%s: beam %d outside 1..%d", who, K, CB_KMAX);
    ASR_REQUIRE(1 + (size_t)K * Tmax <= (size_t)INT_MAX, ASR_E_ARG, "%s: K*Tmax=%zu trie nodes exceed the node index", who, (size_t)K * Tmax);
    ASR_REQUIRE(workspace_bytes >= asr_ctc_beam_lm_workspace_bytes(U, Tmax, K), ASR_E_ARG, "%s: workspace too small", who);
    return ASR_OK;
}

extern "C" int asr_ctc_beam_lm_init(int U, int Tmax, int K, void* workspace, size_t workspace_bytes, asr_stream_t stream) {
    const int rc = cbl_check("asr_ctc_beam_lm_init", U, Tmax, K, workspace, workspace_bytes);
    if (rc != ASR_OK) return rc;
    int* trie = (int*)workspace;
    int* state = (int*)((char*)workspace + cbl_trie_bytes(U, Tmax, K));
    hipLaunchKernelGGL(ctc_beam_lm_init_kernel, dim3(U), dim3(WAVE), 0, (hipStream_t)stream, trie, state, Tmax, K);
    ASR_LAUNCH_CHECK("asr_ctc_beam_lm_init");
    return ASR_OK;
}

extern "C" int asr_ctc_beam_lm_advance(const float* logp, const int* tlen, const float* lm_logp, int U, int Tmax, int V, int K, int cand,
                                       float lm_weight, float len_bonus, int max_frames, int64_t* src_row, int64_t* step_tok,
                                       int* need, int* frame, int* done, void* workspace, size_t workspace_bytes,
                                       asr_stream_t stream) {
    ASR_REQUIRE(logp && tlen && lm_logp && src_row && step_tok && need && frame && done, ASR_E_ARG, "asr_ctc_beam_lm_advance: null pointer");
    ASR_REQUIRE(V > 1, ASR_E_ARG, "asr_ctc_beam_lm_advance: bad dims V=%d", V);
    ASR_REQUIRE(cand >= 0, ASR_E_ARG, "asr_ctc_beam_lm_advance: cand=%d is negative", cand);
    ASR_REQUIRE(max_frames >= 0, ASR_E_ARG, "asr_ctc_beam_lm_advance: max_frames=%d is negative", max_frames);
    const int rc = cbl_check("asr_ctc_beam_lm_advance", U, Tmax, K, workspace, workspace_bytes);
    if (rc != ASR_OK) return rc;
    const int nthr = WAVE * std::min(CB_NW, cdiv(std::max(V - 1, K), WAVE));
    ASR_REQUIRE(nthr >= K && nthr <= CB_NT, ASR_E_ARG, "asr_ctc_beam_lm_advance: %d threads outside the kernel's launch bounds (%d)", nthr, CB_NT);
    CblP p{logp, tlen, lm_logp, (int*)workspace, (int*)((char*)workspace + cbl_trie_bytes(U, Tmax, K)), (long long*)src_row,
           (long long*)step_tok, need, frame, done, Tmax, V, K, cand, max_frames, lm_weight, len_bonus};
    hipLaunchKernelGGL(ctc_beam_lm_advance_kernel, dim3(U), dim3(nthr), 0, (hipStream_t)stream, p);
    ASR_LAUNCH_CHECK("asr_ctc_beam_lm_advance");
    return ASR_OK;
}

extern "C" int asr_ctc_beam_lm_readout(int U, int Tmax, int K, int Lcap, int* out_tokens, int* out_len, float* out_score,
                                       float* out_ctc_score, int* out_n, const void* workspace, size_t workspace_bytes,
                                       asr_stream_t stream) {
    ASR_REQUIRE(out_tokens && out_len && out_score && out_ctc_score && out_n, ASR_E_ARG, "asr_ctc_beam_lm_readout: null pointer");
    const int rc = cbl_check("asr_ctc_beam_lm_readout", U, Tmax, K, workspace, workspace_bytes);
    if (rc != ASR_OK) return rc;
    ASR_REQUIRE(Lcap >= Tmax, ASR_E_ARG, "asr_ctc_beam_lm_readout: Lcap=%d below Tmax=%d (a hypothesis can have one token per frame)", Lcap, Tmax);
    CblOut p{(const int*)workspace, (const int*)((const char*)workspace + cbl_trie_bytes(U, Tmax, K)), out_tokens, out_len, out_score,
             out_ctc_score, out_n, Tmax, K, Lcap};
    hipLaunchKernelGGL(ctc_beam_lm_readout_kernel, dim3(U), dim3(WAVE), 0, (hipStream_t)stream, p);
    ASR_LAUNCH_CHECK("asr_ctc_beam_lm_readout");
    return ASR_OK;
}
