// =================================================================================================================
// Device-side beam bookkeeping: one decoding step of BeamDecoder.forward (reference src/decode.py:104-177) for U
// utterances x `beam` hypothesis rows WITHOUT a device-to-host copy: candidate selection for the CTC scorer
// (`att_prob.topk(ctc_beam_size)`, :129), score fusion (:131-152), per-hypothesis top-k + the <eos> threshold rule
// (Hypothesis.addTopk :214-263), pruning by average score (:175-177), the `finals` list, and the parent / token indices
// the state gathers of the next step need.
//   narrow (asr_beam_candidates, asr_beam_step)           : one wave per row / utterance, a lane owns tokens lane + 64k in
//       registers; vocabularies up to 2048 (64 lanes x VPL tokens).
//   wide   (asr_beam_candidates_wide, asr_beam_step_wide) : a multi-wave workgroup per row strides over V <= WIDE_VMAX.
// Both state the selection order (beam_better), the fused score (BeamFuse) and everything behind a row's picks
// (beam_walk_row, beam_step_tail) once; they differ in how a row's picks are found.
// =================================================================================================================
#include <algorithm>
#include "common.h"

namespace {

constexpr float BEAM_LOG_ZERO = -10000000.0f;      // src/decode.py:11
constexpr int BEAM_MAX = 16, VPL = 32;             // hypotheses per utterance; tokens per lane of the narrow kernels
constexpr int WIDE_NONE = 0x7fffffff;              // the token of "no entry": behind every real one among equal values

// the one selection order: the larger value first, the lower token among equals
__device__ __forceinline__ bool beam_better(float v1, int i1, float v2, int i2) { return v1 > v2 || (v1 == v2 && i1 < i2); }

// the best (value, token) over the wave, in every lane
__device__ __forceinline__ void wave_best(float& wb, int& wi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(wb, o); const int oi = __shfl_xor(wi, o);
        if (beam_better(ob, oi, wb, wi)) { wb = ob; wi = oi; }
    }
}

// One round of the narrow kernels' top-k over a row in registers (v[k] is token lane + 64 k): the best entry above -inf that
// no earlier round took -> (wb, wi) in every lane, wi == WIDE_NONE when the row has run out; its owner marks it taken.
__device__ __forceinline__ void narrow_pick(const float (&v)[VPL], unsigned& taken, int V, int lane, float& wb, int& wi) {
    wb = -INFINITY; wi = WIDE_NONE;
#pragma unroll
    for (int k = 0; k < VPL; ++k) if (!((taken >> k) & 1u) && lane + 64 * k < V && v[k] > wb) { wb = v[k]; wi = lane + 64 * k; }
    wave_best(wb, wi);
    if (wi != WIDE_NONE && (wi & 63) == lane) taken |= 1u << (wi >> 6);
}

// top-C tokens of every row of att (rows, V), descending (ties: lower token first)
__global__ __launch_bounds__(64) void beam_candidates_kernel(const float* __restrict__ att, int* __restrict__ cand, int V, int C) {
    const int row = blockIdx.x, lane = threadIdx.x;
    float v[VPL];
    unsigned taken = 0u;
#pragma unroll
    for (int k = 0; k < VPL; ++k) { const int t = lane + 64 * k; v[k] = t < V ? att[(long)row * V + t] : -INFINITY; }
    for (int c = 0; c < C; ++c) {
        float wb; int wi;
        narrow_pick(v, taken, V, lane, wb, wi);
        if (lane == 0) cand[(long)row * C + c] = (wi == WIDE_NONE) ? 0 : wi;
    }
}

// The fused score of a token (src/decode.py:131-152): with the CTC scorer (1-w) att + w hack, token 0 at log zero, where hack
// is psi - ctcp of a candidate and log zero of any other token; with the LM plus lm_w lm.  Both steps evaluate it here, in
// the operation order of the float32 transcription and without contraction, so they agree bit for bit (the narrow step used
// to leave the contraction to the compiler: its scores moved by at most the rounding of one fma when this became shared).
struct BeamFuse {
    bool ctc, lm; float ctc_w, lm_w;
    __device__ __forceinline__ float operator()(float att, float hack, float lm_logp, int v) const {
#pragma clang fp contract(off)
        float c = att;
        if (ctc) {
            c = (1.f - ctc_w) * c + ctc_w * hack;
            if (v == 0) c = BEAM_LOG_ZERO;
        }
        if (lm) c += lm_w * lm_logp;
        return c;
    }
};

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
    BeamFuse fuse;                 // .ctc <=> psi and cand are given, .lm <=> lm is: set on the host (beam_params)
    float eos_thr;
};

// one live row's picks: n tokens with their fused scores in the order they were picked, and the <eos> rule's operands
struct BeamPicks {
    float val[BEAM_MAX]; int tok[BEAM_MAX];
    float att1, mx; int n, pad;
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

// What the picks of hypothesis i of utterance u do (Hypothesis.addTopk), for the wave of the utterance: <eos> ends the
// hypothesis where the threshold rule holds and joins the pool like any token where it does not, every other pick joins
// the pool, and a hypothesis that ended is inserted into the finals once it is long enough.  -> the search of the
// utterance stops here (beam == 1: its only hypothesis ended)
__device__ __forceinline__ bool beam_walk_row(const BeamP& p, BeamPool& s, int u, int i, int lane, const BeamPicks& sl, int& pool) {
    const int row = u * p.beam + i;
    const float sum_i = p.sum_in[row];
    const int len_i = p.len_in[row], n = min(sl.n, p.beam);
    bool term = false; float term_score = 0.f;
    for (int k2 = 0; k2 < n; ++k2) {
        const float wb = sl.val[k2]; const int wi = sl.tok[k2];
        // operands: the attention log-probs, not the fused scores (src/decode.py:235-242)
        if (wi == 1 && sl.att1 > p.eos_thr * sl.mx) { term = true; term_score = wb; continue; }
        if (lane == 0) beam_pool_push(p, s, pool, i, row, wi, wb, sum_i, len_i);
        ++pool;
    }
    if (!term || p.t < p.min_len[u]) return false;
    final_insert(p, u, lane, p.seq_in + (long)row * p.Lmax, p.sc_in + (long)row * p.Lmax, len_i, 1, term_score, true,
                 (sum_i + term_score) / (float)(len_i + 1));
    return p.beam == 1;
}

// What follows the per-hypothesis picks: pruning of the pool to the `beam` best by average in stable order, the new rows, the
// dead rows, the last-step flush into the finals
__device__ __forceinline__ void beam_step_tail(const BeamP& p, BeamPool& s, int u, int lane, int pool, bool stop) {
    const int beam = p.beam, r0 = u * beam, t = p.t;
    __syncthreads();
    if (stop) { beam_kill_rows(p, r0, 0, lane); if (lane == 0) p.done[u] = 1; return; }
    // prune: stable descending order by average score, keep `beam`
    for (int e = lane; e < pool; e += 64) {
        int rank = 0;
        const float a = s.avg[e];
        for (int o = 0; o < pool; ++o) rank += beam_better(s.avg[o], o, a, e) ? 1 : 0;
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

// One step of utterance blockIdx.x by one wave: picks(p, row, lane) -> the BeamPicks of a live row, in the order of the rows
template <class Picks> __device__ __forceinline__ void beam_step_body(const BeamP& p, BeamPool& s, const Picks& picks) {
    const int u = blockIdx.x, lane = threadIdx.x, r0 = u * p.beam;
    if (p.done[u] || p.t >= p.max_len[u]) { beam_kill_rows(p, r0, 0, lane); if (lane == 0) p.done[u] = 1; return; }
    int pool = 0;
    bool stop = false;
    for (int i = 0; i < p.beam && !stop; ++i) {
        if (!p.alive_in[r0 + i]) continue;                               // uniform
        stop = beam_walk_row(p, s, u, i, lane, picks(p, r0 + i, lane), pool);
    }
    beam_step_tail(p, s, u, lane, pool, stop);
}

// asr_beam_step: the wave fuses the row in registers, picks `beam` times, and lane 0 leaves the (wave-uniform) picks in `out`,
// one instance in LDS that every live row of the utterance uses in turn
struct NarrowPicks {
    BeamPicks& out;
    __device__ __forceinline__ const BeamPicks& operator()(const BeamP& p, int row, int lane) const {
        const int V = p.V;
        const float ctcp_i = p.ctcp_in[row];
        float att[VPL], cur[VPL];
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
            const int v = lane + 64 * k;
            att[k] = v < V ? p.att[(long)row * V + v] : -INFINITY;
            float hack = BEAM_LOG_ZERO;
            if (p.fuse.ctc)
                for (int cc = 0; cc < p.C; ++cc) if (p.cand[(long)row * p.C + cc] == v) hack = p.psi[(long)row * p.C + cc] - ctcp_i;
            cur[k] = v < V ? p.fuse(att[k], hack, p.fuse.lm ? p.lm[(long)row * V + v] : 0.f, v) : -INFINITY;
        }
        float mx = -INFINITY;                                            // the <eos> rule's operands
#pragma unroll
        for (int k = 0; k < VPL; ++k) { const int v = lane + 64 * k; if (v >= 2 && v < V) mx = fmaxf(mx, att[k]); }
        mx = wave_max(mx);
        const float att1 = __shfl(att[0], 1);
        __syncthreads();                                                 // the walk over the previous row's picks is over
        unsigned taken = 0u;
        int n = 0;
        for (; n < p.beam; ++n) {
            float wb; int wi;
            narrow_pick(cur, taken, V, lane, wb, wi);
            if (wi == WIDE_NONE) break;                                  // uniform
            if (lane == 0) { out.val[n] = wb; out.tok[n] = wi; }
        }
        if (lane == 0) { out.att1 = att1; out.mx = mx; out.n = n; }
        __syncthreads();
        return out;
    }
};

__global__ __launch_bounds__(64) void beam_step_kernel(BeamP p) {
    __shared__ BeamPool s;
    __shared__ BeamPicks picks;
    beam_step_body(p, s, NarrowPicks{picks});
}

// =================================================================================================================
// Vocabularies of word and subword size (V <= WIDE_VMAX): a row no longer fits one wave's registers, so a multi-wave
// workgroup owns a ROW and its threads stride over V.
//   wide_topk : the K best of a row in the order of beam_better.  A thread keeps the best token of its own stride that has
//       not been picked; per pick the workgroup reduces these to one winner (one barrier) and only the winner's thread scans
//       its stride again, for the best entry BEHIND the pick in that order - no mask of taken tokens, and the row is read
//       about once, not K times.
//   asr_beam_candidates_wide : wide_topk on the attention log-probs.
//   asr_beam_step_wide, phase A : per live row the fused score on the fly (the C candidates are marked in a V-bit map in LDS,
//       8 KB at the most, so a token costs one LDS word and the C-entry list is walked for candidates only), wide_topk with
//       K = beam, att[1] and max(att[2:]) -> the row's BeamPicks in the workspace.
//   phase B : beam_step_body on the picks in the workspace.
// Nothing in LDS scales with V beyond the bit map; rows are read from global memory (L2 on the re-scans).
// =================================================================================================================
constexpr int WIDE_NT = 512;             // largest workgroup: __launch_bounds__ of the row kernels, checked on the host; the stride over V
constexpr int WIDE_NW = WIDE_NT / WAVE;
constexpr int WIDE_VMAX = 65536, WIDE_CMAX = 32;
constexpr int WIDE_BITS = 32;            // tokens per word of the candidate bit map

struct WideRed { float v[2][WIDE_NW]; int i[2][WIDE_NW]; };

// whole waves, one thread per four tokens up to the launch bound
int wide_threads(int V) { return WAVE * (int)std::min((long)WIDE_NW, (long)cdiv(V, 4 * WAVE)); }

// the best (value, token) over the workgroup; every thread returns it.  `par` alternates between consecutive calls
__device__ __forceinline__ void wide_block_best(float& wb, int& wi, WideRed& red, int par) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    wave_best(wb, wi);
    if (lane == 0) { red.v[par][wave] = wb; red.i[par][wave] = wi; }
    __syncthreads();
    wb = red.v[par][0]; wi = red.i[par][0];
    for (int w = 1; w < nw; ++w) {
        const float ob = red.v[par][w]; const int oi = red.i[par][w];
        if (beam_better(ob, oi, wb, wi)) { wb = ob; wi = oi; }
    }
}

// the best entry above -inf of this thread's stride that lies behind (pv, pi) in the order
template <class Score> __device__ __forceinline__ void wide_scan(const Score& sc, int V, float pv, int pi, float& bv, int& bi) {
    bv = -INFINITY; bi = WIDE_NONE;
    for (int v = threadIdx.x; v < V; v += blockDim.x) {
        const float x = sc(v);
        if (beam_better(pv, pi, x, v) && x > bv) { bv = x; bi = v; }
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

// BeamFuse on a row in global memory; hack is looked up through the bit map
struct WideFused {
    const float* att; const float* lm; const unsigned* bits; const int* cand; const float* hack;
    int C; BeamFuse fuse;
    __device__ __forceinline__ float operator()(int v) const {
        float h = BEAM_LOG_ZERO;
        if (fuse.ctc && ((bits[v / WIDE_BITS] >> (v % WIDE_BITS)) & 1u))
            for (int cc = 0; cc < C; ++cc) if (cand[cc] == v) h = hack[cc];
        return fuse(att[v], h, fuse.lm ? lm[v] : 0.f, v);
    }
};

__global__ __launch_bounds__(WIDE_NT) void beam_step_wide_rows_kernel(BeamP p, BeamPicks* __restrict__ ws) {
    __shared__ WideRed red;
    __shared__ unsigned s_bits[WIDE_VMAX / WIDE_BITS];
    __shared__ int s_cand[WIDE_CMAX];
    __shared__ float s_hack[WIDE_CMAX], s_mx[WIDE_NW];
    const int row = blockIdx.x, u = row / p.beam, tid = threadIdx.x, V = p.V;
    if (p.done[u] || p.t >= p.max_len[u] || !p.alive_in[row]) return;    // uniform: phase B reads no picks of such a row
    const float* att = p.att + (long)row * V;
    if (p.fuse.ctc) {
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
    const WideFused sc{att, p.fuse.lm ? p.lm + (long)row * V : nullptr, s_bits, s_cand, s_hack, p.C, p.fuse};
    BeamPicks& out = ws[row];
    const int n = wide_topk(sc, V, p.beam, out.tok, out.val, red);
    if (tid == 0) {
        mx = s_mx[0];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) mx = fmaxf(mx, s_mx[w]);
        out.att1 = att[1]; out.mx = mx; out.n = n;
    }
}

struct WorkspacePicks {
    const BeamPicks* ws;
    __device__ __forceinline__ const BeamPicks& operator()(const BeamP&, int row, int) const { return ws[row]; }
};

__global__ __launch_bounds__(64) void beam_step_wide_pool_kernel(BeamP p, const BeamPicks* __restrict__ ws) {
    __shared__ BeamPool s;
    beam_step_body(p, s, WorkspacePicks{ws});
}

// ---- host: what the narrow (wide = false) and the wide entries refuse, and their launches -------------------------------
int wide_threads_check(const char* who, int nthr) {
    ASR_REQUIRE(nthr >= WAVE && nthr <= WIDE_NT, ASR_E_ARG, "%s: %d threads outside the kernel's launch bounds (%d)", who, nthr, WIDE_NT);
    return ASR_OK;
}

int beam_candidates_check(const char* who, const float* att_logp, const int* candidates, int rows, int V, int C, bool wide) {
    ASR_REQUIRE(att_logp && candidates, ASR_E_ARG, "%s: null pointer", who);
    const int cmax = wide ? std::min(V, WIDE_CMAX) : V, vmax = wide ? WIDE_VMAX : 64 * VPL;
    ASR_REQUIRE(rows > 0 && V > 1 && C > 0 && C <= cmax, ASR_E_ARG, "%s: bad dims rows=%d V=%d C=%d (1 <= C <= %d)", who, rows, V, C, cmax);
    ASR_REQUIRE(V <= vmax, ASR_E_UNSUPPORTED, "%s: vocabulary %d > %d", who, V, vmax);
    return wide ? wide_threads_check(who, wide_threads(V)) : ASR_OK;
}

int beam_step_check(const char* who, const asr_beam_step_t* a, bool wide, const void* workspace, size_t workspace_bytes) {
    // ctcp_in / ctcp_out are read and written in every mode (0 without CTC), so they are required in every mode
    ASR_REQUIRE(a && a->att_logp && a->alive_in && a->sum_in && a->ctcp_in && a->len_in && a->seq_in && a->score_in && a->alive_out && a->sum_out && a->ctcp_out &&
                a->len_out && a->seq_out && a->score_out && a->last_token && a->parent && a->ctc_index && a->tokens && a->min_len &&
                a->max_len && a->done && a->fin_n && a->fin_len && a->fin_avg && a->fin_seq && a->fin_score && (workspace || !wide), ASR_E_ARG,
                "%s: null pointer", who);
    ASR_REQUIRE(a->U > 0 && a->beam > 0 && a->beam <= BEAM_MAX && a->V > 1 && a->Lmax > 0 && a->t >= 0, ASR_E_ARG,
                "%s: bad dims (beam <= %d)", who, BEAM_MAX);
    // a vocabulary beyond the kernel: a bad argument to the narrow entry (the wide one exists for it), unsupported by the wide one
    const int vmax = wide ? WIDE_VMAX : 64 * VPL;
    ASR_REQUIRE(a->V <= vmax, wide ? ASR_E_UNSUPPORTED : ASR_E_ARG, "%s: vocabulary %d > %d", who, a->V, vmax);
    ASR_REQUIRE((a->psi == nullptr) == (a->candidates == nullptr) && (!a->candidates || a->C > 0), ASR_E_ARG,
                "%s: CTC operands come together, C >= 1", who);
    if (!wide) return ASR_OK;
    ASR_REQUIRE(!a->candidates || a->C <= WIDE_CMAX, ASR_E_ARG, "%s: C = %d > %d", who, a->C, WIDE_CMAX);
    ASR_REQUIRE(workspace_bytes >= asr_beam_step_wide_workspace_bytes(a->U, a->beam), ASR_E_ARG, "%s: workspace too small", who);
    return wide_threads_check(who, wide_threads(a->V));
}

BeamP beam_params(const asr_beam_step_t* a) {
    return BeamP{a->att_logp, a->lm_logp, a->psi, a->candidates, a->alive_in, a->sum_in, a->ctcp_in, a->len_in, a->seq_in, a->score_in,
                 a->alive_out, a->sum_out, a->ctcp_out, a->len_out, a->seq_out, a->score_out, a->last_token, (long long*)a->parent,
                 (long long*)a->ctc_index, (long long*)a->tokens, a->tokens_ld, a->min_len, a->max_len, a->done, a->fin_n, a->fin_len, a->fin_avg,
                 a->fin_seq, a->fin_score, a->U, a->beam, a->V, a->candidates ? a->C : 0, a->Lmax, a->t,
                 BeamFuse{a->candidates != nullptr, a->lm_logp != nullptr, a->ctc_weight, a->lm_weight}, a->eos_threshold};
}

}  // namespace

extern "C" int asr_beam_candidates(const float* att_logp, int* candidates, int rows, int V, int C, asr_stream_t stream) {
    if (const int rc = beam_candidates_check("asr_beam_candidates", att_logp, candidates, rows, V, C, false)) return rc;
    hipLaunchKernelGGL(beam_candidates_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, att_logp, candidates, V, C);
    ASR_LAUNCH_CHECK("asr_beam_candidates");
    return ASR_OK;
}

extern "C" int asr_beam_candidates_wide(const float* att_logp, int* candidates, int rows, int V, int C, asr_stream_t stream) {
    if (const int rc = beam_candidates_check("asr_beam_candidates_wide", att_logp, candidates, rows, V, C, true)) return rc;
    hipLaunchKernelGGL(beam_candidates_wide_kernel, dim3(rows), dim3(wide_threads(V)), 0, (hipStream_t)stream, att_logp, candidates, V, C);
    ASR_LAUNCH_CHECK("asr_beam_candidates_wide");
    return ASR_OK;
}

extern "C" int asr_beam_step(const asr_beam_step_t* a, asr_stream_t stream) {
    if (const int rc = beam_step_check("asr_beam_step", a, false, nullptr, 0)) return rc;
    hipLaunchKernelGGL(beam_step_kernel, dim3(a->U), dim3(64), 0, (hipStream_t)stream, beam_params(a));
    ASR_LAUNCH_CHECK("asr_beam_step");
    return ASR_OK;
}

extern "C" size_t asr_beam_step_wide_workspace_bytes(int U, int beam) {
    if (U <= 0 || beam <= 0 || beam > BEAM_MAX) return 0;
    return (size_t)U * beam * sizeof(BeamPicks);
}

extern "C" int asr_beam_step_wide(const asr_beam_step_t* a, void* workspace, size_t workspace_bytes, asr_stream_t stream) {
    if (const int rc = beam_step_check("asr_beam_step_wide", a, true, workspace, workspace_bytes)) return rc;
    const BeamP p = beam_params(a);
    hipLaunchKernelGGL(beam_step_wide_rows_kernel, dim3(a->U * a->beam), dim3(wide_threads(a->V)), 0, (hipStream_t)stream, p, (BeamPicks*)workspace);
    hipLaunchKernelGGL(beam_step_wide_pool_kernel, dim3(a->U), dim3(64), 0, (hipStream_t)stream, p, (const BeamPicks*)workspace);
    ASR_LAUNCH_CHECK("asr_beam_step_wide");
    return ASR_OK;
}
