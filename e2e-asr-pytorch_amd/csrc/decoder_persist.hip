// Persistent, state-resident form of the teacher-forced decoder loop (forward): ONE launch walks all L steps
// (reference src/asr.py:123-175; the per-step kernels of decoder.hip stay for greedy/beam decoding, fp32 parity mode,
// multi-layer decoders and shapes outside the limits below, and produce the same saved state).
//
// The loop has no cross-utterance dependency except shared weights, so each utterance b gets a CLUSTER of NT workgroups
// (one per TE-frame tile of its encoder output) that runs its own L steps with intra-cluster hand-offs only:
//   * resident for all L steps: the tile's key and enc rows as bf16 in LDS (no HBM re-read per step), W_proj^T, the previous
//     attention row of the utterance, the workgroup's slice of the decoder state (c of UPW hidden units);
//   * per step three all-gathers inside the cluster (data-tagged granules, lstm_persist2.hip's scheme):
//       H: h_{t-1} slices (UPW units per workgroup)      -> query slice q[a], a in the workgroup's QPW outputs
//       Q: query slices                                   -> energies of the tile, local softmax statistics (m, s) and the
//                                                            partial context  sum_f exp(e_f - m) enc[f,:]
//       S: {e[TE], m, s, ctx_partial[E]} records          -> every workgroup rebuilds the utterance's attention row and context
//     then the LSTM cell for the workgroup's UPW units (4*UPW rows of [W_ih(ctx part) | W_hh] streamed as bf16 from L2;
//     the embedding part W_ih[:, :Dd] emb(token) is one batched contraction before the launch);
//   * cluster b lives on XCD b % 8 (workgroup id = 8*slot + xcd under round-robin dispatch); placement is verified by the
//     XCC-id consensus and only then the producers use L2-local stores.
// Waves 0-7 compute and store, waves 8-11 only poll (their vector-memory queue holds nothing else).  The compute waves
// synchronise among themselves through an LDS counter where the polling waves are busy; s_barrier is used where
// the polled data is handed over.
#include "decoder_plan.h"
#include "gemm_plan.h"
#include "decoder_fwd_common.h"

static int g_persist_fwd = -1, g_persist_bwd = -1;   // -1: from env ASR_DEC_PERSIST / ASR_DEC_PERSIST_BWD (default on)
static int g_stream_fwd = -1, g_stream_bwd = -1;     // 1: take the streamed-tile plan (decoder_stream.hip) even where the LDS-resident one exists; -1: env ASR_DEC_STREAM
// bit 0: persistent forward, bit 1: persistent backward, bit 2 / 3: prefer the streamed-tile plan forward / backward (tests, A/B
// runs; shapes without an LDS-resident plan take the streamed one anyway); returns the previous setting
extern "C" int asr_att_decoder_set_persistent(int flags) {
    const int old = (g_persist_fwd != 0 ? 1 : 0) | (g_persist_bwd != 0 ? 2 : 0) | (g_stream_fwd > 0 ? 4 : 0) | (g_stream_bwd > 0 ? 8 : 0);
    g_persist_fwd = flags & 1; g_persist_bwd = (flags >> 1) & 1; g_stream_fwd = (flags >> 2) & 1; g_stream_bwd = (flags >> 3) & 1;
    return old;
}
// what asr_att_decoder_set_persistent has not set comes from the environment, on first use
static void read_switches() {
    if (g_persist_fwd < 0) g_persist_fwd = env_switch("ASR_DEC_PERSIST", 1);
    if (g_persist_bwd < 0) g_persist_bwd = env_switch("ASR_DEC_PERSIST_BWD", 1);
    if (g_stream_fwd < 0) g_stream_fwd = env_switch("ASR_DEC_STREAM", 0);
    if (g_stream_bwd < 0) g_stream_bwd = env_switch("ASR_DEC_STREAM", 0);
}
static FwdPlan fwd_plan(const asr_dec_dims_t& d) { read_switches(); return chosen_plan(persist_plan(d), stream_plan_f(d), g_stream_fwd); }
static BwdPlan bwd_plan(const asr_dec_dims_t& d) { read_switches(); return chosen_plan(persist_plan_b(d), stream_plan_b(d), g_stream_bwd); }

DecPlanInfo dec_fwd_plan_info(const asr_dec_dims_t& d) {
    read_switches();
    const FwdPlan r = persist_plan(d), s = stream_plan_f(d);
    return {chosen_plan(r, s, g_stream_fwd).kind, 0, 0, std::max(r.total, s.total)};
}
DecPlanInfo dec_bwd_plan_info(const asr_dec_dims_t& d) {
    read_switches();
    const BwdPlan r = persist_plan_b(d), s = stream_plan_b(d), pl = chosen_plan(r, s, g_stream_bwd);
    return {pl.kind, pl.NT, std::max(r.NT, s.NT), std::max(r.total, s.total)};
}
float* dec_bwd_dgates(const asr_dec_dims_t& d, void* work) { return bwd_work(d, bwd_plan(d), work).dgates; }

namespace {

// Dynamic LDS of dec_fwd_persist in bytes, for persist_plan.  The kernel keeps its hand-written carve: taking the offsets or the
// lengths from one shared function, as the other three cluster kernels do, changed its scalar-register spill counts.  Every
// term sizes the pointer named beside it, in the order of the kernel's "LDS carve" block - change the two together.
size_t dec_fwd_persist_lds(int TE, int NT, int A, int E, int Ks, int KCP, int UPW, int SG2) {
    const int EPL = 16 * cdiv(TE, 16);                          // the kernel's EPL = 16 * MT
    const ConvGeo cg = conv_geo(EPL, Ks);
    const size_t shorts = (size_t)((TE * A + 7) & ~7)           // s_key
                        + ((TE * E + 7) & ~7)                   // s_enc
                        + EPL * FCVX_LD                         // s_cvx
                        + 8 * cg.IMG_LD                         // s_ximg
                        + 32 * cg.WKP;                          // s_wimg
    const size_t floats = (size_t)2 * KCP                       // s_x2
                        + ((A + 3) & ~3)                        // s_q
                        + ((A + 3) & ~3)                        // s_wg
                        + ((NT * TE + 2 * Ks + 8 + 3) & ~3)     // s_attp (ATP)
                        + NCW * EPL                             // s_epart
                        + ((4 * UPW + 3) & ~3)                  // s_g
                        + (size_t)NT * 2 * SG2;                 // s_stage
    return 2 * shorts + 4 * floats;
}

template <int KNMAX, int TPW>
__global__ __launch_bounds__(64 * (NCW + NPW)) void dec_fwd_persist(PD p) {
    constexpr int TE = 8 * TPW;
    constexpr int MT = (TE + 15) / 16;                                   // 16-frame MFMA tiles of the energy sweep
    constexpr int EPL = 16 * MT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned s_bar;
    __shared__ float s_scale[NCW][32];
    const asr_dec_dims_t& d = p.d;
    const int id = blockIdx.x, xcd = id & 7, slot = id >> 3;
    const int cb = slot / p.NT, j = slot - cb * p.NT;
    const int b = cb * 8 + xcd;
    if (b >= d.B) return;
    const unsigned epoch_ = __builtin_amdgcn_readfirstlane(p.status[EPOCH_WORD]);     // launch epoch of this work area (decoder_cluster.h)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NT = p.NT, A = d.A, E = d.E, Dd = d.Dd, Tp = d.Tp, Kn = d.Kn, Ks = d.Ks, L = d.L;
    const int taps = 2 * Ks + 1;
    const int tau0 = j * TE;
    const int len = min((int)p.enc_len[b], Tp);
    const int tmax = max(len - 1, 0);
    // ---- LDS carve
    unsigned short* s_key = reinterpret_cast<unsigned short*>(smem);                 // [TE/4][A][4] bf16 (four frames innermost)
    unsigned short* s_enc = s_key + ((TE * A + 7) & ~7);                              // [TE][E] bf16
    unsigned short* s_cvx = s_enc + ((TE * E + 7) & ~7);                              // [16*MT][32] bf16 conv tile of the step, slots {hi | lo | hi}
    const ConvGeo cg_ = conv_geo(EPL, Ks);
    unsigned short* s_ximg = s_cvx + EPL * FCVX_LD;                                   // window image of the attention row, {hi, lo} x 4 shifts
    unsigned short* s_wimg = s_ximg + 8 * cg_.IMG_LD;                                 // filter image {hi, lo} x 16 rows (decoder_cluster.h::conv_mfma)
    float* s_x2 = reinterpret_cast<float*>(s_wimg + 32 * cg_.WKP);                    // [2][KCP]  ctx_t | h_{t-1} | 0, by step parity
    float* s_q = s_x2 + 2 * p.KCP;                                                       // [A]
    float* s_wg = s_q + ((A + 3) & ~3);                                               // [A]
    const int WT = (taps + 3) & ~3;                                                    // zero-padded filter row (16-byte units)
    const int ATP = (NT * TE + 2 * Ks + 8 + 3) & ~3;
    float* s_attp = s_wg + ((A + 3) & ~3);                                             // [Ks + NT*TE + Ks + 8]  zero-padded previous attention
    float* s_epart = s_attp + ATP;                                                    // [NCW][16*MT] energy partials of the compute waves
    float* s_g = s_epart + NCW * EPL;                                                 // [4*UPW]
    float* s_stage = s_g + ((4 * p.UPW + 3) & ~3);                                    // [NT][2*SG2]
    if (tid == 0) s_bar = 0u;
    FwdCl cl_ = fwd_cl(p, b, j, s_x2, s_q, s_attp, s_g, s_stage, &s_scale[0][0], epoch_);
    clear_own_records(cl_, tid, blockDim.x);
    __syncthreads();
    cl_.local = xcd_consensus(reinterpret_cast<u64*>(p.status) + 64 + b, NT, p.allow_local, p.status);
    const FwdCl& cl = cl_;

    // ---- resident data
    for (int i = tid; i < TE * A; i += blockDim.x) {
        const int f = i / A, a = i - f * A;
        s_key[((long)(f >> 2) * A + a) * 4 + (f & 3)] = f2bf_bits(p.s.key[((long)b * Tp + min(tau0 + f, tmax)) * A + a]);
    }
    for (int i = tid; i < TE * E; i += blockDim.x) {
        const int f = i / E, c = i - f * E;
        s_enc[i] = f2bf_bits(p.enc[((long)b * Tp + min(tau0 + f, tmax)) * E + c]);
    }
    for (int i = tid; i < EPL * FCVX_LD; i += blockDim.x) s_cvx[i] = 0;
    conv_build_wimg(p.w.Wconv, Kn, taps, cg_, s_wimg, tid, blockDim.x);
    for (int i = tid; i < A; i += blockDim.x) s_wg[i] = p.w.wg[i];
    for (int i = tid; i < 2 * p.KCP; i += blockDim.x) s_x2[i] = 0.f;
    {
        const float uni = 1.f / (float)max(len, 1);
        for (int i = tid; i < ATP; i += blockDim.x) {
            const int tau = i - Ks;
            s_attp[i] = (tau >= 0 && tau < len) ? uni : 0.f;       // initial attention: uniform over the valid frames
        }
    }
    __syncthreads();

    if (wave >= NCW) {
        // =========================== polling role ===========================
        const int gt = tid - 64 * NCW, np = 64 * NPW;
        for (int t = 0; t < L; ++t) {
            if (t > 0) poll_h(cl, t, gt, np);
            DP_JIT(0)
            __syncthreads();                                            // B1
            DP_JIT(1)
            poll_q(cl, t, gt, np);
            DP_JIT(2)
            __syncthreads();                                            // B2
            DP_JIT(3)
            poll_s(cl, t, gt, np);
            DP_JIT(4)
            __syncthreads();                                            // B3
            DP_JIT(5)
        }
        return;
    }

    // =========================== compute role ===========================
    unsigned gen = 0;
    const float bg = p.w.bg[0];
    float c_state = 0.f;                                                // cell state of unit u_base + lane (wave 0, lane < UPW)
    const int RPW = (4 * p.UPW + NCW - 1) / NCW;                        // gate rows per wave
    const int nu_cnt = (((A + 15) >> 4) - wave + NCW - 1) / NCW;
    bf16x8 wpx[FSW_NU];
    float wgu[FSW_NU];
    sweep_operands<KNMAX>(cl, wave, lane, wpx, wgu);
    constexpr int QR = 2;                                               // query rounds with register-resident W_q rows
    QRows<QR> qrows;
    query_rows_load(cl, wave, lane, qrows);
    DP_DECL

    for (int t = 0; t < L; ++t) {
        // thread-index arithmetic of the step is loop invariant: hoisted it becomes dozens of live address registers (and
        // spills); an opaque copy of the indices ties it to the step
        int tz = tid, lz_ = lane;
        asm volatile("" : "+v"(tz), "+v"(lz_));
        const int lane = lz_;
        const long row = (long)b * L + t;
        const FwdStep st{t, row, s_x2 + (t & 1) * p.KCP, cl.xb(t & 1), pair_want(seq_of(t), epoch_), wave, lane, tz};
        const float add_r = cell_add_r(cl, st, RPW);                     // requested now, used in the cell phase
        DP_MARK(0)
        __syncthreads();                                                // B1: s_x holds h_{t-1}
        DP_MARK(1)
        query_slice<QR>(cl, st, qrows);
        DP_MARK(2)
        // ---- location convolution of the tile from the previous attention row (runs while the query is gathered): a Toeplitz
        //      product on the matrix cores (decoder_cluster.h::conv_mfma).  A lane ends up with four kernels of one frame: the
        //      {hi | lo | hi} slots of the sweep's operand row (the A operand of its MFMA) are written straight from the accumulator
        {
            conv_build_ximg(s_attp + tau0, ATP - tau0, cg_, s_ximg, tz, 64 * NCW);
            compute_barrier(&s_bar, gen);
            conv_mfma<NCW>(s_ximg, s_wimg, cg_, MT, wave, lane, [&](int mt, int n, int q4, const f32x4& acc) {
                const int i = 16 * mt + n;
                unsigned short* r = s_cvx + i * FCVX_LD;
#pragma unroll
                for (int pp = 0; pp < 2; ++pp) {
                    const int k0 = 4 * q4 + 2 * pp;
                    if (k0 < Kn && i < TE) {
                        const float v0 = acc[2 * pp], v1 = acc[2 * pp + 1];
                        const __bf16 h0 = (__bf16)v0, h1 = (__bf16)v1;
                        const __bf16 l0 = (__bf16)(v0 - (float)h0), l1 = (__bf16)(v1 - (float)h1);
                        const unsigned hh = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
                        const unsigned ll = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
                        *reinterpret_cast<unsigned*>(r + k0) = hh;
                        *reinterpret_cast<unsigned*>(r + KNMAX + k0) = ll;
                        *reinterpret_cast<unsigned*>(r + 2 * KNMAX + k0) = hh;
                        if (p.s.conv && tau0 + i < Tp) {
                            p.s.conv[(row * Kn + k0) * Tp + tau0 + i] = v0;
                            if (k0 + 1 < Kn) p.s.conv[(row * Kn + k0 + 1) * Tp + tau0 + i] = v1;
                        }
                    }
                }
            });
        }
        DP_MARK(3)
        __syncthreads();                                                // B2: s_q holds q_t, s_cvx the tile's conv
        DP_MARK(4)
        // ---- energies of the tile on the matrix cores (see the backward's sweep_step): wave w owns the 16-column units
        //      w, w + NCW, ...; lp = conv . W_proj as ONE split-bf16 MFMA per 16 x 16 tile, a lane holds column a = 16 u + (lane & 15)
        //      and frames 16 mt + 4 (lane >> 4) + r; its partial energies are summed over the 16 columns of the row with DPP adds
        //      and over the waves through s_epart (fixed order: deterministic)
        {
            int opaque = 0;
            asm volatile("" : "+v"(opaque));                            // keeps the LDS addresses below out of the loop-invariant registers
            const int q = (lane >> 4) + opaque, c = lane & 15;
            float ep[MT][4];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) ep[mt][r] = 0.f;
            float qv[FSW_NU];
#pragma unroll
            for (int nu = 0; nu < FSW_NU; ++nu) qv[nu] = s_q[min(16 * (wave + NCW * nu) + c, A - 1)];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int f0 = 16 * mt + 4 * q;
                const bf16x8 av = *reinterpret_cast<const bf16x8*>(s_cvx + (16 * mt + c) * FCVX_LD + 8 * q);
                const int fg = min(f0, TE - 4) >> 2;
#pragma unroll
                for (int nu = 0; nu < FSW_NU; ++nu) {
                    if (nu < nu_cnt) {
                        const int a = min(16 * (wave + NCW * nu) + c, A - 1);
                        const f32x4 lp = mma16(av, wpx[nu], f32x4{0.f, 0.f, 0.f, 0.f});
                        const uint2 kb = *reinterpret_cast<const uint2*>(s_key + ((long)fg * A + a) * 4);
                        const float key[4] = {__uint_as_float(kb.x << 16), __uint_as_float(kb.x & 0xffff0000u),
                                              __uint_as_float(kb.y << 16), __uint_as_float(kb.y & 0xffff0000u)};
#pragma unroll
                        for (int r = 0; r < 4; ++r) ep[mt][r] += wgu[nu] * tanh_f(key[r] + qv[nu] + tanh_f(lp[r]));
                    }
                }
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = sum16_dpp(ep[mt][r]);                   // sum over the 16 lanes of the row
                    if (c == 0) s_epart[wave * EPL + 16 * mt + 4 * q + r] = v;
                }
        }
        DP_MARK(5)
        compute_barrier(&s_bar, gen);                                   // c3: s_epart complete
        DP_MARK(6)
        // ---- local softmax statistics (every wave for itself) and the tile's partial context
        {
            float ev = NEG_BIG;
            if (lane < TE) {
                float sv = 0.f;
#pragma unroll
                for (int w8 = 0; w8 < NCW; ++w8) sv += s_epart[w8 * EPL + lane];
                if (tau0 + lane < len) ev = (sv + bg) / d.temperature;
            }
            const float m = wave_max_dpp(ev);
            const float wv = (ev > 0.5f * NEG_BIG) ? __expf(ev - m) : 0.f;
            const float ssum = wave_sum_dpp(wv);
            // thread c2: context columns 2*c2, 2*c2+1
            const int c2 = tz;
            float x0 = 0.f, x1 = 0.f;
            if (2 * c2 < E) {
#pragma unroll
                for (int f = 0; f < TE; ++f) {
                    const float wf = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wv), f));
                    const unsigned pr = *reinterpret_cast<const unsigned*>(s_enc + f * E + 2 * c2);
                    x0 += wf * __uint_as_float(pr << 16);
                    x1 += wf * __uint_as_float(pr & 0xffff0000u);
                }
            }
            u64* rec = st.out + cl.offS + (long)j * p.SG2;
            const int ghead = (TE + 2) >> 1;                             // granules of e[TE], m, s
            // context columns 4 at a time as halves (pack4h): the even threads take their neighbour's pair
            const float y0 = __shfl_down(x0, 1), y1 = __shfl_down(x1, 1);
            if (2 * c2 < E && (c2 & 1) == 0) {
                publish_gran(cl.local, rec + ghead + (c2 >> 1), pack4h(x0, x1, y0, y1, st.want));
            }
            // e pairs, (m, s) and the pad granule by the last compute wave's lanes
            if (wave == NCW - 1) {
                const float e0 = __shfl(ev, min(2 * lane, 63)), e1 = __shfl(ev, min(2 * lane + 1, 63));
                if (lane < TE / 2) {
                    publish_gran(cl.local, rec + lane, pack2(e0, e1, st.want));
                } else if (lane == TE / 2) {
                    publish_gran(cl.local, rec + lane, pack2(m, ssum, st.want));
                } else if (lane == TE / 2 + 1 && ghead + E / 4 < p.SG2) {
                    publish_gran(cl.local, rec + p.SG2 - 1, pack2(0.f, 0.f, st.want));
                }
            }
        }
        DP_MARK(7)
        __syncthreads();                                                // B3: s_stage holds every tile's record
        DP_MARK(8)
        // ---- attention row and context of the utterance
        combine_records(cl, st, TE);
        DP_MARK(9)
        compute_barrier(&s_bar, gen);                                   // c5: s_x holds [ctx_t | h_{t-1}]
        DP_MARK(10)
        // ---- LSTM cell: gate pre-activations, then the update of the UPW <= 64 units by wave 0
        cell_rows<10>(cl, st, RPW, add_r);
        DP_MARK(11)
        compute_barrier(&s_bar, gen);                                   // c6: s_g holds the gate pre-activations
        DP_MARK(12)
        cell_update<false>(cl, st, c_state);
        DP_MARK(13)
    }
    DP_DUMP
}

FwdPlan persist_plan(const asr_dec_dims_t& d) {
    if (d.NL != 1 || d.B > 64 || d.A > 16 * FSW_NU * NCW || d.Kn > 10 || (d.E & 7) != 0 || d.Dd > 20 * 32 || d.Tp < 1) return FwdPlan{};
    const int cpx = cdiv(d.B, 8);                       // clusters per XCD
    const int cand[] = {2, 4, 5, 8};
    FwdPlan pl{};
    for (int i = 0; i < 4 && !pl.tpw; ++i) {
        const int nt = cdiv(d.Tp, 8 * cand[i]);
        if (nt <= 30 && cpx * nt <= 32) pl.tpw = cand[i];
    }
    if (!pl.tpw) return FwdPlan{};
    pl.kind = 1; pl.TE = 8 * pl.tpw; pl.NT = cdiv(d.Tp, pl.TE);
    fwd_sizes(d, pl);
    if (pl.UPW > 64 || cdiv(4 * pl.UPW, NCW) > 60) return FwdPlan{};
    pl.lds = dec_fwd_persist_lds(pl.TE, pl.NT, d.A, d.E, d.Ks, pl.KCP, pl.UPW, pl.SG2);
    if (getenv("ASR_DEC_PLAN_DEBUG")) fprintf(stderr, "[asr] resident fwd plan B=%d T'=%d: NT=%d TE=%d UPW=%d LDS=%zu\n", d.B, d.Tp, pl.NT, pl.TE, pl.UPW, pl.lds);
    return pl.lds > 156 * 1024 ? FwdPlan{} : pl;
}

}  // namespace

int dec_fwd_persistent(const asr_dec_dims_t& d, const asr_dec_weights_t& w, const asr_dec_state_t& s, const float* enc,
                       const int64_t* enc_len, void* work, size_t work_bytes, hipStream_t st) {
    read_switches();
    if (!g_persist_fwd) return 1;
    const FwdPlan pl = fwd_plan(d);
    if (pl.kind == 2) return dec_fwd_streamed(d, w, s, enc, enc_len, work, work_bytes, st);
    if (!pl.kind || !work || work_bytes < pl.total || ((uintptr_t)work & 255) != 0 || !s.conv) return 1;
    const FwdWork wk = fwd_work(d, pl, work);
    clear_work(work, wk.xbuf_bytes, st);
    hipLaunchKernelGGL(build_wcat16_kernel, dim3(512), dim3(256), 0, st, w.Wih[0], w.Whh[0], wk.wcat16, 4 * d.Dd, d.Dd, d.E, pl.KCP);
    const int XW = d.Dd + d.E;
    GemmCall embproj{s.xin, w.Wih[0], wk.embproj, nullptr, d.B * d.L, 4 * d.Dd, d.Dd, XW, XW, 4 * d.Dd};
    embproj.prec = ASR_BF16;
    int rc = gemm_run(embproj, st);
    if (rc != ASR_OK) return rc;
    const PD p{d, w, s, enc, enc_len, wk.wcat16, wk.embproj, wk.xbuf, wk.status, pl.NT, pl.TE, pl.UPW, pl.QPW, pl.CPW, pl.HG2, pl.QG2, pl.SG2, pl.KC,
               pl.KCP, xcd_local_allowed()};
    const ClusterLaunch go{"asr_att_decoder_fwd(persistent)", 160 * 1024 - 2048, cluster_grid(d, pl.NT), dim3(64 * (NCW + NPW)), pl.lds, st};
    if (d.Kn <= 4) {
        if (pl.tpw == 2) return go.run<dec_fwd_persist<4, 2>>(p);
        if (pl.tpw == 4) return go.run<dec_fwd_persist<4, 4>>(p);
        if (pl.tpw == 5) return go.run<dec_fwd_persist<4, 5>>(p);
        return go.run<dec_fwd_persist<4, 8>>(p);
    }
    if (pl.tpw == 2) return go.run<dec_fwd_persist<10, 2>>(p);
    if (pl.tpw == 4) return go.run<dec_fwd_persist<10, 4>>(p);
    if (pl.tpw == 5) return go.run<dec_fwd_persist<10, 5>>(p);
    return 1;
}

// =================================================================================================
// Backward of the teacher-forced decoder loop as ONE persistent launch (same cluster-per-utterance scheme as the
// forward; bf16 mode, one decoder layer).  Workgroup (tile j of utterance b) keeps for all L steps
//   * in REGISTERS: its rows of [W_ih(ctx) | W_hh]^T (bf16, 8 rows x 20 columns per lane over all 8 waves), its rows of
//     W_q^T, and the accumulators the per-step kernels had to read-modify-write in HBM every step: d w_g[a], d W_proj[a,:],
//     the cell-state carry;
//   * in LDS: the key tile (bf16), W_proj (bf16, MFMA operand), W_conv;
//   * dkey is accumulated with no-return atomics (one add per address per step, issued by the same thread: deterministic).
// Every workgroup recomputes the (elementwise) cell backward of ALL hidden units from the full dh vector, so a step
// needs three all-gathers inside the cluster (tagged granules):
//   C  {dctx slice, recurrent part of dh_{t-1} for the workgroup's units}
//   Q  per-tile partial of the query gradient,  V  the tile's dconv
//   N  {the tile's gradient wrt the previous attention, query part of dh_{t-1} for the workgroup's units}
// Waves 0..ncw-1 (ncw = ceil(A/64)) compute, three more waves poll; all eight take part in the transposed-weight product.
// =================================================================================================
namespace {

// (constants, PB, the LDS carve, P1 macros, the sweep: decoder_bwd_common.h)
// TEC: frames per tile as a compile-time constant (the bench shape), 0: taken from the plan (any multiple of 4 up to 40)
template <int KNMAX, int TEC>
__global__ __launch_bounds__(512) void dec_bwd_persist(PB p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned s_bar;
    __shared__ float s_red[8];
    constexpr int KP = (KNMAX + 3) & ~3;
    const int TE = TEC ? TEC : p.TE;
    const int MT = (TE + 15) / 16;
    const asr_dec_dims_t& d = p.d;
    const int id = blockIdx.x, xcd = id & 7, slot_id = id >> 3;
    const int cb = slot_id / p.NT, j = slot_id - cb * p.NT;
    const int b = cb * 8 + xcd;
    if (b >= d.B) return;
    const unsigned epoch_ = __builtin_amdgcn_readfirstlane(p.status[EPOCH_WORD]);     // launch epoch of this work area (decoder_cluster.h)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NT = p.NT, A = d.A, E = d.E, Dd = d.Dd, Tp = d.Tp, Kn = d.Kn, Ks = d.Ks, L = d.L;
    const int ncw = (A + 63) >> 6, nct = 64 * ncw, nw = ncw + NPB;       // compute waves / threads, all waves
    const int taps = 2 * Ks + 1, XW = Dd + E, R4 = p.R4;
    const int tau0 = j * TE;
    const int len = min((int)p.enc_len[b], Tp);
    const int tmax = max(len - 1, 0);
    const BCarve cv_ = bwd_carve(TE, KP, A, E, Kn, Ks, NT, p.UPW, p.CG2, p.QG2, p.NG2);
    const int AP = cv_.AP, DW = cv_.DW, PADL = cv_.PADL, WT = cv_.WT, AQ = cv_.AQ;
    const int TW = NT * TE;                                             // padded attention row
    const int CG2f = 2 * p.CG2, NG2f = 2 * p.NG2, QG2f = 2 * p.QG2;
    // ---- LDS carve
    unsigned short* s_sh = reinterpret_cast<unsigned short*>(smem);
    unsigned short* s_key = s_sh + cv_.key;                                              // [TE/4][A][4] bf16 (four frames innermost)
    unsigned short* s_dl = s_sh + cv_.dl;                                                // [TE][AP] bf16  d loc pre-activation
    unsigned short* s_wp16 = s_sh + cv_.wp16;                                            // [16][AP] bf16  W_proj^T, zero padded
    unsigned short* s_dg16 = s_sh + cv_.dg16;                                            // [1280] bf16 dgates of the utterance
    unsigned short* s_wq16 = s_sh + cv_.wq16;                                            // [UPW][AQ] bf16 rows of W_q^T of the own units
    unsigned short* s_cvx = s_sh + cv_.cvx;                                              // [48][32] bf16 conv tile, slots {hi | lo | hi}
    unsigned short* s_cvT = s_sh + cv_.cvT;                                              // [16][CVT_LD] bf16 conv tile transposed
    float* s_f = reinterpret_cast<float*>(s_sh + cv_.shorts);
    float* s_wc = s_f + cv_.wc;                                                          // [Kn*taps]
    float* s_crec = s_f + cv_.crec;                                                      // [NT][CG2*2] records {dctx slice, dh_rec slice}
    float* s_qst = s_f + cv_.qst;                                                        // [NT][QG2*2] dq partials
    float* s_nrec = s_f + cv_.nrec;                                                      // [NT][NG2*2] records {datt_next tile, dh_q slice}
    float* s_dcp = s_f + cv_.dcp;                                                        // [Kn][DW] zero-padded dconv rows
    float* s_de = s_f + cv_.de;                                                          // [48], zero beyond TE
    float* s_out = s_f + cv_.out;                                                        // [RPWB * 8] products of P1
    float* s_hq = s_f + cv_.hq;                                                          // [UPW] query part of dh_{t-1}
    float* s_pt = s_f + cv_.pt;                                                          // [4*Kn*TE] partial sums of datt_next (tap ranges)
    float* s_dcx = s_f + cv_.dcx;                                                        // [E] dctx, contiguous
    float* s_dq = s_f + cv_.dq;                                                          // [A] dq of the utterance
    const long region = (long)NT * (p.CG2 + p.QG2 + p.VG2 + p.NG2);
    auto xb = [&](int parity) { return p.xbuf + ((long)parity * d.B + b) * region; };
    const long offC = 0, offQ = offC + (long)NT * p.CG2, offV = offQ + (long)NT * p.QG2, offN = offV + (long)NT * p.VG2;
    if (tid == 0) s_bar = 0u;
    // clear this producer's records in the L2 (see the forward kernel)
    for (int parity = 0; parity < 2; ++parity) {
        u64* base = xb(parity);
        for (int i = tid; i < p.CG2; i += blockDim.x) st_gran_local(base + offC + (long)j * p.CG2 + i, 0ull);
        for (int i = tid; i < p.QG2; i += blockDim.x) st_gran_local(base + offQ + (long)j * p.QG2 + i, 0ull);
        for (int i = tid; i < p.VG2; i += blockDim.x) st_gran_local(base + offV + (long)j * p.VG2 + i, 0ull);
        for (int i = tid; i < p.NG2; i += blockDim.x) st_gran_local(base + offN + (long)j * p.NG2 + i, 0ull);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const bool local = xcd_consensus(reinterpret_cast<u64*>(p.status) + 64 + b, NT, p.allow_local, p.status);

    // ---- resident data
    for (int i = tid; i < TE * A; i += blockDim.x) {
        const int f = i / A, a = i - f * A;
        s_key[((long)(f >> 2) * A + a) * 4 + (f & 3)] = f2bf_bits(p.s.key[((long)b * Tp + min(tau0 + f, tmax)) * A + a]);
    }
    for (int i = tid; i < 16 * AP; i += blockDim.x) { const int k = i / AP, a = i - k * AP; s_wp16[i] = (k < Kn && a < A) ? f2bf_bits(p.w.Wproj[a * Kn + k]) : (unsigned short)0; }
    for (int i = tid; i < Kn * WT; i += blockDim.x) { const int k = i / WT, jj = i - k * WT; s_wc[i] = (jj < taps) ? p.w.Wconv[k * taps + jj] : 0.f; }
    for (int i = tid; i < 64 * KCHB * 4; i += blockDim.x) s_dg16[i] = 0;
    for (int i = tid; i < NT * NG2f + 8; i += blockDim.x) s_nrec[i] = 0.f;
    for (int i = tid; i < NT * CG2f; i += blockDim.x) s_crec[i] = 0.f;
    for (int i = tid; i < Kn * DW; i += blockDim.x) s_dcp[i] = 0.f;
    for (int i = tid; i < TE * AP; i += blockDim.x) s_dl[i] = 0;
    for (int i = tid; i < 16 * SW_MT * CVX_LD; i += blockDim.x) s_cvx[i] = 0;
    for (int i = tid; i < 16 * CVT_LD; i += blockDim.x) s_cvT[i] = 0;
    for (int i = tid; i < 16 * SW_MT; i += blockDim.x) s_de[i] = 0.f;
    const int u_base = j * p.UPW, c_base = j * p.CPW;
    for (int i = tid; i < p.UPW * AQ; i += blockDim.x) {
        const int ul = i / AQ, aa = i - ul * AQ;
        s_wq16[i] = (aa < A && u_base + ul < Dd) ? f2bf_bits(p.wqT[(long)(u_base + ul) * A + aa]) : (unsigned short)0;
    }
    const int nout = p.CPW + p.UPW;
    // sweep: 16-column units over ALL waves (unit u -> wave u % nw), see sweep_step
    const int nunits = (A + 15) >> 4;
    const int nu_cnt = (nunits - wave + nw - 1) / nw;              // units of this wave (<= SW_NU by the plan)
    const int qsub = lane >> 4, csub = lane & 15;
    // rows of the transposed cell weights are register-resident: compute wave w has outputs w + ncw*o (o < RCB), polling
    // wave pw has RCB*ncw + pw + NPB*o (o < RPB)
    __syncthreads();

    if (wave >= ncw) {
        // =========================== polling role ===========================
        const int gt = tid - nct, np = 64 * NPB;
        const int vp0 = max(0, (tau0 - Ks) / TE), vp1 = min(NT - 1, (tau0 + TE - 1 + Ks) / TE);   // tiles whose dconv this tile's datt_next reads
        const int obase = RCB * ncw + (wave - ncw);
        uint2 wreg[RPB][KCHB];
        DPB_WLOAD(RPB, obase, NPB)
        Sweep<SW_NUP> S;                                                // the polling waves own at most two units (plan)
        sweep_init<KNMAX>(S, p.w.Wproj, p.w.wg, A, Kn, wave, nw, lane);
        for (int t = L - 1; t >= 0; --t) {
            const int s = L - 1 - t;                                     // step counter of this launch (tags, parity)
            const u64 want = pair_want(seq_of(s), epoch_);
            const u64* base = xb(s & 1);
            DP_JIT(6)
            __syncthreads();                                            // Ba: s_dg16 holds the gate gradients of step t
            DPB_P1(RPB, obase, NPB)
            __syncthreads();                                            // Bb: s_out complete
            poll_copy<4>(base + offC, NT * p.CG2 / 2, s_crec, gt, np, want, p.status);
            float qa[SW_NUP];
#pragma unroll
            for (int nu = 0; nu < SW_NUP; ++nu) qa[nu] = p.s.q[((long)b * L + t) * A + min(16 * (wave + nw * nu) + csub, A - 1)];
            DP_JIT(7)
            __syncthreads();                                            // H2
            DP_JIT(8)
            __syncthreads();                                            // X1: s_de, s_cvx, s_cvT complete
            DPB_SWEEP_AND_PUBLISH(const_cast<u64*>(base), SW_NUP)
            __syncthreads();                                            // X2: s_dl complete
            for (int z = 0; z < p.poll_delay; ++z) __builtin_amdgcn_s_sleep(127);
            {   // Q records of all tiles (flat copy) and the dconv tiles V of the tiles within reach of the location filter
                // (they go straight into the zero-padded per-kernel rows s_dcp[k][PADL + prod*TE + f]), as ONE polling sweep
                const int nq = NT * p.QG2 / 2, nv = (vp1 - vp0 + 1) * (p.VG2 / 2);
                const u64* vbase = base + offV + (long)vp0 * p.VG2;
                for (int i0 = gt; i0 < nq + nv; i0 += 10 * np) {
                    u64 lo[10], hi[10];
                    const u64* addr[10];
                    int cnt = 0;
#pragma unroll
                    for (int k = 0; k < 10; ++k) {
                        const int idx = i0 + k * np;
                        if (idx < nq + nv) cnt = k + 1;
                        addr[k] = (idx < nq) ? base + offQ + 2 * (long)idx : vbase + 2 * (long)min(idx - nq, nv - 1);
                    }
                    gather16v<10>(addr, cnt, PAIR_MASK, want, lo, hi, p.status);
#pragma unroll
                    for (int k = 0; k < 10; ++k)
                        if (k < cnt) {
                            const int idx = i0 + k * np;
                            const float v[4] = {lo_f(lo[k]), hi_f(lo[k]), lo_f(hi[k]), hi_f(hi[k])};
                            if (idx < nq) {
                                *reinterpret_cast<float4*>(s_qst + 4 * (long)idx) = make_float4(v[0], v[1], v[2], v[3]);
                            } else {
                                const int g0 = vp0 * p.VG2 + 2 * (idx - nq), prod = g0 / p.VG2, r0 = 2 * (g0 - prod * p.VG2);
#pragma unroll
                                for (int q4 = 0; q4 < 4; ++q4) {
                                    const int r = r0 + q4;
                                    if (r < Kn * TE) { const int kk = r / TE, f = r - kk * TE; s_dcp[kk * DW + PADL + prod * TE + f] = v[q4]; }
                                }
                            }
                        }
                }
            }
            DP_JIT(9)
            __syncthreads();                                            // H3
            DP_JIT(10)
            if (t > 0) poll_copy<4>(base + offN, NT * p.NG2 / 2, s_nrec, gt, np, want, p.status);
            __syncthreads();                                            // H4
        }
        DPB_SWEEP_RESULTS(SW_NUP, true, p.dkey, TE)
        return;
    }

    // =========================== compute role ===========================
    unsigned gen = 0;
    uint2 wreg[RCB][KCHB];
    DPB_WLOAD(RCB, wave, ncw)
    Sweep<SW_NU> S;
    sweep_init<KNMAX>(S, p.w.Wproj, p.w.wg, A, Kn, wave, nw, lane);
    const int a = tid;                                                  // attention column of this thread in the sweep
    const bool aok = a < A;
    const int ac = aok ? a : A - 1;
    const bool uok = tid < Dd;                                          // hidden unit of this thread in the cell backward
    const int uc = uok ? tid : Dd - 1;
    const int ui = uc / p.UPW, uul = uc - ui * p.UPW;                   // its producer and position in the records
    const bool uown = uok && ui == j;
    float dbg = 0.f, dc_carry = 0.f;
    // operands of the cell backward of step L-1 (later steps: requested one step ahead)
    float pgi, pgf, pgg, pgo, pct, pcp, pdh;
    {
        const long r0 = (long)b * L + (L - 1);
        const float* g = p.s.gates + r0 * 4 * Dd + uc;
        pgi = g[0]; pgf = g[Dd]; pgg = g[2 * Dd]; pgo = g[3 * Dd];
        pct = p.s.cs[r0 * Dd + uc];
        pcp = (L > 1) ? p.s.cs[(r0 - 1) * Dd + uc] : 0.f;
        pdh = p.dhs[r0 * Dd + uc];
    }
    DP_DECL

    for (int t = L - 1; t >= 0; --t) {
        // Thread-index arithmetic of the step is loop invariant; hoisted, it becomes ~100 live address registers and the
        // accumulators get spilled instead.  An opaque copy of the index ties it to the step (a few dozen VALU per step).
        int tz = tid, lz_ = lane;
        asm volatile("" : "+v"(tz), "+v"(lz_));
        const int lane = lz_;
        const int s = L - 1 - t;
        const long row = (long)b * L + t;
        const u64 want = pair_want(seq_of(s), epoch_);
        u64* out = xb(s & 1);
        DP_MARK(0)
        // ---- S1: cell backward of ALL hidden units (thread per unit; every workgroup of the cluster computes the same)
        DPB_S1(TE)
        DP_MARK(1)
        __syncthreads();                                                // Ba
        DP_MARK(2)
        // ---- P1: dctx slice and the recurrent part of dh_{t-1} for the own units
        DPB_P1(RCB, wave, ncw)
        DP_MARK(3)
        __syncthreads();                                                // Bb
        DP_MARK(4)
        // ---- C record {dctx slice | dh_rec slice} + global dxin (context part)
        if (tz < p.CG2) DPB_C_GRANULE(tz, RPWB * 8 - 1)
        // ---- operands of P2/P3 that do not depend on the hand-offs: requested now, used behind H2
        float qa[SW_NU];
#pragma unroll
        for (int nu = 0; nu < SW_NU; ++nu) qa[nu] = p.s.q[row * A + min(16 * (wave + nw * nu) + csub, A - 1)];
        const int f2 = tz >> 3, part = tz & 7;                         // P2: 8 threads per frame
        uint4 x[10];
        {
            const unsigned short* er = p.enc16 + ((long)b * Tp + min(tau0 + min(f2, TE - 1), tmax)) * E;
#pragma unroll
            for (int u = 0; u < 10; ++u) x[u] = *reinterpret_cast<const uint4*>(er + 8 * min(part + 8 * u, (E >> 3) - 1));
        }
        float ctx2[2], attv[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) ctx2[h] = p.s.xin[row * XW + Dd + min(tz + nct * h, E - 1)];
#pragma unroll
        for (int h = 0; h < 4; ++h) attv[h] = p.s.att[row * Tp + min(tz + nct * h, Tp - 1)];
        const float attf = p.s.att[row * Tp + min(tau0 + min(f2, TE - 1), Tp - 1)];
        float c0, c1;                                                   // conv tile of the step (stored to LDS behind H2)
        const int cvi0 = tz, cvi1 = tz + nct;
        const int cvk0 = min(cvi0, Kn * TE - 1) / TE, cvf0 = min(cvi0, Kn * TE - 1) - cvk0 * TE;
        const int cvk1 = min(cvi1, Kn * TE - 1) / TE, cvf1 = min(cvi1, Kn * TE - 1) - cvk1 * TE;
        c0 = p.s.conv[(row * Kn + cvk0) * Tp + min(tau0 + cvf0, Tp - 1)];
        c1 = p.s.conv[(row * Kn + cvk1) * Tp + min(tau0 + cvf1, Tp - 1)];
        DP_MARK(5)
        __syncthreads();                                                // H2: s_crec holds the C records of all workgroups
        DP_MARK(6)
        // ---- P2: dattn of the tile, dot over the utterance, de
        {
            for (int e = tz; e < E; e += nct) { const int i = e / p.CPW; s_dcx[e] = s_crec[i * CG2f + (e - i * p.CPW)]; }
            if (cvi0 < Kn * TE) put_cv<KNMAX>(s_cvx, s_cvT, cvf0, cvk0, (tau0 + cvf0 < Tp) ? c0 : 0.f);
            if (cvi1 < Kn * TE) put_cv<KNMAX>(s_cvx, s_cvT, cvf1, cvk1, (tau0 + cvf1 < Tp) ? c1 : 0.f);
            cbar(&s_bar, gen, ncw);
            float v = 0.f;
#pragma unroll
            for (int u = 0; u < 10; ++u) {
                const int ch = part + 8 * u;
                if (8 * ch < E) {
                    const float4 da = *reinterpret_cast<const float4*>(s_dcx + 8 * ch), db = *reinterpret_cast<const float4*>(s_dcx + 8 * ch + 4);
                    v += __uint_as_float(x[u].x << 16) * da.x + __uint_as_float(x[u].x & 0xffff0000u) * da.y +
                         __uint_as_float(x[u].y << 16) * da.z + __uint_as_float(x[u].y & 0xffff0000u) * da.w +
                         __uint_as_float(x[u].z << 16) * db.x + __uint_as_float(x[u].z & 0xffff0000u) * db.y +
                         __uint_as_float(x[u].w << 16) * db.z + __uint_as_float(x[u].w & 0xffff0000u) * db.w;
                }
            }
            v = sum8_dpp(v);
            float dot = 0.f;
#pragma unroll
            for (int h = 0; h < 2; ++h) if (tz + nct * h < E) dot += ctx2[h] * s_dcx[tz + nct * h];
            if (s > 0) {
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const int tau = tz + nct * h;
                    if (tau < len) { const int i = tau / TE; dot += attv[h] * s_nrec[i * NG2f + (tau - i * TE)]; }
                }
            }
            dot = wave_sum_dpp(dot);
            if (lane == 0) s_red[wave] = dot;
            cbar(&s_bar, gen, ncw);
            dot = 0.f;
            for (int w = 0; w < ncw; ++w) dot += s_red[w];
            if (f2 < TE && part == 0) {
                const int tau = tau0 + f2;
                const float dat = v + ((s > 0) ? s_nrec[j * NG2f + f2] : 0.f);
                const float dev = (tau < len) ? attf * (dat - dot) / d.temperature : 0.f;
                s_de[f2] = dev;
                dbg += dev;                                             // d b_g: per-thread partial, added to the slot at the end
            }
        }
        __syncthreads();                                                // X1: s_de, s_cvx, s_cvT complete (the polling waves join the sweep)
        DP_MARK(7)
        // ---- P3: energy backward sweep of this wave's column units + their query-gradient partials (Q record)
        DPB_SWEEP_AND_PUBLISH(out, SW_NU)
        __syncthreads();                                                // X2: s_dl complete
        DP_MARK(8)
        // ---- P4: dconv (TE x Kn) = dl (TE x A) . W_proj (A x Kn) on the matrix cores, one 16-frame tile per wave
        if (wave < MT) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const int m = lane & 15, kq = lane >> 4;
            const unsigned short* ar = s_dl + min(16 * wave + m, TE - 1) * AP + 8 * kq;
            const unsigned short* br = s_wp16 + m * AP + 8 * kq;
            const int nks = (A + 31) >> 5;
            for (int ks = 0; ks < nks; ++ks) {
                const bf16x8 av = *reinterpret_cast<const bf16x8*>(ar + 32 * ks);
                const bf16x8 bv = *reinterpret_cast<const bf16x8*>(br + 32 * ks);
                acc = mma16(av, bv, acc);
            }
            if (m < Kn) {
#pragma unroll
                for (int i = 0; i < 4; i += 2) {
                    const int f = 16 * wave + 4 * kq + i;
                    if (f < TE) {
                        const float v0 = (tau0 + f < len) ? acc[i] : 0.f, v1 = (tau0 + f + 1 < len) ? acc[i + 1] : 0.f;
                        // dconv over the saved conv (for d W_conv after the loop)
                        if (tau0 + f < Tp) p.s.conv[(row * Kn + m) * Tp + tau0 + f] = v0;
                        if (tau0 + f + 1 < Tp) p.s.conv[(row * Kn + m) * Tp + tau0 + f + 1] = v1;
                        u64* dst = out + offV + (long)j * p.VG2 + ((m * TE + f) >> 1);      // record order [k][f]
                        if (local) publish<true>(dst, pack2(v0, v1, want)); else publish<false>(dst, pack2(v0, v1, want));
                    }
                }
            }
        }
        if (tz == nct - 1 && (TE * Kn + 1) / 2 < p.VG2) {
            u64* dst = out + offV + (long)j * p.VG2 + p.VG2 - 1;
            if (local) publish<true>(dst, pack2(0.f, 0.f, want)); else publish<false>(dst, pack2(0.f, 0.f, want));
        }
        DP_MARK(9)
        __syncthreads();                                                // H3: dq partials and dconv tiles of all workgroups
        DP_MARK(10)
        // ---- P5: dq (sum over tiles), its part of dh_{t-1}, datt_next of the tile
        {
            float dqv = 0.f;
            if (aok) for (int i = 0; i < NT; ++i) dqv += s_qst[i * QG2f + a];
            if (aok) s_dq[a] = dqv;
            const int asl = (A + NT - 1) / NT;
            if (aok && a >= j * asl && a < (j + 1) * asl) p.dq[row * A + a] = dqv;     // each workgroup saves a slice
        }
        DP_MARK(13)
        if (t > 0) {
            // datt_next[tau'] = sum_k sum_j W_conv[k][j] * dconv[k][tau' - j + Ks] for the tile's frames:
            // item = (tap range, kernel, group of 4 outputs); four taps per round from three 16-byte LDS reads
            const int ngrp = TE / 4;
            const int nitem = Kn * ngrp;
            const int parts = max(1, min(4, nct / nitem));
            const int gpp = (WT / 4 + parts - 1) / parts;                 // tap groups per part
            for (int it = tz; it < parts * nitem; it += nct) {
                const int pz = it / nitem, o = it - pz * nitem, k = o / ngrp, ig = o - k * ngrp;
                const int g0 = pz * gpp, g1 = min(WT / 4, g0 + gpp);
                // 16-byte units throughout (s_wc rows, the dconv rows and PADL + Ks + tau0 are multiples of 4 floats)
                const float4* wk4 = reinterpret_cast<const float4*>(s_wc) + (k * WT) / 4;
                const float4* q4 = reinterpret_cast<const float4*>(s_dcp) + (k * DW + PADL + Ks + tau0) / 4 + ig;   // q4[0] = q[0..3]
                float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 3
                for (int g = g0; g < g1; ++g) {
                    const float4 w4 = wk4[g];
                    const float4 lo = q4[-g - 1];                       // q[-4..-1] of this tap group
                    const float4 hi = q4[-g];                           // q[0..3]
                    a0 += w4.x * hi.x + w4.y * lo.w + w4.z * lo.z + w4.w * lo.y;
                    a1 += w4.x * hi.y + w4.y * hi.x + w4.z * lo.w + w4.w * lo.z;
                    a2 += w4.x * hi.z + w4.y * hi.y + w4.z * hi.x + w4.w * lo.w;
                    a3 += w4.x * hi.w + w4.y * hi.z + w4.z * hi.y + w4.w * hi.x;
                }
                *reinterpret_cast<float4*>(s_pt + (long)(pz * Kn + k) * TE + 4 * ig) = make_float4(a0, a1, a2, a3);
            }
            DP_MARK(14)
            cbar(&s_bar, gen, ncw);                                     // s_dq, s_pt complete
            // query part of dh_{t-1}: sum_a dq[a] * W_q[a][unit] for the own units (bf16 rows in LDS)
            {
                float dqr[5];
#pragma unroll
                for (int k5 = 0; k5 < 5; ++k5) dqr[k5] = (lane + 64 * k5 < A) ? s_dq[min(lane + 64 * k5, A - 1)] : 0.f;
                for (int ul = wave; ul < p.UPW; ul += ncw) {
                    const unsigned short* wr = s_wq16 + ul * AQ + lane;
                    float acc = 0.f;
#pragma unroll
                    for (int k5 = 0; k5 < 5; ++k5) if (64 * k5 < AQ) acc += dqr[k5] * bf2f(wr[64 * k5]);
                    acc = wave_sum_dpp(acc);
                    if (lane == 0) s_hq[ul] = acc;
                }
            }
            // datt_next of the tile: the tap-range partial sums, 8 threads per frame (s_de is free after the sweep)
            {
                const int i = tz >> 3, sub = tz & 7;
                float sv = 0.f;
                if (i < TE) for (int r = sub; r < parts * Kn; r += 8) sv += s_pt[(long)r * TE + i];
                sv = sum8_dpp(sv);
                if (i < TE && sub == 0) s_de[i] = sv;
            }
            DP_MARK(15)
            cbar(&s_bar, gen, ncw);                                     // s_hq, datt_next complete
            // N record {datt_next tile | dh_q slice}
            if (tz < p.NG2) {
                float v[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int i = 2 * tz + h;
                    v[h] = (i < TE) ? s_de[i] : ((i - TE < p.UPW) ? s_hq[i - TE] : 0.f);
                }
                u64* dst = out + offN + (long)j * p.NG2 + tz;
                if (local) publish<true>(dst, pack2(v[0], v[1], want)); else publish<false>(dst, pack2(v[0], v[1], want));
            }
            // operands of the next step's cell backward (they arrive while the N records are gathered)
            const long r1 = row - 1;
            const float* g = p.s.gates + r1 * 4 * Dd + uc;
            pgi = g[0]; pgf = g[Dd]; pgg = g[2 * Dd]; pgo = g[3 * Dd];
            pct = p.s.cs[r1 * Dd + uc];
            pcp = (t > 1) ? p.s.cs[(r1 - 1) * Dd + uc] : 0.f;
            pdh = p.dhs[r1 * Dd + uc];
        }
        DP_MARK(11)
        __syncthreads();                                                // H4: s_nrec holds the N records for the next step
        DP_MARK(12)
    }
    DP_DUMP
    // ---- results that were accumulated on chip: the slot of this workgroup, the dkey tile
    DPB_SWEEP_RESULTS(SW_NU, true, p.dkey, TE)
    if (dbg != 0.f) atomicAdd(p.slots + ((long)b * NT + j) * p.slot + A * (1 + Kn), dbg);     // slots are zero on entry
}

}  // namespace

int dec_bwd_persistent(const asr_dec_dims_t& d, const asr_dec_weights_t& w, const asr_dec_state_t& s, const int64_t* enc_len,
                       const float* dhs, float* dxin, float* dq, float* dkey, float* slots, int slot, const float* wcatT, const float* wqT,
                       void* work, size_t work_bytes, float** dgates_out, hipStream_t st) {
    read_switches();
    if (!g_persist_bwd) return 1;
    const BwdPlan pl = bwd_plan(d);
    if (pl.kind == 2) return dec_bwd_streamed(d, w, s, enc_len, dhs, dxin, dq, dkey, slots, slot, wcatT, wqT, work, work_bytes, dgates_out, st);
    if (!pl.kind || !work || work_bytes < pl.total || ((uintptr_t)work & 255) != 0 || !s.conv || !s.enc16) return 1;
    const BwdWork wk = bwd_work(d, pl, work);
    *dgates_out = wk.dgates;
    clear_work(work, wk.xbuf_bytes, st);
    hipLaunchKernelGGL(cast_rows_bf16_kernel, dim3(512), dim3(256), 0, st, wcatT, wk.w16, d.Dd + d.E + d.Dd, 4 * d.Dd, pl.R4);
    const PB p{d, w, s, (const unsigned short*)s.enc16, enc_len, dhs, dxin, dq, dkey, slots, wk.dgates, wk.w16, wqT, wk.xbuf, wk.status,
               slot, pl.NT, pl.TE, pl.UPW, pl.CPW, pl.R4, pl.CG2, pl.QG2, pl.VG2, pl.NG2, xcd_local_allowed(), dec_bwd_poll_delay()};
    const ClusterLaunch go{"asr_att_decoder_bwd(persistent)", 160 * 1024 - 4096, cluster_grid(d, pl.NT), dim3(64 * (cdiv(d.A, 64) + NPB)), pl.lds, st};
    if (d.Kn <= 4) return pl.TE == 40 ? go.run<dec_bwd_persist<4, 40>>(p) : go.run<dec_bwd_persist<4, 0>>(p);
    return pl.TE == 40 ? go.run<dec_bwd_persist<10, 40>>(p) : go.run<dec_bwd_persist<10, 0>>(p);
}
