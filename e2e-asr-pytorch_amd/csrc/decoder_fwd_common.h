// Phases that the two forward cluster kernels share (dec_fwd_persist of decoder_persist.hip: tiles resident in LDS; dec_fwd_stream
// of decoder_stream.hip: tiles streamed): the producer's record clear, the H / Q slice gathers of the polling role, the sweep's
// operand fragments, the query slice, the online-softmax combine of the staged records and the LSTM cell.  What differs - how key
// and enc rows reach the sweep, the softmax statistics, the partial context - is written out in the kernel files, and so are the
// barriers and the DP_MARK / DP_JIT points between the phases (the two kernels number them differently).
// Every helper is force-inlined and takes the step's OPAQUE copies of the thread and lane index (FwdStep); none reads threadIdx:
// the loop-invariant address arithmetic would be hoisted out of the step loop again and the accumulators would spill.
#pragma once
#include "decoder_cluster.h"

namespace {

// launch-uniform values of one forward workgroup (tile j of utterance b), built once per kernel
struct FwdCl {
    const asr_dec_dims_t* d;
    const asr_dec_weights_t* w;
    const asr_dec_state_t* s;
    const unsigned short* wcat16;   // (4Dd, KCP) bf16 rows [W_ih[:, Dd:Dd+E] | W_hh | 0-pad]
    const float* embproj;           // (B*L, 4Dd)  W_ih[:, :Dd] . emb(token)
    u64* xbuf;                      // exchange records of the utterance, parity 0
    long xpar;                      // distance of the two parities in granules
    unsigned* status;
    float *s_x2, *s_q, *s_attp, *s_g, *s_stage, *s_scale;      // LDS: [2][KCP], [A], padded attention row, [4*UPW], [NT][2*SG2], [NCW][32]
    int b, j, NT, UPW, QPW, CPW, HG2, QG2, SG2, KCP;
    long offQ, offS;                // first Q / S record of a parity (the H records start at 0)
    bool local;                     // the cluster shares an XCD: L2-local publishes
    unsigned epoch_;
    __device__ __forceinline__ u64* xb(int parity) const { return xbuf + parity * xpar; }
};
template <class P>
__device__ __forceinline__ FwdCl fwd_cl(const P& p, int b, int j, float* s_x2, float* s_q, float* s_attp, float* s_g, float* s_stage, float* s_scale, unsigned epoch_) {
    const long region = (long)p.NT * (p.HG2 + p.QG2 + p.SG2);
    return FwdCl{&p.d, &p.w, &p.s, p.wcat16, p.embproj, p.xbuf + (long)b * region, (long)p.d.B * region, p.status, s_x2, s_q, s_attp, s_g, s_stage, s_scale,
                 b, j, p.NT, p.UPW, p.QPW, p.CPW, p.HG2, p.QG2, p.SG2, p.KCP, (long)p.NT * p.HG2, (long)p.NT * (p.HG2 + p.QG2), false, epoch_};
}
// what a compute wave knows of step t: s_x = [ctx_t | h_{t-1}] of the step's parity, the records it publishes into, its tag, and the
// opaque index copies
struct FwdStep {
    int t;
    long row;                       // b * L + t
    float* s_x;
    u64* out;
    u64 want;
    int wave, lane, tz;
};

__device__ __forceinline__ void publish_gran(bool local, u64* dst, u64 v) { if (local) publish<true>(dst, v); else publish<false>(dst, v); }

// The host memset reaches memory, but granules that an earlier launch stored L2-locally (sc0) can still sit in this
// XCD's L2 with perfectly valid tags (observed: wrong data in the first step after a launch with other inputs; a
// write-through `sc1` store of zeros did NOT displace the resident copy).  Every producer therefore clears its own
// records with the same L2-local store flavour before it joins the consensus - the barrier behind which polling starts.
__device__ __forceinline__ void clear_own_records(const FwdCl& c, int tid, int nthr) {
    for (int parity = 0; parity < 2; ++parity) {
        u64* base = c.xb(parity);
        for (int i = tid; i < c.HG2; i += nthr) st_gran_local(base + (long)c.j * c.HG2 + i, 0ull);
        for (int i = tid; i < c.QG2; i += nthr) st_gran_local(base + c.offQ + (long)c.j * c.QG2 + i, 0ull);
        for (int i = tid; i < c.SG2; i += nthr) st_gran_local(base + c.offS + (long)c.j * c.SG2 + i, 0ull);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// polling role: the NT producers' slices of PW values (G2 granules each) -> dst[prod * PW + i], i < PW, below `limit`
__device__ __forceinline__ void poll_slices(const FwdCl& c, const u64* src, int G2, int PW, int limit, float* dst, u64 want, int gt, int np) {
    for (int i0 = gt; 2 * i0 < c.NT * G2; i0 += np) {
        u64 lo[1], hi[1];
        gather16<1>(src + 2 * i0, 0, 1, PAIR_MASK, want, lo, hi, c.status);
        const int g0 = 2 * i0, prod = g0 / G2, gi = g0 - prod * G2;
        const int u = prod * PW + 2 * gi;             // values 2gi, 2gi+1 (lo), 2gi+2, 2gi+3 (hi) of producer prod
        const float v[4] = {lo_f(lo[0]), hi_f(lo[0]), lo_f(hi[0]), hi_f(hi[0])};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (2 * gi + k < PW && u + k < limit) dst[u + k] = v[k];
    }
}
// H: h_{t-1} of the utterance -> s_x2[parity of t][E ..]
__device__ __forceinline__ void poll_h(const FwdCl& c, int t, int gt, int np) {
    poll_slices(c, c.xb((t - 1) & 1), c.HG2, c.UPW, c.d->Dd, c.s_x2 + (t & 1) * c.KCP + c.d->E, pair_want(seq_of(t - 1), c.epoch_), gt, np);
}
// Q: query of step t -> s_q
__device__ __forceinline__ void poll_q(const FwdCl& c, int t, int gt, int np) {
    poll_slices(c, c.xb(t & 1) + c.offQ, c.QG2, c.QPW, c.d->A, c.s_q, pair_want(seq_of(t), c.epoch_), gt, np);
}
// S: softmax records of all tiles -> s_stage (flat copy)
__device__ __forceinline__ void poll_s(const FwdCl& c, int t, int gt, int np) {
    poll_copy<10>(c.xb(t & 1) + c.offS, c.NT * c.SG2 / 2, c.s_stage, gt, np, pair_want(seq_of(t), c.epoch_), c.status);
}

// sweep operands of this wave's column units (registers): W_proj(a, :) in the {hi, hi, lo} K slots, w_g(a)
template <int KNMAX>
__device__ __forceinline__ void sweep_operands(const FwdCl& c, int wave, int lane, bf16x8 (&wpx)[FSW_NU], float (&wgu)[FSW_NU]) {
    const int A = c.d->A, Kn = c.d->Kn;
    const int q = lane >> 4, cl = lane & 15;
#pragma unroll
    for (int nu = 0; nu < FSW_NU; ++nu) {
        const int a = 16 * (wave + NCW * nu) + cl;
        const bool ok = a < A;
        const float* wr = c.w->Wproj + (long)min(a, A - 1) * Kn;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int slot = 8 * q + i;
            const int k = slot < KNMAX ? slot : (slot < 2 * KNMAX ? slot - KNMAX : slot - 2 * KNMAX);
            const float w = (ok && slot < 3 * KNMAX && k < Kn) ? wr[min(k, Kn - 1)] : 0.f;
            const __bf16 hi = (__bf16)w;
            wpx[nu][i] = (slot < 2 * KNMAX) ? hi : (__bf16)(w - (float)hi);
        }
        wgu[nu] = ok ? c.w->wg[min(a, A - 1)] : 0.f;
    }
}

// operand of the cell phase that does not depend on the step's hand-offs (requested at the step's start): lane r of the wave gets
// embproj + both biases of its gate row
__device__ __forceinline__ float cell_add_r(const FwdCl& c, const FwdStep& st, int RPW) {
    const int Dd = c.d->Dd;
    const int r = st.wave * RPW + st.lane;
    float add_r = 0.f;
    if (st.lane < RPW && r < 4 * c.UPW) {
        const int g = r / c.UPW, ul = r - g * c.UPW, unit = c.j * c.UPW + ul;
        if (unit < Dd) {
            const int grow = g * Dd + unit;
            add_r = c.embproj[st.row * 4 * Dd + grow] + c.w->bih[0][grow] + c.w->bhh[0][grow];
        }
    }
    return add_r;
}

// W_q rows and biases of the first QR query rounds of a wave, register-resident for the whole launch (none for QR = 0)
template <int QR> struct QRows { float w0[QR][5], w1[QR][5], b0[QR], b1[QR]; };
template <> struct QRows<0> {};
template <int QR>
__device__ __forceinline__ void query_rows_load(const FwdCl& c, int wave, int lane, QRows<QR>& qr) {
    const int A = c.d->A, Dd = c.d->Dd, q_base = c.j * c.QPW;
#pragma unroll
    for (int r2 = 0; r2 < QR; ++r2) {
        const int o0 = 2 * wave + 2 * NCW * r2;
        const int a0 = min(q_base + o0, A - 1), a1 = min(q_base + o0 + 1, A - 1);
        qr.b0[r2] = c.w->bq[a0]; qr.b1[r2] = c.w->bq[a1];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int kk = min(lane + 64 * k, Dd - 1);
            qr.w0[r2][k] = c.w->Wq[(long)a0 * Dd + kk];
            qr.w1[r2][k] = c.w->Wq[(long)a1 * Dd + kk];
        }
    }
}

// query slice: outputs q_base + o, two per wave per round, lanes over the reduction, and their publish.  The rounds below QR take
// W_q rows and bias from registers (no L2 round trip on the step's critical path; a bias load inside the lane-0 branch would be a
// round trip per round), the others load them per round.
template <int QR>
__device__ __forceinline__ void query_slice(const FwdCl& c, const FwdStep& st, const QRows<QR>& qr) {
    const int A = c.d->A, E = c.d->E, Dd = c.d->Dd, q_base = c.j * c.QPW;
    const int lane = st.lane;
    const float* Wq = c.w->Wq;
    for (int o0 = 2 * st.wave, rd = 0; o0 < c.QPW; o0 += 2 * NCW, ++rd) {
        float acc0 = 0.f, acc1 = 0.f;
        const int a0 = min(q_base + o0, A - 1), a1 = min(q_base + o0 + 1, A - 1);
        bool res = false;                                            // a register-resident round
        if constexpr (QR > 0) res = rd < QR;
        float b0 = 0.f, b1 = 0.f;
        if (res) {
            if constexpr (QR > 0) {
#pragma unroll
                for (int r2 = 0; r2 < QR; ++r2) if (r2 == rd) { b0 = qr.b0[r2]; b1 = qr.b1[r2]; }
            }
        } else {
            b0 = c.w->bq[a0]; b1 = c.w->bq[a1];
        }
        if (st.t > 0) {
            float w0[5], w1[5];
            if (res) {
                if constexpr (QR > 0) {
#pragma unroll
                    for (int r2 = 0; r2 < QR; ++r2)
                        if (r2 == rd) {
#pragma unroll
                            for (int k = 0; k < 5; ++k) { w0[k] = qr.w0[r2][k]; w1[k] = qr.w1[r2][k]; }
                        }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const int kk = min(lane + 64 * k, Dd - 1);
                    w0[k] = Wq[(long)a0 * Dd + kk];
                    w1[k] = Wq[(long)a1 * Dd + kk];
                }
            }
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const float hv = (lane + 64 * k < Dd) ? st.s_x[E + lane + 64 * k] : 0.f;
                acc0 += w0[k] * hv; acc1 += w1[k] * hv;
            }
            for (int kk = lane + 320; kk < Dd; kk += 64) { const float hv = st.s_x[E + kk]; acc0 += Wq[(long)a0 * Dd + kk] * hv; acc1 += Wq[(long)a1 * Dd + kk] * hv; }
            acc0 = wave_sum_dpp(acc0); acc1 = wave_sum_dpp(acc1);
        }
        if (lane == 0) {
            const float q0 = tanh_f(acc0 + b0), q1 = tanh_f(acc1 + b1);
            publish_gran(c.local, st.out + c.offQ + (long)c.j * c.QG2 + (o0 >> 1), pack2(q0, q1, st.want));      // the hop first
            if (q_base + o0 < A) c.s->q[st.row * A + q_base + o0] = q0;
            if (o0 + 1 < c.QPW && q_base + o0 + 1 < A) c.s->q[st.row * A + q_base + o0 + 1] = q1;
        }
    }
    // pad granule of an odd record length (the gather reads 16-byte pairs)
    if (st.tz == 0 && (c.QPW + 1) / 2 < c.QG2) publish_gran(c.local, st.out + c.offQ + (long)c.j * c.QG2 + c.QG2 - 1, pack2(0.f, 0.f, st.want));
}

// attention row and context of the utterance: online-softmax combine of the staged records {e[TE], m, s, ctx_partial[E] as halves}
// of the NT tiles of TE frames -> s_attp, s_x[0 .. E), the saved att and xin of the own tile / columns
__device__ __forceinline__ void combine_records(const FwdCl& c, const FwdStep& st, int TE) {
    const int E = c.d->E, Dd = c.d->Dd, Tp = c.d->Tp, Ks = c.d->Ks, NT = c.NT;
    const int SG2f = 2 * c.SG2, XW = Dd + E, c_base = c.j * c.CPW;            // floats per staged record
    const int lane = st.lane;
    float* s_scale = c.s_scale + 32 * st.wave;
    float mi = NEG_BIG, si = 0.f;
    if (lane < NT) { mi = c.s_stage[lane * SG2f + TE]; si = c.s_stage[lane * SG2f + TE + 1]; }
    const float M = wave_max_dpp(mi);
    const float wi = (lane < NT) ? si * __expf(mi - M) : 0.f;
    const float S = fmaxf(wave_sum_dpp(wi), 1e-30f);
    const float invS = 1.f / S;
    if (lane < 32) s_scale[lane] = (lane < NT) ? __expf(mi - M) * invS : 0.f;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    for (int tau = st.tz; tau < Tp; tau += 64 * NCW) {
        const int i = tau / TE, f = tau - i * TE;
        const float ev = c.s_stage[i * SG2f + f];
        const float av = (ev > 0.5f * NEG_BIG) ? __expf(ev - M) * invS : 0.f;
        c.s_attp[Ks + tau] = av;
        if (i == c.j) c.s->att[st.row * Tp + tau] = av;
    }
    for (int c2_ = st.tz; 2 * c2_ < E; c2_ += 64 * NCW) {           // two columns per staged word (halves, pack4h)
        float a0 = 0.f, a1 = 0.f;
        for (int i = 0; i < NT; ++i) {
            const unsigned w_ = __float_as_uint(c.s_stage[i * SG2f + TE + 2 + c2_]);
            a0 += h2f_lo(w_) * s_scale[i]; a1 += h2f_hi(w_) * s_scale[i];
        }
        const int cc = 2 * c2_;
        st.s_x[cc] = a0; st.s_x[cc + 1] = a1;
        if (cc >= c_base && cc < c_base + c.CPW) c.s->xin[st.row * XW + Dd + cc] = a0;
        if (cc + 1 >= c_base && cc + 1 < c_base + c.CPW) c.s->xin[st.row * XW + Dd + cc + 1] = a1;
    }
}

// LSTM cell, gate pre-activations: gate rows r = g*UPW + ul of this workgroup, RPW rows per wave, lanes over 16-byte chunks of the
// bf16 rows [W_ih(ctx part) | W_hh] streamed from L2, RB rows per batch of loads - each batch is one exposed L2 round trip.
//   dec_fwd_persist, RB = 10: the 10 rows per wave of the bench shape (80 rows, 8 waves) are ONE round trip, not two.  The phase stays
//     near the L2's bandwidth: 32 workgroups per XCD x 151 KB of rows per step.  Keeping rows in registers across all twelve waves
//     was tried (round 3): the 168-register budget holds 40 of the 80 rows without spilling (4 per polling wave beside its 10-wide
//     polls, 3 per compute wave); cell rows 2.3 -> 1.9 us, but the compute waves' other phases lost as much (stats + ctx 1.2 ->
//     1.8 us) - not adopted.
//   dec_fwd_stream, RB = 8: 38 rows per wave at config 5 are 5 batches, not 8.
template <int RB>
__device__ __forceinline__ void cell_rows(const FwdCl& c, const FwdStep& st, int RPW, float add_r) {
    const int Dd = c.d->Dd, u_base = c.j * c.UPW;
    const int wave = st.wave, lane = st.lane;
    const int nchunk = c.KCP >> 3;
    float mine = 0.f;
#pragma unroll 1
    for (int bt = 0; bt * RB < RPW; ++bt) {
        float part[RB];
#pragma unroll
        for (int rr = 0; rr < RB; ++rr) part[rr] = 0.f;
        for (int ch0 = lane; ch0 < nchunk; ch0 += 128) {
            uint4 wv[RB][2];
#pragma unroll
            for (int rr = 0; rr < RB; ++rr) {
                const int r = min(wave * RPW + bt * RB + rr, 4 * c.UPW - 1);
                const int g = r / c.UPW, ul = r - g * c.UPW;
                const long grow = (long)g * Dd + min(u_base + ul, Dd - 1);
                const unsigned short* wr = c.wcat16 + grow * c.KCP;
                wv[rr][0] = *reinterpret_cast<const uint4*>(wr + 8 * ch0);                                 // in range by the loop condition
                wv[rr][1] = *reinterpret_cast<const uint4*>(wr + 8 * min(ch0 + 64, nchunk - 1));           // clamped, used if in range
            }
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                const int ch = ch0 + 64 * h2;
                if (ch < nchunk) {
                    const float4 xa = *reinterpret_cast<const float4*>(st.s_x + 8 * ch);
                    const float4 xb4 = *reinterpret_cast<const float4*>(st.s_x + 8 * ch + 4);
#pragma unroll
                    for (int rr = 0; rr < RB; ++rr) {
                        const uint4 w4 = wv[rr][h2];
                        part[rr] += __uint_as_float(w4.x << 16) * xa.x + __uint_as_float(w4.x & 0xffff0000u) * xa.y +
                                    __uint_as_float(w4.y << 16) * xa.z + __uint_as_float(w4.y & 0xffff0000u) * xa.w +
                                    __uint_as_float(w4.z << 16) * xb4.x + __uint_as_float(w4.z & 0xffff0000u) * xb4.y +
                                    __uint_as_float(w4.w << 16) * xb4.z + __uint_as_float(w4.w & 0xffff0000u) * xb4.w;
                    }
                }
            }
        }
#pragma unroll
        for (int rr = 0; rr < RB; ++rr) {
            const float sv = wave_sum_dpp(part[rr]);
            if (lane == bt * RB + rr) mine = sv;
        }
    }
    const int r = wave * RPW + lane;
    if (lane < RPW && r < 4 * c.UPW) c.s_g[r] = mine + add_r;
}

// LSTM cell, update of unit u_base + ul by one thread (it keeps the unit's cell state), and the publish of h_t.  TWO_WAVES false:
// UPW <= 64, ul = the lane of wave 0 (dec_fwd_persist); true: UPW <= 128, ul = the thread index over waves 0 and 1 (dec_fwd_stream).
// The other waves leave before the shuffle below: st.wave is wave-uniform, so a wave leaves or stays as a whole.  The hop starts at the publish: the activations use the fast exp /
// rcp forms (1 - 2 ulp) and the granule leaves BEFORE the six stores of the step's saved state (one in-order vector-memory queue
// per wave).  The pairs of a granule never straddle a wave (64 is even).
template <bool TWO_WAVES>
__device__ __forceinline__ void cell_update(const FwdCl& c, const FwdStep& st, float& c_state) {
    if (st.wave >= (TWO_WAVES ? 2 : 1)) return;
    const int ul = TWO_WAVES ? st.tz : st.lane;
    const int Dd = c.d->Dd, unit = c.j * c.UPW + ul;
    const bool uok = ul < c.UPW && unit < Dd;
    float hv = 0.f;
    float ai = 0.f, af = 0.f, ag = 0.f, ao = 0.f;
    if (uok) {
        ai = sigm_f(c.s_g[ul]); af = sigm_f(c.s_g[c.UPW + ul]);
        ag = tanh_f(c.s_g[2 * c.UPW + ul]); ao = sigm_f(c.s_g[3 * c.UPW + ul]);
        c_state = af * c_state + ai * ag;
        hv = ao * tanh_f(c_state);
    }
    const float hn = __shfl_down(hv, 1);
    if (st.t + 1 < c.d->L && (ul & 1) == 0 && ul < 2 * c.HG2) publish_gran(c.local, st.out + (long)c.j * c.HG2 + (ul >> 1), pack2(hv, hn, st.want));
    if (uok) {
        float* go = c.s->gates + st.row * 4 * Dd;
        go[unit] = ai; go[Dd + unit] = af; go[2 * Dd + unit] = ag; go[3 * Dd + unit] = ao;
        c.s->cs[st.row * Dd + unit] = c_state;
        c.s->hs[st.row * Dd + unit] = hv;
    }
}

}  // namespace
