// Second-generation persistent LSTM recurrence for the encoder's working point: bf16 matrix-core operands,
// B <= 16 rows (one MFMA tile), H a multiple of 16.  One launch walks all T steps of both directions
// (nn.LSTM recurrence + its BPTT, reference src/module.py:1023,1049).
//
// What changed against lstm_persist.hip (which stays for fp32 parity mode, B > 16 and odd shapes):
//  * finer cut: workgroup (p, dir) owns 16 hidden units (P = H/16 workgroups per direction), so the serial
//    part of a step (MFMA chain, activations) is 4x shorter and the resident W_hh slice fits in VGPRs
//    (v1 kept 160 registers of weights in AGPRs and copied 4 of them back before every MFMA);
//  * forward: wave g computes gate g (i,f,g,o) for the 16 units: 10 MFMAs at H=320, 4 activations per lane;
//    the gates meet in LDS and wave 0 does the cell update;
//  * the MFMA is issued with the weights as the A operand, so a lane's four accumulator registers are four
//    CONSECUTIVE hidden units of one batch row: every bulk load/store is a 16-byte access and granules pack
//    adjacent units without lane shuffles;
//  * denser granules, the tag costs no payload: forward packs four bf16 h per 8-byte granule and keeps a 2-bit
//    sequence number in bit 14 of the first two (|h| <= 1, so that exponent bit is always 0); backward packs
//    two fp32 partial sums per granule with the sequence number in their mantissa LSBs (2^-23 relative,
//    far below the bf16 operand rounding).  Sequence = ((step >> 1) mod 3) + 1: consecutive occupants of a
//    parity buffer differ, and the memset state 0 is never valid;
//  * wave specialisation: four waves per workgroup do nothing but poll granules into LDS, four compute, publish
//    and move the bulk traffic (saved gates / c / y stores, operand prefetch three steps ahead).  vmcnt retires
//    in issue order, so a poll that shares a wave with bulk stores is not seen before those have completed.
// Hand-off, bounded spins and the abort word are as in lstm_persist.hip (guide form R2).
// The phases this file shares with lstm_persist3.hip (forward gather, granule packing, coefficients and cell backward, partial
// products, the NKS / NTO class lists) are stated once in lstm_persist_common.h.
#include "common.h"
#include <stdlib.h>
#include "handoff.h"
#include "lstm_persist_common.h"
#include "lstm_plan.h"

namespace {

struct P2 {
    float* gates;        // (B,T,ND,4H)
    const float* whh;    // (ND,4H,H)
    const float* bias2;  // fwd: (ND,4H) or null
    float* y;            // fwd: h out (B,T,ND*H);  bwd: dy in
    float* c;            // (B,T,ND,H)
    u64* xbuf;
    unsigned* abort_flag;
    int B, T, H, ND, P;
    int allow_local;     // 1: use XCD-local hand-offs when all workgroups of a direction share an XCD
    int poll_delay;      // the polling waves sleep this many x 128 clocks at the start of a step, while nothing can have been published yet
    unsigned epoch;      // launch counter (tag bits)
};
// units of s_sleep(2) = 128 clocks: the first polling round of a step is started roughly when the producers' stores of that
// step become visible (a round started earlier returns stale data and costs a full round trip, ~0.6 us under this traffic)
#define POLL_DELAY_FWD 12
#define POLL_DELAY_BWD 8

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// Workgroup (p, dir): hidden units u0 = 16p .. 16p+15, 8 waves in two roles:
//   waves 0-3 (compute): wave g = gate g.  MFMA D[row = unit 4q+r][col = b = n] = sum_k W_hh[g*H + u0 + row][k] * h_{t-1}[b][k];
//                        wave 0 also does the cell update and publishes h_t; all bulk global traffic lives here;
//   waves 4-7 (gather):  poll the h_{t-1} granules of all workgroups into the LDS operand tile.  Their vector-memory
//                        queue holds nothing but polls: vmcnt retires in issue order, so a poll issued behind bulk
//                        stores / prefetches would not be seen before those have completed (measured: +1 us per step).
// Exchange buffer xbuf[parity][dir][b][H/4].
__host__ __device__ __forceinline__ long fwd_region(int B, int H) { return (long)B * (H >> 2); }   // granules per (parity, direction)
// tag of a granule: FWD_MASK / fwd_want (lstm_persist_common.h)

template <int NKS>
__global__ __launch_bounds__(512) void lstm_fwd_p2(P2 p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int H = p.H, T = p.T, ND = p.ND, B = p.B;
    if ((int)(blockIdx.x & 7) >= ND) return;
    const int d = blockIdx.x & 7, u0 = (blockIdx.x >> 3) * 16;
    const int tid = threadIdx.x;
    constexpr int LD = NKS * 32 + 8;                         // bf16 elements per operand-tile row (16-byte pad)
    constexpr int CH = (NKS + 3) / 4;                        // 16-byte granule pairs per gather thread: 16 rows * (H/8) / 256
    __bf16* tiles = reinterpret_cast<__bf16*>(smem);         // [2][16][LD]  h_{t-1}, double buffered
    float* gbuf = reinterpret_cast<float*>(smem + 2 * 16 * LD * 2);   // [4][16][20] activated gates of this step
    for (int i = tid; i < 2 * 16 * LD / 2; i += 512) reinterpret_cast<unsigned*>(smem)[i] = 0u;
    const int HG = H >> 2, total = B * HG;
    const long xregion = fwd_region(B, H);               // granules per (parity, direction)
    // granules that an earlier launch stored L2-locally can still sit in this XCD's L2 with valid tags although the host
    // memset has cleared memory: every producer clears its own granules with L2-local stores before it joins the
    // consensus, which is the barrier behind which polling starts (see decoder_persist.hip)
    for (int i = tid; i < 2 * B * 4; i += 512) {
        const int parity = i / (B * 4), r = i - parity * (B * 4), bb = r >> 2, qq = r & 3;
        if ((u0 >> 2) + qq < HG) st_gran_local(p.xbuf + ((long)parity * ND + d) * xregion + (long)bb * HG + (u0 >> 2) + qq, 0ull);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const bool local = xcd_consensus(reinterpret_cast<u64*>(p.abort_flag) + 24 + d, p.P, p.allow_local, p.abort_flag);

    if (tid >= 256) {
        // ---- gather role ----
        const int gt = tid - 256;
        int slot_off[CH];
        const int cnt = fwd_gather_slots<CH>(slot_off, gt, B, HG >> 1, LD);
        LSTM_DIAG_DECL
        for (int s = 0; s < T; ++s) {
            __bf16* tile = tiles + (s & 1) * 16 * LD;
            if (s > 0 && cnt > 0) {
                u64 glo[CH], ghi[CH];
                const u64* src = p.xbuf + ((long)((s - 1) & 1) * ND + d) * xregion + 2 * gt;
                const int sp = fwd_gather_poll<CH>(src, cnt, p.poll_delay, fwd_want(seq_of(s - 1), p.epoch), glo, ghi, p.abort_flag);
                LSTM_DIAG_MARK(0)
                LSTM_DIAG_COUNT(7, sp)
                fwd_gather_store<CH>(tile, slot_off, glo, ghi);
            }
            LSTM_DIAG_MARK(1)
            __syncthreads();
            LSTM_DIAG_MARK(2)
            __syncthreads();
            LSTM_DIAG_MARK(3)
        }
        LSTM_DIAG_DUMP(256, 10)
        return;
    }

    // ---- compute role ----
    const int lane = tid & 63, g = tid >> 6;
    const int n = lane & 15, q = lane >> 4;
    bf16x8 w[NKS];
    {
        const float* wrow = p.whh + ((long)d * 4 * H + (long)g * H + u0 + n) * H;
        float wf[NKS][8];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) wf[ks][e] = wrow[min(ks * 32 + 8 * q + e, H - 1)];      // all loads in flight
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) w[ks][e] = (__bf16)((ks * 32 + 8 * q + e < H) ? wf[ks][e] : 0.f);
    }
    float bias[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[r] = p.bias2 ? p.bias2[(long)d * 4 * H + (long)g * H + u0 + 4 * q + r] : 0.f;

    const bool bok = n < B;
    const int bc = bok ? n : 0;
    const long g_ts = (long)ND * 4 * H, c_ts = (long)ND * H;
    float* gs_base = p.gates + ((long)bc * T * ND + d) * 4 * H + (long)g * H + u0 + 4 * q;
    const long cy_off = ((long)bc * T * ND + d) * H + u0 + 4 * q;
    auto tix = [&](int s_) { return (d == 0) ? s_ : T - 1 - s_; };
    auto ldx = [&](int s_) -> float4 {
#ifndef ASR_NOIO
        if (s_ < T && bok) return *reinterpret_cast<const float4*>(gs_base + (long)tix(s_) * g_ts);
#endif
        return make_float4(0.f, 0.f, 0.f, 0.f);
    };
    float4 xgA = ldx(0), xgB = ldx(1), xgC = ldx(2);
    float4 cst = make_float4(0.f, 0.f, 0.f, 0.f);
    LSTM_DIAG_DECL

    for (int s = 0; s < T; ++s) {
        const long t = tix(s);
        const __bf16* tile = tiles + (s & 1) * 16 * LD;
        LSTM_DIAG_MARK(7)
        __syncthreads();                         // h_{t-1} tile complete
        LSTM_DIAG_MARK(0)
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (s > 0) {
            bf16x8 hb[NKS];
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) hb[ks] = *reinterpret_cast<const bf16x8*>(tile + n * LD + ks * 32 + 8 * q);
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) acc = mma16(w[ks], hb[ks], acc);
        }
        float a[4];
        const float xr[4] = {xgA.x, xgA.y, xgA.z, xgA.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float pre = acc[r] + xr[r] + bias[r];
            a[r] = (g == 2) ? tanh_f(pre) : sigm_f(pre);
        }
        const float4 o_gate = make_float4(a[0], a[1], a[2], a[3]);
        *reinterpret_cast<float4*>(gbuf + (g * 16 + n) * 20 + 4 * q) = o_gate;
        LSTM_DIAG_MARK(1)
        __syncthreads();                         // the four gates of this step are in LDS
        LSTM_DIAG_MARK(2)
        if (g == 0) {
            const float4 gi = *reinterpret_cast<const float4*>(gbuf + (0 * 16 + n) * 20 + 4 * q);
            const float4 gf = *reinterpret_cast<const float4*>(gbuf + (1 * 16 + n) * 20 + 4 * q);
            const float4 gg = *reinterpret_cast<const float4*>(gbuf + (2 * 16 + n) * 20 + 4 * q);
            const float4 go = *reinterpret_cast<const float4*>(gbuf + (3 * 16 + n) * 20 + 4 * q);
            cst.x = gf.x * cst.x + gi.x * gg.x; cst.y = gf.y * cst.y + gi.y * gg.y;
            cst.z = gf.z * cst.z + gi.z * gg.z; cst.w = gf.w * cst.w + gi.w * gg.w;
            const float4 o_h = make_float4(go.x * tanh_f(cst.x), go.y * tanh_f(cst.y), go.z * tanh_f(cst.z), go.w * tanh_f(cst.w));
            if (s + 1 < T && bok) {
                const u64 v = h_granule(h_bits(o_h.x), h_bits(o_h.y), h_bits(o_h.z), h_bits(o_h.w));
                u64* dst = p.xbuf + ((long)(s & 1) * ND + d) * xregion + n * HG + (u0 >> 2) + q;
                if (local) publish<true>(dst, v | fwd_want(seq_of(s), p.epoch));
                else publish<false>(dst, v | fwd_want(seq_of(s), p.epoch));
            }
#ifndef ASR_NOIO
            if (bok) {
                *reinterpret_cast<float4*>(p.c + cy_off + t * c_ts) = cst;
                *reinterpret_cast<float4*>(p.y + cy_off + t * c_ts) = o_h;
            }
#endif
        }
        LSTM_DIAG_MARK(3)
        // saved activated gate (for BPTT) and the input-projection operand three steps ahead
#ifndef ASR_NOIO
        if (bok) *reinterpret_cast<float4*>(gs_base + t * g_ts) = o_gate;
#endif
        xgA = xgB; xgB = xgC; xgC = ldx(s + 3);
        LSTM_DIAG_MARK(4)
    }
    LSTM_DIAG_DUMP(0, 2)
}

// ------------------------------------------------------------------------------------------------
// backward (BPTT), reduce-scatter form
// ------------------------------------------------------------------------------------------------
// Workgroup (me, dir) owns units j0 = 16*me .. +15: it turns their dh into the four gate-pre-activation
// gradients (K = 64 reduction index nl = g*16 + jl) and multiplies by its W_hh rows: a PARTIAL dh_{t-1}[b, all H].
// MFMA D[row = k' unit 4q+r of output tile][col = b = n].  Output tile tcol (16 units) belongs to workgroup tcol.
// Waves 0-3: cell backward, MFMA, publish, bulk traffic.  Waves 4-7: poll and sum the producers' partials
// (wave 4+k sums producers [k*NTO, (k+1)*NTO)).
// Exchange buffer xbuf[parity][dir][consumer][producer][b][8 pairs of fp32].
// tag of a granule: BWD_MASK / bwd_want (lstm_persist_common.h)

template <int NTO>
__global__ __launch_bounds__(512) void lstm_bwd_p2(P2 p) {
    __shared__ __attribute__((aligned(16))) __bf16 tile[16 * 72];     // [b][64 + 8] dgates of this slice
    __shared__ __attribute__((aligned(16))) float s_part[4 * 256];   // [producer group][b][16]
    const int H = p.H, T = p.T, ND = p.ND, B = p.B, P = p.P;
    if ((int)(blockIdx.x & 7) >= ND) return;
    const int d = blockIdx.x & 7, me = blockIdx.x >> 3, j0 = me * 16;
    const int tid = threadIdx.x;
    constexpr int LD = 72;
    for (int i = tid; i < 16 * LD / 2; i += 512) reinterpret_cast<unsigned*>(tile)[i] = 0u;
    const long per_par = (long)ND * P * P * B * 8;
    // clear this producer's granules in the L2 (see lstm_fwd_p2): [parity][dir][consumer][me][b][8]
    for (int i = tid; i < 2 * P * B * 8; i += 512) {
        const int parity = i / (P * B * 8), r = i - parity * (P * B * 8), pc = r / (B * 8), rr = r - pc * (B * 8);
        st_gran_local(p.xbuf + (long)parity * per_par + (long)d * P * P * B * 8 + (((long)pc * P + me) * B * 8) + rr, 0ull);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const bool local = xcd_consensus(reinterpret_cast<u64*>(p.abort_flag) + 24 + d, P, p.allow_local, p.abort_flag);

    if (tid >= 256) {
        // ---- gather role: (row gb, unit quad g4) x producer group gq (NTO = ceil(P/4) producers each) ----
        const int gt = tid - 256;
        const int gslot = gt & 63, gb = gslot >> 2, g4 = gslot & 3, gq = gt >> 6;
        const int pp_lo = gq * NTO, cntp = max(0, min(P - pp_lo, NTO));
        LSTM_DIAG_DECL
        for (int s = 0; s < T; ++s) {
            if (s > 0) {
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gb < B && cntp > 0) {
                    for (int z = 0; z < p.poll_delay; ++z) __builtin_amdgcn_s_sleep(2);
                    const u64* src = p.xbuf + (long)((s - 1) & 1) * per_par + (((long)d * P + me) * P + pp_lo) * B * 8 + gb * 8 + 2 * g4;
                    u64 glo[NTO], ghi[NTO];
                    gather16<NTO>(src, (long)B * 8, cntp, BWD_MASK, bwd_want(seq_of(s - 1), p.epoch), glo, ghi, p.abort_flag);
                    a = bwd_sum_partials<NTO>(glo, ghi, cntp);
                }
                LSTM_DIAG_MARK(0)
                *reinterpret_cast<float4*>(s_part + gq * 256 + gb * 16 + 4 * g4) = a;
            }
            LSTM_DIAG_MARK(1)
            __syncthreads();
            LSTM_DIAG_MARK(2)
            __syncthreads();
            LSTM_DIAG_MARK(3)
        }
        LSTM_DIAG_DUMP(256, 10)
        return;
    }

    // ---- compute role ----
    const int lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, q = lane >> 4;
    // resident weights, A operand: row = output unit kp = 16*tcol + n, k = nl = 32*ks + 8q + e
    bf16x8 w[NTO][2];
    {
        float wf[NTO][2][8];
#pragma unroll
        for (int ot = 0; ot < NTO; ++ot) {
            const int tcol = min(wave + 4 * ot, P - 1);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int nl = ks * 32 + 8 * q + e;
                    wf[ot][ks][e] = p.whh[((long)d * 4 * H + (long)(nl >> 4) * H + j0 + (nl & 15)) * H + tcol * 16 + n];
                }
        }
#pragma unroll
        for (int ot = 0; ot < NTO; ++ot)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int e = 0; e < 8; ++e) w[ot][ks][e] = (__bf16)wf[ot][ks][e];
    }

    // element owned by this thread in the cell backward: (row eb, unit j0 + ej)
    const int eb = tid >> 4, ej = tid & 15;
    const bool eok = eb < B;
    const int ebc = eok ? eb : 0;
    const long g_ts = (long)ND * 4 * H, c_ts = (long)ND * H;
    float* ge = p.gates + ((long)ebc * T * ND + d) * 4 * H + j0 + ej;
    const long cy_e = ((long)ebc * T * ND + d) * H + j0 + ej;
    auto tix = [&](int s_) { return (d == 0) ? T - 1 - s_ : s_; };
    struct Raw { float dy, gi, gf, gg, go, c, cp; };
    auto load_raw = [&](int s_) -> Raw {
        Raw r{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (s_ < T && eok) {
            const int t = tix(s_);
            const int tp = (d == 0) ? t - 1 : t + 1;
            const bool has_cp = (d == 0) ? (t > 0) : (t < T - 1);
            const float* gp = ge + (long)t * g_ts;
            r.dy = p.y[cy_e + (long)t * c_ts];
            r.gi = gp[0]; r.gf = gp[H]; r.gg = gp[2 * (long)H]; r.go = gp[3 * (long)H];
            r.c = p.c[cy_e + (long)t * c_ts];
            r.cp = p.c[cy_e + (long)(has_cp ? tp : t) * c_ts];
            if (!has_cp) r.cp = 0.f;
        }
        return r;
    };
    auto coef_of = [&](const Raw& r) -> Coef { return make_coef(r.dy, r.gi, r.gf, r.gg, r.go, r.c, r.cp); };

    Coef coef = coef_of(load_raw(0));
    Raw rawB = load_raw(1);
    Raw rawC = load_raw(2);
    float carry = 0.f;
    LSTM_DIAG_DECL

    for (int s = 0; s < T; ++s) {
        LSTM_DIAG_MARK(7)
        __syncthreads();                         // recurrent partial sums of step s are in s_part
        LSTM_DIAG_MARK(0)
        // cell backward of the owned element -> bf16 operand tile
        float dgv[4];
        {
            float dh = coef.dy;
            if (s > 0) dh += s_part_sum(s_part, tid);
            const CellGrad cg = cell_bwd(coef, dh, carry);
            dgv[0] = cg.d0; dgv[1] = cg.d1; dgv[2] = cg.d2; dgv[3] = cg.d3;
            carry = cg.carry;
            if (eok) {
                tile[eb * LD + ej] = (__bf16)dgv[0];
                tile[eb * LD + 16 + ej] = (__bf16)dgv[1];
                tile[eb * LD + 32 + ej] = (__bf16)dgv[2];
                tile[eb * LD + 48 + ej] = (__bf16)dgv[3];
            }
        }
        LSTM_DIAG_MARK(1)
        __syncthreads();
        LSTM_DIAG_MARK(2)
        // partial dh_{prev}[b, k'] for every k', handed to the owner of k'
        if (s + 1 < T) {
            const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(tile + n * LD + 8 * q);
            const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(tile + n * LD + 32 + 8 * q);
            u64* dst = p.xbuf + (long)(s & 1) * per_par + (long)d * P * P * B * 8;
            const u64 want = bwd_want(seq_of(s), p.epoch);
            f32x4 acc[NTO];
#pragma unroll
            for (int ot = 0; ot < NTO; ++ot) acc[ot] = bwd_partial(w[ot][0], w[ot][1], b0, b1);
#pragma unroll
            for (int ot = 0; ot < NTO; ++ot) {
                const int tcol = wave + 4 * ot;
                if (tcol < P && n < B) {
                    u64* o = dst + (((long)tcol * P + me) * B + n) * 8 + 2 * q;
                    u64 v0, v1;
                    bwd_granules(acc[ot], want, v0, v1);
                    if (local) { publish<true>(o, v0); publish<true>(o + 1, v1); }
                    else { publish<false>(o, v0); publish<false>(o + 1, v1); }
                }
            }
        }
        LSTM_DIAG_MARK(3)
        // gradients wrt the gate pre-activations replace the saved gates; operands three steps ahead; next coefficients
        if (eok) {
            float* gp = ge + (long)tix(s) * g_ts;
            gp[0] = dgv[0]; gp[H] = dgv[1]; gp[2 * (long)H] = dgv[2]; gp[3 * (long)H] = dgv[3];
        }
        coef = coef_of(rawB);
        rawB = rawC;
        rawC = load_raw(s + 3);
        LSTM_DIAG_MARK(4)
    }
    LSTM_DIAG_DUMP(0, 2)
}

unsigned next_epoch() { static unsigned e = 1; return e++; }

}  // namespace

LstmPass lstm_gen2_pass(int B, int H, int ND, bool bf16, bool bwd) {
    if (!bf16 || B > 16 || H % 16 != 0 || H > 512) return LstmPass{false, 0};
    const size_t P = H / 16;
    return LstmPass{true, 256 + 2 * (size_t)ND * (bwd ? P * P * B * 8 : (size_t)fwd_region(B, H)) * sizeof(u64)};
}

#define FWD2_CASE(NKS_) \
    if (nks <= NKS_) return launch_checked(lstm_fwd_p2<NKS_>, dim3(8 * p.P), dim3(512), 2 * 16 * (NKS_ * 32 + 8) * 2 + 4 * 16 * 20 * 4, st, "asr_lstm_fwd(persistent v2)", p);
#define BWD2_CASE(NTO_) \
    if (nto <= NTO_) return launch_checked(lstm_bwd_p2<NTO_>, dim3(8 * p.P), dim3(512), 0, st, "asr_lstm_bwd(persistent v2)", p);

// Clear the pass's bytes of the workspace (status block + both granule buffers), then the one launch; every planned shape
// (lstm_gen2_pass) has an instantiation.
int lstm_persistent2(float* gates, const float* whh, const float* bias2, float* y, float* c, bool bwd,
                     int B, int T, int H, int ND, void* ws, hipStream_t st) {
    hipMemsetAsync(ws, 0, lstm_gen2_pass(B, H, ND, true, bwd).bytes, st);
    const P2 p{gates, whh, bwd ? nullptr : bias2, y, c, (u64*)((char*)ws + 256), (unsigned*)ws, B, T, H, ND, H / 16,
               xcd_local_allowed(),
               poll_delays("ASR_LSTM_POLL_DELAY_FWD", "ASR_LSTM_POLL_DELAY_BWD", POLL_DELAY_FWD, POLL_DELAY_BWD, bwd), next_epoch()};
    const int nks = (H + 31) / 32, nto = (p.P + 3) / 4;
    if (bwd) { LSTM_G23_NTO(BWD2_CASE) }
    else { LSTM_G23_NKS(FWD2_CASE) }
    ASR_REQUIRE(false, ASR_E_UNSUPPORTED, "asr_lstm_%s(persistent v2): no kernel for H=%d", bwd ? "bwd" : "fwd", H);
}
