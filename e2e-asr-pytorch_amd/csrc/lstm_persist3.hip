// Third-generation persistent LSTM recurrence (bf16 contraction mode, H % 16 == 0, H <= 512): the encoder's
// working point.  One launch walks all T steps of both directions (nn.LSTM recurrence + its BPTT, reference
// src/module.py:1023,1049) for up to 16 * (8 / ND) utterances.
//
// What changed against lstm_persist2.hip:
//  * BATCH-SLICED GROUPS, ONE PER XCD.  The recurrences of different utterances are independent, and a step is bound by
//    what one workgroup has to take in from its peers (the whole h_{t-1} of its batch rows, ~10 B/clk per CU on the
//    bypass-load path), not by arithmetic.  So the batch is cut into NS = 8/ND slices and the launch runs 8 independent
//    groups (direction x slice) of P = H/16 workgroups, group g on the workgroups with blockIdx % 8 == g (one XCD under
//    round-robin dispatch; verified at run time by the XCC-id consensus, never assumed).  At B = 16 a workgroup polls
//    2.5 KB per step instead of 10 KB, 160 of the 256 compute units work instead of 40, and B <= 64 fits one launch.
//  * GATE-MINOR STORAGE.  Pre-activations / activated gates / gate gradients are stored (B,T,ND,H,4) = [unit][i,f,g,o]
//    (the input-projection contraction writes that order because the bf16 copy of W_ih is stored row-permuted,
//    elementwise.hip: asr_lstm_pack_weights).  With the MFMA rows ordered unit*4+gate a lane's four accumulator
//    registers are the four gates of ONE (unit, batch row): the cell update is lane-local, the LDS gate rendez-vous and
//    the second barrier of a step are gone, and every bulk access of a lane is one 8-byte word.
//  * bf16 STORAGE of everything but the cell state: gates, h (y) and dy are bf16 in HBM (half the bytes of v2);
//    y is written with one zero row of padding on both sides in time ((B,T+2,ND*H), frame t at row t+1), which lets
//    the recurrent weight gradient read h_{t-1} / h_{t+1} as plain shifted rows.
//  * the launch epoch of the tags is extended by rotating the exchange region of a caller-owned, persistent workspace
//    (see asr_hip.h): a (region, tag) pair repeats only every 32 (forward) / 32 (backward) launches of that workspace.
// Hand-off primitives, bounded spins and the abort word: handoff.h (guide form R2).
// The phases this file shares with lstm_persist2.hip (forward gather, granule packing, coefficients and cell backward, partial
// products, the NKS / NTO class lists) are stated once in lstm_persist_common.h.
#include "common.h"
#include <stdlib.h>
#include "handoff.h"
#include "lstm_persist_common.h"
#include "lstm_plan.h"

namespace {

constexpr int HDR_BYTES = 1024;         // status block: abort word, per-group consensus words (u64 8..15), modes (26..33), diag (64..)
// TWO status blocks per workspace, used by launch epoch parity: a launch works in block (epoch & 1) and clears the OTHER one for
// its successor (first workgroup, before anything else) - the per-launch `hipMemsetAsync` of the header is gone (eight fill
// launches per training step on the critical stream).  A fresh / scrubbed workspace is all zero.
constexpr int HDR_SLOTS = 2;
constexpr int FWD_REGIONS = 8, BWD_REGIONS = 2;

struct P3 {
    unsigned short* gates;   // (B,T,ND,H,4) bf16
    const float* whh;        // (ND,4H,H) fp32, reference row order [gate][unit]
    unsigned short* y;       // fwd: h out, padded (B,T+2,ND*H) bf16;  bwd: dy in, (B,T,ND*H) bf16
    float* c;                // (B,T,ND,H)
    u64* xbuf;               // exchange region of this launch
    unsigned* abort_flag;
    unsigned* clear_next;    // status block of the next launch on this workspace: cleared by workgroup 0
    int B, T, H, ND, P, NS, BS;
    int allow_local, poll_delay;
    unsigned epoch;
    unsigned char* dump;     // backward: 8 KB per workgroup where the memory operations of inactive lanes land (see lstm_bwd_p3)
    unsigned region_bytes;   // exchange region + dump area (buffer descriptor of the publishes)
};

// granule tags: FWD_MASK / fwd_want, BWD_MASK / bwd_want (lstm_persist_common.h)

// two adjacent granules (16-byte aligned pair) in ONE 16-byte store: `sc0` keeps the line in this XCD's L2 (consumers on the
// same XCD), `sc1` writes it through (any placement).  A 16-byte store is one fabric write like an 8-byte one.
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_p3;
// (a buffer store the compiler counts: with hidden inline-asm stores in the queue its counted `s_waitcnt vmcnt(N)` for the
// operand prefetch waited for the publishes just issued - 0.45 us per step)
__device__ __forceinline__ void publish_pair(__amdgpu_buffer_rsrc_t rsrc, unsigned byte_off, u64 v0, u64 v1, bool local) {
    const u32x4_p3 v = {(unsigned)v0, (unsigned)(v0 >> 32), (unsigned)v1, (unsigned)(v1 >> 32)};
    if (local) __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, byte_off, 0, 1);        // sc0
    else __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, byte_off, 0, 16);             // sc1
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// Workgroup pw of group (d, slice): hidden units u0 = 16 pw .. +15 for batch rows b0 .. b0+nb-1 (nb <= 16).
//   waves 0-3 (compute): wave w owns units u0+4w .. +3, ALL four gates.  MFMA D[row = 4*unit + gate][col = b]
//                        = sum_k W_hh[gate*H + u0+4w+unit][k] * h_{t-1}[b][k]; lane (n = b, q = unit) holds the four
//                        gates of its unit in the four accumulator registers -> cell update without leaving the lane;
//                        three lane shuffles collect the wave's four h of a batch row into one 8-byte granule.
//   waves 4-7 (gather):  poll the h_{t-1} granules of the group's P workgroups into the LDS operand tile (nothing else in
//                        their vector-memory queue, so a poll is never stuck behind bulk traffic).
// Exchange region: [group][parity][b (16)][H/4] granules.
template <int NKS, int CH>            // CH = 16-byte granule pairs per gather thread: ceil(rows * (H/8) / 256)
__global__ __launch_bounds__(512) void lstm_fwd_p3(P3 p) {
    if (blockIdx.x == 0 && threadIdx.x < HDR_BYTES / 4) p.clear_next[threadIdx.x] = 0u;      // the successor's status block (see HDR_SLOTS)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int H = p.H, T = p.T, ND = p.ND;
    const int gid = blockIdx.x & 7, pw = blockIdx.x >> 3;
    const int d = gid % ND, slice = gid / ND;
    if (slice >= p.NS) return;
    const int b0 = slice * p.BS, nb = min(p.BS, p.B - b0);
    if (nb <= 0) return;
    const int u0 = pw * 16;
    const int tid = threadIdx.x;
    constexpr int LD = NKS * 32 + 8;                         // bf16 elements per operand-tile row (16-byte pad)
    __bf16* tiles = reinterpret_cast<__bf16*>(smem);         // [2][16][LD]  h_{t-1}, double buffered
    for (int i = tid; i < 2 * 16 * LD / 2; i += 512) reinterpret_cast<unsigned*>(smem)[i] = 0u;
    const int HG = H >> 2;
    u64* xg = p.xbuf + (long)gid * 2 * 16 * HG;              // this group's [parity][16][HG]
    // clear this producer's granules (both parities) with L2-local stores before the consensus, behind which polling
    // starts: a line an earlier launch left in this XCD's L2 with a matching tag cannot survive that
    for (int i = tid; i < 2 * 16 * 4; i += 512) {
        const int parity = i >> 6, r = i & 63, bb = r >> 2, qq = r & 3;
        st_gran_local(xg + ((long)parity * 16 + bb) * HG + (u0 >> 2) + qq, 0ull);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const bool local = xcd_consensus(reinterpret_cast<u64*>(p.abort_flag) + 8 + gid, p.P, p.allow_local, p.abort_flag);

    if (tid >= 256) {
        // ---- gather role ----
        const int gt = tid - 256;
        int slot_off[CH];
        const int cnt = fwd_gather_slots<CH>(slot_off, gt, nb, HG >> 1, LD);       // the slice's rows are contiguous
        LSTM_DIAG_DECL
        for (int s = 0; s < T; ++s) {
            __bf16* tile = tiles + (s & 1) * 16 * LD;
            if (s > 0 && cnt > 0) {
                u64 glo[CH], ghi[CH];
                const u64* src = xg + (long)((s - 1) & 1) * 16 * HG + 2 * gt;
                fwd_gather_poll<CH>(src, cnt, p.poll_delay, fwd_want(seq_of(s - 1), p.epoch), glo, ghi, p.abort_flag);
                LSTM_DIAG_MARK(0)
                fwd_gather_store<CH>(tile, slot_off, glo, ghi);
            }
            LSTM_DIAG_MARK(1)
            __syncthreads();
            LSTM_DIAG_MARK(2)
        }
        LSTM_DIAG_DUMP(256, 72)
        return;
    }

    // ---- compute role ----
    const int lane = tid & 63, w = tid >> 6;
    const int n = lane & 15, q = lane >> 4;
    bf16x8 wreg[NKS];
    {
        // A operand row m = lane & 15 = 4*unit + gate
        const float* wrow = p.whh + ((long)d * 4 * H + (long)(n & 3) * H + u0 + 4 * w + (n >> 2)) * H;
        float wf[NKS][8];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) wf[ks][e] = wrow[min(ks * 32 + 8 * q + e, H - 1)];      // all loads in flight
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) wreg[ks][e] = (__bf16)((ks * 32 + 8 * q + e < H) ? wf[ks][e] : 0.f);
    }
    const bool bok = n < nb;
    const int bg = b0 + (bok ? n : 0);
    const int unit = u0 + 4 * w + q;
    const long g_ts = (long)ND * 4 * H, c_ts = (long)ND * H;
    unsigned short* gs_base = p.gates + ((long)bg * T * ND + d) * 4 * H + (long)unit * 4;
    float* c_base = p.c + ((long)bg * T * ND + d) * H + unit;
    unsigned short* y_base = p.y + ((long)bg * (T + 2) + 1) * c_ts + (long)d * H + u0 + 4 * w;      // row t+1; 4 units of this wave
    // the time pads of y (rows 0 and T+1 = h_{-1} / h_T = 0, read by the shifted rows of the weight-gradient contraction) are
    // zeroed here by the lanes that store this wave's h, instead of two fill launches per layer from the host
    if (bok && q == 0) {
        *reinterpret_cast<uint2*>(y_base - c_ts) = make_uint2(0u, 0u);
        *reinterpret_cast<uint2*>(y_base + (long)T * c_ts) = make_uint2(0u, 0u);
    }
    auto tix = [&](int s_) { return (d == 0) ? s_ : T - 1 - s_; };
    auto ldx = [&](int s_) -> uint2 {
        if (s_ < T && bok) return *reinterpret_cast<const uint2*>(gs_base + (long)tix(s_) * g_ts);
        return make_uint2(0u, 0u);
    };
    // The pre-activations are requested four steps ahead into FOUR NAMED registers and the time loop is unrolled by four:
    // a rotation (xgA = xgB; ...) moves a register whose load has just been issued, so the compiler must wait for it -
    // `s_waitcnt vmcnt(0)` at the loop's back edge, i.e. every step drained the whole vector-memory queue (0.47 us/step).
    uint2 xg0 = ldx(0), xg1 = ldx(1), xg2 = ldx(2), xg3 = ldx(3);
    float cst = 0.f;
    LSTM_DIAG_DECL
    int s = 0;

#define FWD3_STEP(XG)                                                                                                       \
    {                                                                                                                       \
        const long t = tix(s);                                                                                              \
        const __bf16* tile = tiles + (s & 1) * 16 * LD;                                                                     \
        LSTM_DIAG_MARK(7)                                                                                                       \
        __syncthreads();                         /* h_{t-1} tile complete */                                                \
        LSTM_DIAG_MARK(0)                                                                                                       \
        f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};                                                        \
        if (s > 0) {                                                                                                        \
            bf16x8 hb[NKS];                                                                                                 \
            _Pragma("unroll") for (int ks = 0; ks < NKS; ++ks) hb[ks] = *reinterpret_cast<const bf16x8*>(tile + n * LD + ks * 32 + 8 * q); \
            _Pragma("unroll") for (int ks = 0; ks < NKS; ++ks) {         /* two independent accumulation chains */          \
                if (ks & 1) acc2 = mma16(wreg[ks], hb[ks], acc2); else acc = mma16(wreg[ks], hb[ks], acc);                   \
            }                                                                                                               \
        }                                                                                                                   \
        const float gi = sigm_f(acc[0] + acc2[0] + bf2f((unsigned short)(XG.x & 0xFFFFu)));                                 \
        const float gf = sigm_f(acc[1] + acc2[1] + bf2f((unsigned short)(XG.x >> 16)));                                     \
        const float gg = tanh_f(acc[2] + acc2[2] + bf2f((unsigned short)(XG.y & 0xFFFFu)));                                 \
        const float go = sigm_f(acc[3] + acc2[3] + bf2f((unsigned short)(XG.y >> 16)));                                     \
        cst = gf * cst + gi * gg;                                                                                           \
        const float hv = go * tanh_f(cst);                                                                                 \
        LSTM_DIAG_MARK(1)                                                                                                       \
        /* the wave's four units of batch row n sit in lanes n, n+16, n+32, n+48: collect them in lane n */                 \
        const unsigned hb16 = h_bits(hv);                                                                                   \
        const unsigned h1 = __shfl(hb16, n + 16), h2 = __shfl(hb16, n + 32), h3 = __shfl(hb16, n + 48);                      \
        if (q == 0 && bok) {                                                                                                \
            const u64 v = h_granule(hb16, h1, h2, h3);                                                                      \
            if (s + 1 < T) {                                                                                                \
                u64* dst = xg + ((long)(s & 1) * 16 + n) * HG + (u0 >> 2) + w;                                              \
                if (local) publish<true>(dst, v | fwd_want(seq_of(s), p.epoch));                                           \
                else publish<false>(dst, v | fwd_want(seq_of(s), p.epoch));                                                \
            }                                                                                                               \
            *reinterpret_cast<u64*>(y_base + t * c_ts) = v;                                                                 \
        }                                                                                                                   \
        LSTM_DIAG_MARK(2)                                                                                                       \
        /* saved activated gates (for BPTT), cell state, and the pre-activations four steps ahead */                        \
        if (bok) {                                                                                                          \
            uint2 o;                                                                                                        \
            o.x = (unsigned)f2bf_bits(gi) | ((unsigned)f2bf_bits(gf) << 16);                                                \
            o.y = (unsigned)f2bf_bits(gg) | ((unsigned)f2bf_bits(go) << 16);                                                \
            *reinterpret_cast<uint2*>(gs_base + t * g_ts) = o;                                                              \
            c_base[t * c_ts] = cst;                                                                                         \
        }                                                                                                                   \
        XG = ldx(s + 4);                                                                                                    \
        LSTM_DIAG_MARK(3)                                                                                                       \
        if (++s >= T) break;                                                                                                \
    }

    for (;;) { FWD3_STEP(xg0) FWD3_STEP(xg1) FWD3_STEP(xg2) FWD3_STEP(xg3) }
#undef FWD3_STEP
    LSTM_DIAG_DUMP(0, 64)
}

// ------------------------------------------------------------------------------------------------
// backward (BPTT), reduce-scatter form
// ------------------------------------------------------------------------------------------------
// Workgroup (me) of group (d, slice) owns units j0 = 16*me .. +15 of its batch rows: it turns their dh into the four
// gate-pre-activation gradients (reduction index k = 4*unit + gate, 64 of them) and multiplies by its W_hh rows: a PARTIAL
// dh_{t-1}[b, all H].  MFMA D[row = k' (unit of output tile tcol)][col = b].  Output tile tcol belongs to workgroup tcol.
// Waves 0-3: cell backward, MFMA, publish, bulk traffic.  Waves 4-7: poll and sum the producers' partials.
// Exchange region: [group][parity][consumer][producer][b (BS)][8 granules of two fp32].
template <int NTO>
__global__ __launch_bounds__(512) void lstm_bwd_p3(P3 p) {
    if (blockIdx.x == 0 && threadIdx.x < HDR_BYTES / 4) p.clear_next[threadIdx.x] = 0u;      // the successor's status block (see HDR_SLOTS)
    __shared__ __attribute__((aligned(16))) __bf16 tile[16 * 72];     // [b][64 + 8] dgates of this slice, k = 4*unit + gate
    __shared__ __attribute__((aligned(16))) float s_part[4 * 256];   // [producer group][b][16]
    const int H = p.H, T = p.T, ND = p.ND, P = p.P, BS = p.BS;
    const int gid = blockIdx.x & 7, me = blockIdx.x >> 3;
    const int d = gid % ND, slice = gid / ND;
    if (slice >= p.NS) return;
    const int b0 = slice * BS, nb = min(BS, p.B - b0);
    if (nb <= 0) return;
    const int j0 = me * 16;
    const int tid = threadIdx.x;
    constexpr int LD = 72;
    for (int i = tid; i < 16 * LD / 2; i += 512) reinterpret_cast<unsigned*>(tile)[i] = 0u;
    for (int i = tid; i < 4 * 256; i += 512) s_part[i] = 0.f;
    const long per_par = (long)P * P * BS * 8;
    u64* xg = p.xbuf + (long)gid * 2 * per_par;
    // clear this producer's granules in the L2 (see lstm_fwd_p3): [parity][consumer][me][b][8]
    for (int i = tid; i < 2 * P * BS * 8; i += 512) {
        const int parity = i / (P * BS * 8), r = i - parity * (P * BS * 8), pc = r / (BS * 8), rr = r - pc * (BS * 8);
        st_gran_local(xg + (long)parity * per_par + (((long)pc * P + me) * BS * 8) + rr, 0ull);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const bool local = xcd_consensus(reinterpret_cast<u64*>(p.abort_flag) + 8 + gid, P, p.allow_local, p.abort_flag);

    if (tid >= 256) {
        // ---- gather role: (row gb, unit quad g4) x producer group gq (NTO = ceil(P/4) producers each) ----
        const int gt = tid - 256;
        const int gslot = gt & 63, gb = gslot >> 2, g4 = gslot & 3, gq = gt >> 6;
        const int pp_lo = gq * NTO, cntp = max(0, min(P - pp_lo, NTO));
        LSTM_DIAG_DECL
        for (int s = 0; s < T; ++s) {
            if (s > 0) {
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gb < nb && cntp > 0) {
                    for (int z = 0; z < p.poll_delay; ++z) __builtin_amdgcn_s_sleep(2);
                    const u64* src = xg + (long)((s - 1) & 1) * per_par + (((long)me * P + pp_lo) * BS + gb) * 8 + 2 * g4;
                    u64 glo[NTO], ghi[NTO];
                    gather16<NTO>(src, (long)BS * 8, cntp, BWD_MASK, bwd_want(seq_of(s - 1), p.epoch), glo, ghi, p.abort_flag);
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
        LSTM_DIAG_DUMP(256, 72)
        return;
    }

    // ---- compute role ----
    const int lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, q = lane >> 4;
    // resident weights, A operand: row = output unit kp = 16*tcol + n, reduction index k = 32*ks + 8q + e = 4*unit + gate
    bf16x8 wreg[NTO][2];
    {
        float wf[NTO][2][8];
#pragma unroll
        for (int ot = 0; ot < NTO; ++ot) {
            const int tcol = min(wave + 4 * ot, P - 1);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int k = ks * 32 + 8 * q + e;
                    wf[ot][ks][e] = p.whh[((long)d * 4 * H + (long)(k & 3) * H + j0 + (k >> 2)) * H + tcol * 16 + n];
                }
        }
#pragma unroll
        for (int ot = 0; ot < NTO; ++ot)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int e = 0; e < 8; ++e) wreg[ot][ks][e] = (__bf16)wf[ot][ks][e];
    }

    // element owned by this thread in the cell backward: (row eb, unit j0 + ej)
    const int eb = tid >> 4, ej = tid & 15;
    const bool eok = eb < nb;
    const int ebg = b0 + (eok ? eb : 0);
    // Every vector-memory operation of the time loop is issued by EVERY lane on EVERY path (inactive lanes read a valid
    // address and write into this workgroup's dump area): with operations under lane- or step-dependent conditions the
    // compiler's count of outstanding operations differs per path and it falls back to `s_waitcnt vmcnt(0)`.
    unsigned char* dump_wg = p.dump + (long)blockIdx.x * 512 * 16;
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(p.xbuf, 0, p.region_bytes, 0x00020000);
    const unsigned dump_off = (unsigned)(dump_wg - reinterpret_cast<unsigned char*>(p.xbuf)) + (unsigned)tid * 16u;
    const long g_ts = (long)ND * 4 * H, c_ts = (long)ND * H;
    unsigned short* ge = p.gates + ((long)ebg * T * ND + d) * 4 * H + (long)(j0 + ej) * 4;
    const long cy_e = ((long)ebg * T * ND + d) * H + j0 + ej;
    auto tix = [&](int s_) { return (d == 0) ? T - 1 - s_ : s_; };
    // raw operands of one step exactly as loaded (no arithmetic on them here: a conversion or a select right behind the
    // load makes the compiler wait for it at once and the prefetch distance collapses to zero)
    struct Raw { unsigned dy; float c, cp, cpm; uint2 g; };
    auto load_raw = [&](int s_) -> Raw {
        Raw r{0u, 0.f, 0.f, 0.f, make_uint2(0u, 0u)};
        {
            const int t = tix(min(s_, T - 1));
            const int tp = (d == 0) ? t - 1 : t + 1;
            const bool has_cp = (d == 0) ? (t > 0) : (t < T - 1);
            r.g = *reinterpret_cast<const uint2*>(ge + (long)t * g_ts);
            r.dy = p.y[cy_e + (long)t * c_ts];
            r.c = p.c[cy_e + (long)t * c_ts];
            r.cp = p.c[cy_e + (long)(has_cp ? tp : t) * c_ts];
            r.cpm = has_cp ? 1.f : 0.f;
        }
        return r;
    };
    auto coef_of = [&](const Raw& r) -> Coef {
        const float gi = bf2f((unsigned short)(r.g.x & 0xFFFFu)), gf = bf2f((unsigned short)(r.g.x >> 16));
        const float gg = bf2f((unsigned short)(r.g.y & 0xFFFFu)), go = bf2f((unsigned short)(r.g.y >> 16));
        return make_coef(bf2f((unsigned short)r.dy), gi, gf, gg, go, r.c, r.cp * r.cpm);
    };

    // operands four steps ahead in FOUR NAMED register sets, time loop unrolled by four (no register rotation: see
    // lstm_fwd_p3); the coefficients of step s+1 are formed at the end of step s, off the hand-off's critical path
    Raw raw0 = load_raw(0), raw1 = load_raw(1), raw2 = load_raw(2), raw3 = load_raw(3);
    Coef coef = coef_of(raw0);
    float carry = 0.f;
    LSTM_DIAG_DECL
    int s = 0;

#define BWD3_STEP(RCUR, RNEXT)                                                                                              \
    {                                                                                                                       \
        LSTM_DIAG_MARK(7)                                                                                                       \
        __syncthreads();                         /* recurrent partial sums of step s are in s_part */                       \
        LSTM_DIAG_MARK(0)                                                                                                       \
        /* cell backward of the owned element -> bf16 operand tile (k = 4*unit + gate) and the saved-gates slot */          \
        uint2 dg16;                                                                                                         \
        {                                                                                                                   \
            float dh = coef.dy;                                                                                             \
            if (s > 0) dh += s_part_sum(s_part, tid);                                                                       \
            const CellGrad cg = cell_bwd(coef, dh, carry);                                                                  \
            carry = cg.carry;                                                                                               \
            dg16.x = (unsigned)f2bf_bits(cg.d0) | ((unsigned)f2bf_bits(cg.d1) << 16);                                       \
            dg16.y = (unsigned)f2bf_bits(cg.d2) | ((unsigned)f2bf_bits(cg.d3) << 16);                                       \
            if (eok) *reinterpret_cast<uint2*>(tile + eb * LD + 4 * ej) = dg16;      /* LDS */                              \
        }                                                                                                                   \
        LSTM_DIAG_MARK(1)                                                                                                       \
        __syncthreads();                                                                                                    \
        LSTM_DIAG_MARK(2)                                                                                                       \
        /* partial dh_{prev}[b, k'] for every k', handed to the owner of k' */                                              \
        {                                                                                                                   \
            const bf16x8 bq0 = *reinterpret_cast<const bf16x8*>(tile + n * LD + 8 * q);                                     \
            const bf16x8 bq1 = *reinterpret_cast<const bf16x8*>(tile + n * LD + 32 + 8 * q);                                \
            u64* dst = xg + (long)(s & 1) * per_par;                                                                        \
            const u64 want = bwd_want(seq_of(s), p.epoch);                                                                 \
            f32x4 acc[NTO];                                                                                                 \
            _Pragma("unroll") for (int ot = 0; ot < NTO; ++ot) acc[ot] = bwd_partial(wreg[ot][0], wreg[ot][1], bq0, bq1);    \
            _Pragma("unroll") for (int ot = 0; ot < NTO; ++ot) {                                                            \
                const int tcol = wave + 4 * ot;                                                                             \
                const bool pok = tcol < P && n < nb && s + 1 < T;                                                           \
                u64* o = dst + (((long)min(tcol, P - 1) * P + me) * BS + min(n, BS - 1)) * 8 + 2 * q;                         \
                const unsigned off = pok ? (unsigned)(reinterpret_cast<unsigned char*>(o) - reinterpret_cast<unsigned char*>(p.xbuf)) : dump_off; \
                u64 v0, v1;                                                                                                 \
                bwd_granules(acc[ot], want, v0, v1);                                                                        \
                publish_pair(xrsrc, off, v0, v1, local);                                                                    \
            }                                                                                                               \
        }                                                                                                                   \
        LSTM_DIAG_MARK(3)                                                                                                       \
        /* gradients wrt the gate pre-activations replace the saved gates; next coefficients; operands four steps ahead */  \
        *(eok ? reinterpret_cast<uint2*>(ge + (long)tix(s) * g_ts) : reinterpret_cast<uint2*>(dump_wg + tid * 16)) = dg16;    \
        coef = coef_of(RNEXT);                                                                                              \
        RCUR = load_raw(s + 4);                                                                                             \
        LSTM_DIAG_MARK(4)                                                                                                       \
        if (++s >= T) break;                                                                                                \
    }

    for (;;) { BWD3_STEP(raw0, raw1) BWD3_STEP(raw1, raw2) BWD3_STEP(raw2, raw3) BWD3_STEP(raw3, raw0) }
#undef BWD3_STEP
    LSTM_DIAG_DUMP(0, 64)
}

size_t fwd3_region_bytes(int H) { return (size_t)8 * 2 * 16 * (H / 4) * sizeof(u64); }
size_t bwd3_dump_bytes(int H) { return (size_t)8 * (H / 16) * 512 * 16; }
size_t bwd3_region_bytes(int H, int BS) { const size_t P = H / 16; return (size_t)8 * 2 * P * P * BS * 8 * sizeof(u64) + bwd3_dump_bytes(H); }
int slice_rows(int B, int ND) { const int NS = 8 / ND; return (B + NS - 1) / NS; }

// every workgroup of the launch must be resident at the same time: the grid against what the device can hold beside
// `reserved_cus` compute units that another stream may be using (data-parallel all-reduce kernels)
template <typename K>
bool fits_resident(K kernel, int grid_active, size_t lds, int reserved_cus) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 512, lds) != hipSuccess || per_cu < 1) return false;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return false;
    if (per_cu > 2) per_cu = 2;          // the occupancy API can over-report by one block per CU (guide): stay well inside
    return (long)grid_active <= (long)(cus - reserved_cus) * per_cu;
}

bool lstm3_shape_ok(int B, int H, int ND) { return H % 16 == 0 && H >= 16 && H <= 512 && B >= 1 && B <= 16 * (8 / ND) && (ND == 1 || ND == 2); }

// What both passes of a launch share: shape and workspace checks, the status block by launch parity, the exchange region by
// rotation, the P3 fill.  false: no plan.
bool make_p3(P3& p, unsigned short* gates, const float* whh, unsigned short* y, float* c, int B, int T, int H, int ND,
             void* ws, size_t ws_bytes, unsigned epoch, bool bwd) {
    if (!lstm3_shape_ok(B, H, ND) || !ws || ((uintptr_t)ws & 255) != 0) return false;
    if (ws_bytes < lstm_gen3_pass(B, H, ND, bwd).bytes) return false;
    const int BS = slice_rows(B, ND);
    const size_t rbytes = bwd ? bwd3_region_bytes(H, BS) : fwd3_region_bytes(H);
    if (bwd && rbytes >= (1ull << 31)) return false;             // the publishes address the region through a buffer descriptor
    const unsigned rot = bwd ? (epoch >> 4) % BWD_REGIONS : (epoch >> 2) % FWD_REGIONS;
    unsigned* hdr = (unsigned*)((char*)ws + (size_t)(epoch & 1u) * HDR_BYTES);
    unsigned* hdr_next = (unsigned*)((char*)ws + (size_t)((epoch + 1u) & 1u) * HDR_BYTES);
    u64* region = (u64*)((char*)ws + HDR_SLOTS * HDR_BYTES + (size_t)rot * rbytes);
    p = P3{gates, whh, y, c, region, hdr, hdr_next, B, T, H, ND, H / 16, 8 / ND, BS, xcd_local_allowed(),
           poll_delays("ASR_LSTM3_POLL_DELAY_FWD", "ASR_LSTM3_POLL_DELAY_BWD", 6, 4, bwd), epoch,
           bwd ? (unsigned char*)region + rbytes - bwd3_dump_bytes(H) : nullptr, bwd ? (unsigned)rbytes : 0u};
    return true;
}

// 1 when the grid would not be resident
template <typename KernelT>
int launch_p3(KernelT kernel, const P3& p, size_t lds, int reserved_cus, hipStream_t st, const char* name) {
    const int groups = p.ND * ((p.B + p.BS - 1) / p.BS);
    if (!fits_resident(kernel, groups * p.P, lds, reserved_cus)) return 1;
    return launch_checked(kernel, dim3(8 * p.P), dim3(512), lds, st, name, p);
}

}  // namespace

LstmPass lstm_gen3_pass(int B, int H, int ND, bool bwd) {
    if (!lstm3_shape_ok(B, H, ND)) return LstmPass{false, 0};
    return LstmPass{true, HDR_SLOTS * HDR_BYTES + (bwd ? BWD_REGIONS * bwd3_region_bytes(H, slice_rows(B, ND)) : FWD_REGIONS * fwd3_region_bytes(H))};
}

#define FWD3_LAUNCH(NKS_, CH_) return launch_p3(lstm_fwd_p3<NKS_, CH_>, p, 2 * 16 * (NKS_ * 32 + 8) * 2, reserved_cus, st, "asr_lstm3_fwd");
#define FWD3_CASE(NKS_)                                                                                                     \
    if (nks <= NKS_) {                                                                                                      \
        constexpr int CHMAX = (NKS_ + 3) / 4;                                                                               \
        const int ch = (p.BS * (H / 8) + 255) / 256;                                                                        \
        if (ch <= 1) FWD3_LAUNCH(NKS_, 1)                                                                                   \
        else if (ch <= 2 || CHMAX <= 2) FWD3_LAUNCH(NKS_, (CHMAX < 2 ? CHMAX : 2))                                          \
        else FWD3_LAUNCH(NKS_, CHMAX)                                                                                       \
    }
#define BWD3_CASE(NTO_) \
    if (nto <= NTO_) return launch_p3(lstm_bwd_p3<NTO_>, p, 0, reserved_cus, st, "asr_lstm3_bwd");

// Return ASR_OK when launched, 1 when the shape has no plan (or the grid would not be resident), negative on error.
int lstm_persistent3(unsigned short* gates, const float* whh, unsigned short* y, float* c, bool bwd, int B, int T, int H, int ND,
                     void* ws, size_t ws_bytes, unsigned epoch, int reserved_cus, hipStream_t st) {
    P3 p;
    if (!make_p3(p, gates, whh, y, c, B, T, H, ND, ws, ws_bytes, epoch, bwd)) return 1;
    const int nks = (H + 31) / 32, nto = (p.P + 3) / 4;
    if (bwd) { LSTM_G23_NTO(BWD3_CASE) }
    else { LSTM_G23_NKS(FWD3_CASE) }
    return 1;
}
