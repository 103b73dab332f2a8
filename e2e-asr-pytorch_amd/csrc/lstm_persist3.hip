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
#include <atomic>
#include "handoff.h"
#include "lstm_persist_common.h"
#include "lstm_plan.h"

namespace {

constexpr int HDR_BYTES = 1024;         // status block: abort word, per-group consensus words (u64 8..15), modes (26..33), backward form (34), diag (64..)
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
    if (blockIdx.x == 0 && tid == 0) reinterpret_cast<u64*>(p.abort_flag)[34] = 1ull;       // status: backward form (1 reduce-scatter, 2 gather)
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

// ------------------------------------------------------------------------------------------------
// backward (BPTT), gather form: groups of at most 4 batch rows (BS <= 4)
// ------------------------------------------------------------------------------------------------
// What is exchanged is dh itself, as in dec_bwd_persist: workgroup `me` publishes dh_{prev}[b][16 me .. +15] of its nb rows
// (nb x 64 bytes per step) and polls the whole BS x H vector; every workgroup then recomputes the elementwise cell backward of
// ALL BS x H elements, so there is no gate-gradient all-gather and no P-way sum of partials.
//   waves 4-7 (gather):  poll the 16-byte pairs (4 units of one row) of dh, run the cell backward of exactly those elements
//                        (they keep the elements' dc carry for the whole launch) from coefficients the compute waves left in
//                        LDS, write the bf16 gate-gradient tile [b][k = 4*unit + gate].  LDS traffic only.
//   one barrier
//   waves 0-3 (compute): wave w owns output units j0 + 4w .. +3.  The 12 MFMA columns that are no batch row carry the split
//                        of K = 4H in quarters: A row m = 4*u + kq = W_hh of output unit u over quarter kq, B column
//                        n = 4*kq + b = row b's gate gradients of quarter kq.  Lane (n, q) finds the partial of (unit q, row
//                        n & 3, quarter n >> 2) in accumulator register n >> 2; two DPP steps sum the quarters.  Then: publish,
//                        store the own 16 units' gate gradients over the saved gates, form the coefficients of step s+2 for
//                        all elements (thread ct: elements ct, ct + 256, ...) into LDS, request the operands of step s+4.
// Both LDS buffers (tile, coefficients) are double buffered by step parity: what the gather waves read or write between the
// barriers of steps s-1 and s is buffer s & 1, what the compute waves fill there is the other one.
// SAVED GATES ARE READ BY EVERY WORKGROUP OF THE GROUP and overwritten by their owner: the owner stores the gradients of step
// x behind its barrier of step x, i.e. behind the dh of step x-1 of every peer, which a peer publishes behind ITS barrier x-1
// and so behind its coefficient fill of step x (done in the tail of step x-2: the loaded values were consumed).  Steps 0 and
// 1 are filled before the XCD consensus, which no workgroup leaves before all have arrived.
// Exchange region: [group][parity][b (BS)][H/2] granules of two fp32, tagged like the partial sums of lstm_bwd_p3.
// The two forms lay the same region out differently, and the switch may change between launches on one workspace (tests,
// A/B runs; a training run keeps one form).  What protects such a switch is not the 4-bit epoch of the tag alone: in either
// form every producer clears ALL slots it will publish to in this launch - both parities, all BS rows, i.e. every slot a
// consumer of this launch polls - before the consensus, behind which polling starts.  A granule the other form left in a
// slot, whatever its tag, does not survive that.
template <int NKS>
__global__ __launch_bounds__(512) void lstm_bwd_g3(P3 p) {
    constexpr int CH = (NKS + 7) / 8;      // 16-byte pairs per gather thread:  ceil(4 * (H/4) / 256)
    constexpr int CE = (NKS + 1) / 2;      // elements per compute thread:      ceil(4 * H / 256)
    if (blockIdx.x == 0 && threadIdx.x < HDR_BYTES / 4) p.clear_next[threadIdx.x] = 0u;      // the successor's status block (see HDR_SLOTS)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int H = p.H, T = p.T, ND = p.ND, P = p.P, BS = p.BS;
    const int gid = blockIdx.x & 7, me = blockIdx.x >> 3;
    const int d = gid % ND, slice = gid / ND;
    if (slice >= p.NS) return;
    const int b0 = slice * BS, nb = min(BS, p.B - b0);
    if (nb <= 0) return;
    const int j0 = me * 16;
    const int tid = threadIdx.x;
    const int LD = 4 * H + 8;                                // bf16 per tile row (16-byte pad)
    const int NE = 4 * H;                                    // element slots of one coefficient plane
    const int tile_elems = 2 * 4 * LD + NKS * 32;            // [2][4][LD] + what the last padded k-step reads behind the end
    __bf16* tiles = reinterpret_cast<__bf16*>(smem);
    float* coefs = reinterpret_cast<float*>(smem + (size_t)tile_elems * 2);      // [2][7][NE]
    for (int i = tid; i < tile_elems / 2; i += 512) reinterpret_cast<unsigned*>(smem)[i] = 0u;
    const int HG = H >> 1;
    u64* xg = p.xbuf + (long)gid * 2 * BS * HG;              // this group's [parity][BS][HG]
    // clear this producer's granules in the L2 (see lstm_fwd_p3)
    for (int i = tid; i < 2 * BS * 8; i += 512) {
        const int parity = i / (BS * 8), r = i - parity * (BS * 8);
        st_gran_local(xg + ((long)parity * BS + (r >> 3)) * HG + (j0 >> 1) + (r & 7), 0ull);
    }
    if (blockIdx.x == 0 && tid == 0) reinterpret_cast<u64*>(p.abort_flag)[34] = 2ull;       // status: backward form (1 reduce-scatter, 2 gather)

    const long g_ts = (long)ND * 4 * H, c_ts = (long)ND * H;
    auto tix = [&](int s_) { return (d == 0) ? T - 1 - s_ : s_; };
    // ---- compute role, part 1: the elements whose coefficients this thread forms, their operands of steps 0..3, the
    //      coefficients of steps 0 and 1 ----
    const int ct = tid & 255;
    long e_off[CE];                                          // (row, unit) of element ct + 256 i in c / dy; x 4 in the gates
    bool e_ok[CE];
#pragma unroll
    for (int i = 0; i < CE; ++i) {
        const int E = ct + 256 * i;
        e_ok[i] = E < nb * H;
        const int Ec = e_ok[i] ? E : 0, erow = Ec / H, eunit = Ec - erow * H;
        e_off[i] = ((long)(b0 + erow) * T * ND + d) * H + eunit;
    }
    // raw operands exactly as loaded, every load by every lane on every path (see lstm_bwd_p3); c_{t-+1} is the c of the
    // neighbouring step's set.  A request past the end (s_ >= T) repeats step T-1: its gates may by then hold their owner's
    // gradients, so that set is garbage by design - it only feeds fill_coef(s >= T), whose buffer no step reads, and as
    // rn.c the factor cpm = 0 (c itself is never written by a backward).
    struct Raw { uint2 g[CE]; unsigned dy[CE]; float c[CE]; };
    auto load_raw = [&](int s_) -> Raw {
        Raw r;
        const long t = tix(min(s_, T - 1));
#pragma unroll
        for (int i = 0; i < CE; ++i) {
            r.g[i] = *reinterpret_cast<const uint2*>(p.gates + 4 * (e_off[i] + t * c_ts));
            r.dy[i] = p.y[e_off[i] + t * c_ts];
            r.c[i] = p.c[e_off[i] + t * c_ts];
        }
        return r;
    };
    auto fill_coef = [&](int s_, const Raw& r, const Raw& rn) {
        float* dst = coefs + (s_ & 1) * 7 * NE + ct;
        const float cpm = (s_ + 1 < T) ? 1.f : 0.f;
#pragma unroll
        for (int i = 0; i < CE; ++i) {
            const float gi = bf2f((unsigned short)(r.g[i].x & 0xFFFFu)), gf = bf2f((unsigned short)(r.g[i].x >> 16));
            const float gg = bf2f((unsigned short)(r.g[i].y & 0xFFFFu)), go = bf2f((unsigned short)(r.g[i].y >> 16));
            const Coef k = make_coef(bf2f((unsigned short)r.dy[i]), gi, gf, gg, go, r.c[i], rn.c[i] * cpm);
            if (e_ok[i]) {
                float* o = dst + 256 * i;
                o[0] = k.dy; o[NE] = k.c1; o[2 * NE] = k.c2; o[3 * NE] = k.c3; o[4 * NE] = k.c4; o[5 * NE] = k.c5; o[6 * NE] = k.f;
            }
        }
    };
    Raw raw0, raw1, raw2, raw3;
    if (tid < 256) {
        raw0 = load_raw(0); raw1 = load_raw(1); raw2 = load_raw(2); raw3 = load_raw(3);
        fill_coef(0, raw0, raw1);
        fill_coef(1, raw1, raw2);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const bool local = xcd_consensus(reinterpret_cast<u64*>(p.abort_flag) + 8 + gid, P, p.allow_local, p.abort_flag);

    if (tid >= 256) {
        // ---- gather role: pairs gt, gt + 256 of the group's nb x H/4 ----
        const int gt = tid - 256;
        const int total2 = nb * (H >> 2);
        int tile_off[CH], cnt = 0;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int idx = gt + 256 * i;
            const int ic = idx < total2 ? idx : 0, row = ic / (H >> 2);
            tile_off[i] = row * LD + 16 * (ic - row * (H >> 2));
            if (idx < total2) cnt = i + 1;
        }
        float carry[CH][4];
#pragma unroll
        for (int i = 0; i < CH; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) carry[i][e] = 0.f;
        LSTM_DIAG_DECL
        for (int s = 0; s < T; ++s) {
            if (cnt > 0) {
                // coefficients of step s: in LDS since before the previous barrier
                f32x4 kf[CH][7];
                const float* ksrc = coefs + (s & 1) * 7 * NE + 4 * gt;
#pragma unroll
                for (int i = 0; i < CH; ++i)
#pragma unroll
                    for (int k = 0; k < 7; ++k) kf[i][k] = *reinterpret_cast<const f32x4*>(ksrc + k * NE + (i < cnt ? 1024 * i : 0));
                u64 glo[CH], ghi[CH];
#pragma unroll
                for (int i = 0; i < CH; ++i) glo[i] = ghi[i] = 0ull;
                if (s > 0) {
                    for (int z = 0; z < p.poll_delay; ++z) __builtin_amdgcn_s_sleep(2);
                    const u64* src = xg + (long)((s - 1) & 1) * BS * HG + 2 * gt;
                    gather16<CH>(src, 512, cnt, BWD_MASK, bwd_want(seq_of(s - 1), p.epoch), glo, ghi, p.abort_flag);
                }
                LSTM_DIAG_MARK(0)
                __bf16* tile = tiles + (s & 1) * 4 * LD;
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    if (i < cnt) {
                        const f32x4 dh = bwd_untag(glo[i], ghi[i]);
                        uint2 o[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const Coef k{kf[i][0][e], kf[i][1][e], kf[i][2][e], kf[i][3][e], kf[i][4][e], kf[i][5][e], kf[i][6][e]};
                            const CellGrad cg = cell_bwd(k, k.dy + dh[e], carry[i][e]);
                            carry[i][e] = cg.carry;
                            o[e] = dgates_bits(cg);
                        }
                        uint4* dst = reinterpret_cast<uint4*>(tile + tile_off[i]);
                        dst[0] = make_uint4(o[0].x, o[0].y, o[1].x, o[1].y);
                        dst[1] = make_uint4(o[2].x, o[2].y, o[3].x, o[3].y);
                    }
                }
            }
            LSTM_DIAG_MARK(1)
            __syncthreads();
            LSTM_DIAG_MARK(2)
        }
        LSTM_DIAG_DUMP(256, 72)
        return;
    }

    // ---- compute role, part 2 ----
    const int lane = tid & 63, w = tid >> 6;
    const int n = lane & 15, q = lane >> 4;
    const int kq = n >> 2;                                   // as A row: quarter of K held;  as B / D column: quarter of K summed
    bf16x8 wreg[NKS];
    {
        // A operand row m = n = 4*u + kq: W_hh[k][j0 + 4w + u] over k = kq*H + kk, kk = 32 ks + 8 q + e, k = 4*unit + gate
        const int ucol = j0 + 4 * w + (n >> 2), qa = n & 3;
        float wf[NKS][8];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = qa * H + min(ks * 32 + 8 * q + e, H - 1);
                wf[ks][e] = p.whh[((long)d * 4 * H + (long)(k & 3) * H + (k >> 2)) * H + ucol];
            }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) wreg[ks][e] = (__bf16)((ks * 32 + 8 * q + e < H) ? wf[ks][e] : 0.f);
    }
    // the own element (row eb, unit j0 + ej) whose gate gradients this thread stores over the saved gates
    const int eb = tid >> 4, ej = tid & 15;
    const bool eok = eb < nb;
    const int ebg = b0 + (eok ? eb : 0);
    unsigned char* dump_wg = p.dump + (long)blockIdx.x * 512 * 16;
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(p.xbuf, 0, p.region_bytes, 0x00020000);
    const unsigned dump_off = (unsigned)(dump_wg - reinterpret_cast<unsigned char*>(p.xbuf)) + (unsigned)tid * 16u;
    unsigned short* ge = p.gates + ((long)ebg * T * ND + d) * 4 * H + (long)(j0 + ej) * 4;
    const int own_off = (eok ? eb : 0) * LD + 4 * (j0 + ej);
    const int frag_off = (n & 3) * LD + kq * H + 8 * q;
    // the wave's four units of row n & 3 go out from lane (n, q = 0), n < nb
    const bool pub = q == 0 && n < nb;
    const unsigned pub_off = (unsigned)((reinterpret_cast<unsigned char*>(xg + (long)min(n, BS - 1) * HG + ((j0 + 4 * w) >> 1)))
                                        - reinterpret_cast<unsigned char*>(p.xbuf));
    const unsigned par_bytes = (unsigned)(BS * HG * 8);
    LSTM_DIAG_DECL
    int s = 0;

#define BWDG_STEP(RCUR, RA, RB)                                                                                             \
    {                                                                                                                       \
        const __bf16* tile = tiles + (s & 1) * 4 * LD;                                                                      \
        /* operands four steps ahead, requested IN FRONT of this step's stores: the coefficient fill below needs the set   \
           requested one step ago, and behind the stores its counted wait would also wait for the publish to be acknowledged */ \
        RCUR = load_raw(s + 4);                                                                                             \
        LSTM_DIAG_MARK(7)                                                                                                   \
        __syncthreads();                         /* gate-gradient tile of step s complete */                                \
        LSTM_DIAG_MARK(0)                                                                                                   \
        bf16x8 hb[NKS];                                                                                                     \
        _Pragma("unroll") for (int ks = 0; ks < NKS; ++ks) hb[ks] = *reinterpret_cast<const bf16x8*>(tile + frag_off + ks * 32); \
        f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};                                                        \
        _Pragma("unroll") for (int ks = 0; ks < NKS; ++ks) {             /* two independent accumulation chains */          \
            if (ks & 1) acc2 = mma16(wreg[ks], hb[ks], acc2); else acc = mma16(wreg[ks], hb[ks], acc);                       \
        }                                                                                                                   \
        const float p0 = acc[0] + acc2[0], p1 = acc[1] + acc2[1], p2 = acc[2] + acc2[2], p3 = acc[3] + acc2[3];              \
        float dhp = kq == 0 ? p0 : kq == 1 ? p1 : kq == 2 ? p2 : p3;                                                        \
        dhp = row_ror_add<8>(dhp);                                                                                          \
        dhp = row_ror_add<4>(dhp);               /* dh_{prev}[row n & 3][unit j0 + 4w + q], in all four lanes of the row */ \
        LSTM_DIAG_MARK(1)                                                                                                   \
        {                                                                                                                   \
            const unsigned v0 = __float_as_uint(dhp);                                                                       \
            const unsigned v1 = __shfl(v0, n + 16), v2 = __shfl(v0, n + 32), v3 = __shfl(v0, n + 48);                        \
            const f32x4 quad = {dhp, __uint_as_float(v1), __uint_as_float(v2), __uint_as_float(v3)};                         \
            u64 g0, g1;                                                                                                     \
            bwd_granules(quad, bwd_want(seq_of(s), p.epoch), g0, g1);                                                       \
            const unsigned off = (pub && s + 1 < T) ? pub_off + (unsigned)(s & 1) * par_bytes : dump_off;                   \
            publish_pair(xrsrc, off, g0, g1, local);                                                                        \
        }                                                                                                                   \
        LSTM_DIAG_MARK(2)                                                                                                   \
        /* the own units' gradients replace the saved gates; coefficients of step s+2 */                                   \
        {                                                                                                                   \
            const uint2 dg16 = *reinterpret_cast<const uint2*>(tile + own_off);                                             \
            *(eok ? reinterpret_cast<uint2*>(ge + (long)tix(s) * g_ts) : reinterpret_cast<uint2*>(dump_wg + tid * 16)) = dg16; \
        }                                                                                                                   \
        LSTM_DIAG_MARK(3)                                                                                                   \
        fill_coef(s + 2, RA, RB);                                                                                           \
        LSTM_DIAG_MARK(4)                                                                                                   \
        if (++s >= T) break;                                                                                                \
    }

    for (;;) { BWDG_STEP(raw0, raw2, raw3) BWDG_STEP(raw1, raw3, raw0) BWDG_STEP(raw2, raw0, raw1) BWDG_STEP(raw3, raw1, raw2) }
#undef BWDG_STEP
    LSTM_DIAG_DUMP(0, 64)
}

size_t fwd3_region_bytes(int H) { return (size_t)8 * 2 * 16 * (H / 4) * sizeof(u64); }
size_t bwd3_dump_bytes(int H) { return (size_t)8 * (H / 16) * 512 * 16; }
// the backward region is sized by the reduce-scatter form; the gather form's [8][2][BS][H/2] granules (64 BS H bytes against
// 4 BS H^2) fit in front of the same dump area for every H >= 16, so one workspace serves either kernel
size_t bwd3_region_bytes(int H, int BS) { const size_t P = H / 16; return (size_t)8 * 2 * P * P * BS * 8 * sizeof(u64) + bwd3_dump_bytes(H); }
size_t bwdg3_exchange_bytes(int H, int BS) { return (size_t)8 * 2 * BS * (H / 2) * sizeof(u64); }
size_t bwdg3_lds_bytes(int H, int NKS) { return (size_t)(2 * 4 * (4 * H + 8) + NKS * 32) * 2 + (size_t)2 * 7 * 4 * H * sizeof(float); }
int slice_rows(int B, int ND) { const int NS = 8 / ND; return (B + NS - 1) / NS; }

// ASR_LSTM3_BWD / asr_lstm16_set_bwd_form: 1 = gather form (lstm_bwd_g3) for groups of at most 4 rows, 0 = reduce-scatter form
// (lstm_bwd_p3) everywhere.  The environment is read once; the setter is for A/B runs and tests within one process.
constexpr int BWD_FORM_DEFAULT = 1;
std::atomic<int> g_bwd_form{-1};
int bwd_form() {
    int f = g_bwd_form.load(std::memory_order_relaxed);
    if (f >= 0) return f;
    int unset = -1;                                          // a setter that got in first keeps its value
    g_bwd_form.compare_exchange_strong(unset, env_int("ASR_LSTM3_BWD", BWD_FORM_DEFAULT) != 0 ? 1 : 0);
    return g_bwd_form.load(std::memory_order_relaxed);
}

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
    if (bwd && bwdg3_exchange_bytes(H, BS) > rbytes - bwd3_dump_bytes(H)) return false;      // the gather form's granules end where the dump area starts
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

// the gather form's tile and coefficient buffers pass 64 KB of dynamic LDS from H = 240 on
template <int NKS>
int launch_bwdg3(const P3& p, int reserved_cus, hipStream_t st) {
    static unsigned char attr_[32] = {0};
    if (first_on_device(attr_))          // the widest H of the class (the kernel has static LDS too: not the whole 160 KB)
        hipFuncSetAttribute((const void*)lstm_bwd_g3<NKS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bwdg3_lds_bytes(32 * NKS, NKS));
    return launch_p3(lstm_bwd_g3<NKS>, p, bwdg3_lds_bytes(p.H, NKS), reserved_cus, st, "asr_lstm3_bwd");
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
#define BWDG3_CASE(NKS_) \
    if (nks <= NKS_) return launch_bwdg3<NKS_>(p, reserved_cus, st);

int lstm_gen3_set_bwd_form(int form) {
    const int old = bwd_form();
    if (form == 0 || form == 1) g_bwd_form.store(form);
    return old;
}
bool lstm_gen3_bwd_gather(int B, int H, int ND) { return bwd_form() == 1 && lstm3_shape_ok(B, H, ND) && slice_rows(B, ND) <= 4 && H <= LSTM_G3_BWDG_MAX_H; }

// Return ASR_OK when launched, 1 when the shape has no plan (or the grid would not be resident), negative on error.
int lstm_persistent3(unsigned short* gates, const float* whh, unsigned short* y, float* c, bool bwd, int B, int T, int H, int ND,
                     void* ws, size_t ws_bytes, unsigned epoch, int reserved_cus, hipStream_t st) {
    P3 p;
    if (!make_p3(p, gates, whh, y, c, B, T, H, ND, ws, ws_bytes, epoch, bwd)) return 1;
    const int nks = (H + 31) / 32, nto = (p.P + 3) / 4;
    if (bwd && lstm_gen3_bwd_gather(B, H, ND)) {
        // one workgroup per compute unit (LDS): where that grid is not resident beside `reserved_cus`, the reduce-scatter form may be
        const int rc = [&]() -> int { LSTM_G3_BWDG_NKS(BWDG3_CASE) return 1; }();
        if (rc != 1) return rc;
    }
    if (bwd) { LSTM_G23_NTO(BWD3_CASE) }
    else { LSTM_G23_NKS(FWD3_CASE) }
    return 1;
}
