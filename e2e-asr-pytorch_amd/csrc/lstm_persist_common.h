// What the persistent LSTM recurrence kernels share (lstm_persist.hip, lstm_persist2.hip, lstm_persist3.hip): granule tags,
// the diagnostic / jitter macros of the time loops, the checked launch, and the phases and class lists common to generations
// 2 and 3.  Include after handoff.h.
// Everything here is `static` per translation unit.
#pragma once
#include "handoff.h"

namespace {

// ---- phase marks of a time loop -----------------------------------------------------------------------------------------
// Diagnostic build (make diag, -DASR_DIAG): a wave accumulates the wall time (100 MHz s_memrealtime ticks) of each phase of a
// step and LSTM_DIAG_DUMP writes the eight sums into the status block (u64 words from `word`) for thread `thr` of workgroup 0.
// Race-detector build (make jitter, -DASR_JITTER, see decoder_persist.hip): a pseudo-random sleep at every phase boundary of
// every wave; only the third generation has been run that way (tools/jitter_lstm.py), the second generation's marks compile
// but are unexercised.  The marks expect the kernel's parameter struct `p` (abort_flag, epoch) and its step counter `s` in scope.
#ifdef ASR_DIAG
#define LSTM_DIAG_DECL unsigned long long dg_t = __builtin_amdgcn_s_memrealtime(), dg_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define LSTM_DIAG_MARK(k) { __builtin_amdgcn_sched_barrier(0); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); unsigned long long n_ = __builtin_amdgcn_s_memrealtime(); dg_acc[k] += n_ - dg_t; dg_t = n_; __builtin_amdgcn_sched_barrier(0); }
#define LSTM_DIAG_COUNT(k, v) { dg_acc[k] += (v); }
#define LSTM_DIAG_DUMP(thr, word) { if (blockIdx.x == 0 && threadIdx.x == (thr)) { unsigned long long* o = (unsigned long long*)p.abort_flag + (word); for (int k = 0; k < 8; ++k) o[k] = dg_acc[k]; } }
#elif defined(ASR_JITTER)
__device__ __forceinline__ void lstm_jitter(unsigned k, unsigned step, unsigned epoch) {
    unsigned h = (blockIdx.x * 0x9E3779B1u) ^ ((threadIdx.x >> 6) * 0x85EBCA6Bu) ^ (k * 0xC2B2AE35u) ^ (step * 0x27D4EB2Fu) ^ (epoch * 0x165667B1u);
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
    h = __builtin_amdgcn_readfirstlane(h);
    if ((h & 7u) == 0u) {
        const unsigned n = (h >> 3) & 31u;
        for (unsigned i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(4);
    }
}
#define LSTM_DIAG_DECL
#define LSTM_DIAG_MARK(k) lstm_jitter(k, (unsigned)s, p.epoch);
#define LSTM_DIAG_COUNT(k, v) { (void)(v); }
#define LSTM_DIAG_DUMP(thr, word)
#else
#define LSTM_DIAG_DECL
#define LSTM_DIAG_MARK(k)
#define LSTM_DIAG_COUNT(k, v) { (void)(v); }
#define LSTM_DIAG_DUMP(thr, word)
#endif

// ---- granule tags -------------------------------------------------------------------------------------------------------
// forward: a granule is four bf16 h; bit 14 of each (always 0 for |h| <= 1) carries the tag: step sequence in elements 0,1,
// launch epoch in elements 2,3 (the epoch keeps granules of an earlier launch, which can survive in an L2 with valid
// sequence bits, from being accepted)
constexpr u64 FWD_MASK = (1ull << 14) | (1ull << 30) | (1ull << 46) | (1ull << 62);
__device__ __forceinline__ u64 fwd_want(unsigned seq, unsigned epoch) {
    return ((u64)(seq & 1u) << 14) | ((u64)(seq >> 1) << 30) | ((u64)(epoch & 1u) << 46) | ((u64)((epoch >> 1) & 1u) << 62);
}
// backward: a granule is two fp32 partial sums; the three mantissa LSBs of both = 2-bit step sequence + 4-bit launch epoch
constexpr u64 BWD_MASK = 7ull | (7ull << 32);
__device__ __forceinline__ u64 bwd_want(unsigned seq, unsigned epoch) {
    epoch = 2u + epoch % 14u;             // epoch field 2..15: non-zero tag bits in BOTH words (see pair_want, decoder_persist.hip)
    const unsigned tag = ((epoch & 15u) << 2) | seq;
    return (u64)(tag & 7u) | ((u64)(tag >> 3) << 32);
}

// ---- phases of generations 2 and 3 --------------------------------------------------------------------------------------
// lstm_persist2.hip and lstm_persist3.hip differ in who owns which rows, in the order of the gate index and in the storage
// type; the straight-line bodies between the marks and barriers of their time loops are the same and stand here once.  Marks,
// barriers, the loops, the loads of the resident weights and of a step's operands and every bulk store stay in the kernels.
// forward gather: thread gt of 256 takes the 16-byte granule pairs gt, gt + 256, ... of `rows` contiguous rows of HG2 pairs;
// slot_off = where a pair lands in the operand tile (row stride LD bf16), -1 beyond the end.  Returns the number of pairs.
template <int CH>
__device__ __forceinline__ int fwd_gather_slots(int (&slot_off)[CH], int gt, int rows, int HG2, int LD) {
    const int total2 = rows * HG2;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int idx = gt + 256 * i;
        slot_off[i] = (idx < total2) ? (idx / HG2) * LD + (idx % HG2) * 8 : -1;
        if (idx < total2) cnt = i + 1;
    }
    return cnt;
}
// one step's poll of this thread's pairs (src + 512 i) after the start-of-step sleep; returns the polling rounds it took
template <int CH>
__device__ __forceinline__ int fwd_gather_poll(const u64* src, int cnt, int poll_delay, u64 want, u64 (&glo)[CH], u64 (&ghi)[CH], unsigned* abort_flag) {
    for (int z = 0; z < poll_delay; ++z) __builtin_amdgcn_s_sleep(2);
    return gather16<CH>(src, 512, cnt, FWD_MASK, want, glo, ghi, abort_flag);
}
// ... and the polled pairs, tags stripped, into the operand tile
template <int CH>
__device__ __forceinline__ void fwd_gather_store(__bf16* tile, const int (&slot_off)[CH], const u64 (&glo)[CH], const u64 (&ghi)[CH]) {
#pragma unroll
    for (int i = 0; i < CH; ++i)
        if (slot_off[i] >= 0) {
            u64* dst = reinterpret_cast<u64*>(tile + slot_off[i]);
            dst[0] = glo[i] & ~FWD_MASK;
            dst[1] = ghi[i] & ~FWD_MASK;
        }
}

// forward granule payload: bit 14 of a bf16 is clear for every |x| < 2; clearing it (only NaN/Inf are affected, and those
// still reach the loss through y) keeps the tag bits of the granule intact.  The publisher ORs fwd_want() in.
__device__ __forceinline__ unsigned h_bits(float h) { return f2bf_bits(h) & 0xBFFFu; }
__device__ __forceinline__ u64 h_granule(unsigned b0, unsigned b1, unsigned b2, unsigned b3) {
    return (u64)b0 | ((u64)b1 << 16) | ((u64)b2 << 32) | ((u64)b3 << 48);
}

// backward gather: the four partial sums of `cntp` polled producers' pairs, in producer order.  The sleep and the poll stay
// in the kernels: moved in here, the polling loop of both generations came out longer (+0.05 us per step, measured).
template <int NTO>
__device__ __forceinline__ float4 bwd_sum_partials(const u64 (&glo)[NTO], const u64 (&ghi)[NTO], int cntp) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int i = 0; i < NTO; ++i)
        if (i < cntp) {
            a0 += __uint_as_float((unsigned)glo[i] & ~7u);
            a1 += __uint_as_float((unsigned)(glo[i] >> 32) & ~7u);
            a2 += __uint_as_float((unsigned)ghi[i] & ~7u);
            a3 += __uint_as_float((unsigned)(ghi[i] >> 32) & ~7u);
        }
    return make_float4(a0, a1, a2, a3);
}

// backward: what one step's cell backward needs of the saved forward values, formed a step ahead of its use
struct Coef { float dy, c1, c2, c3, c4, c5, f; };
__device__ __forceinline__ Coef make_coef(float dy, float gi, float gf, float gg, float go, float c, float cp) {
    const float tc = tanh_f(c);
    return Coef{dy,
                go * (1.f - tc * tc),     // d c / d h
                gg * gi * (1.f - gi),     // d i_pre / d c
                cp * gf * (1.f - gf),     // d f_pre / d c
                gi * (1.f - gg * gg),     // d g_pre / d c
                tc * go * (1.f - go),     // d o_pre / d h
                gf};
}
// the recurrent part of dh: the four gather waves' partial sums of this thread's element, s_part[producer group][256]
__device__ __forceinline__ float s_part_sum(const float* s_part, int tid) {
    return (s_part[tid] + s_part[256 + tid]) + (s_part[512 + tid] + s_part[768 + tid]);
}
// cell backward of one element: the four gate pre-activation gradients and the new carry.  By value: written through an
// array reference, gen 3's time loop came out with other vector-memory counts (the same holds for bwd_partial).
struct CellGrad { float d0, d1, d2, d3, carry; };
__device__ __forceinline__ CellGrad cell_bwd(Coef k, float dh, float carry) {
    const float dc = dh * k.c1 + carry;
    return CellGrad{dc * k.c2, dc * k.c3, dc * k.c4, dh * k.c5, dc * k.f};
}
// backward: the partial product of one output tile (two MFMAs over the 64 reduction indices) ...
__device__ __forceinline__ f32x4 bwd_partial(bf16x8 w0, bf16x8 w1, bf16x8 b0, bf16x8 b1) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = mma16(w0, b0, acc);
    return mma16(w1, b1, acc);
}
// ... and its four sums as two tagged granules (the tag replaces the three mantissa LSBs)
__device__ __forceinline__ void bwd_granules(f32x4 acc, u64 want, u64& v0, u64& v1) {
    v0 = ((u64)(__float_as_uint(acc[0]) & ~7u) | ((u64)(__float_as_uint(acc[1]) & ~7u) << 32)) | want;
    v1 = ((u64)(__float_as_uint(acc[2]) & ~7u) | ((u64)(__float_as_uint(acc[3]) & ~7u) << 32)) | want;
}

// ---- gather form of the third generation's backward (lstm_bwd_g3) ---------------------------------------------------------
// v + v of the lane ROR places to the right within its row of 16 lanes (DPP row_ror): no LDS, no barrier
template <int ROR>
__device__ __forceinline__ float row_ror_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + ROR, 0xF, 0xF, false));
}
// the two tagged granules of a polled 16-byte pair -> four fp32 dh, tag bits cleared
__device__ __forceinline__ f32x4 bwd_untag(u64 lo, u64 hi) {
    f32x4 v;
    v[0] = __uint_as_float((unsigned)lo & ~7u);
    v[1] = __uint_as_float((unsigned)(lo >> 32) & ~7u);
    v[2] = __uint_as_float((unsigned)hi & ~7u);
    v[3] = __uint_as_float((unsigned)(hi >> 32) & ~7u);
    return v;
}
// one element's gate-gradient quadruple as four bf16
__device__ __forceinline__ uint2 dgates_bits(CellGrad cg) {
    uint2 o;
    o.x = (unsigned)f2bf_bits(cg.d0) | ((unsigned)f2bf_bits(cg.d1) << 16);
    o.y = (unsigned)f2bf_bits(cg.d2) | ((unsigned)f2bf_bits(cg.d3) << 16);
    return o;
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// integer environment variable (poll delays: units of s_sleep(2) = 128 clocks; the callers read them once per process)
inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
// poll delay of a pass from a generation's two variables, read on the first call (one call site per translation unit)
inline int poll_delays(const char* env_fwd, const char* env_bwd, int dflt_fwd, int dflt_bwd, bool bwd) {
    static const int d[2] = {env_int(env_fwd, dflt_fwd), env_int(env_bwd, dflt_bwd)};
    return d[bwd];
}
// The instantiation classes of generations 2 and 3, ascending (a shape takes the first that holds it): NKS = 32-column
// k-steps of the forward (H <= 32 NKS), NTO = output tiles per compute wave of the backward (H <= 64 NTO).
#define LSTM_G23_NKS(X) X(1) X(2) X(4) X(6) X(8) X(10) X(12) X(16)
#define LSTM_G23_NTO(X) X(1) X(2) X(3) X(4) X(5) X(6) X(8)
// ... and of the third generation's gather-form backward (NKS = k-steps of one quarter of K = 4H): H <= 384.  At NKS = 16 the
// four operand sets of 8 elements per thread no longer fit the 256 registers of a wave (91 spilled, measured at build).
#define LSTM_G3_BWDG_NKS(X) X(1) X(2) X(4) X(6) X(8) X(10) X(12)
constexpr int LSTM_G3_BWDG_MAX_H = 384;

// Launches kernel<<<grid, block, lds, st>>>(p); ASR_OK, or ASR_E_LAUNCH with the runtime's message under `name`.
template <typename KernelT, typename ParamT>
int launch_checked(KernelT kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, const char* name, const ParamT& p) {
    hipLaunchKernelGGL(kernel, grid, block, lds, st, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { asr_set_error("%s: launch failed: %s", name, hipGetErrorString(e)); return ASR_E_LAUNCH; }
    return ASR_OK;
}

}  // namespace
