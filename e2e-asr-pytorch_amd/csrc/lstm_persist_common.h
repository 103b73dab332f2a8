// What the persistent LSTM recurrence kernels share (lstm_persist.hip, lstm_persist2.hip, lstm_persist3.hip): granule tags,
// the diagnostic / jitter macros of the time loops and the checked launch.  Include after handoff.h.
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

// ---- host ---------------------------------------------------------------------------------------------------------------
// integer environment variable (poll delays: units of s_sleep(2) = 128 clocks; the callers read them once per process)
inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

// Launches kernel<<<grid, block, lds, st>>>(p); ASR_OK, or ASR_E_LAUNCH with the runtime's message under `name`.
template <typename KernelT, typename ParamT>
int launch_checked(KernelT kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, const char* name, const ParamT& p) {
    hipLaunchKernelGGL(kernel, grid, block, lds, st, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { asr_set_error("%s: launch failed: %s", name, hipGetErrorString(e)); return ASR_E_LAUNCH; }
    return ASR_OK;
}

}  // namespace
