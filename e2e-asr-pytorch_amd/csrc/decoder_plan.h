// Host side of the four cluster launchers (decoder_persist.hip: dec_fwd_persist, dec_bwd_persist; decoder_stream.hip:
// dec_fwd_stream, dec_bwd_stream), each piece written once: the plans of a shape, the carve of a launch's work area, the launch
// sequence, the environment switches the launchers read.  Host code only; `static` per translation unit.
#pragma once
#include "decoder_bwd_common.h"

namespace {

inline int even_up(int x) { return (x + 1) & ~1; }
// a cluster is the NT workgroups of one utterance; workgroup id = 8 * (slot on the XCD) + XCD, ceil(B/8) clusters per XCD
inline dim3 cluster_grid(const asr_dec_dims_t& d, int NT) { return dim3(8 * cdiv(d.B, 8) * NT); }
inline int dec_bwd_poll_delay() {
    static const int units = [] { const char* e = getenv("ASR_DEC_BWD_POLL_DELAY"); return e ? atoi(e) : 0; }();
    return units;
}

// 256-byte aligned blocks of a work area, front to back.  With base = nullptr only the sizes mean anything.
struct WorkCarver {
    uintptr_t p;
    template <class T> T* take(size_t bytes) { T* r = (T*)p; p += align_up256(bytes); return r; }
};

// ---- forward ----------------------------------------------------------------------------------------------------------------
// kind 0: no plan (everything else 0), 1: tiles resident in LDS (dec_fwd_persist), 2: streamed tiles (dec_fwd_stream: TE is
// the kernel's TEB, tpw unused)
struct FwdPlan { int kind, tpw, NT, TE, UPW, QPW, CPW, HG2, QG2, SG2, KC, KCP; size_t lds, total; };
struct FwdWork { unsigned* status; u64* xbuf; unsigned short* wcat16; float* embproj; unsigned short* key16t; size_t xbuf_bytes, total; };

inline FwdWork fwd_work(const asr_dec_dims_t& d, const FwdPlan& pl, void* base) {
    WorkCarver c{(uintptr_t)base};
    FwdWork w;
    w.status = c.take<unsigned>(4096);
    w.xbuf = c.take<u64>(2 * (size_t)d.B * pl.NT * (pl.HG2 + pl.QG2 + pl.SG2) * sizeof(u64));
    w.xbuf_bytes = c.p - (uintptr_t)w.xbuf;
    w.wcat16 = c.take<unsigned short>((size_t)4 * d.Dd * pl.KCP * 2);
    w.embproj = c.take<float>((size_t)d.B * d.L * 4 * d.Dd * sizeof(float));
    w.key16t = c.take<unsigned short>(pl.kind == 2 ? (size_t)d.B * pl.NT * ((pl.TE + 31) / 32) * 4 * d.A * 16 : 0);      // pair image (odd tile counts are padded)
    w.total = c.p - (uintptr_t)base;
    return w;
}
// what follows from kind, NT and TE in both forward plans: the shares of a workgroup, the granules per record, the work area
inline void fwd_sizes(const asr_dec_dims_t& d, FwdPlan& pl) {
    pl.UPW = cdiv(d.Dd, pl.NT); pl.QPW = cdiv(d.A, pl.NT); pl.CPW = cdiv(d.E, pl.NT);
    pl.HG2 = even_up((pl.UPW + 1) / 2); pl.QG2 = even_up((pl.QPW + 1) / 2); pl.SG2 = even_up((pl.TE + 2) / 2 + d.E / 4);      // record: e pairs, (m, s), context as halves
    pl.KC = d.E + d.Dd; pl.KCP = (pl.KC + 7) & ~7;
    pl.total = fwd_work(d, pl, nullptr).total;
}

FwdPlan persist_plan(const asr_dec_dims_t& d);       // decoder_persist.hip, next to the kernel whose LDS it sizes by hand

inline FwdPlan stream_plan_f(const asr_dec_dims_t& d) {
    if (d.NL != 1 || d.B > 64 || d.B < 1 || d.A > 16 * FSW_NU * NCW || d.Kn > 10 || (d.E & 7) != 0 || d.E > 8 * 64 * NCW || d.Dd > 20 * 32 || d.Tp < 1) return FwdPlan{};
    FwdPlan pl{};
    pl.kind = 2; pl.NT = std::min(30, 32 / cdiv(d.B, 8));
    pl.TE = 16 * cdiv(d.Tp, 16 * pl.NT);
    fwd_sizes(d, pl);
    if (pl.UPW > 120 || cdiv(4 * pl.UPW, NCW) > 60) return FwdPlan{};
    const FCarve c = fwd_carve(pl.TE, pl.NT, d.A, d.E, d.Kn, d.Ks, pl.KCP, pl.UPW, pl.SG2);
    if (c.NG < 1) return FwdPlan{};
    pl.lds = 2 * (size_t)c.shorts + 4 * (size_t)c.floats;
    if (getenv("ASR_DEC_PLAN_DEBUG")) fprintf(stderr, "[asr] streamed fwd plan B=%d T'=%d: NT=%d TEB=%d UPW=%d LDS=%zu\n", d.B, d.Tp, pl.NT, pl.TE, pl.UPW, pl.lds);
    return pl.lds > 156 * 1024 ? FwdPlan{} : pl;
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// kind as above (1: dec_bwd_persist, 2: dec_bwd_stream, TE is its TEB)
struct BwdPlan { int kind, TE, NT, UPW, CPW, R4, CG2, QG2, VG2, NG2; size_t lds, total; };
struct BwdWork { unsigned* status; u64* xbuf; unsigned short* w16; float* dgates; unsigned short* key16t; float* dkT; size_t xbuf_bytes, dkt_bytes, total; };

inline BwdWork bwd_work(const asr_dec_dims_t& d, const BwdPlan& pl, void* base) {
    WorkCarver c{(uintptr_t)base};
    BwdWork w;
    w.status = c.take<unsigned>(4096);
    w.xbuf = c.take<u64>(2 * (size_t)d.B * pl.NT * (pl.CG2 + pl.QG2 + pl.VG2 + pl.NG2) * sizeof(u64));
    w.xbuf_bytes = c.p - (uintptr_t)w.xbuf;
    w.w16 = c.take<unsigned short>((size_t)(d.Dd + d.E + d.Dd) * pl.R4 * 2);
    w.dgates = c.take<float>((size_t)d.B * d.L * 4 * d.Dd * sizeof(float));
    const size_t image = pl.kind == 2 ? (size_t)d.B * pl.NT * pl.TE * d.A : 0;      // streamed tiles: key and dkey in the sweep's layout
    w.key16t = c.take<unsigned short>(image * 2);
    w.dkT = c.take<float>(image * 4);
    w.dkt_bytes = c.p - (uintptr_t)w.dkT;
    w.total = c.p - (uintptr_t)base;
    return w;
}
// what follows from kind, NT and TE in both backward plans
inline void bwd_sizes(const asr_dec_dims_t& d, BwdPlan& pl) {
    pl.UPW = cdiv(d.Dd, pl.NT); pl.CPW = cdiv(d.E, pl.NT);
    pl.R4 = (4 * d.Dd + 7) & ~7;
    pl.CG2 = even_up((pl.CPW + pl.UPW + 1) / 2); pl.QG2 = even_up(d.A / 2); pl.VG2 = even_up((pl.TE * d.Kn + 1) / 2); pl.NG2 = even_up((pl.TE + pl.UPW + 1) / 2);
    pl.total = bwd_work(d, pl, nullptr).total;
}

inline BwdPlan persist_plan_b(const asr_dec_dims_t& d) {
    if (d.NL != 1 || d.B > 64 || d.A > 320 || d.A < 16 || d.Kn > 10 || (d.E & 7) != 0 || (d.A & 1) != 0 || d.Dd > 64 * KCHB || d.L < 1) return BwdPlan{};
    const int cpx = cdiv(d.B, 8);
    const int ncw = cdiv(d.A, 64), nct = 64 * ncw;
    if (d.Dd > nct || d.E > 2 * nct || d.E > 640 || d.Tp > 4 * nct) return BwdPlan{};
    // frames per tile: the smallest multiple of 4 (most tiles, fewest weight rows and sweep frames per workgroup) whose tiles
    // fit the XCD (32 CUs per XCD, ceil(B/8) clusters each), the register-resident weight rows and the LDS
    // Second pass (short encoder outputs, e.g. T' = 150 behind a VGG front-end): more workgroups than the frames need.  The
    // weight rows of the cell and the context columns are spread over ALL tiles of an utterance, so a short utterance can run
    // out of register rows before it runs out of frames; tiles past T' hold rows only (every frame access of the kernel is
    // clamped to the utterance and every frame store guarded by T', as for the tiles past a short utterance of a ragged batch).
    for (int pass = 0; pass < 2; ++pass)
    for (int TE = 8; TE <= 40; TE += 4) {
        const int nt_frames = cdiv(d.Tp, TE);
        const int nt_hi = pass == 0 ? nt_frames : std::min(30, 32 / cpx);
        for (int nt = nt_frames + pass; nt <= nt_hi; ++nt) {
            if (nt > 30 || cpx * nt > 32 || 8 * TE > nct || d.Kn * TE > 2 * nct) continue;
            BwdPlan pl{};
            pl.kind = 1; pl.TE = TE; pl.NT = nt;
            bwd_sizes(d, pl);
            if (pl.UPW > 64 || pl.UPW + pl.CPW > RCB * ncw + RPB * NPB || (TE + pl.UPW + 1) / 2 + 1 > nct) continue;
            if (pl.NT * pl.QG2 * 2 < NPB * 64 * 11) continue;       // s_qst doubles as the stage of the polling waves' partial accumulators
            const BCarve cv = bwd_carve(TE, 12, d.A, d.E, d.Kn, d.Ks, pl.NT, pl.UPW, pl.CG2, pl.QG2, pl.NG2);
            pl.lds = 2 * (size_t)cv.shorts + 4 * (size_t)cv.floats;
            if (getenv("ASR_DEC_PLAN_DEBUG")) fprintf(stderr, "[asr] resident bwd plan B=%d T'=%d: NT=%d TE=%d LDS=%zu\n", d.B, d.Tp, pl.NT, pl.TE, pl.lds);
            if (pl.lds <= 160 * 1024 - 4096) return pl;
        }
    }
    return BwdPlan{};
}

inline BwdPlan stream_plan_b(const asr_dec_dims_t& d) {
    if (d.NL != 1 || d.B > 64 || d.B < 1 || d.A > 320 || d.A < 16 || d.Kn > 10 || (d.E & 7) != 0 || (d.A & 1) != 0 || d.Dd > 64 * KCHB || d.L < 1 || d.Tp < 1) return BwdPlan{};
    const int ncw = cdiv(d.A, 64), nct = 64 * ncw;
    if (d.Dd > nct || d.E > 2 * nct || d.E > 640 || d.Tp > 6 * nct || d.Kn * 16 * SW_MT > 2 * nct) return BwdPlan{};
    if (cdiv(d.A, 16) > SW_NU * ncw + SW_NUP * NPB) return BwdPlan{};           // sweep units over all waves
    BwdPlan pl{};
    pl.kind = 2; pl.NT = std::min(30, 32 / cdiv(d.B, 8));
    pl.TE = 16 * cdiv(d.Tp, 16 * pl.NT);
    bwd_sizes(d, pl);
    const SBCarve cv = sbwd_carve(pl.TE, d.A, d.E, d.Kn, d.Ks, pl.NT, pl.UPW, pl.CPW, pl.CG2, pl.QG2, pl.NG2);
    pl.lds = 2 * (size_t)cv.shorts + 4 * (size_t)cv.floats;
    if (getenv("ASR_DEC_PLAN_DEBUG")) fprintf(stderr, "[asr] streamed bwd plan B=%d T'=%d: NT=%d TEB=%d UPW=%d LDS=%zu\n", d.B, d.Tp, pl.NT, pl.TE, pl.UPW, pl.lds);
    return pl.lds > 160 * 1024 - 4096 ? BwdPlan{} : pl;
}

// the plan a shape takes: the resident one unless the streamed one is preferred and exists
template <class Plan> Plan chosen_plan(const Plan& resident, const Plan& streamed, int prefer_streamed) {
    return (resident.kind && !(prefer_streamed && streamed.kind)) ? resident : streamed;
}

// ---- launch -----------------------------------------------------------------------------------------------------------------
// Every workgroup of a cluster waits for its peers: the dynamic-LDS limit of the kernel (set once per device and kernel - the
// marks below belong to the instantiation of run<K>), the residency of the whole grid, the kernel, the epoch of its work area.
// Returns 1 when the grid is not resident (the caller falls back to the per-step kernels).
struct ClusterLaunch {
    const char* who;
    int lds_cap;
    dim3 grid, block;
    size_t lds;
    hipStream_t st;
    template <auto K, class P> int run(const P& p) const {
        static unsigned char attr_[32];
        if (first_on_device(attr_)) hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, lds_cap);
        if (!grid_resident(K, (int)grid.x, (int)block.x, lds)) return 1;
        hipLaunchKernelGGL(K, grid, block, lds, st, p);
        hipLaunchKernelGGL(bump_epoch_kernel, dim3(1), dim3(1), 0, st, p.status);
        ASR_LAUNCH_CHECK(who);
        return ASR_OK;
    }
};

}  // namespace
