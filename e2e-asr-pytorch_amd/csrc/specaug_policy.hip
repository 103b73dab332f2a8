// SpecAugment policies (data.audio.augment as a mapping): a time warp, up to 8 frequency masks and up to 32 time
// masks per utterance, filled with the utterance's mean or with zero.  Out of place on the padded batch x (B,T,D) -> out (B,T,D):
// the warp is a gather along time, so x is read only.  Every length is taken as n = min(max(len, 0), T).
//
// Draws.  Word group k of utterance b is philox4x32(counter (b, k, 3, 0), key (seed lo, seed hi)); a group uses r0, r1.
//   group 0       the warp, active iff warp > 0 && n >= 2 warp + 1: w0 = warp + r0 % (n - 2 warp), w = r1 % (2 warp + 1) - warp,
//                 c = clamp(w0 + w, 1, n - 2).  The source knot w0 moves to the destination frame c.
//   group 1 + j   frequency mask j < freq_masks: Fw = min(freq_width, D), f = r0 % (Fw + 1), f0 = r1 % (D - f + 1): [f0, f0 + f)
//   group 9 + j   time mask j < cnt, cnt = time_count_pm ? min(time_masks, n time_count_pm / 1000) : time_masks:
//                 Tw = min(time_width, n time_ratio_pm / 1000), t = r0 % (Tw + 1), t0 = r1 % (n - t + 1): [t0, t0 + t)
// The record of an utterance is int32 {w0, c, (f0, fend) x 8, (t0, tend) x 32}, 82 words, (0, 0) where a group is inactive.
// draws_in has that layout and replaces the RNG: the warp is off unless 1 <= w0 <= n - 2 && 1 <= c <= n - 2, bands are clamped
// into [0, D] and [0, n] with end >= start.  draws_out receives the record as applied.
//
// Warp.  Destination frame t < n reads source position s(t): t <= c: num = t w0, den = c, base = 0; otherwise num = (t - c)
// (n - 1 - w0), den = n - 1 - c, base = w0.  i = base + num / den, r = num % den in integers; out = x[i] when r == 0, else
// x[i] + float(r) / float(den) * (x[i + 1] - x[i]) in float32.  Both ends and the knot are held; i + 1 <= n - 1 whenever r != 0.
//
// Fill.  zero: 0.0f.  mean: v = float32(sum / (n D)) over the n D valid INPUT values, one value for every mask of the utterance;
// PA_SPLIT workgroups per utterance form float64 partial sums at fixed slots, every workgroup of the second launch adds the
// slots in one fixed order.  No atomics: two calls give the same bits.  With fill = zero that launch is skipped.
//
// Output.  t < n: the fill inside any band, else the warped value (a masked element loads nothing); rows t >= n are copies of x.
// Rows move as float4 where D % 4 == 0 and both bases are 16-byte aligned, as single floats otherwise.
#include "common.h"

namespace {

constexpr int PA_SPLIT = 64;        // partial sums per utterance: one per lane of the wave that adds them
constexpr int PA_GRID = 64;         // workgroups per utterance of the apply launch at most; beyond that they stride
constexpr int PA_FM = 8, PA_TM = 32;
constexpr int PA_GROUPS = 1 + PA_FM + PA_TM;       // 41
constexpr int PA_REC = 2 * PA_GROUPS;              // 82

struct PolicyArgs {
    int B, T, D, warp, fm, fw, tm, tw, tr_pm, tc_pm, fill;
    uint64_t seed;
};

__device__ __forceinline__ int pa_len(const int64_t* lens, int b, int T) {
    const int64_t l = lens[b];
    return (int)(l < 0 ? 0 : (l > T ? T : l));
}

// entry k of the record of utterance b: (lo, hi) = (w0, c) for k == 0, a band otherwise
__device__ __forceinline__ void policy_group(int k, int b, int n, const PolicyArgs& p, const int* __restrict__ draws_in, int& lo, int& hi) {
    lo = hi = 0;
    if (draws_in) {
        const int a = draws_in[(long)b * PA_REC + 2 * k], e = draws_in[(long)b * PA_REC + 2 * k + 1];
        if (k == 0) {
            if (a >= 1 && a <= n - 2 && e >= 1 && e <= n - 2) { lo = a; hi = e; }
        } else {
            const int ext = (k < 1 + PA_FM) ? p.D : n;
            lo = min(max(a, 0), ext);
            hi = min(max(e, lo), ext);
        }
        return;
    }
    uint32_t r[4];
    philox4x32((uint32_t)b, (uint32_t)k, 3u, 0u, (uint32_t)p.seed, (uint32_t)(p.seed >> 32), r);
    if (k == 0) {
        if (p.warp > 0 && (long)n >= 2L * p.warp + 1) {
            const int w0 = p.warp + (int)(r[0] % (uint32_t)(n - 2 * p.warp));
            const int w = (int)(r[1] % (uint32_t)(2 * p.warp + 1)) - p.warp;
            lo = w0;
            hi = min(max(w0 + w, 1), n - 2);
        }
    } else if (k < 1 + PA_FM) {
        if (k - 1 < p.fm) {
            const uint32_t Fw = (uint32_t)min(p.fw, p.D);
            const int f = (int)(r[0] % (Fw + 1u));
            lo = (int)(r[1] % ((uint32_t)(p.D - f) + 1u));
            hi = lo + f;
        }
    } else {
        const int cnt = p.tc_pm ? (int)min((long)p.tm, (long)n * p.tc_pm / 1000) : p.tm;
        if (k - 1 - PA_FM < cnt) {
            const uint32_t Tw = (uint32_t)min((long)p.tw, (long)n * p.tr_pm / 1000);
            const int t = (int)(r[0] % (Tw + 1u));
            lo = (int)(r[1] % ((uint32_t)(n - t) + 1u));
            hi = lo + t;
        }
    }
}

template <int V> struct PaVec;
template <> struct PaVec<1> {
    float v[1];
    __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
    __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
};
template <> struct PaVec<4> {
    float v[4];
    __device__ __forceinline__ void load(const float* p) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
    __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// float64 partial sums of the n D valid values of utterance b: slot sp owns a contiguous range, a thread every 256th vector of it
template <int V>
__global__ __launch_bounds__(256) void policy_sum_kernel(const float* __restrict__ x, const int64_t* __restrict__ lens,
                                                         double* __restrict__ part, int B, int T, int D) {
    __shared__ double s_red[4];
    const int b = blockIdx.x / PA_SPLIT, sp = blockIdx.x % PA_SPLIT, tid = threadIdx.x;
    const int n = pa_len(lens, b, T);
    const float* xb = x + (long)b * T * D;
    const long total = (long)n * D / V;              // V == 4 only where D % 4 == 0
    const long per = (total + PA_SPLIT - 1) / PA_SPLIT, i0 = sp * per, i1 = min(total, i0 + per);
    double sum = 0.0;
#pragma unroll 4
    for (long i = i0 + tid; i < i1; i += 256) {
        PaVec<V> a;
        a.load(xb + i * V);
        if constexpr (V == 4) sum += ((double)a.v[0] + (double)a.v[1]) + ((double)a.v[2] + (double)a.v[3]);
        else sum += (double)a.v[0];
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((tid & 63) == 0) s_red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) part[(long)b * PA_SPLIT + sp] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// one pass: read x once, write out once.  Workgroup (b, blk) of gx per utterance; a thread walks the (row, vector) pairs
// blk 256 + tid, + gx 256, ... of the T x D / V grid of its utterance, row and column kept apart so that the walk needs no division
// inside the loop and nothing leaves 32 bits except the byte offset; the one division left is num / den of a warped row.
template <int V>
__global__ __launch_bounds__(256) void policy_apply_kernel(const float* __restrict__ x, const int64_t* __restrict__ lens,
                                                           float* __restrict__ out, const int* __restrict__ draws_in,
                                                           int* __restrict__ draws_out, const double* __restrict__ part,
                                                           PolicyArgs p, int gx) {
    __shared__ int s_rec[PA_REC];
    __shared__ int s_tb[2 * PA_TM], s_fb[2 * PA_FM], s_cnt[2];
    __shared__ float s_fill;
    const int b = blockIdx.x / gx, blk = blockIdx.x % gx, tid = threadIdx.x;
    const int T = p.T, D = p.D;
    const int n = pa_len(lens, b, T);
    if (tid < PA_GROUPS) {
        int lo, hi;
        policy_group(tid, b, n, p, draws_in, lo, hi);
        s_rec[2 * tid] = lo;
        s_rec[2 * tid + 1] = hi;
    }
    if (tid < 64) {                                  // the first wave: PA_SPLIT slots, added in one fixed tree
        double s = (p.fill == 0 && n > 0) ? part[(long)b * PA_SPLIT + tid] : 0.0;
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (tid == 0) s_fill = (p.fill == 0 && n > 0) ? (float)(s / ((double)n * (double)D)) : 0.f;
    }
    __syncthreads();
    if (tid == 0) {                                  // the non-empty bands, packed
        int nt = 0, nf = 0;
        for (int j = 0; j < PA_FM; ++j) {
            const int lo = s_rec[2 + 2 * j], hi = s_rec[3 + 2 * j];
            if (hi > lo) { s_fb[2 * nf] = lo; s_fb[2 * nf + 1] = hi; ++nf; }
        }
        for (int j = 0; j < PA_TM; ++j) {
            const int lo = s_rec[2 + 2 * PA_FM + 2 * j], hi = s_rec[3 + 2 * PA_FM + 2 * j];
            if (hi > lo) { s_tb[2 * nt] = lo; s_tb[2 * nt + 1] = hi; ++nt; }
        }
        s_cnt[0] = nt;
        s_cnt[1] = nf;
    }
    if (blk == 0 && draws_out && tid < PA_REC) draws_out[(long)b * PA_REC + tid] = s_rec[tid];
    __syncthreads();
    const int w0 = s_rec[0], c = s_rec[1], nt = s_cnt[0], nf = s_cnt[1];
    const bool warped = w0 > 0;                      // an active warp has 1 <= w0, c <= n - 2
    const float fillv = s_fill;
    const float* xb = x + (long)b * T * D;
    float* ob = out + (long)b * T * D;
    const int Dv = D / V;
    const unsigned first = (unsigned)blk * 256u + (unsigned)tid, stride = (unsigned)gx * 256u;
    const int dt = (int)(stride / (unsigned)Dv), dc = (int)(stride % (unsigned)Dv);
    long t = first / (unsigned)Dv;
    int col = (int)(first % (unsigned)Dv);
    constexpr unsigned FULL = (1u << V) - 1u;
    while (t < T) {
        const long off = t * D + (long)col * V;
        PaVec<V> val;
        if (t >= n) {
            val.load(xb + off);
        } else {
            unsigned cm = 0;
            for (int j = 0; j < nt; ++j) if (t >= s_tb[2 * j] && t < s_tb[2 * j + 1]) cm = FULL;
            for (int j = 0; j < nf; ++j) {
                const int f0 = s_fb[2 * j], f1 = s_fb[2 * j + 1];
#pragma unroll
                for (int e = 0; e < V; ++e) cm |= (unsigned)(col * V + e >= f0 && col * V + e < f1) << e;
            }
            if (cm != FULL) {
                if (!warped) {
                    val.load(xb + off);
                } else {
                    const int ti = (int)t;
                    uint64_t num;
                    uint32_t den;
                    long base;
                    if (ti <= c) { num = (uint64_t)ti * (uint64_t)w0; den = (uint32_t)c; base = 0; }
                    else { num = (uint64_t)(ti - c) * (uint64_t)(n - 1 - w0); den = (uint32_t)(n - 1 - c); base = w0; }
                    uint32_t q, r;
                    if ((num >> 32) == 0) { q = (uint32_t)num / den; r = (uint32_t)num % den; }
                    else { q = (uint32_t)(num / den); r = (uint32_t)(num % den); }
                    const float* src = xb + (base + (long)q) * D + (long)col * V;
                    val.load(src);
                    if (r != 0) {
                        PaVec<V> nxt;
                        nxt.load(src + D);
                        const float w = (float)r / (float)den;          // correctly rounded: the build sets no fast-math
#pragma unroll
                        for (int e = 0; e < V; ++e) val.v[e] = val.v[e] + w * (nxt.v[e] - val.v[e]);
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < V; ++e) if (cm & (1u << e)) val.v[e] = fillv;
        }
        val.store(ob + off);
        col += dc;
        t += dt;
        if (col >= Dv) { col -= Dv; ++t; }
    }
}

}  // namespace

extern "C" size_t asr_specaug_policy_workspace_bytes(int B) { return (size_t)(B > 0 ? B : 0) * PA_SPLIT * sizeof(double); }

extern "C" int asr_specaug_policy(const float* x, const int64_t* lens, float* out, const int* draws_in, int* draws_out,
                                  int B, int T, int D, int warp, int freq_masks, int freq_width, int time_masks, int time_width,
                                  int time_ratio_pm, int time_count_pm, int fill, uint64_t seed,
                                  void* workspace, size_t workspace_bytes, asr_stream_t stream) {
    ASR_REQUIRE(x && lens && out, ASR_E_ARG, "asr_specaug_policy: null x, lens or out");
    ASR_REQUIRE(B > 0 && T > 0 && D > 0, ASR_E_ARG, "asr_specaug_policy: B = %d, T = %d, D = %d must be positive", B, T, D);
    ASR_REQUIRE(freq_masks >= 0 && freq_masks <= PA_FM, ASR_E_ARG, "asr_specaug_policy: freq_masks = %d outside 0..%d", freq_masks, PA_FM);
    ASR_REQUIRE(time_masks >= 0 && time_masks <= PA_TM, ASR_E_ARG, "asr_specaug_policy: time_masks = %d outside 0..%d", time_masks, PA_TM);
    ASR_REQUIRE(warp >= 0 && freq_width >= 0 && time_width >= 0, ASR_E_ARG,
                "asr_specaug_policy: warp = %d, freq_width = %d, time_width = %d must not be negative", warp, freq_width, time_width);
    ASR_REQUIRE(time_ratio_pm >= 0 && time_ratio_pm <= 1000 && time_count_pm >= 0 && time_count_pm <= 1000, ASR_E_ARG,
                "asr_specaug_policy: time_ratio_pm = %d, time_count_pm = %d outside 0..1000", time_ratio_pm, time_count_pm);
    ASR_REQUIRE(fill == 0 || fill == 1, ASR_E_ARG, "asr_specaug_policy: fill = %d is neither 0 (mean) nor 1 (zero)", fill);
    const size_t bytes = (size_t)B * T * D * sizeof(float);
    const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
    ASR_REQUIRE(xa + bytes <= oa || oa + bytes <= xa, ASR_E_ARG, "asr_specaug_policy: x and out overlap (the warp gathers along time)");
    ASR_REQUIRE(fill == 1 || workspace, ASR_E_ARG, "asr_specaug_policy: fill = mean needs a workspace");
    if (workspace)
        ASR_REQUIRE(workspace_bytes >= asr_specaug_policy_workspace_bytes(B) && ((uintptr_t)workspace & 7) == 0, ASR_E_ARG,
                    "asr_specaug_policy: workspace too small or not 8-byte aligned");
    ASR_REQUIRE((long)B * PA_SPLIT <= 0x7fffffffL, ASR_E_ARG, "asr_specaug_policy: B = %d is beyond one grid axis", B);
    const bool vec = (D % 4 == 0) && ((xa | oa) & 15) == 0;
    const long per_utt = (long)T * (vec ? D / 4 : D);
    const int gx = (int)std::min((per_utt + 255) / 256, (long)PA_GRID);
    const PolicyArgs p = {B, T, D, warp, freq_masks, freq_width, time_masks, time_width, time_ratio_pm, time_count_pm, fill, seed};
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
    if (fill == 0) {
        if (vec) hipLaunchKernelGGL(policy_sum_kernel<4>, dim3(B * PA_SPLIT), dim3(256), 0, st, x, lens, part, B, T, D);
        else hipLaunchKernelGGL(policy_sum_kernel<1>, dim3(B * PA_SPLIT), dim3(256), 0, st, x, lens, part, B, T, D);
    }
    if (vec) hipLaunchKernelGGL(policy_apply_kernel<4>, dim3(B * gx), dim3(256), 0, st, x, lens, out, draws_in, draws_out, part, p, gx);
    else hipLaunchKernelGGL(policy_apply_kernel<1>, dim3(B * gx), dim3(256), 0, st, x, lens, out, draws_in, draws_out, part, p, gx);
    ASR_LAUNCH_CHECK("asr_specaug_policy");
    return ASR_OK;
}
