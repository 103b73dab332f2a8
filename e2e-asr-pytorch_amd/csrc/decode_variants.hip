// Beam-search attention of the model variants (scaled-dot / location-aware, any number of heads, value projection or not):
// one output position of BeamDecoder.forward (reference src/decode.py:104-116, the attention of src/asr.py:331-364 at batch
// size one) for U utterances x rows_per_utt hypothesis rows, with the keys / values held once per utterance (not per row).
//
// asr_beam_attend: one workgroup per (utterance, head) serves every hypothesis row of that utterance, so each key and value
// row is read once per position.  Three phases, one thread per frame in the first two:
//   1. energies of all rows for frame t (the key row is read once for all rows; q / w_g indices are wave-uniform);
//   2. masked temperature softmax per row (block reductions of four rows at a time);
//   3. context: threads own 8-column chunks of the value row and a slice of the frames; slices are summed through LDS in a
//      fixed order (deterministic: a row's result does not depend on how many utterances share the launch).
// The energies live in LDS while rows_per_utt * T' fits in 48 KiB (beam 8 up to T' = 1536); above that they are staged in
// the caller's attn output rows themselves (same arithmetic, global memory instead of LDS).
#include "common.h"

namespace {

constexpr int BA_THREADS = 256;
constexpr int BA_RG = 4;                        // hypothesis rows per register group
constexpr int BA_LDS_E_FLOATS = 12288;          // 48 KiB of resident energies
constexpr int BA_RED_FLOATS = BA_THREADS * 8;   // context slice partials (8 KiB)

template <bool BF16>
__device__ __forceinline__ float ld1(const void* base, long i) {
    if (BF16) return __uint_as_float((unsigned)((const unsigned short*)base)[i] << 16);
    return ((const float*)base)[i];
}

// 8 consecutive elements from element index i; vec: 16-byte aligned and in range, else guarded scalar loads (0 past n)
template <bool BF16>
__device__ __forceinline__ void ld8(const void* base, long i, int n, bool vec, float (&v)[8]) {
    if (vec) {
        if (BF16) {
            const uint4 w = *(const uint4*)((const unsigned short*)base + i);
            const unsigned u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[2 * k] = __uint_as_float(u[k] << 16);
                v[2 * k + 1] = __uint_as_float(u[k] & 0xffff0000u);
            }
        } else {
            const float4 a = *(const float4*)((const float*)base + i), b = *(const float4*)((const float*)base + i + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (k < n) ? ld1<BF16>(base, i + k) : 0.f;
    }
}

// four row values reduced over the block at once (max or sum)
template <bool MAX>
__device__ __forceinline__ void block_reduce4(float (&v)[BA_RG], float* s_red) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < BA_RG; ++j) v[j] = MAX ? wave_max(v[j]) : wave_sum(v[j]);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < BA_RG; ++j) s_red[w * BA_RG + j] = v[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < BA_RG; ++j) {
        float t = MAX ? -INFINITY : 0.f;
        for (int i = 0; i < BA_THREADS / 64; ++i) t = MAX ? fmaxf(t, s_red[i * BA_RG + j]) : t + s_red[i * BA_RG + j];
        v[j] = t;
    }
}

template <bool BF16, bool LOC, bool RESIDENT>
__global__ __launch_bounds__(BA_THREADS) void beam_attend_kernel(asr_beam_attend_t a, float inv_temp, bool vec_k, bool vec_v, bool vec_l) {
    extern __shared__ float s_mem[];
    __shared__ float s_red[(BA_THREADS / 64) * BA_RG];
    float* s_part = s_mem;                      // BA_RED_FLOATS
    float* s_e = s_mem + BA_RED_FLOATS;         // rows_per_utt x T' (RESIDENT)
    const int tid = threadIdx.x;
    const int u = blockIdx.x / a.NH, n = blockIdx.x % a.NH, nv = (a.NHv == 1) ? 0 : n;
    const int rows = a.rows_per_utt, Tp = a.Tp, A = a.A, Dv = a.Dv;
    const int r0 = u * rows;
    const int L = (int)min((long)a.enc_len[u], (long)Tp);
    auto erow = [&](int i) -> float* {
        return RESIDENT ? s_e + (long)i * Tp : a.attn + (long)(r0 + i) * a.attn_ld + (long)n * Tp;
    };
    const long kbase = ((long)u * a.NH + n) * Tp * a.ld_k;
    const long vbase = ((long)u * a.NHv + nv) * Tp * a.ld_v;

    // ---- 1. energies e[i][t] / temperature, t < L
    for (int g0 = 0; g0 < rows; g0 += BA_RG) {
        for (int t = tid; t < L; t += BA_THREADS) {
            float acc[BA_RG] = {0.f, 0.f, 0.f, 0.f};
            const long krow = kbase + (long)t * a.ld_k;
            for (int a0 = 0; a0 < A; a0 += 8) {
                const int kn = min(8, A - a0);
                float k8[8];
                ld8<BF16>(a.key, krow + a0, kn, vec_k && kn == 8, k8);
#pragma unroll
                for (int j = 0; j < BA_RG; ++j) {
                    if (g0 + j >= rows) break;
                    const int r = r0 + g0 + j;
                    const float* qr = a.q + ((long)r * a.NH + n) * A + a0;
                    if (LOC) {
                        float l8[8];
                        ld8<false>(a.loc, ((long)r * Tp + t) * a.ld_l + a0, kn, vec_l && kn == 8, l8);
#pragma unroll
                        for (int k = 0; k < 8; ++k)
                            if (k < kn) acc[j] += a.wg[a0 + k] * tanhf(k8[k] + qr[k] + l8[k]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 8; ++k)
                            if (k < kn) acc[j] += qr[k] * k8[k];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < BA_RG; ++j)
                if (g0 + j < rows) erow(g0 + j)[t] = ((LOC ? acc[j] + a.bg[0] : acc[j])) * inv_temp;
        }
    }
    __syncthreads();

    // ---- 2. softmax over t < L per row, exact zeros past L in the attn output
    for (int g0 = 0; g0 < rows; g0 += BA_RG) {
        float m[BA_RG], s[BA_RG];
#pragma unroll
        for (int j = 0; j < BA_RG; ++j) {
            m[j] = -INFINITY;
            if (g0 + j < rows)
                for (int t = tid; t < L; t += BA_THREADS) m[j] = fmaxf(m[j], erow(g0 + j)[t]);
        }
        block_reduce4<true>(m, s_red);
#pragma unroll
        for (int j = 0; j < BA_RG; ++j) {
            s[j] = 0.f;
            if (g0 + j < rows)
                for (int t = tid; t < L; t += BA_THREADS) s[j] += expf(erow(g0 + j)[t] - m[j]);
        }
        block_reduce4<false>(s, s_red);
#pragma unroll
        for (int j = 0; j < BA_RG; ++j) {
            if (g0 + j >= rows) break;
            const float inv = (s[j] > 0.f) ? 1.f / s[j] : 0.f;
            float* e = erow(g0 + j);
            float* out = a.attn + (long)(r0 + g0 + j) * a.attn_ld + (long)n * Tp;
            for (int t = tid; t < Tp; t += BA_THREADS) {
                const float p = (t < L) ? expf(e[t] - m[j]) * inv : 0.f;
                if (RESIDENT && t < L) e[t] = p;
                out[t] = p;
            }
        }
    }
    __syncthreads();

    // ---- 3. ctx[r, n*Dv + c] = sum_{t<L} attn[r,t] value[u, nv, t, c]
    const int nch = (Dv + 7) / 8;
    const int S = (nch >= BA_THREADS) ? 1 : BA_THREADS / nch;
    const int slice = (S == 1) ? 0 : tid / nch;
    const bool active = slice < S;
    auto accumulate = [&](int g0, int c, float (&acc)[BA_RG][8]) {
#pragma unroll
        for (int j = 0; j < BA_RG; ++j)
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[j][k] = 0.f;
        const int cn = min(8, Dv - c * 8);
        for (int t = slice; t < L; t += S) {
            float v8[8];
            ld8<BF16>(a.value, vbase + (long)t * a.ld_v + c * 8, cn, vec_v && cn == 8, v8);
#pragma unroll
            for (int j = 0; j < BA_RG; ++j) {
                if (g0 + j >= rows) break;
                const float p = erow(g0 + j)[t];
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[j][k] += p * v8[k];
            }
        }
    };
    for (int g0 = 0; g0 < rows; g0 += BA_RG) {
        float acc[BA_RG][8];
        if (S == 1) {
            // every thread owns whole columns: no reduction, no barrier
            for (int c = tid; c < nch; c += BA_THREADS) {
                accumulate(g0, c, acc);
                const int cn = min(8, Dv - c * 8);
#pragma unroll
                for (int j = 0; j < BA_RG; ++j) {
                    if (g0 + j >= rows) break;
                    float* out = a.ctx + (long)(r0 + g0 + j) * a.ctx_ld + (long)n * Dv + c * 8;
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (k < cn) out[k] = acc[j][k];
                }
            }
        } else {
            // S frame slices per column chunk; the partials of one row at a time are summed through s_part in slice order.
            // The barriers stay in block-uniform control flow (the idle threads tid >= S * nch share waves with active ones).
            if (active) accumulate(g0, tid % nch, acc);
#pragma unroll
            for (int j = 0; j < BA_RG; ++j) {
                if (g0 + j >= rows) break;
                __syncthreads();
                if (active)
#pragma unroll
                    for (int k = 0; k < 8; ++k) s_part[(slice * nch + tid % nch) * 8 + k] = acc[j][k];
                __syncthreads();
                float* out = a.ctx + (long)(r0 + g0 + j) * a.ctx_ld + (long)n * Dv;
                for (int col = tid; col < Dv; col += BA_THREADS) {
                    float v = 0.f;
                    for (int sl = 0; sl < S; ++sl) v += s_part[sl * nch * 8 + col];
                    out[col] = v;
                }
            }
        }
    }
}

template <bool BF16, bool LOC>
void launch(const asr_beam_attend_t& a, bool resident, bool vk, bool vv, bool vl, hipStream_t st) {
    const size_t lds = sizeof(float) * (BA_RED_FLOATS + (resident ? (size_t)a.rows_per_utt * a.Tp : 0));
    if (resident)
        hipLaunchKernelGGL((beam_attend_kernel<BF16, LOC, true>), dim3(a.U * a.NH), dim3(BA_THREADS), lds, st, a, 1.f / a.temperature, vk, vv, vl);
    else
        hipLaunchKernelGGL((beam_attend_kernel<BF16, LOC, false>), dim3(a.U * a.NH), dim3(BA_THREADS), lds, st, a, 1.f / a.temperature, vk, vv, vl);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int asr_beam_attend(const asr_beam_attend_t* args, asr_stream_t stream) {
    ASR_REQUIRE(args, ASR_E_ARG, "asr_beam_attend: null args");
    const asr_beam_attend_t& a = *args;
    ASR_REQUIRE(a.key && a.value && a.q && a.enc_len && a.attn && a.ctx, ASR_E_ARG, "asr_beam_attend: null pointer");
    ASR_REQUIRE(a.mode == ASR_ATT_DOT || a.mode == ASR_ATT_LOC, ASR_E_ARG, "asr_beam_attend: mode %d", a.mode);
    ASR_REQUIRE(a.mode == ASR_ATT_DOT || (a.loc && a.wg && a.bg), ASR_E_ARG, "asr_beam_attend: loc mode needs loc, wg, bg");
    ASR_REQUIRE(a.U > 0 && a.rows_per_utt > 0 && a.NH > 0 && (a.NHv == 1 || a.NHv == a.NH) && a.Tp > 0 && a.A > 0 && a.Dv > 0 &&
                    a.temperature > 0.f && a.ld_k >= a.A && a.ld_v >= a.Dv && a.attn_ld >= (long)a.NH * a.Tp &&
                    a.ctx_ld >= (long)a.NH * a.Dv && (a.mode == ASR_ATT_DOT || a.ld_l >= a.A) && (a.kv_bf16 == 0 || a.kv_bf16 == 1),
                ASR_E_ARG, "asr_beam_attend: bad dims");
    ASR_REQUIRE(a.rows_per_utt <= ASR_BEAM_ATTEND_MAX_ROWS, ASR_E_UNSUPPORTED, "asr_beam_attend: rows_per_utt %d above %d", a.rows_per_utt,
                ASR_BEAM_ATTEND_MAX_ROWS);
    ASR_REQUIRE(a.Tp <= ASR_BEAM_ATTEND_MAX_T, ASR_E_UNSUPPORTED, "asr_beam_attend: T' %d above %d", a.Tp, ASR_BEAM_ATTEND_MAX_T);
    const int vw = a.kv_bf16 ? 8 : 4;           // elements per 16 bytes
    const bool vk = a.ld_k % vw == 0 && aligned16(a.key);
    const bool vv = a.ld_v % vw == 0 && aligned16(a.value);
    const bool vl = a.mode == ASR_ATT_LOC && a.ld_l % 4 == 0 && aligned16(a.loc);
    const bool resident = (long)a.rows_per_utt * a.Tp <= BA_LDS_E_FLOATS;
    hipStream_t st = (hipStream_t)stream;
    const bool loc = a.mode == ASR_ATT_LOC;
    if (a.kv_bf16) {
        if (loc) launch<true, true>(a, resident, vk, vv, vl, st); else launch<true, false>(a, resident, vk, vv, vl, st);
    } else {
        if (loc) launch<false, true>(a, resident, vk, vv, vl, st); else launch<false, false>(a, resident, vk, vv, vl, st);
    }
    ASR_LAUNCH_CHECK("asr_beam_attend");
    return ASR_OK;
}

extern "C" int asr_beam_attend_resident_max_t(int rows_per_utt) {
    return rows_per_utt > 0 ? BA_LDS_E_FLOATS / rows_per_utt : 0;
}
