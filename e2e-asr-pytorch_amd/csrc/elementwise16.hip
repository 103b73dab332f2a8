// HBM-bound glue kernels of the bf16-storage encoder stack (bf16 contraction mode): casts, the per-step bf16 weight
// copies of an RNN layer, dropout + time down-sampling, activation backward and bias-gradient column sums on bf16
// tensors (reference RNNLayer.forward, src/module.py:1040-1081, and its autograd).  16 bytes per lane everywhere.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

__device__ __forceinline__ float bf2f(unsigned short v) { return __uint_as_float((unsigned)v << 16); }
__device__ __forceinline__ unsigned pack2(float a, float b) { return (unsigned)f2bf_bits(a) | ((unsigned)f2bf_bits(b) << 16); }
__device__ __forceinline__ void unpack8(const u32x4_t& v, float (&f)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = __uint_as_float(v[i] << 16); f[2 * i + 1] = __uint_as_float(v[i] & 0xFFFF0000u); }
}
__device__ __forceinline__ u32x4_t pack8(const float (&f)[8]) {
    u32x4_t v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = pack2(f[2 * i], f[2 * i + 1]);
    return v;
}

inline int grid_for(long n) { long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g)); }
inline uint32_t drop_thresh(float p) {
    if (p <= 0.f) return 0u;
    double v = (double)p * 4294967296.0;
    return v >= 4294967295.0 ? 4294967295u : (uint32_t)v;
}

__global__ void cast_to_bf16_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, long n) {
    const long n8 = n >> 3;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        const float4 a = reinterpret_cast<const float4*>(src)[2 * i], b = reinterpret_cast<const float4*>(src)[2 * i + 1];
        const float f[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        reinterpret_cast<u32x4_t*>(dst)[i] = pack8(f);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 7)) dst[(n8 << 3) + threadIdx.x] = f2bf_bits(src[(n8 << 3) + threadIdx.x]);
}
__global__ void cast_to_f32_kernel(const unsigned short* __restrict__ src, float* __restrict__ dst, long n, int accum) {
    const long n8 = n >> 3;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        float f[8];
        unpack8(reinterpret_cast<const u32x4_t*>(src)[i], f);
        float4* d = reinterpret_cast<float4*>(dst) + 2 * i;
        if (accum) {
            const float4 a = d[0], b = d[1];
            d[0] = make_float4(a.x + f[0], a.y + f[1], a.z + f[2], a.w + f[3]);
            d[1] = make_float4(b.x + f[4], b.y + f[5], b.z + f[6], b.w + f[7]);
        } else {
            d[0] = make_float4(f[0], f[1], f[2], f[3]);
            d[1] = make_float4(f[4], f[5], f[6], f[7]);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 7)) {
        const long j = (n8 << 3) + threadIdx.x;
        const float v = bf2f(src[j]);
        dst[j] = accum ? dst[j] + v : v;                                 // not 0.f + v: that turns -0 into +0
    }
}

// bf16 copies of one RNN layer's contraction weights, rebuilt from the fp32 master once per step:
//   wih16  (ND*4H, Din): W_ih rows re-ordered gate-minor: row d*4H + u*4 + g  <-  reference row d*4H + g*H + u
//   wihT16 (Din, ND*4H): its transpose (operand of the input-gradient contraction)
//   bias   (ND*4H) fp32: b_ih + b_hh in the same row order (added by the input projection's epilogue)
//   pj16 (D,D), pjT16 (D,D): the projection weight and its transpose (optional)
struct PackP {
    const float* wih; const float* bih; const float* bhh; const float* pj;
    unsigned short* wih16; unsigned short* wihT16; float* bias; unsigned short* pj16; unsigned short* pjT16;
    int H, ND, Din, D;
};
__global__ __launch_bounds__(256) void pack_weights_kernel(PackP p) {
    __shared__ float tile[32][33];
    const int G = p.ND * 4 * p.H;
    // job list: tiles of 32x32 of W_ih (rows permuted) then of pj
    const int tr_ih = (G + 31) / 32, tc_ih = (p.Din + 31) / 32;
    const int n_ih = tr_ih * tc_ih;
    const int tr_pj = p.pj ? (p.D + 31) / 32 : 0, n_pj = tr_pj * tr_pj;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8
    for (int job = blockIdx.x; job < n_ih + n_pj; job += gridDim.x) {
        const bool ih = job < n_ih;
        const int j = ih ? job : job - n_ih;
        const int tcn = ih ? tc_ih : tr_pj;
        const int r0 = (j / tcn) * 32, c0 = (j % tcn) * 32;
        const int R = ih ? G : p.D, C = ih ? p.Din : p.D;
        const float* src = ih ? p.wih : p.pj;
        unsigned short* dst = ih ? p.wih16 : p.pj16;
        unsigned short* dstT = ih ? p.wihT16 : p.pjT16;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = r0 + ty + 8 * k, c = c0 + tx;            // r = destination (gate-minor) row
            float v = 0.f;
            if (r < R && c < C) {
                int rs = r;
                if (ih) { const int h4 = 4 * p.H, blk = r / h4, rr = r - blk * h4; rs = blk * h4 + (rr & 3) * p.H + (rr >> 2); }
                v = src[(long)rs * C + c];
                dst[(long)r * C + c] = f2bf_bits(v);
            }
            tile[ty + 8 * k][tx] = v;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + ty + 8 * k, r = r0 + tx;
            if (r < R && c < C) dstT[(long)c * R + r] = f2bf_bits(tile[tx][ty + 8 * k]);
        }
    }
    if (blockIdx.x == 0)
        for (int r = threadIdx.x; r < G; r += 256) {
            const int h4 = 4 * p.H, blk = r / h4, rr = r - blk * h4, rs = blk * h4 + (rr & 3) * p.H + (rr >> 2);
            p.bias[r] = p.bih[rs] + p.bhh[rs];
        }
}

// dropout + time down-sampling on bf16: y (B, T [+2 padded], D) -> z (B,T2,Dz);  the keep decision of element (b,t,k) is
// Philox(seed, flat index (b*T + t)*D + k) exactly as in the fp32 kernels (asr_dropout_mask exports it).
struct Ds16P { const unsigned short* src; unsigned short* dst; long y_bstride, y_off; int B, T, D, T2, rate, style; float scale; uint32_t thresh; uint64_t seed; };
template <bool BWD>
__global__ void dropout_downsample16_kernel(Ds16P p) {
    // forward: src = y (time rows at y_off + b*y_bstride + t*D), dst = z;  backward: src = dz, dst = dy (B,T,D) fully written
    const int D8 = p.D >> 3;
    const long rows = (long)p.B * p.T, total8 = rows * D8;
    for (long j = blockIdx.x * (long)blockDim.x + threadIdx.x; j < total8; j += (long)gridDim.x * blockDim.x) {
        const long row = j / D8;
        const int k8 = (int)(j - row * D8);
        const int b = (int)(row / p.T), t = (int)(row - (long)b * p.T);
        long zi = -1;
        if (p.style == 0) {
            if (t % p.rate == 0 && t / p.rate < p.T2) zi = ((long)b * p.T2 + t / p.rate) * p.D + 8 * k8;
        } else {
            if (t < p.T2 * p.rate) zi = ((long)b * p.T2 + t / p.rate) * ((long)p.D * p.rate) + (long)(t % p.rate) * p.D + 8 * k8;
        }
        const long i = 8 * j;                                            // flat index in y: two Philox blocks
        if (!BWD && zi < 0) continue;
        float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (zi >= 0) {
            const long yi = p.y_off + (long)b * p.y_bstride + (long)t * p.D + 8 * k8;
            unpack8(*reinterpret_cast<const u32x4_t*>(p.src + (BWD ? zi : yi)), f);
            uint32_t r[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
            if (p.thresh != 0) {
                const uint64_t blk = (uint64_t)i >> 2;
                philox4x32((uint32_t)blk, (uint32_t)(blk >> 32), 0u, 0u, (uint32_t)p.seed, (uint32_t)(p.seed >> 32), r);
                philox4x32((uint32_t)(blk + 1), (uint32_t)((blk + 1) >> 32), 0u, 0u, (uint32_t)p.seed, (uint32_t)(p.seed >> 32), r + 4);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = (r[e] >= p.thresh) ? f[e] * p.scale : 0.f;
        }
        *reinterpret_cast<u32x4_t*>(p.dst + (BWD ? i : zi)) = pack8(f);
    }
}

__global__ void act_bwd16_kernel(const unsigned short* __restrict__ dout, const unsigned short* __restrict__ out,
                                 unsigned short* __restrict__ dpre, long n8, int act) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        float g[8], o[8];
        unpack8(reinterpret_cast<const u32x4_t*>(dout)[i], g);
        unpack8(reinterpret_cast<const u32x4_t*>(out)[i], o);
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = (act == ASR_ACT_TANH) ? g[e] * (1.f - o[e] * o[e]) : ((o[e] > 0.f) ? g[e] : 0.f);
        reinterpret_cast<u32x4_t*>(dpre)[i] = pack8(g);
    }
}

// column sums of a bf16 (M,N) matrix (row stride lda), added into out[perm(col)] (and out2): 8 columns per thread
__global__ __launch_bounds__(256) void colsum16_kernel(const unsigned short* __restrict__ A, long lda, int M, int N,
                                                       float* __restrict__ out, float* __restrict__ out2, int rows_per_block, int permH) {
    __shared__ float red[8][32][9];
    const int cg = threadIdx.x & 31, grp = threadIdx.x >> 5;        // 32 column groups of 8 x 8 row groups
    const int col = (blockIdx.x * 32 + cg) * 8;
    const int r0 = blockIdx.y * rows_per_block, r1 = min(M, r0 + rows_per_block);
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (col < N) {
        int r = r0 + grp;
        for (; r + 8 < r1; r += 16) {
            float a[8], b[8];
            unpack8(*reinterpret_cast<const u32x4_t*>(A + (long)r * lda + col), a);
            unpack8(*reinterpret_cast<const u32x4_t*>(A + (long)(r + 8) * lda + col), b);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += a[e] + b[e];
        }
        for (; r < r1; r += 8) {
            float a[8];
            unpack8(*reinterpret_cast<const u32x4_t*>(A + (long)r * lda + col), a);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += a[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[grp][cg][e] = s[e];
    __syncthreads();
    const int c = threadIdx.x;                                      // 256 columns of this block
    const int gc = blockIdx.x * 256 + c;
    if (gc < N) {
        float v = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) v += red[g][c >> 3][c & 7];
        int oc = gc;
        if (permH > 0) { const int h4 = 4 * permH, blk = gc / h4, rr = gc - blk * h4; oc = blk * h4 + (rr & 3) * permH + (rr >> 2); }
        atomicAdd(out + oc, v);
        if (out2) atomicAdd(out2 + oc, v);
    }
}

}  // namespace

extern "C" int asr_cast_bf16(const float* src, void* dst, long n, asr_stream_t stream) {
    ASR_REQUIRE(src && dst && n > 0, ASR_E_ARG, "asr_cast_bf16: bad args");
    ASR_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, ASR_E_ARG, "asr_cast_bf16: 16-byte alignment");
    hipLaunchKernelGGL(cast_to_bf16_kernel, dim3(grid_for(n / 8 + 1)), dim3(256), 0, (hipStream_t)stream, src, (unsigned short*)dst, n);
    ASR_LAUNCH_CHECK("asr_cast_bf16");
    return ASR_OK;
}

extern "C" int asr_cast_f32(const void* src, float* dst, long n, int accum, asr_stream_t stream) {
    ASR_REQUIRE(src && dst && n > 0, ASR_E_ARG, "asr_cast_f32: bad args");
    ASR_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, ASR_E_ARG, "asr_cast_f32: 16-byte alignment");
    hipLaunchKernelGGL(cast_to_f32_kernel, dim3(grid_for(n / 8 + 1)), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)src, dst, n, accum);
    ASR_LAUNCH_CHECK("asr_cast_f32");
    return ASR_OK;
}

extern "C" int asr_rnn_pack_weights(const float* w_ih, const float* b_ih, const float* b_hh, const float* pj,
                                    void* w_ih16, void* w_ihT16, float* bias, void* pj16, void* pjT16,
                                    int H, int ND, int Din, int D, asr_stream_t stream) {
    ASR_REQUIRE(w_ih && b_ih && b_hh && w_ih16 && w_ihT16 && bias, ASR_E_ARG, "asr_rnn_pack_weights: null pointer");
    ASR_REQUIRE(H > 0 && (ND == 1 || ND == 2) && Din > 0, ASR_E_ARG, "asr_rnn_pack_weights: bad dims");
    ASR_REQUIRE(!pj || (pj16 && pjT16 && D > 0), ASR_E_ARG, "asr_rnn_pack_weights: projection copies missing");
    PackP p{w_ih, b_ih, b_hh, pj, (unsigned short*)w_ih16, (unsigned short*)w_ihT16, bias, (unsigned short*)pj16, (unsigned short*)pjT16, H, ND, Din, D};
    hipLaunchKernelGGL(pack_weights_kernel, dim3(1024), dim3(256), 0, (hipStream_t)stream, p);
    ASR_LAUNCH_CHECK("asr_rnn_pack_weights");
    return ASR_OK;
}

extern "C" int asr_dropout_downsample16_fwd(const void* y, long y_bstride, long y_off, void* z, int B, int T, int D, int T2, int rate,
                                            int style, float p, uint64_t seed, asr_stream_t stream) {
    ASR_REQUIRE(y && z && B > 0 && T > 0 && D > 0 && T2 > 0 && rate >= 1, ASR_E_ARG, "asr_dropout_downsample16_fwd: bad args");
    ASR_DS_REQUIRE("asr_dropout_downsample16_fwd");
    ASR_REQUIRE(D % 8 == 0 && y_bstride % 8 == 0 && y_off % 8 == 0 && (((uintptr_t)y | (uintptr_t)z) & 15) == 0, ASR_E_UNSUPPORTED,
                "asr_dropout_downsample16_fwd: rows of 8 bf16, 16-byte aligned");
    Ds16P a{(const unsigned short*)y, (unsigned short*)z, y_bstride, y_off, B, T, D, T2, rate, style, 1.f / (1.f - p), drop_thresh(p), seed};
    hipLaunchKernelGGL(dropout_downsample16_kernel<false>, dim3(grid_for((long)B * T * (D / 8))), dim3(256), 0, (hipStream_t)stream, a);
    ASR_LAUNCH_CHECK("asr_dropout_downsample16_fwd");
    return ASR_OK;
}

extern "C" int asr_dropout_downsample16_bwd(const void* dz, void* dy, int B, int T, int D, int T2, int rate, int style,
                                            float p, uint64_t seed, asr_stream_t stream) {
    ASR_REQUIRE(dz && dy && B > 0 && T > 0 && D > 0 && T2 > 0 && rate >= 1, ASR_E_ARG, "asr_dropout_downsample16_bwd: bad args");
    ASR_DS_REQUIRE("asr_dropout_downsample16_bwd");
    ASR_REQUIRE(D % 8 == 0 && (((uintptr_t)dz | (uintptr_t)dy) & 15) == 0, ASR_E_UNSUPPORTED, "asr_dropout_downsample16_bwd: rows of 8 bf16, 16-byte aligned");
    Ds16P a{(const unsigned short*)dz, (unsigned short*)dy, (long)T * D, 0, B, T, D, T2, rate, style, 1.f / (1.f - p), drop_thresh(p), seed};
    hipLaunchKernelGGL(dropout_downsample16_kernel<true>, dim3(grid_for((long)B * T * (D / 8))), dim3(256), 0, (hipStream_t)stream, a);
    ASR_LAUNCH_CHECK("asr_dropout_downsample16_bwd");
    return ASR_OK;
}

extern "C" int asr_act_bwd16(const void* dout, const void* out, void* dpre, long n, int act, asr_stream_t stream) {
    ASR_REQUIRE(dout && out && dpre && n > 0 && n % 8 == 0, ASR_E_ARG, "asr_act_bwd16: bad args (n must be a multiple of 8)");
    ASR_REQUIRE(act == ASR_ACT_TANH || act == ASR_ACT_RELU, ASR_E_ARG, "asr_act_bwd16: bad act");
    hipLaunchKernelGGL(act_bwd16_kernel, dim3(grid_for(n / 8)), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)dout,
                       (const unsigned short*)out, (unsigned short*)dpre, n / 8, act);
    ASR_LAUNCH_CHECK("asr_act_bwd16");
    return ASR_OK;
}

extern "C" int asr_colsum16(const void* A, long lda, int M, int N, float* out, float* out2, int perm_h, asr_stream_t stream) {
    ASR_REQUIRE(A && out && M > 0 && N > 0 && lda >= N, ASR_E_ARG, "asr_colsum16: bad args");
    ASR_REQUIRE(N % 8 == 0 && lda % 8 == 0 && ((uintptr_t)A & 15) == 0, ASR_E_UNSUPPORTED, "asr_colsum16: rows of 8 bf16, 16-byte aligned");
    ASR_REQUIRE(perm_h == 0 || N % (4 * perm_h) == 0, ASR_E_ARG, "asr_colsum16: perm_h does not divide N");
    int rows_per_block = 512;
    while (rows_per_block > 32 && (long)cdiv(N, 256) * cdiv(M, rows_per_block) < 1024) rows_per_block >>= 1;
    dim3 grid(cdiv(N, 256), cdiv(M, rows_per_block));
    hipLaunchKernelGGL(colsum16_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned short*)A, lda, M, N, out, out2, rows_per_block, perm_h);
    ASR_LAUNCH_CHECK("asr_colsum16");
    return ASR_OK;
}
