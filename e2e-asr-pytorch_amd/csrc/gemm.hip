// MFMA contraction kernel for every "large-M" linear map on the training path:
//   C[i,j] (+)= act( sum_r opA(i,r) * opB(r,j) + bias[j] )
// opA is stored either [i][r] (a_kc=1, reduction index contiguous) or [r][i] (a_kc=0);
// opB is stored either [j][r] (b_kc=1) or [r][j] (b_kc=0).
//   a_kc=1,b_kc=1 : y = x W^T          (nn.Linear forward; reference src/module.py:1079, src/asr.py:30,345)
//   a_kc=1,b_kc=0 : dx = dy W          (its input gradient)
//   a_kc=0,b_kc=0 : dW = dy^T x        (its weight gradient; reduction over B*T rows, split over blocks)
// Operands live in HBM as fp32; PREC selects the MFMA: bf16 inputs (converted while staging into LDS,
// f32 accumulate) or exact f32-input MFMA (parity mode).
// Tile: 128x128x32 per 256-thread workgroup, 4 waves as 2x2, each wave 4x4 tiles of 16x16.
#include "gemm_plan.h"
#include <stdlib.h>

namespace {

constexpr int BM = 128, BN = 128, BK = 32;
constexpr int NT = 256;

// source row offset and validity of tap (dt,df) for pixel row m
__device__ __forceinline__ bool conv_tap(int m, int tap, int cT, int cF, long& src_row) {
    const int f = m % cF, t = (m / cF) % cT;
    const int dt = tap / 3 - 1, df = tap % 3 - 1;
    src_row = (long)m + (long)dt * cF + df;
    return (unsigned)(t + dt) < (unsigned)cT && (unsigned)(f + df) < (unsigned)cF;
}

// One operand tile in LDS.  KC=true : image [row][k] (row = i or j), k contiguous.
//                           KC=false: image [k][row], row contiguous (same as memory).
template <bool BF16, bool KC> struct TileLayout;
template <> struct TileLayout<true, true>   { static constexpr int LD = BK;      static constexpr int ELEMS = 128 * BK; };
template <> struct TileLayout<true, false>  { static constexpr int LD = 128 + 8; static constexpr int ELEMS = BK * (128 + 8); };
template <> struct TileLayout<false, true>  { static constexpr int LD = BK + 1;  static constexpr int ELEMS = 128 * (BK + 1); };
template <> struct TileLayout<false, false> { static constexpr int LD = 128 + 4; static constexpr int ELEMS = BK * (128 + 4); };

// Global -> registers: each thread fetches 4 x float4 of a 128 x 32 operand tile.
//  KC : element (row, k) at base[row*ld + k];  thread -> row = tid/8 + 32q, k4 = (tid%8)*4
//  !KC: element (row, k) at base[k*ld + row];  thread -> k = tid/32 + 8q, row4 = (tid%32)*4
// rmask(k) gives validity of reduction index k (used for the shifted/masked wgrad operand).
template <bool KC>
__device__ __forceinline__ void fetch_tile(const float* __restrict__ base, long ld, int row0, int nrows,
                                           int k0, int kend, int vec, int seqT, int shift, float4 (&r)[4],
                                           int conv = 0, int cT = 0, int cF = 0, int cC = 0) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (conv) {
            // element (pixel row m, k = tap*cC + ci) = image[(m + dt*cF + df)*cC + ci]
            int m, k;
            if (KC) { m = row0 + (tid >> 3) + 32 * q; k = k0 + (tid & 7) * 4; }
            else    { m = k0 + (tid >> 5) + 8 * q;   k = row0 + (tid & 31) * 4; }
            const int mend = KC ? nrows : kend, kk_end = KC ? kend : nrows;
            if (m < mend && k < kk_end) {
                float e[4] = {0.f, 0.f, 0.f, 0.f};
                if (vec && (cC & 3) == 0 && k + 3 < kk_end) {   // vec: the image base is 16-byte aligned (gemm_plan)
                    long src;
                    if (conv_tap(m, k / cC, cT, cF, src)) {
                        const float4 t4 = *reinterpret_cast<const float4*>(base + src * cC + (k % cC));
                        e[0] = t4.x; e[1] = t4.y; e[2] = t4.z; e[3] = t4.w;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        long src;
                        if (k + i < kk_end && conv_tap(m, (k + i) / cC, cT, cF, src)) e[i] = base[src * cC + ((k + i) % cC)];
                    }
                }
                v = make_float4(e[0], e[1], e[2], e[3]);
            }
        } else if (KC) {
            int row = row0 + (tid >> 3) + 32 * q;
            int k = k0 + (tid & 7) * 4;
            if (row < nrows) {
                const float* p = base + (long)row * ld + k;
                if (vec && k + 3 < kend) {
                    v = *reinterpret_cast<const float4*>(p);
                } else {
                    if (k + 0 < kend) v.x = p[0];
                    if (k + 1 < kend) v.y = p[1];
                    if (k + 2 < kend) v.z = p[2];
                    if (k + 3 < kend) v.w = p[3];
                }
            }
        } else {
            int k = k0 + (tid >> 5) + 8 * q;
            int row = row0 + (tid & 31) * 4;
            bool ok = k < kend;
            long ksrc = k;
            if (seqT > 0) {
                int t = k % seqT + shift;
                ok = ok && (t >= 0) && (t < seqT);
                ksrc = (long)k + shift;
            }
            if (ok) {
                const float* p = base + ksrc * ld + row;
                if (vec && row + 3 < nrows) {
                    v = *reinterpret_cast<const float4*>(p);
                } else {
                    if (row + 0 < nrows) v.x = p[0];
                    if (row + 1 < nrows) v.y = p[1];
                    if (row + 2 < nrows) v.z = p[2];
                    if (row + 3 < nrows) v.w = p[3];
                }
            }
        }
        r[q] = v;
    }
}

// Fast variant of fetch_tile for the common case (no convolution, 16-byte aligned rows, the contiguous extent a
// multiple of 4): every load is issued unconditionally from a CLAMPED address and zeroed afterwards by a select.
// (Loads under lane-dependent conditions are compiled into a branch + `s_waitcnt vmcnt(0)` each: the 8 loads of a tile
// became 8 serialized round trips per k-step, which - not bandwidth, not the MFMA - set the speed of this kernel.)
template <bool KC>
__device__ __forceinline__ void fetch_tile_fast(const float* __restrict__ base, long ld, int row0, int nrows,
                                                int k0, int kend, int seqT, int shift, float4 (&r)[4]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        bool ok;
        const float* ptr;
        if (KC) {
            const int row = row0 + (tid >> 3) + 32 * q;
            const int k = k0 + (tid & 7) * 4;
            ok = row < nrows && k < kend;                       // kend % 4 == 0: a float4 is all in or all out
            ptr = base + (long)min(row, nrows - 1) * ld + min(k, kend - 4);
        } else {
            const int k = k0 + (tid >> 5) + 8 * q;
            const int row = row0 + (tid & 31) * 4;
            ok = k < kend && row < nrows;                       // nrows % 4 == 0
            long ksrc = min(k, kend - 1);
            if (seqT > 0) {
                const int t = k % seqT + shift;
                ok = ok && (t >= 0) && (t < seqT);
                ksrc = min(max(ksrc + shift, 0L), (long)kend - 1);
            }
            ptr = base + ksrc * ld + min(row, nrows - 4);
        }
        const float4 v = *reinterpret_cast<const float4*>(ptr);
        r[q] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// bf16-storage loaders: a 128 x 32 operand tile is 8 KB = two 16-byte loads per thread.
//  KC : thread -> row = tid/4 + 64q, k8 = (tid%4)*8      (K % 8 == 0, rows 16-byte aligned)
//  !KC: thread -> k = tid/16 + 16q, row8 = (tid%16)*8    (row extent % 8 == 0)
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
template <bool KC>
__device__ __forceinline__ void fetch_tile16(const unsigned short* __restrict__ base, long ld, int row0, int nrows,
                                             int k0, int kend, int seqT, int shift, int padT, u32x4_t (&r)[2]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        bool ok;
        const unsigned short* ptr;
        if (KC) {
            const int row = row0 + (tid >> 2) + 64 * q;
            const int k = k0 + (tid & 3) * 8;
            ok = row < nrows && k < kend;
            ptr = base + (long)min(row, nrows - 1) * ld + min(k, kend - 8);
        } else {
            const int k = k0 + (tid >> 4) + 16 * q;
            const int row = row0 + (tid & 15) * 8;
            ok = k < kend && row < nrows;
            long ksrc = min(k, kend - 1);
            if (seqT > 0) {
                if (padT) {
                    ksrc = ksrc + 2 * (ksrc / seqT) + 1 + shift;
                } else {
                    const int t = k % seqT + shift;
                    ok = ok && (t >= 0) && (t < seqT);
                    ksrc = min(max(ksrc + shift, 0L), (long)kend - 1);
                }
            }
            ptr = base + ksrc * ld + min(row, nrows - 8);
        }
        const u32x4_t v = *reinterpret_cast<const u32x4_t*>(ptr);
        r[q] = ok ? v : (u32x4_t){0u, 0u, 0u, 0u};
    }
}
template <bool KC>
__device__ __forceinline__ void stash_tile16(void* lds, const u32x4_t (&r)[2]) {
    const int tid = threadIdx.x;
    constexpr int LD = TileLayout<true, KC>::LD;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        int a, b;
        if (KC) { a = (tid >> 2) + 64 * q; b = (tid & 3) * 8; }
        else    { a = (tid >> 4) + 16 * q; b = (tid & 15) * 8; }
        *reinterpret_cast<u32x4_t*>(reinterpret_cast<unsigned short*>(lds) + a * LD + b) = r[q];
    }
}

template <bool BF16, bool KC>
__device__ __forceinline__ void stash_tile(void* lds, const float4 (&r)[4]) {
    const int tid = threadIdx.x;
    constexpr int LD = TileLayout<BF16, KC>::LD;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int a, b;   // a = leading index of the image, b = contiguous index
        if (KC) { a = (tid >> 3) + 32 * q; b = (tid & 7) * 4; }
        else    { a = (tid >> 5) + 8 * q;  b = (tid & 31) * 4; }
        if (BF16) {
            __bf16* s = reinterpret_cast<__bf16*>(lds) + a * LD + b;
            bf16x4 v;
            v[0] = (__bf16)r[q].x; v[1] = (__bf16)r[q].y; v[2] = (__bf16)r[q].z; v[3] = (__bf16)r[q].w;
            *reinterpret_cast<bf16x4*>(s) = v;
        } else {
            float* s = reinterpret_cast<float*>(lds) + a * LD + b;
            if (KC) { s[0] = r[q].x; s[1] = r[q].y; s[2] = r[q].z; s[3] = r[q].w; }
            else    { *reinterpret_cast<float4*>(s) = r[q]; }
        }
    }
}

// Fragment of a 16-row slab starting at `row0` of the tile for MFMA k-step `ks`.
template <bool KC>
__device__ __forceinline__ bf16x8 frag_bf16(const void* lds, int row0, int ks) {
    const int lane = threadIdx.x & 63;
    const __bf16* s = reinterpret_cast<const __bf16*>(lds);
    const int row = row0 + (lane & 15);
    const int k = ks * 32 + 8 * (lane >> 4);
    if (KC) {
        constexpr int LD = TileLayout<true, true>::LD;
        return *reinterpret_cast<const bf16x8*>(s + row * LD + k);
    } else {
        // [k][row] image (the operand's memory order): two hardware-transposed reads.  Per 16-lane group g the
        // instruction takes a block of 4 k-rows x 16 rows; lane 4q+p supplies the address of (k-row q, rows 4p..4p+3)
        // and lane i receives row i of the four k-rows, i.e. k = 8g+q for its own MFMA row.  EXEC is all ones here.
        constexpr int LD = TileLayout<true, false>::LD;
        typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
        const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
        const __bf16* a0 = s + (ks * 32 + 8 * g + q) * LD + row0 + 4 * pp;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a0);
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(a0 + 4 * LD));
        bf16x8 v;
        v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3]; v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
        return v;
    }
}
template <bool KC>
__device__ __forceinline__ float frag_f32(const void* lds, int row0, int ks) {
    const int lane = threadIdx.x & 63;
    const float* s = reinterpret_cast<const float*>(lds);
    const int row = row0 + (lane & 15);
    const int k = ks * 4 + (lane >> 4);
    if (KC) return s[row * TileLayout<false, true>::LD + k];
    else    return s[k * TileLayout<false, false>::LD + row];
}

// FAST: both operands qualify for fetch_tile_fast; the generic loader (ragged extents, convolution operand) is then not
// compiled in at all - it alone costs ~80 VGPRs and halves the occupancy (2 -> 4 workgroups per CU).
template <bool BF16, bool AKC, bool BKC, bool FAST, bool IO16 = false>
__global__ __launch_bounds__(NT, (FAST && BF16) ? 3 : 1) void gemm_kernel(GemmP p) {
    constexpr int A_BYTES = TileLayout<BF16, AKC>::ELEMS * (BF16 ? 2 : 4);
    constexpr int B_BYTES = TileLayout<BF16, BKC>::ELEMS * (BF16 ? 2 : 4);
    __shared__ __attribute__((aligned(16))) unsigned char smem[A_BYTES + B_BYTES];
    void* As = smem;
    void* Bs = smem + A_BYTES;

    // Tile order.  Workgroup i of a launch runs on XCD i % 8 (round-robin dispatch) and each XCD has its own 4 MB L2;
    // a CU takes in only ~10 B/clk from beyond its L2 but 64 B/clk from it, and at 128 x 128 tiles fed from fp32
    // operands that fabric rate, not the MFMA, sets the speed.  So each XCD gets a contiguous band of (z, row-tile)
    // pairs, walks it column group by column group (gx column tiles whose B operand slices fit the L2 together), and
    // inside a group row by row with the column fastest: the A slice of a row is fetched once per group and the
    // group's B slices stay resident for the whole band.  (Speed only: any placement gives the same result.)
    int bx, by, bz;
    if (p.plain_order) {
        const int id = blockIdx.x;
        bx = id % p.nx; by = (id / p.nx) % p.ny; bz = id / (p.nx * p.ny);
        if (bz >= p.nz) return;
    } else {
        const int id = blockIdx.x, xcd = id & 7, local = id >> 3;
        const int per_g = p.rpb * p.gx;
        const int xg = local / per_g, rr = local - xg * per_g;
        const int yb = rr / p.gx, xi = rr - yb * p.gx;
        const int rrow = xcd * p.rpb + yb;
        bx = xg * p.gx + xi;
        if (bx >= p.nx || rrow >= p.ny * p.nz) return;
        bz = rrow / p.ny;
        by = rrow - bz * p.ny;
    }
    const int zb = bz / p.splits;
    const int zs = bz % p.splits;
    const float* A = IO16 ? p.A : p.A + (long)zb * p.sA;
    const float* B = IO16 ? p.B : p.B + (long)zb * p.sB;
    float* C = p.C + (long)zb * p.sC;
    const unsigned short* A16 = reinterpret_cast<const unsigned short*>(p.A) + (long)zb * p.sA;
    const unsigned short* B16 = reinterpret_cast<const unsigned short*>(p.B) + (long)zb * p.sB;

    const int i0 = by * BM;
    const int j0 = bx * BN;

    // reduction range of this split (multiple of BK)
    const int ktiles = (p.K + BK - 1) / BK;
    const int per = (ktiles + p.splits - 1) / p.splits;
    const int kt0 = zs * per;
    const int kt1 = min(ktiles, kt0 + per);
    if (kt0 >= kt1) return;

    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int wr = wave >> 1, wc = wave & 1;

    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    float4 ra[4], rb[4];
    u32x4_t ha[2], hb[2];
    auto fetch = [&](int kk) {
        if (IO16) {
            fetch_tile16<AKC>(A16, p.lda, i0, p.M, kk, p.K, 0, 0, 0, ha);
            fetch_tile16<BKC>(B16, p.ldb, j0, p.N, kk, p.K, BKC ? 0 : p.seqT, p.bshift, p.bpadT, hb);
            return;
        }
        if (FAST || p.fastA) fetch_tile_fast<AKC>(A, p.lda, i0, p.M, kk, p.K, 0, 0, ra);
        else fetch_tile<AKC>(A, p.lda, i0, p.M, kk, p.K, p.vecA, 0, 0, ra, p.convA, p.cT, p.cF, p.cC);
        if (FAST || p.fastB) fetch_tile_fast<BKC>(B, p.ldb, j0, p.N, kk, p.K, BKC ? 0 : p.seqT, p.bshift, rb);
        else fetch_tile<BKC>(B, p.ldb, j0, p.N, kk, p.K, p.vecB, BKC ? 0 : p.seqT, p.bshift, rb, p.convB, p.cT, p.cF, p.cC);
    };
    fetch(kt0 * BK);

    for (int kt = kt0; kt < kt1; ++kt) {
        if (IO16) { stash_tile16<AKC>(As, ha); stash_tile16<BKC>(Bs, hb); }
        else { stash_tile<BF16, AKC>(As, ra); stash_tile<BF16, BKC>(Bs, rb); }
        __syncthreads();
        if (kt + 1 < kt1) fetch((kt + 1) * BK);
        if (BF16) {
            bf16x8 fa[4], fb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) fa[a] = frag_bf16<AKC>(As, wr * 64 + a * 16, 0);
#pragma unroll
            for (int b = 0; b < 4; ++b) fb[b] = frag_bf16<BKC>(Bs, wc * 64 + b * 16, 0);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = mma16(fa[a], fb[b], acc[a][b]);
        } else {
#pragma unroll
            for (int ks = 0; ks < BK / 4; ++ks) {
                float fa[4], fb[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) fa[a] = frag_f32<AKC>(As, wr * 64 + a * 16, ks);
#pragma unroll
                for (int b = 0; b < 4; ++b) fb[b] = frag_f32<BKC>(Bs, wc * 64 + b * 16, ks);
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc[a][b] = mma16(fa[a], fb[b], acc[a][b]);
            }
        }
        __syncthreads();
    }

    // epilogue: C/D map col = lane&15, row = 4*(lane>>4) + reg
    const bool first_split = (zs == 0);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int col = j0 + wc * 64 + b * 16 + (lane & 15);
            if (col >= p.N) continue;
            const float bv = (p.bias != nullptr && first_split) ? p.bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int row = i0 + wr * 64 + a * 16 + 4 * (lane >> 4) + r;
                if (row >= p.M) continue;
                float v = acc[a][b][r] + bv;
                if (IO16 && p.c16) {
                    if (p.act == ASR_ACT_TANH) v = tanhf(v);
                    else if (p.act == ASR_ACT_RELU) v = fmaxf(v, 0.f);
                    reinterpret_cast<unsigned short*>(p.C)[(long)zb * p.sC + (long)row * p.ldc + col] = f2bf_bits(v);
                    continue;
                }
                if (IO16 && p.permH > 0) {
                    const int h4 = 4 * p.permH, blk = row / h4, rr = row - blk * h4;
                    row = blk * h4 + (rr & 3) * p.permH + (rr >> 2);
                }
                float* dst = C + (long)row * p.ldc + col;
                if (p.splits > 1) {
                    atomicAdd(dst, v);
                } else {
                    if (p.act == ASR_ACT_TANH) v = tanhf(v);
                    else if (p.act == ASR_ACT_RELU) v = fmaxf(v, 0.f);
                    if (p.accum) v += *dst;
                    *dst = v;
                }
            }
        }
    }
}

int gemm_plain_order_forced() {
    static int plain = -1;
    if (plain < 0) { const char* e = getenv("ASR_GEMM_PLAIN_ORDER"); plain = (e && e[0] == '1') ? 1 : 0; }
    return plain;
}

// The 20 instantiations, by [BF16][a_kc][b_kc][FAST][IO16]: bf16 storage exists for the bf16 MFMA and the fast loaders only
typedef void (*GemmKernel)(GemmP);
#define IO16_false(A, B) nullptr
#define IO16_true(A, B) gemm_kernel<true, A, B, true, true>
#define LOADERS(BF, A, B) {{gemm_kernel<BF, A, B, false>, nullptr}, {gemm_kernel<BF, A, B, true>, IO16_##BF(A, B)}}
#define LAYOUTS(BF) {{LOADERS(BF, false, false), LOADERS(BF, false, true)}, {LOADERS(BF, true, false), LOADERS(BF, true, true)}}
const GemmKernel gemm_kernels[2][2][2][2][2] = {LAYOUTS(false), LAYOUTS(true)};

}  // namespace

// Launch parameters of gemm_kernel for a checked call, then the plan of the launch: tile counts, XCD band geometry, loader
// qualification, tile order and the number of workgroups.
int gemm_plan(const GemmCall& c, bool io16, KernelPlan<GemmP>& pl) {
    GemmP& p = pl.p;
    p = GemmP{};
    p.A = (const float*)c.A; p.B = (const float*)c.B; p.C = (float*)c.C; p.bias = c.bias;
    p.M = c.M; p.N = c.N; p.K = c.K; p.lda = c.lda; p.ldb = c.ldb; p.ldc = c.ldc;
    p.sA = c.sA; p.sB = c.sB; p.sC = c.sC; p.batch = c.batch; p.splits = c.splits;
    p.act = c.act; p.accum = c.accum; p.seqT = c.seqT; p.bshift = c.bshift;
    p.c16 = c.c_bf16; p.permH = c.perm_h; p.bpadT = c.b_time_padded;
    if (c.conv_F > 0) { p.convA = c.a_kc ? 1 : 0; p.convB = 1 - p.convA; p.cT = c.conv_T; p.cF = c.conv_F; p.cC = c.conv_C; }
    // float4 loads: 16-byte aligned rows (a convolution operand is read by pixel: only its base counts).  vecB also covers the
    // shifted operand: its rows are read at an offset and stay 16-byte aligned because ldb % 4 == 0
    p.vecA = (io16 || (((uintptr_t)c.A & 15) == 0 && (p.convA || ((c.lda % 4) == 0 && (c.sA % 4) == 0)))) ? 1 : 0;
    p.vecB = (io16 || (((uintptr_t)c.B & 15) == 0 && (p.convB || ((c.ldb % 4) == 0 && (c.sB % 4) == 0)))) ? 1 : 0;
    p.nx = cdiv(p.N, BN); p.ny = cdiv(p.M, BM); p.nz = p.batch * p.splits;
    p.rpb = cdiv((long)p.ny * p.nz, 8);
    const long b_slice = (long)BN * cdiv(p.K, p.splits) * (long)(io16 ? 2 : sizeof(float));      // B operand bytes of one column tile
    long gx = (5L << 19) / (b_slice > 0 ? b_slice : 1);                              // ~2.5 MB of B slices per group
    p.gx = (int)(gx < 1 ? 1 : (gx > p.nx ? p.nx : gx));
    p.ngx = cdiv(p.nx, p.gx);
    // fast loader: no convolution operand, 16-byte aligned rows, contiguous extent a multiple of 4 and at least one float4
    p.fastA = (!p.convA && p.vecA && (c.a_kc ? (p.K % 4 == 0 && p.K >= 4) : (p.M % 4 == 0 && p.M >= 4))) ? 1 : 0;
    p.fastB = (!p.convB && p.vecB && (c.b_kc ? (p.K % 4 == 0 && p.K >= 4) : (p.N % 4 == 0 && p.N >= 4))) ? 1 : 0;
    // measured (tools/bench_gemm.py): the banded order wins when a row of tiles is short (N <= 1024: projection and input-
    // gradient shapes, 1.15-1.2x) and loses for wide outputs and split reductions, which keep the natural order
    p.plain_order = (gemm_plain_order_forced() || p.nz > 1 || p.nx > 8) ? 1 : 0;
    const long nblk = p.plain_order ? (long)p.nx * p.ny * p.nz : 8L * p.rpb * p.ngx * p.gx;
    ASR_REQUIRE(nblk < (1L << 31), ASR_E_UNSUPPORTED, "asr_gemm: %ld tiles", nblk);
    pl.kernel = gemm_kernels[io16 || c.prec == ASR_BF16][c.a_kc != 0][c.b_kc != 0][io16 || (p.fastA && p.fastB)][io16];
    pl.grid = (unsigned)nblk; pl.block = NT; pl.lds = 0;
    pl.who = io16 ? "asr_gemm16" : "asr_gemm";
    const int out[8] = {p.fastA, p.fastB, p.plain_order, p.nx, p.ny, p.nz, p.gx, p.ngx};
    for (int i = 0; i < 8; ++i) pl.out[i] = out[i];
    return ASR_OK;
}
int gemm_launch(const KernelPlan<GemmP>& pl, hipStream_t st) { return launch_plan(pl, st); }

// Argument checks of asr_gemm, then its plan (shared by the launch and the asr_gemm_plan query).
static int gemm32_plan(const GemmCall& c, KernelPlan<GemmP>& pl) {
    ASR_REQUIRE(c.A && c.B && c.C, ASR_E_ARG, "asr_gemm: null operand");
    ASR_REQUIRE(c.M > 0 && c.N > 0 && c.K > 0 && c.batch > 0, ASR_E_ARG, "asr_gemm: bad dims M=%d N=%d K=%d batch=%d", c.M, c.N, c.K, c.batch);
    ASR_REQUIRE(c.splits >= 1, ASR_E_ARG, "asr_gemm: splits must be >= 1");
    ASR_REQUIRE(!(c.splits > 1 && (c.act != ASR_ACT_NONE || !c.accum)), ASR_E_ARG,
                "asr_gemm: split reduction requires accum=1 and no activation");
    ASR_REQUIRE(!(c.seqT > 0 && c.b_kc), ASR_E_ARG, "asr_gemm: shifted reduction rows need b_kc=0");
    ASR_REQUIRE(c.prec == ASR_F32 || c.prec == ASR_BF16, ASR_E_ARG, "asr_gemm: bad prec %d", c.prec);
    ASR_REQUIRE(c.ldc >= c.N, ASR_E_ARG, "asr_gemm: ldc < N");
    return gemm_plan(c, false, pl);
}
int gemm_run(const GemmCall& c, hipStream_t st) {
    KernelPlan<GemmP> pl;
    const int rc = gemm32_plan(c, pl);
    return rc != ASR_OK ? rc : gemm_launch(pl, st);
}

extern "C" int asr_gemm(const float* A, const float* B, float* C, const float* bias,
                        int M, int N, int K, long lda, long ldb, long ldc,
                        int a_kc, int b_kc, int act, int accum, int splits,
                        int batch, long sA, long sB, long sC, int seqT, int bshift,
                        int prec, asr_stream_t stream) {
    GemmCall c{A, B, C, bias, M, N, K, lda, ldb, ldc, a_kc, b_kc, act, accum, splits, seqT, bshift, batch, sA, sB, sC};
    c.prec = prec;
    return gemm_run(c, (hipStream_t)stream);
}

// The plan asr_gemm launches with for these arguments (host arithmetic only: nothing is launched, no pointer is followed).
extern "C" int asr_gemm_plan(const float* A, const float* B, float* C, const float* bias,
                             int M, int N, int K, long lda, long ldb, long ldc,
                             int a_kc, int b_kc, int act, int accum, int splits,
                             int batch, long sA, long sB, long sC, int seqT, int bshift,
                             int prec, int out[8]) {
    ASR_REQUIRE(out, ASR_E_ARG, "asr_gemm_plan: null out");
    GemmCall c{A, B, C, bias, M, N, K, lda, ldb, ldc, a_kc, b_kc, act, accum, splits, seqT, bshift, batch, sA, sB, sC};
    c.prec = prec;
    KernelPlan<GemmP> pl;
    const int rc = gemm32_plan(c, pl);
    if (rc != ASR_OK) return rc;
    for (int i = 0; i < 8; ++i) out[i] = pl.out[i];
    return ASR_OK;
}

static int nt_fast_enabled() {
    static const int on = [] { const char* e = getenv("ASR_GEMM16_NT"); return (e && e[0] == '0') ? 0 : 1; }();
    return on;
}

// The plan of one asr_gemm16 call: the route and that kernel's plan.
struct Gemm16Plan {
    KernelPlan<GemmP> generic; KernelPlan<G16P> nt; KernelPlan<T16P> tn;
    int generic_rc = ASR_OK;         // route 0: what gemm_plan answered
    const int* out(int route) const { return route == 0 ? generic.out : (route == 2 ? tn.out : nt.out); }
};
// Argument checks of asr_gemm16 and the kernel the call takes: 0 = the generic bf16-storage kernel (gemm_kernel IO16),
// 1 / 3 = gemm16_nt_kernel at 128 x 128 / 256 x 256, 2 = gemm16_tn_kernel; negative = refused.  Host arithmetic only.
static int gemm16_plan(const GemmCall& c, Gemm16Plan& pl) {
    ASR_REQUIRE(c.A && c.B && c.C, ASR_E_ARG, "asr_gemm16: null operand");
    ASR_REQUIRE(c.M > 0 && c.N > 0 && c.K > 0 && c.splits >= 1, ASR_E_ARG, "asr_gemm16: bad dims M=%d N=%d K=%d", c.M, c.N, c.K);
    ASR_REQUIRE(!(c.splits > 1 && (c.act != ASR_ACT_NONE || !c.accum || c.c_bf16)), ASR_E_ARG, "asr_gemm16: split reduction needs an fp32 accumulating output");
    ASR_REQUIRE(!(c.c_bf16 && (c.accum || c.perm_h)), ASR_E_ARG, "asr_gemm16: a bf16 output is written, not accumulated or permuted");
    ASR_REQUIRE(!(c.seqT > 0 && c.b_kc), ASR_E_ARG, "asr_gemm16: shifted reduction rows need b_kc=0");
    ASR_REQUIRE(c.ldc >= c.N, ASR_E_ARG, "asr_gemm16: ldc < N");
    // 16-byte loads of 8 bf16 along the contiguous index of each operand
    ASR_REQUIRE((((uintptr_t)c.A | (uintptr_t)c.B) & 15) == 0 && c.lda % 8 == 0 && c.ldb % 8 == 0, ASR_E_UNSUPPORTED, "asr_gemm16: operands must be 16-byte aligned with row strides that are multiples of 8");
    ASR_REQUIRE((c.a_kc ? c.K : c.M) % 8 == 0 && (c.b_kc ? c.K : c.N) % 8 == 0, ASR_E_UNSUPPORTED, "asr_gemm16: contiguous extents must be multiples of 8");
    ASR_REQUIRE(c.perm_h == 0 || c.M % (4 * c.perm_h) == 0, ASR_E_ARG, "asr_gemm16: perm_h does not divide M");
    // the direct-to-LDS kernels of gemm16.hip where the call has their form and its shape qualifies, else the generic kernel
    if (c.a_kc && c.b_kc && c.c_bf16 && c.splits == 1 && nt_fast_enabled() && gemm16_nt_plan(c, pl.nt)) return pl.nt.route;
    if (!c.a_kc && !c.b_kc && !c.c_bf16 && c.accum && c.act == ASR_ACT_NONE && c.bias == nullptr && nt_fast_enabled() &&
        gemm16_tn_plan(c, pl.tn)) return pl.tn.route;
    pl.generic_rc = gemm_plan(c, true, pl.generic);
    return 0;
}

extern "C" int asr_gemm16_route(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long lda, long ldb, long ldc,
                                int a_kc, int b_kc, int act, int accum, int splits, int c_bf16, int perm_h,
                                int seqT, int bshift, int b_time_padded) {
    GemmCall c{A, B, C, bias, M, N, K, lda, ldb, ldc, a_kc, b_kc, act, accum, splits, seqT, bshift};
    c.c_bf16 = c_bf16; c.perm_h = perm_h; c.b_time_padded = b_time_padded;
    Gemm16Plan pl;
    return gemm16_plan(c, pl);
}

// Contraction on bf16 operands in HBM (the encoder stack's activations, gate gradients and the bf16 weight copies):
// same index conventions as asr_gemm; C is bf16 (c_bf16 = 1: bias + activation epilogue, no accumulation) or fp32
// (accumulate / split reduction, optional gate-minor -> reference row permutation for LSTM weight gradients).
extern "C" int asr_gemm16(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long lda, long ldb, long ldc,
                          int a_kc, int b_kc, int act, int accum, int splits, int c_bf16, int perm_h,
                          int seqT, int bshift, int b_time_padded, asr_stream_t stream) {
    GemmCall c{A, B, C, bias, M, N, K, lda, ldb, ldc, a_kc, b_kc, act, accum, splits, seqT, bshift};
    c.c_bf16 = c_bf16; c.perm_h = perm_h; c.b_time_padded = b_time_padded;
    Gemm16Plan pl;
    const int route = gemm16_plan(c, pl);
    if (route < 0) return route;
    if (route == 2) return gemm16_tn_launch(pl.tn, (hipStream_t)stream);
    if (route != 0) return gemm16_nt_launch(pl.nt, (hipStream_t)stream);
    return pl.generic_rc != ASR_OK ? pl.generic_rc : gemm_launch(pl.generic, (hipStream_t)stream);
}

// The plan behind asr_gemm16_route's answer (host arithmetic only).  Returns the route and fills out[8]:
//   0 (generic kernel): the entries of asr_gemm_plan {fastA, fastB, plain_order, nx, ny, nz, gx, ngx} at bf16 operand size;
//   1 / 3 (NT kernel):  {tiles along N, tiles along M, tile rows, tile columns, 0...};
//   2 (TN kernel):      {tiles along I, tiles along J, reduction slices after clipping, k-steps per slice, LDS stages
//                        (ASR_GEMM16_TN_STAGES), workgroups, 0, 0}.
extern "C" int asr_gemm16_plan(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long lda, long ldb, long ldc,
                               int a_kc, int b_kc, int act, int accum, int splits, int c_bf16, int perm_h,
                               int seqT, int bshift, int b_time_padded, int out[8]) {
    ASR_REQUIRE(out, ASR_E_ARG, "asr_gemm16_plan: null out");
    GemmCall c{A, B, C, bias, M, N, K, lda, ldb, ldc, a_kc, b_kc, act, accum, splits, seqT, bshift};
    c.c_bf16 = c_bf16; c.perm_h = perm_h; c.b_time_padded = b_time_padded;
    Gemm16Plan pl;
    const int route = gemm16_plan(c, pl);
    if (route < 0) return route;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (route == 0 && pl.generic_rc != ASR_OK) return pl.generic_rc;
    for (int i = 0; i < 8; ++i) out[i] = pl.out(route)[i];
    return route;
}

// 3x3 / stride 1 / pad 1 convolution over channel-last images as an implicit GEMM.
//   mode 0 (forward / dgrad): out[(b,t,f), n] (+)= act( sum_{tap,ci} img[(b,t+dt,f+df), ci] * w[n][tap*C + ci] + bias[n] )
//   mode 1 (wgrad)          : dw[n][tap*C + ci] += sum_{(b,t,f)} dout[(b,t,f), n] * img[(b,t+dt,f+df), ci]
// Argument checks of asr_conv3x3, then its plan (shared by the launch and the asr_conv3x3_plan query).
static int conv3x3_plan(const float* img, const float* w_or_dout, float* out, const float* bias,
                        int B, int T, int F, int C, int N, int mode, int act, int accum, int prec, KernelPlan<GemmP>& pl) {
    ASR_REQUIRE(img && w_or_dout && out, ASR_E_ARG, "asr_conv3x3: null pointer");
    ASR_REQUIRE(B > 0 && T > 0 && F > 0 && C > 0 && N > 0, ASR_E_ARG, "asr_conv3x3: bad dims");
    ASR_REQUIRE(mode == 0 || mode == 1, ASR_E_ARG, "asr_conv3x3: bad mode %d", mode);
    ASR_REQUIRE(prec == ASR_F32 || prec == ASR_BF16, ASR_E_ARG, "asr_conv3x3: bad prec %d", prec);
    ASR_REQUIRE(act == ASR_ACT_NONE || act == ASR_ACT_TANH || act == ASR_ACT_RELU, ASR_E_ARG, "asr_conv3x3: bad act %d", act);
    ASR_REQUIRE(accum == 0 || accum == 1, ASR_E_ARG, "asr_conv3x3: bad accum %d", accum);
    ASR_REQUIRE((long)B * T * F < (1L << 31), ASR_E_UNSUPPORTED, "asr_conv3x3: more than 2^31 pixels");
    ASR_REQUIRE(9L * C < (1L << 31), ASR_E_UNSUPPORTED, "asr_conv3x3: more than 2^31 / 9 channels");
    const int rows = B * T * F, K9 = 9 * C;
    GemmCall c{img, w_or_dout, out, bias, rows, N, K9, C, K9, N};
    if (mode == 1) {
        // wgrad: C[i = n, j = (tap,ci)] += sum_r dout[r, i] * conv(img)[r, j]
        ASR_REQUIRE(accum == 1 && act == ASR_ACT_NONE && bias == nullptr, ASR_E_ARG, "asr_conv3x3: wgrad accumulates without epilogue");
        c = gemm_wgrad_call(w_or_dout, img, out, N, K9, rows, N, C, K9, rows >= 65536 ? 32 : (rows >= 4096 ? 8 : 1));
    }
    c.act = act; c.accum = accum; c.prec = prec;
    c.conv_T = T; c.conv_F = F; c.conv_C = C;
    const int rc = gemm_plan(c, false, pl);
    pl.who = "asr_conv3x3";
    return rc;
}

extern "C" int asr_conv3x3(const float* img, const float* w_or_dout, float* out, const float* bias,
                           int B, int T, int F, int C, int N, int mode, int act, int accum, int prec, asr_stream_t stream) {
    KernelPlan<GemmP> pl;
    const int rc = conv3x3_plan(img, w_or_dout, out, bias, B, T, F, C, N, mode, act, accum, prec, pl);
    return rc != ASR_OK ? rc : gemm_launch(pl, (hipStream_t)stream);
}

// The plan asr_conv3x3 launches with for these arguments (host arithmetic only: nothing is launched, no pointer is followed).
extern "C" int asr_conv3x3_plan(const float* img, const float* w_or_dout, float* out, const float* bias,
                                int B, int T, int F, int C, int N, int mode, int act, int accum, int prec, int plan[8]) {
    ASR_REQUIRE(plan, ASR_E_ARG, "asr_conv3x3_plan: null out");
    KernelPlan<GemmP> pl;
    const int rc = conv3x3_plan(img, w_or_dout, out, bias, B, T, F, C, N, mode, act, accum, prec, pl);
    if (rc != ASR_OK) return rc;
    for (int i = 0; i < 8; ++i) plan[i] = pl.out[i];
    return ASR_OK;
}
