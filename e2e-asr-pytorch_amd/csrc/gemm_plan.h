// Host side of the contraction kernels (gemm.hip, gemm16.hip).  A caller states ONE contraction as a GemmCall.  Each of the three
// kernels contributes ONE plan function, defined next to it, that turns a call into "does not qualify" or a KernelPlan (the
// filled kernel parameters, the launch geometry, the instantiation and the eight entries a plan query reports), and ONE launch
// of such a plan.  Planning is pure host arithmetic: no device call, no pointer followed.  Who asks what:
//   asr_gemm, asr_gemm_plan, gemm_run (decoder*.hip, frontend.hip)   the fp32 entry's checks, then gemm_plan
//   asr_gemm16, asr_gemm16_route, asr_gemm16_plan                    the bf16 entry's checks, then the first of gemm16_nt_plan,
//                                                                    gemm16_tn_plan, gemm_plan (bf16 storage) that takes the call
//   asr_conv3x3, asr_conv3x3_plan                                    the fp32 convolution entry's checks, then gemm_plan on a call with conv_F > 0
//   asr_conv3x3_16 / asr_conv3x3_16_wgrad (vgg16.hip)                gemm16_nt_plan / gemm16_tn_plan on a call with conv_F > 0
// Every entry plans once and launches, or reports, exactly that plan.
#pragma once
#include "common.h"

// C[i,j] (+)= act( sum_r opA(i,r) * opB(r,j) + bias[j] ), the index conventions of asr_gemm (gemm.hip).  Operands are fp32, or
// bf16 for the bf16 entry and kernels.  Everything after ldc defaults to "nothing special".
struct GemmCall {
    const void* A; const void* B; void* C; const float* bias;
    int M, N, K;
    long lda, ldb, ldc;
    int a_kc = 1, b_kc = 1;                          // the default is y = x W^T
    int act = ASR_ACT_NONE, accum = 0, splits = 1;
    int seqT = 0, bshift = 0;                        // seqT > 0: reduction row (b,t) of B is read at (b, t + bshift), zero outside
    int batch = 1; long sA = 0, sB = 0, sC = 0;      // fp32 entry only
    int c_bf16 = 0, perm_h = 0, b_time_padded = 0;   // bf16 entry only
    int prec = ASR_BF16;                             // fp32 entry: which MFMA
    // conv_F > 0: a 3x3 convolution over a channel-last image of conv_T x conv_F pixels and conv_C channels, whose pixels are
    // the rows of one operand.  gemm_kernel: that operand is A where a_kc = 1, else B.  gemm16_nt_kernel: X, a zero-bordered
    // image with the border counted in conv_T / conv_F (conv_C = 0: X holds explicit patches, only the border of the output is
    // masked), C fp32 where c_bf16 = 0.  gemm16_tn_kernel: the nine taps of the weight gradient, B shifted by rows of conv_F.
    int conv_T = 0, conv_F = 0, conv_C = 0;
};
// dW (I,J) += sum over R rows of dy[r,i] * x[r,j], the reduction cut into `splits` slices
inline GemmCall gemm_wgrad_call(const void* dy, const void* x, float* dW, int I, int J, int R, long lddy, long ldx, long lddW, int splits) {
    GemmCall c{dy, x, dW, nullptr, I, J, R, lddy, ldx, lddW};
    c.a_kc = c.b_kc = 0; c.accum = 1; c.splits = splits;
    return c;
}

struct GemmP {
    const float* A; const float* B; float* C; const float* bias;
    int M, N, K;
    long lda, ldb, ldc;
    long sA, sB, sC;
    int batch, splits;
    int act, accum;
    int seqT, bshift;
    int vecA, vecB;
    // implicit 3x3 convolution over a channel-last image (rows = (b,t,f), cT x cF pixels, cC channels):
    // the conv operand's reduction/column index k = tap*cC + ci addresses pixel (t+dt, f+df), zero outside.
    int convA, convB, cT, cF, cC;
    // XCD-aware tile order (see gemm_kernel): column tiles, row tiles, z slices, rows per XCD band, column group width
    int nx, ny, nz, rpb, gx, ngx, plain_order;
    int fastA, fastB;      // operand qualifies for fetch_tile_fast
    // bf16-storage variant (IO16 kernels): A and B are bf16 in HBM (element strides as above), C is bf16 (c16 = 1) or fp32;
    // permH > 0: output row i of a (ND*4H)-row weight gradient computed in gate-minor order [unit][gate] is stored at the
    // reference's row (i / 4H)*4H + (i & 3)*H + (i % 4H >> 2);  bpadT = 1: the shifted B operand lives in a time-padded
    // buffer (B,seqT+2,.) - reduction row r = (b,t) is read at padded row b*(seqT+2) + t + 1 + bshift, always valid
    int c16, permH, bpadT;
};

struct G16P {
    const unsigned short* X; const unsigned short* W; unsigned short* C; const float* bias;
    int M, N, K;
    long ldx, ldw, ldc;
    int act;
    unsigned xbytes, wbytes;
    int ntx, nty;            // tiles along N, along M
    // CONV instantiation only: rows are the pixels of a zero-bordered channel-last image (B, T2, F2, C) and k-step kt of the
    // 9*C-deep reduction reads the rows shifted by its tap (convC > 0), border rows are stored as zeros (maskF2 > 0)
    int convC, maskF2, maskT2;
    float* C32;              // CONV only: when set, the result goes here as fp32 (pre-activations that a LayerNorm normalises next)
};

struct T16P {
    const unsigned short* A; const unsigned short* B; float* C;
    int I, J, R;                 // C is (I,J); reduction over R rows
    long lda, ldb, ldc;
    unsigned abytes, bbytes;
    int nti, ntj, splits, per;   // tiles along I and J, reduction slices, k-steps per slice
    int seqT, bshift, permH;
    float inv_seqT;
    int tapF2;                   // > 0: NINE contractions in one launch, the taps of a 3x3 convolution's weight gradient: tap
                                 // (dt, df) reads B at row r + dt*tapF2 + df (rows outside [0, R) are zeros) and writes C at column tap*J
};

// One planned launch of a kernel whose parameter struct is P.
template <class P> struct KernelPlan {
    P p;
    void (*kernel)(P) = nullptr;
    unsigned grid = 0, block = 0, lds = 0;       // workgroups, threads, dynamic LDS bytes
    int route = 0;                               // asr_gemm16_route's number for this kernel
    const char* who = "";                        // entry named when the launch fails
    int out[8] = {};                             // what the plan query reports (layouts: asr_gemm16_plan, gemm.hip)
};
template <class P> int launch_plan(const KernelPlan<P>& pl, hipStream_t st) {
    hipLaunchKernelGGL(pl.kernel, dim3(pl.grid), dim3(pl.block), pl.lds, st, pl.p);
    ASR_LAUNCH_CHECK(pl.who);
    return ASR_OK;
}

// gemm.hip, gemm_kernel: takes every call that passed its entry's checks; fp32 storage, or bf16 storage (io16: prec, batch
// and strides unused).  ASR_OK or a negative error with its message set (more than 2^31 tiles).
int gemm_plan(const GemmCall& c, bool io16, KernelPlan<GemmP>& pl);
int gemm_launch(const KernelPlan<GemmP>& pl, hipStream_t st);
// what asr_gemm does: its argument checks, gemm_plan, gemm_launch
int gemm_run(const GemmCall& c, hipStream_t st);

// gemm16.hip, gemm16_nt_kernel (x W^T, bf16 out; route 1 at 128 x 128 tiles, 3 at 256 x 256) and gemm16_tn_kernel (weight
// gradients; route 2): false = the call does not qualify.  The caller has checked that the call has the kernel's form.
bool gemm16_nt_plan(const GemmCall& c, KernelPlan<G16P>& pl);
int gemm16_nt_launch(const KernelPlan<G16P>& pl, hipStream_t st);
bool gemm16_tn_plan(const GemmCall& c, KernelPlan<T16P>& pl);
int gemm16_tn_launch(const KernelPlan<T16P>& pl, hipStream_t st);
