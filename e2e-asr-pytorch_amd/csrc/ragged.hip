// Data movement of the length-aware batched encoder pass (src/ragged.py): a padded batch of utterances of different
// lengths goes through the UNCHANGED recurrence launches (asr_lstm_fwd / asr_lstm16_fwd) and still computes what the
// unpadded pass of every utterance computes.  Direction 0 of the recurrence walks t = 0.. from the zero state: frames
// 0..n-1 of a row see exactly the unpadded pass.  Direction 1 walks t = T-1.. from the zero state: it sees the unpadded pass
// when the row's gate pre-activations are RIGHT-ALIGNED (frame t of the utterance at time row t + T - n), so that the walk
// starts on the utterance's true last frame.  Two copy kernels (bit-exact, no arithmetic) and one store kernel:
//
//   asr_ragged_align   gates (B,T,ND,W) -> gates (B,T,ND,W): direction 0 copied at t < n, direction 1 shifted right by
//                      T - n, zeros everywhere else (no source row at or past n is read).
//   asr_ragged_unalign y (B,T,ND*H) -> z (B,T2,Dz): direction 1 shifted back, the layer's time down-sampling taken in the
//                      same pass ('drop': frame t2*rate; 'concat': frames t2*rate .. t2*rate+rate-1 side by side), exact
//                      zeros in every row past the row's output length (ceil(n/rate) / n/rate frames).
//   asr_ragged_zero_tail  in place on an activation of a convolutional front-end seen as (B,Ttot,W): exact zeros in time rows
//                      t_off + n .. t_off + T - 1 of every batch row, so that the next 3 x 3 convolution reads at t >= n the
//                      zero padding the unpadded pass reads there (src/vgg.py: conv_stack_lens).  Nothing is read; valid
//                      frames and the border rows of a bordered image (t_off = 1, Ttot = T + 2) are not touched.
//
// All serve the fp32 layouts (elem_bytes = 4: gates (B,T,ND,4H), y (B,T,ND*H)) and the bf16 ones (elem_bytes = 2: gates16
// (B,T,ND,H,4) whose (H,4) block is W = 4H contiguous elements, time-padded y16 through src_bstride / src_off).
// Memory-bound: a thread moves 16 bytes along the contiguous extent when the extents and addresses allow it, one element
// otherwise; a workgroup of 256 threads covers 256 / lanes-per-row rows, so the grid follows the data; the (b,t)
// decomposition and the length are per row, not per element.  No LDS.
#include "common.h"

namespace {

struct RgP {
    const void* src;
    void* dst;
    const int64_t* lens;      // (B) valid frames of every row; clamped to [0,T] on the device
    long src_bstride, src_off;       // elements: src[src_off + b*src_bstride + ...] (unalign only)
    int B, T, ND, W;          // W: elements per (b,t,direction)
    int T2, rate, style;      // unalign: output frames, down-sampling
    int lanes_log2;           // threads per row = 1 << lanes_log2 (<= 256)
    long rows;                // destination rows
};

__device__ __forceinline__ int clamp_len(const int64_t* lens, int b, int T) {
    const int64_t n = lens[b];
    return n < 0 ? 0 : (n > T ? T : (int)n);
}

template <typename V> __device__ __forceinline__ V zero_of();
template <> __device__ __forceinline__ uint4 zero_of<uint4>() { return make_uint4(0u, 0u, 0u, 0u); }
template <> __device__ __forceinline__ uint32_t zero_of<uint32_t>() { return 0u; }
template <> __device__ __forceinline__ uint16_t zero_of<uint16_t>() { return (uint16_t)0; }

// V = the unit a thread moves; Wv = W in units of V.  Destination row = (b,t): ND * Wv units.
template <typename V>
__global__ void ragged_align_kernel(RgP p, int Wv) {
    const int lanes = 1 << p.lanes_log2;
    const long row = (long)blockIdx.x * (256 >> p.lanes_log2) + (threadIdx.x >> p.lanes_log2);
    if (row >= p.rows) return;
    const int b = (int)(row / p.T), t = (int)(row - (long)b * p.T);
    const int n = clamp_len(p.lens, b, p.T);
    const V* src = static_cast<const V*>(p.src);
    V* dst = static_cast<V*>(p.dst) + row * ((long)p.ND * Wv);
    for (int d = 0; d < p.ND; ++d) {
        const int ts = d == 0 ? t : t - (p.T - n);                   // source frame of this time row
        const bool ok = d == 0 ? t < n : ts >= 0;
        const V* s = src + (((long)b * p.T + (ok ? ts : 0)) * p.ND + d) * Wv;
        for (int k = threadIdx.x & (lanes - 1); k < Wv; k += lanes) dst[(long)d * Wv + k] = ok ? s[k] : zero_of<V>();
    }
}

// Destination row = (b,t2): segs * ND * Hv units, segs = rate for 'concat' and 1 for 'drop'; Hv = H in units of V.
template <typename V>
__global__ void ragged_unalign_kernel(RgP p, int Hv) {
    const int lanes = 1 << p.lanes_log2;
    const long row = (long)blockIdx.x * (256 >> p.lanes_log2) + (threadIdx.x >> p.lanes_log2);
    if (row >= p.rows) return;
    const int b = (int)(row / p.T2), t2 = (int)(row - (long)b * p.T2);
    const int n = clamp_len(p.lens, b, p.T);
    const int segs = p.style == 0 ? 1 : p.rate;
    const int nout = p.style == 0 ? (n + p.rate - 1) / p.rate : n / p.rate;
    const bool ok = t2 < nout;
    const int Dv = p.ND * Hv;                                        // units per source frame
    const V* src = static_cast<const V*>(p.src) + p.src_off + (long)b * p.src_bstride;      // src_off, src_bstride in units of V
    V* dst = static_cast<V*>(p.dst) + row * ((long)segs * Dv);
    for (int sd = 0; sd < segs * p.ND; ++sd) {
        const int seg = sd / p.ND, d = sd - seg * p.ND;
        // valid rows only: t2*rate + seg <= n-1, plus the shift T-n of direction 1 <= T-1
        const int ts = ok ? t2 * p.rate + seg + (d == 1 ? p.T - n : 0) : 0;
        const V* s = src + (long)ts * Dv + (long)d * Hv;
        for (int k = threadIdx.x & (lanes - 1); k < Hv; k += lanes) dst[(long)sd * Hv + k] = ok ? s[k] : zero_of<V>();
    }
}

struct ZtP {
    void* buf;
    const int64_t* lens;      // (B); clamped to [0,T] on the device
    long bstride, off;        // units of V: one batch row (Ttot * Wv), the first interior time row (t_off * Wv)
    int T, Wv, chunks;        // workgroups per batch row
};

// The tail of batch row b is ONE contiguous span: (T - n) time rows of Wv units behind time row t_off + n.  `chunks`
// workgroups stride over it; those that start behind its end (all of them when n = T) return without a store.
template <typename V>
__global__ void ragged_zero_tail_kernel(ZtP p) {
    const int b = blockIdx.x / p.chunks, chunk = blockIdx.x - b * p.chunks;
    const int n = clamp_len(p.lens, b, p.T);
    const long span = (long)(p.T - n) * p.Wv;
    V* dst = static_cast<V*>(p.buf) + (long)b * p.bstride + p.off + (long)n * p.Wv;
    for (long k = (long)chunk * 256 + threadIdx.x; k < span; k += (long)p.chunks * 256) dst[k] = zero_of<V>();
}

inline int lanes_log2_for(int units) {                // smallest power of two >= units, at most 256 threads per row
    int l = 0;
    while (l < 8 && (1 << l) < units) ++l;
    return l;
}

}  // namespace

extern "C" int asr_ragged_align(const void* src, void* dst, const int64_t* lens, int B, int T, int ND, int W, int elem_bytes,
                                asr_stream_t stream) {
    ASR_REQUIRE(src && dst && lens, ASR_E_ARG, "asr_ragged_align: null pointer");
    ASR_REQUIRE(src != dst, ASR_E_ARG, "asr_ragged_align: cannot run in place");
    ASR_REQUIRE(B > 0 && T > 0 && W > 0 && (ND == 1 || ND == 2), ASR_E_ARG, "asr_ragged_align: bad dims");
    ASR_REQUIRE(elem_bytes == 4 || elem_bytes == 2, ASR_E_ARG, "asr_ragged_align: elem_bytes must be 4 (fp32) or 2 (bf16)");
    ASR_REQUIRE((long)B * T < (1L << 31) / 256, ASR_E_UNSUPPORTED, "asr_ragged_align: %ld time rows", (long)B * T);
    ASR_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & (uintptr_t)(elem_bytes - 1)) == 0, ASR_E_ARG, "asr_ragged_align: unaligned");
    const int per = 16 / elem_bytes;
    const bool vec = W % per == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const int Wv = vec ? W / per : W;
    RgP p{src, dst, lens, 0, 0, B, T, ND, W, 0, 1, 0, lanes_log2_for(Wv), (long)B * T};
    const dim3 grid(cdiv(p.rows, 256 >> p.lanes_log2)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (vec)                  hipLaunchKernelGGL(ragged_align_kernel<uint4>, grid, block, 0, st, p, Wv);
    else if (elem_bytes == 4) hipLaunchKernelGGL(ragged_align_kernel<uint32_t>, grid, block, 0, st, p, Wv);
    else                      hipLaunchKernelGGL(ragged_align_kernel<uint16_t>, grid, block, 0, st, p, Wv);
    ASR_LAUNCH_CHECK("asr_ragged_align");
    return ASR_OK;
}

extern "C" int asr_ragged_unalign(const void* src, long src_bstride, long src_off, void* dst, const int64_t* lens, int B, int T,
                                  int ND, int H, int T2, int rate, int style, int elem_bytes, asr_stream_t stream) {
    ASR_REQUIRE(src && dst && lens, ASR_E_ARG, "asr_ragged_unalign: null pointer");
    ASR_REQUIRE(src != dst, ASR_E_ARG, "asr_ragged_unalign: cannot run in place");
    ASR_REQUIRE(B > 0 && T > 0 && H > 0 && (ND == 1 || ND == 2) && T2 > 0, ASR_E_ARG, "asr_ragged_unalign: bad dims");
    ASR_REQUIRE(rate >= 1 && rate <= 64 && (style == 0 || style == 1), ASR_E_ARG, "asr_ragged_unalign: bad down-sampling");
    ASR_REQUIRE(elem_bytes == 4 || elem_bytes == 2, ASR_E_ARG, "asr_ragged_unalign: elem_bytes must be 4 (fp32) or 2 (bf16)");
    ASR_REQUIRE(src_off >= 0 && src_bstride >= src_off + (long)T * ND * H, ASR_E_ARG,
                "asr_ragged_unalign: batch stride %ld does not hold offset %ld + %d frames", src_bstride, src_off, T);
    ASR_REQUIRE((long)B * T2 < (1L << 31) / 256, ASR_E_UNSUPPORTED, "asr_ragged_unalign: %ld output rows", (long)B * T2);
    ASR_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & (uintptr_t)(elem_bytes - 1)) == 0, ASR_E_ARG, "asr_ragged_unalign: unaligned");
    const int per = 16 / elem_bytes;
    const bool vec = H % per == 0 && src_bstride % per == 0 && src_off % per == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const int Hv = vec ? H / per : H;
    RgP p{src, dst, lens, vec ? src_bstride / per : src_bstride, vec ? src_off / per : src_off, B, T, ND, H, T2, rate, style,
          lanes_log2_for(Hv), (long)B * T2};
    const dim3 grid(cdiv(p.rows, 256 >> p.lanes_log2)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (vec)                  hipLaunchKernelGGL(ragged_unalign_kernel<uint4>, grid, block, 0, st, p, Hv);
    else if (elem_bytes == 4) hipLaunchKernelGGL(ragged_unalign_kernel<uint32_t>, grid, block, 0, st, p, Hv);
    else                      hipLaunchKernelGGL(ragged_unalign_kernel<uint16_t>, grid, block, 0, st, p, Hv);
    ASR_LAUNCH_CHECK("asr_ragged_unalign");
    return ASR_OK;
}

extern "C" int asr_ragged_zero_tail(void* buf, const int64_t* lens, int B, int T, int Ttot, int t_off, int W, int elem_bytes,
                                    asr_stream_t stream) {
    ASR_REQUIRE(buf && lens, ASR_E_ARG, "asr_ragged_zero_tail: null pointer");
    ASR_REQUIRE(B > 0 && T > 0 && W > 0 && t_off >= 0 && (long)t_off + T <= Ttot, ASR_E_ARG,
                "asr_ragged_zero_tail: bad dims (B %d, T %d behind %d of %d time rows, W %d)", B, T, t_off, Ttot, W);
    ASR_REQUIRE(elem_bytes == 4 || elem_bytes == 2, ASR_E_ARG, "asr_ragged_zero_tail: elem_bytes must be 4 (fp32) or 2 (bf16)");
    ASR_REQUIRE((long)B * Ttot < (1L << 31) / 256, ASR_E_UNSUPPORTED, "asr_ragged_zero_tail: %ld time rows", (long)B * Ttot);
    ASR_REQUIRE(((uintptr_t)buf & (uintptr_t)(elem_bytes - 1)) == 0, ASR_E_ARG, "asr_ragged_zero_tail: unaligned");
    const int per = 16 / elem_bytes;
    const bool vec = W % per == 0 && ((uintptr_t)buf & 15) == 0;          // then every time row starts on 16 bytes
    const int Wv = vec ? W / per : W;
    const long most = ((long)T * Wv + 255) / 256;                        // workgroups that cover a whole row's T frames once
    ZtP p{buf, lens, (long)Ttot * Wv, (long)t_off * Wv, T, Wv, (int)(most < 256 ? most : 256)};
    const dim3 grid((unsigned)((long)B * p.chunks)), block(256);          // B * chunks <= B * 256 < 2^31 by the row bound
    hipStream_t st = (hipStream_t)stream;
    if (vec)                  hipLaunchKernelGGL(ragged_zero_tail_kernel<uint4>, grid, block, 0, st, p);
    else if (elem_bytes == 4) hipLaunchKernelGGL(ragged_zero_tail_kernel<uint32_t>, grid, block, 0, st, p);
    else                      hipLaunchKernelGGL(ragged_zero_tail_kernel<uint16_t>, grid, block, 0, st, p);
    ASR_LAUNCH_CHECK("asr_ragged_zero_tail");
    return ASR_OK;
}
