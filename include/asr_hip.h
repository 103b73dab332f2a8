/*
 * libasr_hip.so — C ABI of the MI355X (gfx950) joint CTC-attention ASR training hot path.
 *
 * The reference (DanielLin94144/E2E-ASR-Pytorch) has no FFI: every entry point below replaces a
 * PyTorch call site on the path  src/asr.py:89-177 (ASR.forward) -> bin/train_asr.py:229-253 (losses,
 * backward); the citation next to each function names the reference lines it stands in for.
 *
 * Conventions
 *   - plain C types only; every tensor pointer is a DEVICE pointer to dense row-major fp32 (or the
 *     stated integer type) owned by the caller and valid until `stream` reaches the call;
 *   - no entry point allocates device memory or synchronises the stream: scratch space is passed in
 *     by the caller (sizes are documented per call);
 *   - returns ASR_OK (0) or a negative ASR_E_* code; asr_last_error() gives a thread-local message;
 *   - `prec` selects the matrix-core type of the contractions: ASR_BF16 (bf16 MFMA operands, fp32
 *     accumulate, fp32 everywhere else) or ASR_F32 (exact fp32-input MFMA, parity mode);
 *   - `stream` is a hipStream_t passed as void*.
 */
#ifndef ASR_HIP_H
#define ASR_HIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASR_OK 0
#define ASR_E_ARG (-1)
#define ASR_E_LAUNCH (-2)
#define ASR_E_UNSUPPORTED (-3)

#define ASR_F32 0
#define ASR_BF16 1

#define ASR_ACT_NONE 0
#define ASR_ACT_TANH 1
#define ASR_ACT_RELU 2

typedef void* asr_stream_t;

const char* asr_last_error(void);
int asr_version(void);
/* "gfx950" — the only architecture this library carries code objects for. */
const char* asr_device_arch(void);

/* ------------------------------------------------------------------------------------------------
 * Contractions (replace nn.Linear / torch.mm / bmm and their autograd: src/module.py:1078-1079 `pj`,
 * src/asr.py:29-32 `ctc_layer`, src/asr.py:292-293,345 `proj_q/proj_k`, src/asr.py:213 `char_trans`,
 * the input half of nn.LSTM src/module.py:1023, and torch.bmm src/module.py:1114).
 *   C[i,j] (+)= act( sum_r opA(i,r) opB(r,j) + bias[j] ),  i<M, j<N, r<K
 *   a_kc=1: A element (i,r) at A[i*lda+r];   a_kc=0: at A[r*lda+i]
 *   b_kc=1: B element (r,j) at B[j*ldb+r];   b_kc=0: at B[r*ldb+j]
 *   accum=1: add into C;  splits>1: the reduction is cut into `splits` slices added with fp32 atomics
 *            (needs accum=1, act=NONE);  batch>1 with element strides sA/sB/sC.
 *   seqT>0 (b_kc=0 only): reduction index r enumerates (b,t) with t = r % seqT; B is read at row
 *            r+bshift and treated as zero when t+bshift falls outside [0,seqT) — the h_{t-1}/h_{t+1}
 *            operand of the recurrent weight gradient.
 */
int asr_gemm(const float* A, const float* B, float* C, const float* bias,
             int M, int N, int K, long lda, long ldb, long ldc,
             int a_kc, int b_kc, int act, int accum, int splits,
             int batch, long sA, long sB, long sC, int seqT, int bshift,
             int prec, asr_stream_t stream);
/* The plan asr_gemm launches with for the same arguments (without the stream): out = {fastA, fastB, plain_order, nx, ny,
 * nz, gx, ngx} - whether operand A / B takes the unconditional 16-byte loader (otherwise the masked one), whether the tiles
 * run in natural order (otherwise in XCD bands), column tiles, row tiles, batch * splits, column tiles per group and the
 * number of groups of the banded order.  Pure host arithmetic from the code the launch itself uses: no device call, the
 * pointers are looked at for their alignment only.  Returns what asr_gemm would return for refused arguments. */
int asr_gemm_plan(const float* A, const float* B, float* C, const float* bias,
                  int M, int N, int K, long lda, long ldb, long ldc,
                  int a_kc, int b_kc, int act, int accum, int splits,
                  int batch, long sA, long sB, long sC, int seqT, int bshift,
                  int prec, int out[8]);

/* ------------------------------------------------------------------------------------------------
 * Encoder BiLSTM time recurrence (the sequential half of nn.LSTM(bidirectional, batch_first),
 * src/module.py:1023,1049; zero initial state; padded frames are processed like the reference does).
 *   gates (B,T,ND,4H): in  = x W_ih^T + b_ih + b_hh for every frame (asr_gemm, gate order i,f,g,o)
 *                      out = activated gates (saved for backward)
 *   whh   (ND,4H,H)  : weight_hh_l0 [, weight_hh_l0_reverse]
 *   bias2 (ND,4H)    : optional second bias (bias_hh) added here when `gates` only carries bias_ih
 *   y     (B,T,ND*H) : h of both directions (forward half first);  c (B,T,ND,H): cell states
 * Backward consumes dy (gradient wrt y) and overwrites `gates` with the gradient wrt the gate
 * pre-activations, from which the caller forms dW_ih, dW_hh (shifted rows), db and dx with asr_gemm.
 * workspace: asr_lstm_workspace_bytes(B,H,ND), 256B aligned.  With a workspace both passes run as ONE persistent
 * launch each (weights resident in registers, h / partial-dh exchanged between workgroups through tagged
 * granules in the workspace; its first 32-bit word is an abort flag that stays 0 on success); shapes without a
 * persistent plan, a NULL workspace (forward) or ASR_LSTM_PERSIST=0 use one launch per time step.
 */
size_t asr_lstm_workspace_bytes(int B, int H, int ND);
/* 1 (default, or env ASR_LSTM_PERSIST) = persistent single-launch recurrence, 0 = one launch per step,
 * 2 = persistent but first-generation kernels only (A/B measurements); returns the old value. */
int asr_lstm_set_persistent(int on);
/* which implementation the two calls below take for this shape: 0 = launch per time step, 1 = first-generation
 * persistent kernel, 2 = second-generation persistent kernel (tests assert the plan the bench shape must get).
 * Both calls launch from the same host plan (csrc/lstm_plan.h).  The answer describes a call with a workspace of
 * asr_lstm_workspace_bytes and 16-byte aligned tensors: alignment and the workspace are properties of a CALL, which the
 * query cannot see, and demote at launch time - gates, y or c not 16-byte aligned: 2 -> 1; a workspace shorter than the
 * generation needs: the next older generation, at last one launch per step; asr_lstm_fwd without a workspace, or with one
 * that is not 256-byte aligned: one launch per step at once (asr_lstm_bwd rejects such a call with ASR_E_ARG).
 * 1 covers both passes only where the first generation has a kernel for both (forward: H <= 320, B <= 64; backward:
 * H % 16 == 0, B <= 64, an instantiated tile shape); a pass it does not cover runs one launch per step. */
int asr_lstm_plan(int B, int T, int H, int ND, int prec);
int asr_lstm_fwd(float* gates, const float* whh, const float* bias2, float* y, float* c,
                 int B, int T, int H, int ND, int prec,
                 void* workspace, size_t workspace_bytes, asr_stream_t stream);
int asr_lstm_bwd(float* gates, const float* whh, const float* dy, const float* c,
                 int B, int T, int H, int ND, int prec,
                 void* workspace, size_t workspace_bytes, asr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * bf16-STORAGE ENCODER STACK (bf16 contraction mode; the same reference call sites as above: nn.LSTM + Dropout +
 * down-sampling + tanh(Linear) of RNNLayer.forward, src/module.py:1040-1081, and their autograd).  Activations, gate
 * pre-activations / gradients and h live in HBM as bf16, the cell state and every parameter gradient as fp32:
 *   gates16 (B,T,ND,H,4) bf16, GATE-MINOR: [unit][i,f,g,o]; in = x W_ih^T + b_ih + b_hh, out = activated gates (forward);
 *           in = activated gates, out = gradient wrt the pre-activations (backward)
 *   y16     (B,T+2,ND*H) bf16: h of frame t at time row t+1; rows 0 and T+1 (h_{-1} / h_T) are ZEROED by asr_lstm16_fwd:
 *           the recurrent weight gradient reads h_{t-1} / h_{t+1} as shifted rows of this buffer
 *   dy16    (B,T,ND*H) bf16;  c (B,T,ND,H) fp32;  whh (ND,4H,H) fp32 in the REFERENCE row order [gate][unit]
 * asr_rnn_pack_weights builds, once per step, the bf16 contraction operands from the fp32 master weights: W_ih with rows
 * re-ordered gate-minor (so that the input projection writes gates16 directly) and its transpose, b_ih + b_hh in that
 * order, the projection weight and its transpose.  Weight gradients computed in gate-minor order are stored at the
 * reference's rows (perm_h of asr_gemm16 / asr_colsum16).
 * The recurrence runs as ONE persistent launch of 8 independent groups (direction x batch slice, one per XCD) of H/16
 * workgroups: B <= 16 * (8/ND), H % 16 == 0, H <= 512 (asr_lstm16_workspace_bytes returns 0 otherwise: use the fp32
 * entry points).  workspace: CALLER-OWNED and PERSISTENT per (layer, pass), zero-filled once at allocation, 256B aligned;
 * `epoch` = number of launches this workspace has seen (the caller increments it): it is folded into the granule tags
 * and selects the exchange region, so a (region, tag) pair repeats only every 32 launches of the same workspace.
 * `reserved_cus`: compute units another stream may occupy meanwhile (data-parallel all-reduce): the launch is refused
 * (ASR_E_UNSUPPORTED) unless all its workgroups fit beside them (occupancy query).  The workspace starts with TWO 1 KB status
 * blocks used by launch parity: a launch reports in block (epoch & 1) - its first 32-bit word is the abort word (see "Status
 * word" below) - and clears the other block for its successor, so consecutive launches on a workspace MUST carry consecutive
 * epochs and an uncollected abort word of launch k-1 must be folded before launch k starts (it lives in the block k clears).
 */
size_t asr_lstm16_workspace_bytes(int B, int H, int ND, int backward);
int asr_lstm16_fwd(void* gates16, const float* whh, void* y16, float* c, int B, int T, int H, int ND,
                   void* workspace, size_t workspace_bytes, unsigned epoch, int reserved_cus, asr_stream_t stream);
int asr_lstm16_bwd(void* gates16, const float* whh, const void* dy16, const float* c, int B, int T, int H, int ND,
                   void* workspace, size_t workspace_bytes, unsigned epoch, int reserved_cus, asr_stream_t stream);
/* asr_lstm16_bwd has two kernels.  Form 1 (default, "gather"): for batch slices of at most 4 rows (ceil(B / (8/ND)) <= 4) the
 * workgroups exchange dh and each recomputes the elementwise cell backward of its whole slice.  Form 0 ("reduce-scatter"):
 * partial products handed to the owners of their columns; it serves larger slices always, and every shape when selected by
 * ASR_LSTM3_BWD=0 in the environment (read once) or asr_lstm16_set_bwd_form(0) (0 / 1 sets, anything else only asks; returns
 * the former value; the switch is one atomic word, safe to set from any thread, and a launch reads it once).
 * asr_lstm16_bwd_form: the form the PLAN names for a shape under the current switch - not what a launch will do: it ignores
 * asr_lstm_set_persistent(0) (no third-generation kernel runs at all) and the residency fall-back (a gather-form grid that does
 * not fit beside reserved_cus runs form 0).  What a launch did run is in its status block: it writes the form (1 reduce-scatter,
 * 2 gather) into 64-bit word 34.  Both forms take the same workspace. */
int asr_lstm16_set_bwd_form(int form);
int asr_lstm16_bwd_form(int B, int H, int ND);
/* asr_gemm on bf16 operands in HBM (same index conventions).  c_bf16 = 1: C bf16 = act(sum + bias), written;
 * c_bf16 = 0: C fp32, accumulated (accum / splits as asr_gemm), output row i stored at the reference row
 * (i / 4h)*4h + (i & 3)*h + (i % 4h >> 2) when perm_h = h > 0.  b_time_padded = 1 (with seqT, bshift): the reduction rows
 * of B live in a time-padded buffer (.,seqT+2,.), row (b,t) is read at padded row b*(seqT+2) + t + 1 + bshift.
 * Contiguous extents and row strides must be multiples of 8 elements, bases 16-byte aligned. */
int asr_gemm16(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long lda, long ldb, long ldc,
               int a_kc, int b_kc, int act, int accum, int splits, int c_bf16, int perm_h,
               int seqT, int bshift, int b_time_padded, asr_stream_t stream);
/* Which kernel asr_gemm16 takes for the same arguments (without the stream): 0 = the generic bf16-storage kernel, 1 = the
 * direct-to-LDS NT kernel at 128 x 128, 2 = the TN (weight-gradient) kernel, 3 = the NT kernel at 256 x 256 (ASR_GEMM16_BIG=1);
 * a negative ASR_E_* for arguments asr_gemm16 refuses.  Pure host arithmetic from the code the launch itself uses: no device
 * call, the pointers are looked at for their alignment only. */
int asr_gemm16_route(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long lda, long ldb, long ldc,
                     int a_kc, int b_kc, int act, int accum, int splits, int c_bf16, int perm_h,
                     int seqT, int bshift, int b_time_padded);
/* The plan behind that route (same arguments, host arithmetic only): returns the route and fills out[8] -
 *   route 0: the entries of asr_gemm_plan {fastA, fastB, plain_order, nx, ny, nz, gx, ngx} at bf16 operand size;
 *   route 1 / 3: {tiles along N, tiles along M, tile rows, tile columns, 0, 0, 0, 0};
 *   route 2: {tiles along M, tiles along N, reduction slices after clipping to the k-steps, k-steps per slice, LDS stages
 *             (ASR_GEMM16_TN_STAGES: 1, 2 or 4), workgroups, 0, 0}. */
int asr_gemm16_plan(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long lda, long ldb, long ldc,
                    int a_kc, int b_kc, int act, int accum, int splits, int c_bf16, int perm_h,
                    int seqT, int bshift, int b_time_padded, int out[8]);
int asr_rnn_pack_weights(const float* w_ih, const float* b_ih, const float* b_hh, const float* pj,
                         void* w_ih16, void* w_ihT16, float* bias, void* pj16, void* pjT16,
                         int H, int ND, int Din, int D, asr_stream_t stream);
/* fp32 <-> bf16 (accum = 1: dst += src, one float32 add per element; accum = 0: dst = src with the sign of zero kept).
 * asr_cast_bf16 rounds to nearest, ties to even: FLT_MAX and everything above the largest bf16 value's tie go to infinity,
 * +-0 and +-infinity keep their sign, NaN stays NaN.  SUBNORMAL float32 inputs are rounded like every other value
 * (nearest-even onto the bf16 subnormals, which share float32's exponent range); they are not flushed to zero.
 * src and dst 16-byte aligned, n > 0; anything else returns ASR_E_ARG and launches nothing. */
int asr_cast_bf16(const float* src, void* dst, long n, asr_stream_t stream);
int asr_cast_f32(const void* src, float* dst, long n, int accum, asr_stream_t stream);
/* the bf16 forms of asr_dropout_downsample_*, asr_act_bwd and asr_colsum2 (same Philox mask: flat index (b*T+t)*D+k);
 * y is addressed as y[y_off + b*y_bstride + t*D + k] (elements), which covers the time-padded y16; only those B*T rows of y
 * are read.  Kept values are bf16(float32(y) * float32(1 / (1 - p))), one float32 product and one nearest-even rounding.
 * D, y_bstride, y_off multiples of 8 and 16-byte aligned bases, else ASR_E_UNSUPPORTED; p, style and T2 are checked as for
 * the fp32 entry points below (ASR_E_ARG).  asr_act_bwd16: n % 8 == 0 and act = ASR_ACT_TANH / ASR_ACT_RELU, else ASR_E_ARG.
 * asr_colsum16: N % 8, lda % 8 or a misaligned A return ASR_E_UNSUPPORTED; lda < N or a perm_h > 0 with N % (4 perm_h) != 0
 * return ASR_E_ARG.  A refused call launches nothing and touches no output. */
int asr_dropout_downsample16_fwd(const void* y, long y_bstride, long y_off, void* z, int B, int T, int D, int T2, int rate,
                                 int style, float p, uint64_t seed, asr_stream_t stream);
int asr_dropout_downsample16_bwd(const void* dz, void* dy, int B, int T, int D, int T2, int rate, int style,
                                 float p, uint64_t seed, asr_stream_t stream);
int asr_act_bwd16(const void* dout, const void* out, void* dpre, long n, int act, asr_stream_t stream);
int asr_colsum16(const void* A, long lda, int M, int N, float* out, float* out2, int perm_h, asr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Dropout + time down-sampling between the LSTM and `pj` (src/module.py:1059-1076).
 *   style 0 'drop'  : z[b,t2,:]      = drop(y)[b, t2*rate, :]          z is (B,T2,D)
 *   style 1 'concat': z[b,t2,i*D+:]  = drop(y)[b, t2*rate+i, :]        z is (B,T2,D*rate)
 * keep(element) = Philox4x32-10(seed, flat index in y) >= p*2^32, kept values scaled by 1/(1-p);
 * asr_dropout_mask exports the same {0,1} mask (tests feed it to the oracle).  p = 0: no dropout.
 * Backward writes the full dy (B,T,D), zeros where nothing flowed.
 * keep in full: element i of y draws word i & 3 of Philox block i >> 2 - counter (low, high word of the block index, 0, 0),
 * key (low, high word of seed) - and is kept iff that word >= floor(float32(p) * 2^32), saturated at 2^32 - 1; the scale is
 * the float32 quotient 1 / (1 - p) and a kept value the float32 product y * scale.
 * Refused with ASR_E_ARG, nothing launched, by all four down-sampling entry points (fp32 and bf16):
 *   - p outside [0, 1) (asr_dropout_mask refuses it too);
 *   - style other than 0 or 1;
 *   - a T2 that asks for frames y does not have: style 0 with (T2 - 1) * rate >= T, style 1 with T2 * rate > T.
 * A SMALLER T2 than the caller's usual ceil(T / rate) resp. T / rate is legal: the forward drops the tail of y, the backward
 * writes zeros there.
 */
int asr_dropout_downsample_fwd(const float* y, float* z, int B, int T, int D, int T2, int rate, int style,
                               float p, uint64_t seed, asr_stream_t stream);
int asr_dropout_downsample_bwd(const float* dz, float* dy, int B, int T, int D, int T2, int rate, int style,
                               float p, uint64_t seed, asr_stream_t stream);
int asr_dropout_mask(float* mask, long n, float p, uint64_t seed, asr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Ragged batch through the unchanged recurrence launches (csrc/ragged.hip, src/ragged.py): inference on a padded batch
 * whose row b holds lens[b] valid frames (int64 on the device, clamped to [0,T] there).  Pure copies, bit-exact;
 * elem_bytes = 4 (fp32 layouts) or 2 (bf16 layouts); out of place (src != dst); no allocation, no synchronisation.
 *   asr_ragged_align  : gates (B,T,ND,W) -> dst of the same shape, W = 4H contiguous elements per (b,t,direction) in
 *                       both storage modes.  dst[b,t,0] = src[b,t,0] for t < n, dst[b,t,1] = src[b,t-(T-n),1] for
 *                       t >= T-n (the reverse walk then STARTS on the row's last valid frame), zeros elsewhere; source rows
 *                       at t >= n are never read.
 *   asr_ragged_unalign: y -> z with direction 1 shifted back and the layer's time down-sampling taken in the same pass.
 *                       y[b,t,d*H+j] is read at src[src_off + b*src_bstride + t*ND*H + d*H + j] (elements; the
 *                       time-padded y16 (B,T+2,ND*H) is src_bstride = (T+2)*ND*H, src_off = ND*H).  With
 *                       s_d = (d == 1 ? T-n : 0):
 *                         style 0 'drop'  : z (B,T2,ND*H),      z[b,t2,d*H+j]        = y[b, t2*rate + s_d, d*H+j]
 *                         style 1 'concat': z (B,T2,rate*ND*H), z[b,t2,i*ND*H+d*H+j] = y[b, t2*rate+i + s_d, d*H+j]
 *                       for t2 < ceil(n/rate) resp. n/rate (the frames the unpadded pass produces); every other row of z
 *                       is exactly 0.  ND = 1 shifts nothing and still zeroes the padding (with rate = 1: a masked copy).
 * Any extent is accepted: 16-byte accesses when W resp. H, the strides and the addresses allow them, element-wise else.
 * Null pointers, src == dst, bad dims / rate / style / elem_bytes or a batch stride that cannot hold T frames behind
 * src_off return ASR_E_ARG; B*T resp. B*T2 >= 2^23 rows returns ASR_E_UNSUPPORTED; nothing is launched then. */
int asr_ragged_align(const void* src, void* dst, const int64_t* lens, int B, int T, int ND, int W, int elem_bytes,
                     asr_stream_t stream);
int asr_ragged_unalign(const void* src, long src_bstride, long src_off, void* dst, const int64_t* lens, int B, int T,
                       int ND, int H, int T2, int rate, int style, int elem_bytes, asr_stream_t stream);
/* Zero tails for a convolutional front-end on a padded batch (src/vgg.py::conv_stack_lens).  In place, stores only: buf is
 * seen as (B, Ttot, W) elements of elem_bytes 4 or 2, and time rows t_off + clamp(lens[b],0,T) .. t_off + T - 1 of every batch
 * row b become exact zeros - what the next 3 x 3 convolution of the unpadded pass reads behind the row's last frame.  Nothing
 * else is written and nothing is read: valid frames, the rows in front of t_off and behind t_off + T keep their contents.
 *   unbordered fp32 image (B,t,f,C)    : T = Ttot = t, t_off = 0, W = f*C, elem_bytes 4
 *   zero-bordered image (B,t+2,f+2,C)  : T = t, Ttot = t+2, t_off = 1, W = (f+2)*C, elem_bytes 2 (bf16 activations) or 4 (the
 *                                        fp32 pre-activations of a CNNLayerNorm)
 * 16-byte stores when W*elem_bytes is a multiple of 16 and buf is 16-byte aligned, element-wise else; a batch row without a
 * tail costs its workgroups one read of lens[b].  Null pointers, B, T, W < 1, t_off < 0, t_off + T > Ttot, another
 * elem_bytes or a buf that is not elem_bytes-aligned return ASR_E_ARG; B*Ttot >= 2^23 rows returns ASR_E_UNSUPPORTED;
 * nothing is launched then. */
int asr_ragged_zero_tail(void* buf, const int64_t* lens, int B, int T, int Ttot, int t_off, int W, int elem_bytes,
                         asr_stream_t stream);

/* dpre = dout * act'(out) for act in {TANH, RELU} (autograd of torch.tanh / nn.ReLU on the path). */
int asr_act_bwd(const float* dout, const float* out, float* dpre, long n, int act, asr_stream_t stream);
/* out[j] += sum_i A[i*lda + j]  (bias gradients).  M <= 128: the sum is formed in a fixed order and added to out[j] once;
 * larger M: row blocks add their partial sums atomically, in any order. */
int asr_colsum(const float* A, long lda, int M, int N, float* out, asr_stream_t stream);
/* the same sums added to two vectors (an LSTM's bias_ih and bias_hh gradients are the same column sums); out2 may be NULL */
int asr_colsum2(const float* A, long lda, int M, int N, float* out, float* out2, asr_stream_t stream);
/* row-wise log_softmax (src/asr.py:120) and the backward of log_softmax(ReLU(.)) of the CTC head
 * (src/asr.py:29-32,120): dpre = (act > 0) ? dlogp - exp(logp) * rowsum(dlogp) : 0. */
int asr_log_softmax(const float* x, float* out, long rows, int V, asr_stream_t stream);
int asr_logsoftmax_relu_bwd(const float* dlogp, const float* logp, const float* act, float* dpre,
                            long rows, int V, asr_stream_t stream);
/* LayerNorm over the last axis (+ optional fused ReLU): nn.LayerNorm in RNNLayer.ln (src/module.py:1031,1057)
 * and CNNLayerNorm (src/module.py:546-550).  stats (rows,2) = mean, rstd.  dw/db are accumulated. */
int asr_layernorm_fwd(const float* x, const float* w, const float* b, float* y, float* stats,
                      long rows, int n, float eps, int relu, asr_stream_t stream);
int asr_layernorm_bwd(const float* dy, const float* x, const float* w, const float* b, const float* stats,
                      float* dx, float* dw, float* db, long rows, int n, int relu, asr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * CTC loss, torch.nn.CTCLoss(blank=0, zero_infinity=False) with reduction 'mean' as called at
 * bin/train_asr.py:135,237 (inputs are batch-major here: logp (B,T,V)).
 *   nll (B) per-utterance negative log-likelihood; *loss = mean_b nll_b / max(target_len_b,1)
 *   grad (B,T,V) = gscale * d loss / d logits in the folded form torch returns for log-softmax inputs
 *   (exp(logp) - posterior), exactly 0 for t >= input_len; +inf / NaN for infeasible alignments.
 * workspace: asr_ctc_loss_workspace_bytes(B,T,L) (alpha lattice).
 * Limit: 2*L+1 <= 1024 lattice states (L = padded target width <= 511 tokens), one state per thread of a workgroup;
 * longer targets return ASR_E_UNSUPPORTED; so does a vocabulary of which one frame of log-probs does not fit beside the lattice
 * buffers in 60 KB of LDS (V <= 15342 - 3 * (2L+1): about 15 300 classes for short targets, 12 273 at L = 511).
 */
size_t asr_ctc_loss_workspace_bytes(int B, int T, int L);
int asr_ctc_loss(const float* logp, const int64_t* targets, const int64_t* input_len, const int64_t* target_len,
                 float* nll, float* loss, float* grad, int B, int T, int V, int L, float gscale,
                 void* workspace, size_t workspace_bytes, asr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Sequence loss of the attention decoder + gradient (bin/train_asr.py:131-134,245; src/util.py:11-25).
 *   mode 0: CrossEntropyLoss(ignore_index=0);  mode 1: LabelSmoothingLoss(classes, smoothing)
 *   logits (B,L,V); targets (B,target_ld) int64; dlogits = gscale * d loss / d logits; accum2: scratch of 4 floats, 8-byte aligned (loss sum as 64-bit fixed point: order-independent, + count).
 */
int asr_xent(const float* logits, const int64_t* targets, long target_ld, float* dlogits, float* loss,
             float* accum2, int B, int L, int V, int mode, int classes, float smoothing, float gscale,
             asr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Attention decoder loop (src/asr.py:123-175; Attention.forward :333-364; LocationAwareAttention
 * src/module.py:1152-1173; Decoder.forward src/asr.py:259-266; pre_embed :35,128-133), num_head = 1,
 * v_proj = False, teacher forcing (tf_rate = 1) when `teacher` is given, greedy argmax otherwise.
 */
#define ASR_MAX_DEC_LAYERS 4
typedef struct {
    int B, Tp, E;       /* batch, encoder frames T', encoder feature dim */
    int A, Q;           /* attention dim, query dim = Dd*NL */
    int Dd, NL, V;      /* decoder LSTM dim, layers, vocabulary */
    int Kn, Ks;         /* loc_kernel_num, loc_kernel_size (taps = 2*Ks+1) */
    int L;              /* decode steps */
    float temperature;
} asr_dec_dims_t;

typedef struct {        /* reference state_dict tensors */
    const float *Wq, *bq;            /* attention.proj_q  (A,Q),(A) */
    const float *Wk, *bk;            /* attention.proj_k  (A,E),(A) */
    const float *Wconv;              /* attention.att_layer.loc_conv.weight (Kn,1,2Ks+1) */
    const float *Wproj;              /* attention.att_layer.loc_proj.weight (A,Kn) */
    const float *wg, *bg;            /* attention.att_layer.gen_energy (1,A),(1) */
    const float *emb;                /* pre_embed.weight (V,Dd) */
    const float *Wih[ASR_MAX_DEC_LAYERS], *Whh[ASR_MAX_DEC_LAYERS];   /* decoder.layers.weight_{ih,hh}_l* */
    const float *bih[ASR_MAX_DEC_LAYERS], *bhh[ASR_MAX_DEC_LAYERS];
    const float *Wc, *bc;            /* decoder.char_trans (V,Dd),(V) */
} asr_dec_weights_t;

typedef struct {        /* gradient accumulators, same shapes (+=) */
    float *Wq, *bq, *Wk, *bk, *Wconv, *Wproj, *wg, *bg, *emb;
    float *Wih[ASR_MAX_DEC_LAYERS], *Whh[ASR_MAX_DEC_LAYERS], *bih[ASR_MAX_DEC_LAYERS], *bhh[ASR_MAX_DEC_LAYERS];
    float *Wc, *bc;
} asr_dec_grads_t;

typedef struct {        /* forward outputs / saved activations, caller-allocated */
    float* key;         /* (B,Tp,A)   tanh(proj_k(enc)) */
    float* att;         /* (B,L,Tp)   attention weights per step (= att_seq of the reference, num_head 1) */
    float* q;           /* (B,L,A)    tanh(proj_q(.)) */
    float* xin;         /* (B,L,Dd+E) decoder input [embedding | context] */
    float* gates;       /* (B,L,NL,4Dd) activated gates; overwritten with pre-activation gradients by backward */
    float* cs;          /* (B,L,NL,Dd) */
    float* hs;          /* (B,L,NL,Dd) */
    float* logits;      /* (B,L,V)    att_output */
    float* energy;      /* (B,Tp)     scratch */
    float* conv;        /* (B,L,Kn,Tp) location-convolution output per step, kept for backward; may be NULL for inference */
    void* key16;        /* (B,Tp,A) bf16 working copy of key for the step kernels; NULL = read the fp32 tensor (fp32 mode) */
    void* enc16;        /* (B,Tp,E) bf16 working copy of enc, filled by asr_att_decoder_fwd; NULL = read enc */
    void* work;         /* optional scratch (256B aligned, asr_att_decoder_fwd_work_bytes) enabling the single-launch forward.  Its first
                         * 4 KB are a status block: abort word first, and a word in which asr_att_decoder_fwd records whether it took the
                         * single launch.  asr_att_decoder_bwd reads that record, so hand it the state with the area as the forward left it. */
    size_t work_bytes;
    int64_t* tokens;    /* (B,L)      input token of each step (<sos>=0 first) */
} asr_dec_state_t;

int asr_att_decoder_fwd(const asr_dec_dims_t* dims, const asr_dec_weights_t* weights,
                        const float* enc, const int64_t* enc_len, const int64_t* teacher, int teacher_ld,
                        const asr_dec_state_t* state, int prec, asr_stream_t stream);
size_t asr_att_decoder_bwd_workspace_bytes(const asr_dec_dims_t* dims);
/* bit 0 / bit 1: run the teacher-forced forward / backward loop as one persistent launch where the shape has a plan
 * (default on, env ASR_DEC_PERSIST / ASR_DEC_PERSIST_BWD); bit 2 / bit 3: prefer the streamed-tile plan (csrc/decoder_stream.hip)
 * forward / backward even where the LDS-resident plan exists (env ASR_DEC_STREAM=1); returns the previous flags.  For A/B tests. */
int asr_att_decoder_set_persistent(int flags);
/* Which plan asr_att_decoder_fwd / _bwd take for this shape (reference loop: src/asr.py:123-175): 0 = per-step kernels,
 * 1 = one persistent launch with the key / enc tiles resident in LDS (B <= 16 x T' <= 640, B <= 8 up to T' = 750 / 850),
 * 2 = one persistent launch with the tiles streamed from L2 / HBM (any T', B <= 64: the reference's B = 8 batches of up to
 * 3 400 frames, src/collect_batch.py:21-24, and BASELINE config 5). */
int asr_att_decoder_fwd_plan(const asr_dec_dims_t* dims);
int asr_att_decoder_bwd_plan(const asr_dec_dims_t* dims);
/* Which instantiation of the forward energy kernel the per-step path (asr_att_decoder_fwd without a persistent plan,
 * asr_att_decoder_step) launches for this shape: *knmax in {4, 10, 16} is the location-filter count it is compiled for,
 * *tpw in {2, 4, 5, 8} the encoder frames per wave.  Host code only; ASR_E_ARG on a null pointer or dims the step refuses. */
int asr_att_decoder_energy_plan(const asr_dec_dims_t* dims, int* knmax, int* tpw);
/* tiles per utterance when asr_att_decoder_bwd runs the whole loop as ONE persistent launch (0: no plan for this shape,
 * the per-step kernels run); offset of that launch's 4 KB status block (abort word first) inside the workspace. */
int asr_att_decoder_bwd_persistent_tiles(const asr_dec_dims_t* dims);
size_t asr_att_decoder_bwd_status_offset(const asr_dec_dims_t* dims);
/* bytes of state->work that let asr_att_decoder_fwd run the teacher-forced loop as ONE persistent launch (0: shape has no plan) */
size_t asr_att_decoder_fwd_work_bytes(const asr_dec_dims_t* dims);
/* dlogits (B,L,V) in; denc (B,Tp,E) accumulated (+=); parameter gradients accumulated into `grads`.
 * workspace must be 256B aligned. */
int asr_att_decoder_bwd(const asr_dec_dims_t* dims, const asr_dec_weights_t* weights, const asr_dec_grads_t* grads,
                        const float* enc, const int64_t* enc_len, const asr_dec_state_t* state,
                        const float* dlogits, float* denc,
                        void* workspace, size_t workspace_bytes, int prec, asr_stream_t stream);

/* The same in two halves, for callers that overlap the parameter gradients with later work: asr_att_decoder_bwd_ex with
 * defer_params != 0 stops when the gradient wrt the encoder output is complete (denc; the critical path of the backward
 * pass) and reports in *looped_out which loop implementation ran; asr_att_decoder_bwd_params then computes every parameter
 * gradient of the decoder from the SAME workspace and saved state - on any stream, once the first half has completed
 * there.  asr_att_decoder_bwd = _ex(defer_params 0).  (Reference: one autograd backward, /root/reference/src/asr.py:155-249.) */
int asr_att_decoder_bwd_ex(const asr_dec_dims_t* dims, const asr_dec_weights_t* weights, const asr_dec_grads_t* grads,
                           const float* enc, const int64_t* enc_len, const asr_dec_state_t* state,
                           const float* dlogits, float* denc,
                           void* workspace, size_t workspace_bytes, int prec, int defer_params, int* looped_out,
                           asr_stream_t stream);
int asr_att_decoder_bwd_params(const asr_dec_dims_t* dims, const asr_dec_weights_t* weights, const asr_dec_grads_t* grads,
                               const float* enc, const int64_t* enc_len, const asr_dec_state_t* state, const float* dlogits,
                               void* workspace, size_t workspace_bytes, int looped, int prec, asr_stream_t stream);
/* asr_att_decoder_bwd_ex with an outside gradient on the decoder states: dhs_ext (B,L,Dd), the gradient wrt the TOP layer's
 * h_t of every step (what ASR.forward returns as dec_state; the embedding regulariser reads it, src/plugin.py), is added to
 * dh_top = dlogits W_c by one elementwise launch on `stream` before the first recurrence kernel.  dhs_ext = NULL is
 * asr_att_decoder_bwd_ex itself: the same launches with the same arguments. */
int asr_att_decoder_bwd_hs(const asr_dec_dims_t* dims, const asr_dec_weights_t* weights, const asr_dec_grads_t* grads,
                           const float* enc, const int64_t* enc_len, const asr_dec_state_t* state,
                           const float* dlogits, const float* dhs_ext, float* denc,
                           void* workspace, size_t workspace_bytes, int prec, int defer_params, int* looped_out,
                           asr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Word-embedding regulariser and embedding-fused decoding (reference src/plugin.py::EmbeddingRegularizer), fp32, csrc/emb_fuse.hip.
 * Every sum below has a fixed order (no float atomics): equal inputs give equal bits.
 *
 * asr_emb_cos_loss: nn.CosineEmbeddingLoss(reduction='none') with target +1 between x (B*L,E) and table[label] (table (V,E),
 *   label (B,label_ld) int64), pad rows masked, per-utterance mean, batch mean (src/plugin.py:145-155), forward and backward
 *   in one call:
 *     cos_r = <x_r, y_r> / sqrt((|x_r|^2 + 1e-12) (|y_r|^2 + 1e-12))          (ATen's formula; its epsilon is the FLOAT constant 1e-12)
 *     w_r   = 1 / (B count_b) when label_r != 0, else 0;  count_b = non-pad labels of the row's utterance
 *     *loss = sum_r w_r (1 - cos_r);  dx (B*L,E) = d loss / d x;  dy (B*L,E) = d loss / d (gathered table rows), or NULL when
 *     the table is frozen (asr_embedding_bwd scatters it into the table's gradient).  All three are written, not accumulated.
 *   An utterance WITHOUT a non-pad label contributes 0 and gets zero gradients; the reference divides 0 by 0 there and returns
 *   NaN.  Real transcripts end in <eos> and never do this.  A label outside [0,V) counts as pad.
 *   row_loss: scratch of B*L floats (the per-row terms, summed in row order by one workgroup).
 *   E >= 1 of any size, 2 <= V <= 65536.
 *
 * asr_emb_fuse_fwd: out (N,V) = log((1 - lam_v) softmax(dec_logit)_v + lam_v softmax(relu(temp_v) emb_logit)_v + 1e-8)
 *   (src/plugin.py:103-123).  dec_logit rows are dec_ld >= V apart, emb_logit and out are dense.
 *   temp: RAW temperature, relu applied here; temp_stride 0 = one scalar, 1 = one value per token.  temp <= 0: uniform p_emb.
 *   lam: lam_stride as for temp; lam_sigmoid != 0: lam_v = sigmoid(lam[v]) (the learnable forms), else lam[v] itself.
 *   lam = 0 gives log(p_dec + 1e-8) as computed, lam = 1 log(p_emb + 1e-8).  Both softmaxes subtract their row maximum.
 *   stats (N,2): log-sum-exp of dec_logit and of relu(temp) emb_logit, kept for the backward.
 *   argmax: NULL, or int64 with row r at argmax[r * argmax_ld]: the index of the largest out value, the lowest on a tie.
 *   2 <= V <= 65536: one wave per row up to V = 2048, one workgroup per row above.
 * asr_emb_fuse_bwd: d_dec_logit, d_emb_logit (N,V dense, written) from dout (N,V dense); the probabilities are formed again
 *   from the logits and stats.  g = dout / (fused + 1e-8); each softmax backward is p (dp - <dp, p>).
 *   d_temp / d_lam_raw: NULL, or the gradient wrt the RAW parameter (1 or V entries by its stride, written): d_temp carries
 *   1[temp > 0], d_lam_raw carries sigmoid' when lam_sigmoid.  They need `work`: N * (temp_stride ? V : 1) floats when d_temp is
 *   asked for plus N * (lam_stride ? V : 1) when d_lam_raw is (the per-row terms, summed over the rows in a fixed order).
 *
 * asr_row_normalize_fwd / _bwd: y = x / max(||x||_2, 1e-12) per row of x (N,E) (F.normalize(x, dim=-1), src/plugin.py:107-108)
 *   and dx from dy.  A row below the epsilon is x / 1e-12 with dx = dy / 1e-12, as in torch; an all-zero row (row 0 of an
 *   embedding table with padding_idx 0) stays zero and gets a ZERO gradient, where torch returns dy / 1e-12.
 */
int asr_emb_cos_loss(const float* x, const float* table, const int64_t* label, long label_ld, float* loss, float* dx, float* dy,
                     float* row_loss, int B, int L, int E, int V, asr_stream_t stream);
int asr_emb_fuse_fwd(const float* dec_logit, long dec_ld, const float* emb_logit, const float* temp, int temp_stride,
                     const float* lam, int lam_stride, int lam_sigmoid, float* out, float* stats, int64_t* argmax, long argmax_ld,
                     int N, int V, asr_stream_t stream);
int asr_emb_fuse_bwd(const float* dout, const float* dec_logit, long dec_ld, const float* emb_logit, const float* temp,
                     int temp_stride, const float* lam, int lam_stride, int lam_sigmoid, const float* stats, float* d_dec_logit,
                     float* d_emb_logit, float* d_temp, float* d_lam_raw, float* work, int N, int V, asr_stream_t stream);
int asr_row_normalize_fwd(const float* x, float* y, long N, int E, asr_stream_t stream);
int asr_row_normalize_bwd(const float* dy, const float* x, float* dx, long N, int E, asr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Flat-buffer step: global-norm clip + NaN guard (src/solver.py:96-103) fused with torch.optim.Adadelta
 * (src/optim.py:29,53-54).  normsq: device pointer to the sum of squares of `grad` (asr_sumsq);
 * grad_mul is applied to the stored gradient first (1/world_size when the buffer holds an all-reduced sum).
 *
 * Status word.  A persistent launch (asr_lstm_*, asr_att_decoder_*) whose workgroups could not hand data to each other
 * within a bounded number of polls (workgroups not co-resident, e.g. the GPU shared with another stream's kernels) sets
 * the abort word = the first 32-bit word of its workspace / status block and returns garbage.  The entry points never
 * synchronise, so the caller folds those words into ONE sticky device word after the step's launches:
 *   asr_status_collect(abort_words[n <= 32] (HOST array of device pointers), n, status): bit i of *status is set when
 *   abort word i is non-zero.  asr_adadelta_step(..., status, ...) refuses the update while *status != 0 (like the
 *   NaN guard); the host reads the word wherever it synchronises anyway and raises (src/step.py, src/solver.py).
 */
int asr_sumsq(const float* x, long n, double* out, asr_stream_t stream);
int asr_scale(float* x, long n, float k, asr_stream_t stream);
/* The loss mix with every scalar on the device (bin/train_asr.py:229-248: total = w ctc + (1 - w) att, then backward):
 *   asr_loss_mix  : out[0] = a[0] wa[0] + b[0] wb[0]  (b, wb may be NULL) - the forward and, with a = grad_output, each branch of the backward;
 *   asr_scale_dev : out[i] = in[i] alpha[0] - a loss kernel's stored gradient times its grad_output (autograd of CTCLoss / CrossEntropy). */
int asr_scale_dev(const float* in, float* out, long n, const float* alpha, asr_stream_t stream);
int asr_loss_mix(const float* a, const float* wa, const float* b, const float* wb, float* out, asr_stream_t stream);
int asr_status_collect(const void* const* abort_words, int n, unsigned* status, asr_stream_t stream);
int asr_adadelta_step(float* param, const float* grad, float* square_avg, float* acc_delta, long n,
                      float lr, float rho, float eps, float weight_decay, float clip,
                      const double* normsq, float grad_mul, const unsigned* status, asr_stream_t stream);
/* torch.optim.Adam (the reference's LM trainer: /root/reference/bin/train_lm.py:38, src/optim.py:27-28) behind the same clip /
 * NaN guard / status refusal; bias corrections in double.  `step_counter` (device, may be NULL): number of updates APPLIED so
 * far - the kernel uses *step_counter + 1 and the call advances it only when the update was applied (torch advances its step
 * on applied steps only); with NULL, `step` = 1-based update count from the host.  max_exp_avg_sq: amsgrad state or NULL. */
int asr_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, long n,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int step, float clip,
                  const double* normsq, float grad_mul, const unsigned* status, unsigned long long* step_counter, asr_stream_t stream);
/* Embedding gradient (nn.Embedding backward of the RNN-LM, /root/reference/src/lm.py:16,28): demb[v,:] += sum of the rows r
 * of dy (rows x width, leading dimension dy_ld) with idx[r] == v; fixed summation order. */
int asr_embedding_bwd(const float* dy, long dy_ld, const int64_t* idx, float* demb, int rows, int width, int V, asr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Acoustic front-end, batched on the GPU (the reference runs it per utterance in DataLoader workers).
 *   asr_fbank: ExtractAudioFeature.forward (src/audio.py:158-171, 231-244).  wav (B,N) fp32 zero-padded,
 *     wav_len (B) samples; out (B,T,nmel), T >= 1 + (max(wav_len)-1)/hop, frames beyond an utterance are 0.
 *     dft_table (2*(n_fft/2+1), win): rows f = cos, rows nb+f = -sin of 2*pi*f*(m + (n_fft-win)/2)/n_fft;
 *     mel_fb (nmel, n_fft/2+1); window (win).  Tables are built by the host (src/audio.py).
 *   asr_delta_stack: Delta + Postprocess (src/audio.py:59-93, 108-121).  x (B,T,F), lens (B) frames,
 *     filters (channels, taps) as Delta._create_filters builds them; out (B,T,channels*F) channel-major.
 *   asr_specaug: Augment (src/audio.py:364-406), in place on x (B,T,D) using lens.  draws_in (B,6) int32 =
 *     {t, t0, tend, f, f0, fend} in the reference's draw order, or NULL to draw on the device
 *     (Philox, seed); draws_out (B,6) optional: the draws as applied.
 * Edges, the same for all four entry points:
 *   - a length is taken as min(length, padded extent): wav_len against N, lens against T; a length <= 0 is an empty utterance
 *     (asr_fbank and asr_delta_stack write zero rows, SpecAugment leaves it alone);
 *   - asr_fbank refuses an even n_fft (ASR_E_ARG, nothing launched): its frame count 1 + (n-1)/hop is that of centre padding
 *     with an odd n_fft.  An utterance of n samples owns rows [0, 1 + (n-1)/hop), n <= 1 gives zeros;
 *   - SpecAugment device draws, with r0..r5 the Philox words of (seed, utterance) and len = min(lens[b], T):
 *       t = r0 % min(time_width, max(len, 1)),  t0 = r1 % max(len - t, 1),  tend = t0 + r2 % t   (t == 0: no time mask)
 *       f = r3 % min(freq_width, D),            f0 = r4 % (D - f),          fend = f0 + r5 % f   (f == 0: no frequency mask)
 *     so that 0 <= t0 <= tend <= len and 0 <= f0 <= fend <= D always.  For len >= time_width and D >= freq_width these are the
 *     reference's draws; below, where the reference raises (randint over an empty range), the mask width is drawn below the
 *     utterance's own extent.  The time band is filled with the mean of the valid len x D region, the frequency band with the
 *     mean after that fill;
 *   - caller-supplied draws_in are clamped into the utterance before use: t0 to [0, len], tend to [t0, len], f0 to [0, D],
 *     fend to [f0, D]; t == 0 / f == 0 switch the band off as in the reference.  No draw can store outside len x D.
 *   asr_cmvn: CMVN.forward (src/audio.py:31-34, mode 'global', placed after Delta and before Postprocess / Augment by
 *     create_transform :477-478), in place on x (B,T,D) fp32 using lens: with len = min(lens[b], T), every column d of
 *     utterance b becomes (x - mean) / (eps + std), mean and std over its len valid frames only, std the unbiased one
 *     (divisor len - 1), eps added to the standard deviation.  Two launches on `stream`, no host sync, no atomics: 16 workgroups
 *     per utterance and 64-column tile form float64 (count, mean, M2) moments over disjoint frame ranges (Welford per thread, Chan
 *     merges in a fixed order, no sum of squares), the second launch merges them in range order and normalises in float64,
 *     rounding once to fp32.  Two calls on the same input give the same bits.  workspace: asr_cmvn_workspace_bytes(B, D)
 *     bytes, 8-byte aligned, contents irrelevant.  stats_out (B,2,D) or NULL: [b,0,d] = mean, [b,1,d] = unbiased std, fp32-rounded.
 *     Edges: rows t >= len are neither read nor written; len <= 0 leaves the utterance alone (stats_out entries 0);
 *     len == 1 turns the valid row into NaN as the reference does (0 / (eps + NaN); stats_out std NaN, mean the row itself);
 *     a constant column gives exactly 0.  Refused with ASR_E_ARG, nothing launched: a null x, lens or workspace, B, T or D <= 0,
 *     B > 65535, workspace_bytes below asr_cmvn_workspace_bytes(B, D), a workspace that is not 8-byte aligned.
 */
size_t asr_fbank_workspace_bytes(int B, int T, int win, int n_fft);
int asr_fbank(const float* wav, const int64_t* wav_len, float* out, const float* dft_table, const float* mel_fb,
              const float* window, int B, int N, int T, int win, int hop, int n_fft, int nmel,
              float preemph, float ref_db, float min_db,
              void* workspace, size_t workspace_bytes, asr_stream_t stream);
int asr_delta_stack(const float* x, const int64_t* lens, float* out, const float* filters,
                    int B, int T, int F, int channels, int taps, asr_stream_t stream);
int asr_specaug(float* x, const int64_t* lens, const int* draws_in, int* draws_out, int B, int T, int D,
                int time_width, int freq_width, uint64_t seed, asr_stream_t stream);
/* the same with the reductions spread over 16 workgroups per utterance (two launches; workspace of asr_specaug_workspace_bytes(B)) */
size_t asr_specaug_workspace_bytes(int B);
int asr_specaug_ws(float* x, const int64_t* lens, const int* draws_in, int* draws_out, int B, int T, int D,
                   int time_width, int freq_width, uint64_t seed, void* workspace, size_t workspace_bytes, asr_stream_t stream);
size_t asr_cmvn_workspace_bytes(int B, int D);
int asr_cmvn(float* x, const int64_t* lens, float* stats_out /* (B,2,D) mean, std or NULL */, int B, int T, int D, float eps,
             void* workspace, size_t workspace_bytes, asr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * SpecAugment policies (data.audio.augment as a mapping): time warp, up to 8 frequency masks, up to 32 time
 * masks, mean or zero fill.  Out of place: x (B,T,D) fp32 is read only, out (B,T,D) must not overlap it.  Every length is taken
 * as n = min(max(lens[b], 0), T).  At most two launches on `stream`, no allocation, no host sync, no atomics: two calls give
 * the same bits.
 *   Draws: word group k of utterance b is philox4x32(counter (b, k, 3, 0), key (seed lo, seed hi)); a group uses r0, r1.
 *     group 0: the warp, active iff warp > 0 && n >= 2 warp + 1; w0 = warp + r0 % (n - 2 warp), w = r1 % (2 warp + 1) - warp,
 *       c = clamp(w0 + w, 1, n - 2): source frame w0 lands on destination frame c;
 *     group 1 + j, j < freq_masks: Fw = min(freq_width, D), f = r0 % (Fw + 1), f0 = r1 % (D - f + 1), band [f0, f0 + f);
 *     group 9 + j, j < cnt, cnt = time_count_pm ? min(time_masks, n time_count_pm / 1000) : time_masks:
 *       Tw = min(time_width, n time_ratio_pm / 1000), t = r0 % (Tw + 1), t0 = r1 % (n - t + 1), band [t0, t0 + t).
 *   Record: (B,82) int32 per utterance {w0, c, (f0, fend) x 8, (t0, tend) x 32}, (0, 0) where a group is inactive.  draws_out
 *     (or NULL) receives it as applied.  draws_in (or NULL) has the same layout and replaces the RNG: the warp is off unless
 *     1 <= w0 <= n - 2 && 1 <= c <= n - 2, bands are clamped into [0, D] and [0, n] with end >= start.
 *   Warp: destination frame t < n reads source position base + num / den: t <= c: num = t w0, den = c, base = 0; otherwise
 *     num = (t - c)(n - 1 - w0), den = n - 1 - c, base = w0.  With i = base + num / den and r = num % den in integers the value
 *     is x[i] when r == 0, else x[i] + float(r) / float(den) * (x[i + 1] - x[i]) in fp32.  Warp off: out = x bit for bit.
 *   Fill: 1 = exactly 0.0f; 0 = one value per utterance, float32(sum / (n D)) over the n D valid values of x, the sum formed in
 *     float64 at fixed slots and added in a fixed order (with fill = 1 that launch is skipped and workspace may be NULL).
 *   Output: t < n: the fill inside any band, else the warped value; rows t >= n, and an utterance with n == 0, are copies of x.
 *   workspace: asr_specaug_policy_workspace_bytes(B) bytes, 8-byte aligned, contents irrelevant.
 * Refused with ASR_E_ARG, nothing launched: a null x, lens or out; B, T or D <= 0; freq_masks outside 0..8, time_masks outside
 * 0..32; a negative warp, freq_width or time_width; a per-mille value outside 0..1000; fill outside {0, 1}; x and out that
 * overlap; a workspace below the stated size or not 8-byte aligned; a NULL workspace with fill = 0; B beyond 2^25.
 */
size_t asr_specaug_policy_workspace_bytes(int B);
int asr_specaug_policy(const float* x, const int64_t* lens, float* out, const int* draws_in, int* draws_out,
                       int B, int T, int D, int warp, int freq_masks, int freq_width, int time_masks, int time_width,
                       int time_ratio_pm, int time_count_pm, int fill /* 0 mean, 1 zero */, uint64_t seed,
                       void* workspace, size_t workspace_bytes, asr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Waveform augmentation (data.audio.time_aug; ReadAudio.augmenter src/audio.py:283-309: Gaussian noise p = 0.3, time stretch
 * p = 0.3, pitch shift p = 0.5), in place on wav (B,N) fp32 using wav_len; DESIGN.md 4.14 is the recipe.  All stages keep every
 * length; samples n >= min(wav_len[b], N) are neither read nor written.
 *   draws (B,6) fp32 = {noise_on, amp, stretch_on, rate, pitch_on, semitones}.  asr_wave_draws fills draws_out from draws_in, or,
 *     when that is NULL, from two Philox4x32-10 blocks (b, 0, 3, 0) and (b, 0, 4, 0) keyed by seed: u_i = fp32(r_i) * 2^-32,
 *     switches u < 0.3 / 0.3 / 0.5, values lo + u * (hi - lo) over (0.001, 0.01), (0.8, 1.25), (-4, 4), all in fp32 without
 *     contraction.  Switches come out as 0 / 1.  The stretch switch is recorded 0 when len <= n_fft/2 (no reflect padding) or the
 *     rate is outside [0.5, 2] or NaN; the pitch switch likewise with its rate 2^(-semitones/12).  rates_out (B,2) or NULL:
 *     {stretch rate, pitch rate} as fp32, 0 where the switch is off - what the four kernels below read.
 *   rates: rate of utterance b at rates[b * rate_stride].  The rates live on the device, so a bad one cannot be refused by the
 *     host: an utterance whose rate is outside [0.5, 2] (0, NaN) or whose len <= n_fft/2 is skipped by every kernel.
 *   table (2 * n_fft) fp32: n_fft/2 twiddles (cos, -sin)(2 pi k / n_fft) interleaved, then the periodic Hann window.
 *   asr_wave_noise: x[n] += amp * z[n] where noise_on; z as stated in csrc/wave_aug.hip (Box-Muller, Philox (n/4, b, 5, 0)).
 *   asr_wave_stft: spec (B, F = 1 + N/hop, n_fft/2 + 1) complex fp32, hop = n_fft/4, centred, reflect padding; an utterance
 *     writes its 1 + len/hop frames.
 *   asr_wave_pvoc: out (B, 2F, n_fft/2 + 1) complex; an utterance writes ceil(n_frames / rate) frames.
 *   asr_wave_istft: overlap-add to M = round(len / rate) samples (half to even).  keep_len = 1: dst[b * dst_stride + m] for
 *     m < len, zeros from M on (dst_stride >= N; the wave itself); keep_len = 0: m < M (dst_stride >= 2N).
 *   asr_wave_resample: wav[b][i], i < len, = the band-limited interpolation of src[b * src_stride + 0..M) at i / rate
 *     (src_stride >= 2N).
 *   asr_wave_augment: asr_wave_draws, asr_wave_noise, then stft -> pvoc -> istft(keep_len) with the stretch rates, then
 *     stft -> pvoc -> istft -> resample with the pitch rates, in slices of utterances whose spectrograms fit 256 MiB; bit for bit
 *     what the single entry points give.  workspace: asr_wave_augment_workspace_bytes(B, N, n_fft) bytes (0 for bad
 *     arguments), 16-byte aligned, contents irrelevant.  No allocation, no host sync, no atomics: two calls give the same bits.
 * Refused with ASR_E_ARG, nothing launched: a null pointer (draws_in, draws_out of asr_wave_augment and rates_out may be NULL),
 * B or N <= 0, B > 65535, N > 2^28, n_fft not a power of two in 64..2048, rate_stride <= 0, a stride below the stated one, keep_len
 * other than 0 / 1, a short or misaligned workspace.
 */
int asr_wave_draws(const int64_t* wav_len, const float* draws_in, float* draws_out, float* rates_out, int B, int N, int n_fft,
                   uint64_t seed, asr_stream_t stream);
int asr_wave_noise(float* wav, const int64_t* wav_len, const float* draws, int B, int N, uint64_t seed, asr_stream_t stream);
int asr_wave_stft(const float* wav, const int64_t* wav_len, const float* rates, int rate_stride, const float* table, float* spec,
                  int B, int N, int n_fft, asr_stream_t stream);
int asr_wave_pvoc(const float* spec, const int64_t* wav_len, const float* rates, int rate_stride, float* out, int B, int N,
                  int n_fft, asr_stream_t stream);
int asr_wave_istft(const float* out_spec, const int64_t* wav_len, const float* rates, int rate_stride, const float* table,
                   float* dst, long dst_stride, int keep_len, int B, int N, int n_fft, asr_stream_t stream);
int asr_wave_resample(const float* src, long src_stride, const int64_t* wav_len, const float* rates, int rate_stride, float* wav,
                      int B, int N, int n_fft, asr_stream_t stream);
size_t asr_wave_augment_workspace_bytes(int B, int N, int n_fft);
int asr_wave_augment(float* wav, const int64_t* wav_len, const float* draws_in, float* draws_out, const float* table, int B,
                     int N, int n_fft, uint64_t seed, void* workspace, size_t workspace_bytes, asr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * VGG front-ends (VGGExtractor src/module.py:659-716, VGGExtractor_LN :582-657) on channel-last images
 * (B,T,F,C).  asr_conv3x3 = nn.Conv2d(k=3, stride 1, pad 1) as an implicit GEMM on MFMA:
 *   mode 0: out[(b,t,f), n] (+)= act( sum_{tap,ci} img[(b,t+dt,f+df), ci] * w[n][tap*C+ci] + bias[n] )
 *           (forward with the (Co, 9*Ci) weight copy; input gradient with the flipped (Ci, 9*Co) copy)
 *   mode 1: dw[n][tap*C+ci] += sum_pixels dout[pixel, n] * img[pixel shifted by tap, ci]   (w_or_dout = dout)
 * asr_conv_weight_permute builds those copies from / folds the gradient back into the reference's
 * (Co,Ci,3,3) tensors (modes 0,1,2).  asr_maxpool2x2_* = nn.MaxPool2d(2, stride 2[, ceil_mode]); idx keeps
 * the arg-max (0..3 = 2 dt + df; of equal maxima the first in that order); T2 x F2 windows with 1 <= T2 <= ceil(T/2),
 * 1 <= F2 <= ceil(F/2) - anything larger is refused by the forward AND the backward (ASR_E_ARG, nothing launched); the
 * backward writes all of dx, zeros where no window reaches or the element was not the arg-max.
 * asr_ln_freq_* = CNNLayerNorm (LayerNorm over F, affine per f) + optional ReLU; the backward takes F <= 128 (ASR_E_UNSUPPORTED);
 * stats (rows*C, 2).  asr_permute_last2: out[r,b,a] = in[r,a,b] (channel-major <-> channel-last).
 * asr_conv3x3 refuses, before anything is launched and with `out` untouched: a NULL img / w_or_dout / out or a dim <= 0
 * (ASR_E_ARG); mode other than 0 or 1, prec other than ASR_F32 / ASR_BF16, act other than ASR_ACT_NONE / _TANH / _RELU, accum
 * other than 0 or 1 (ASR_E_ARG); mode 1 without accum = 1, with an activation or with a bias (ASR_E_ARG: the weight gradient
 * is added onto dw, in 8 reduction slices from 4096 pixels and 32 from 65536, by fp32 atomics); B*T*F >= 2^31 or 9*C >= 2^31
 * (ASR_E_UNSUPPORTED).  The image is read with 16-byte loads where C % 4 == 0 and img is 16-byte aligned, element by
 * element otherwise; w_or_dout, out and bias need 4-byte alignment only.
 * asr_conv3x3_plan: the plan asr_conv3x3 launches with for the same arguments (without the stream), the eight entries of
 * asr_gemm_plan {fastA, fastB, plain_order, nx, ny, nz, gx, ngx} - mode 0: A = the image (fastA = 0), nx = column tiles of
 * N, ny = tiles of the B*T*F pixels, nz = 1; mode 1: B = the image (fastB = 0), nx = column tiles of 9*C, ny = row tiles of
 * N, nz = reduction slices.  Host arithmetic from the function the launch itself plans with: no device call, the pointers are
 * looked at for their alignment only.  Returns what asr_conv3x3 returns for refused arguments (plan untouched).
 */
int asr_conv3x3(const float* img, const float* w_or_dout, float* out, const float* bias,
                int B, int T, int F, int C, int N, int mode, int act, int accum, int prec, asr_stream_t stream);
int asr_conv3x3_plan(const float* img, const float* w_or_dout, float* out, const float* bias,
                     int B, int T, int F, int C, int N, int mode, int act, int accum, int prec, int plan[8]);

/* ---- bf16 VGG front-end (bf16 contraction mode), csrc/vgg16.hip ----------------------------------------------------
 * The same layers - nn.Conv2d(k 3, stride 1, pad 1) + ReLU / CNNLayerNorm, nn.MaxPool2d(2, 2[, ceil_mode]) of
 * /root/reference/src/module.py:599-614 (VGGExtractor_LN) and :670-681 (VGGExtractor) - on ZERO-BORDERED channel-last bf16
 * images P(T,F,C) = (B, T+2, F+2, C): a tap of the 3x3 stencil is then a constant row shift of the pixel-row matrix and the
 * convolution is an implicit GEMM on the direct-to-LDS bf16 contraction kernel (no bounds tests, no fp32 staging).
 *   asr_vgg16_im2col      feature (B,T,Cin*F) fp32 -> patch matrix (B*(T+2)*(F+2), Kp) bf16 of the FIRST layer (Cin = 4: K = 36 -> Kp 40)
 *   asr_conv_weight_pack16 (Co,Ci,3,3) fp32 -> (Co, Kp) bf16 [tap*Ci+ci] (mode 0) / flipped (Ci, Kp) [tap*Co+co] (mode 1: input gradient)
 *   asr_conv3x3_16        out P(T,F,N) = act(conv(img) + bias), borders written as zeros; implicit = 1: img = P(T,F,C), C % 64 == 0,
 *                         K = 9*C; implicit = 0: img = an explicit (rows, K) patch matrix over the same pixel grid
 *   asr_conv3x3_16_wgrad  dw (N, ldw)[n][tap*C+ci] += sum_rows dout[row,n] img[row+shift(tap),ci]: nine shifted-row TN contractions in
 *                         one launch (rows shifted outside the image read as zeros)
 *   asr_conv_weight_fold  (Co,Ci,3,3) += (Co, ld)[tap*Ci+ci]
 *   asr_maxpool2x2_16_*   on bordered images; idx: one byte per element of the bordered output
 *                         out_f32 = 1: `out` is fp32 (no activation) - the pre-activations a CNNLayerNorm normalises next (rounded to bf16
 *                         first, their rounding error would be amplified by mean / std)
 *   asr_ln_freq16_*       CNNLayerNorm (LayerNorm over the F interior pixels, affine per f) + ReLU: x fp32 bordered in, y / dy / dx bf16
 *                         bordered; stats (B*(T+2)*C, 2); dconv_bias (C, may be NULL) += per-channel sum of dx in fp32 = the gradient of
 *                         the bias of the convolution in front (analytically zero)
 *   asr_vgg16_output[_bwd] P(T,F,C) <-> (B, T, C*F) bf16, the encoder layout (channel-major), and its adjoint */
int asr_vgg16_im2col(const float* feature, void* x1, int B, int T, int F, int Cin, int Kp, asr_stream_t stream);
int asr_conv_weight_pack16(const float* src, void* dst, int Co, int Ci, int Kp, int mode, asr_stream_t stream);
int asr_conv_weight_fold(const float* src, float* dst, int Co, int Ci, int ld, asr_stream_t stream);
int asr_conv3x3_16(const void* img, const void* w, void* out, const float* bias, int B, int T, int F, int C, int N, int K, int implicit,
                   int act, int out_f32, asr_stream_t stream);
int asr_conv3x3_16_wgrad(const void* img, const void* dout, float* dw, int B, int T, int F, int C, int N, int ldw, int splits,
                         asr_stream_t stream);
int asr_maxpool2x2_16_fwd(const void* x, void* y, unsigned char* idx, int B, int T, int F, int C, int T2, int F2, asr_stream_t stream);
int asr_maxpool2x2_16_bwd(const void* dy, const unsigned char* idx, void* dx, int B, int T, int F, int C, int T2, int F2, asr_stream_t stream);
int asr_ln_freq16_fwd(const float* x, const float* w, const float* b, void* y, float* stats, int B, int T, int F, int C, float eps, int relu,
                      asr_stream_t stream);
int asr_ln_freq16_bwd(const void* dy, const float* x, const float* w, const float* b, const float* stats, void* dx, float* dw, float* db,
                      float* dconv_bias, int B, int T, int F, int C, int relu, asr_stream_t stream);
int asr_vgg16_output(const void* img, void* out, int B, int T, int F, int C, asr_stream_t stream);
int asr_vgg16_output_bwd(const void* dout, void* g, int B, int T, int F, int C, asr_stream_t stream);
int asr_conv_weight_permute(const float* src, float* dst, int Co, int Ci, int mode, asr_stream_t stream);
int asr_maxpool2x2_fwd(const float* x, float* y, unsigned char* idx, int B, int T, int F, int C, int T2, int F2, asr_stream_t stream);
int asr_maxpool2x2_bwd(const float* dy, const unsigned char* idx, float* dx, int B, int T, int F, int C, int T2, int F2,
                       asr_stream_t stream);
int asr_ln_freq_fwd(const float* x, const float* w, const float* b, float* y, float* stats, long rows, int F, int C,
                    float eps, int relu, asr_stream_t stream);
int asr_ln_freq_bwd(const float* dy, const float* x, const float* w, const float* b, const float* stats,
                    float* dx, float* dw, float* db, long rows, int F, int C, int relu, asr_stream_t stream);
int asr_permute_last2(const float* in, float* out, long rows, int A, int Bd, asr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Model variants outside the shipped configs (csrc/variants.hip, composed step by step by src/variants.py
 * as the reference's own Python loop does, src/asr.py:131-170).  All fp32, all row-major.
 *   asr_masked_softmax_fwd/bwd : BaseAttention._attend (src/module.py:1110-1118): attn = softmax(energy / temperature) over
 *                                t < len[row / NH], exactly 0 beyond; rows = B * NH ordered b * NH + head (src/module.py:1107).
 *   asr_loc_energy_fwd/bwd     : LocationAwareAttention.forward (src/module.py:1176-1182) for any num_head:
 *                                energy[r,t] = gen_energy(tanh(key[r,t,:] + q[r,:] + tanh(loc_pre[r / NH,t,:]))); loc_pre (B,T,D) is the
 *                                loc_proj output BEFORE its tanh.  bwd: dkey += (same key at every decoder step), dq / dloc_pre written,
 *                                dwg / dbg += (parameter gradients).
 *   asr_loc_conv_fwd/bwd       : loc_conv = nn.Conv1d(NH, Kn, 2 Ks + 1, padding Ks, bias False) on prev_att (B,NH,T), output already
 *                                transposed to (B,T,Kn) (src/module.py:1176); bwd: dprev written (may be NULL), dW +=.
 *   asr_lstm_cell_fwd/bwd      : nn.LSTM cell on gx + gh (both (N,4D), biases inside; gate order i,f,g,o) with its backward
 *                                (decoder layers, src/asr.py:204,262); act (N,4D) = activated gates, dgates (N,4D) serves both halves.
 *   asr_gru_cell_fwd/bwd       : nn.GRU cell (decoder module GRU, src/asr.py:203-204): gi, gh (N,3D) gate order r,z,n; saved (N,4D) =
 *                                r | z | n | gh_n; bwd: dgi, dgh (N,3D) and the direct part of dh_prev (= dh * z).
 *   asr_gru_fwd/bwd            : nn.GRU(bidirectional, batch_first) time recurrence of an encoder layer (src/module.py:1023,1049; zero
 *                                initial state, padded frames processed like the reference does): gi (B,T,ND,3H) = x W_ih^T + b_ih,
 *                                whhT (ND,H,3H) = weight_hh transposed, bhh (ND,3H); y (B,T,ND*H); saved (B,T,ND,4H).
 *                                bwd: whh (ND,3H,H) as stored; dgi / dgh (B,T,ND,3H) from which the caller forms dW_ih, db_ih, dx and
 *                                dW_hh (shifted rows, asr_gemm seqT), db_hh.
 */
int asr_masked_softmax_fwd(const float* energy, const int64_t* len, int rows, int NH, int T, float temperature, float* attn, asr_stream_t stream);
int asr_masked_softmax_bwd(const float* attn, const float* dattn, int rows, int T, float temperature, float* denergy, asr_stream_t stream);
int asr_loc_energy_fwd(const float* key, const float* q, const float* loc_pre, const float* wg, const float* bg,
                       int B, int NH, int T, int D, float* energy, asr_stream_t stream);
int asr_loc_energy_bwd(const float* key, const float* q, const float* loc_pre, const float* wg, const float* denergy,
                       int B, int NH, int T, int D, float* dkey, float* dq, float* dloc_pre, float* dwg, float* dbg, asr_stream_t stream);
int asr_loc_conv_fwd(const float* prev_att, const float* W, int B, int NH, int T, int Kn, int Ks, float* out, asr_stream_t stream);
int asr_loc_conv_bwd(const float* dout, const float* prev_att, const float* W, int B, int NH, int T, int Kn, int Ks,
                     float* dprev, float* dW, asr_stream_t stream);
int asr_lstm_cell_fwd(const float* gx, const float* gh, const float* c_prev, int N, int D, float* act, float* h, float* c, asr_stream_t stream);
int asr_lstm_cell_bwd(const float* act, const float* c_prev, const float* c, const float* dh, const float* dc, int N, int D,
                      float* dgates, float* dc_prev, asr_stream_t stream);
int asr_gru_cell_fwd(const float* gi, const float* gh, const float* h_prev, int N, int D, float* saved, float* h, asr_stream_t stream);
int asr_gru_cell_bwd(const float* saved, const float* h_prev, const float* dh, int N, int D, float* dgi, float* dgh, float* dh_prev,
                     asr_stream_t stream);
int asr_gru_fwd(const float* gi, const float* whhT, const float* bhh, int B, int T, int H, int ND, float* y, float* saved, asr_stream_t stream);
int asr_gru_bwd(const float* dy, const float* y, const float* saved, const float* whh, int B, int T, int H, int ND,
                float* dgi, float* dgh, asr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Single-direction nn.GRU recurrence of the RNN language model (module 'GRU', reference src/lm.py:18; gate order r,z,n),
 * one launch per time step with MFMA in `prec` (bf16 operands / fp32 accumulate, or fp32).  Any 1 <= H <= 2048; a larger H
 * returns ASR_E_UNSUPPORTED.
 *   asr_gru_rec_fwd : gi (B,T,3H) = x W_ih^T + b_ih (asr_gemm); whh (3H,H) = weight_hh as stored; bhh (3H); h0 (B,H) the
 *                     initial state or NULL for zeros (must not alias y).  Writes y (B,T,H) and, unless NULL,
 *                     saved (B,T,4H) = r | z | n | gh_n (gh_n = (h_{t-1} W_hh^T + b_hh)_n, the layout of asr_gru_cell_fwd).
 *                     T = 1 with h0 = the previous state and saved = NULL is one decode step.
 *   asr_gru_rec_bwd : dy (B,T,H), y / saved / h0 as given to and written by the forward; whh (3H,H).  Writes dgi, dgh
 *                     (B,T,3H) (gradients wrt gi and gh = h_{t-1} W_hh^T + b_hh) and, unless NULL, dh0 (B,H).  The caller
 *                     forms dW_ih, db_ih, dx, dW_hh (asr_gemm with seqT / bshift) and db_hh from them.  workspace: 16-byte
 *                     aligned, asr_gru_rec_workspace_bytes(B, H) bytes (transposed W_hh and the carried gradient).
 */
size_t asr_gru_rec_workspace_bytes(int B, int H);
int asr_gru_rec_fwd(const float* gi, const float* whh, const float* bhh, const float* h0, int B, int T, int H, int prec,
                    float* y, float* saved, asr_stream_t stream);
int asr_gru_rec_bwd(const float* dy, const float* y, const float* saved, const float* h0, const float* whh, int B, int T, int H,
                    int prec, float* dgi, float* dgh, float* dh0, void* workspace, size_t workspace_bytes, asr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Beam-search inference (BeamDecoder.forward src/decode.py:65-183), batched over live hypotheses.
 *   asr_att_decoder_keys : key = tanh(proj_k(enc)) once per utterance (src/asr.py:345).
 *   asr_att_decoder_step : ONE decode step t for all dims->B rows of `state` (each row = one hypothesis at step t):
 *                          the caller sets state->tokens[:,t] and, for t>0, the step t-1 entries of hs/cs/att of
 *                          every row; outputs att/xin/gates/cs/hs/logits[:,t]   (src/decode.py:107-116).
 *   asr_ctc_prefix_init / asr_ctc_prefix_score : CTCPrefixScore.init_state / cheap_compute (src/ctc.py:19-27,68-107)
 *                          for N hypotheses x C candidates: logp (T,V); r_prev (N,T,2); candidates (N,C) int32;
 *                          prefix_len, last_token (N) int32; psi (N,C); r_out (N,C,T,2).  fp32, logzero = -1e8.
 *   asr_lstm_cell        : pointwise LSTM cell on gate pre-activations (N,4D) + both biases (RNNLM step, src/lm.py:27-37;
 *                          the projections are asr_gemm);  c_prev may be NULL (zero state).
 *   asr_gather_rows      : dst[r,:] = src[idx[r],:]  (embedding lookup, state re-ordering after pruning).
 *   asr_masked_copy_rows : dst[r,:] = src[r,:] for the rows with mask[r] != 0 (mask (rows) int32), the others untouched;
 *                          src_ld, dst_ld >= width.  The CTC-only search keeps the new LM rows of the extended slots with it.
 */
int asr_att_decoder_keys(const asr_dec_dims_t* dims, const asr_dec_weights_t* weights, const float* enc,
                         float* key, int prec, asr_stream_t stream);
int asr_att_decoder_step(const asr_dec_dims_t* dims, const asr_dec_weights_t* weights,
                         const float* enc, const int64_t* enc_len, const asr_dec_state_t* state, int t,
                         int prec, asr_stream_t stream);
int asr_ctc_prefix_init(const float* logp, float* r, int T, int V, asr_stream_t stream);
int asr_ctc_prefix_score(const float* logp, const float* r_prev, const int* candidates, const int* prefix_len,
                         const int* last_token, float* psi, float* r_out, int N, int C, int T, int V,
                         asr_stream_t stream);
int asr_lstm_cell(const float* gates_pre, const float* bias_ih, const float* bias_hh, const float* c_prev,
                  float* h, float* c, int N, int D, asr_stream_t stream);
int asr_gather_rows(const float* src, const int64_t* idx, float* dst, int rows, int width, long src_ld, long dst_ld,
                    int nsrc, asr_stream_t stream);
int asr_masked_copy_rows(const float* src, const int* mask, float* dst, int rows, int width, long src_ld, long dst_ld,
                         asr_stream_t stream);

/* Device-side beam bookkeeping: one output position of BeamDecoder.forward (src/decode.py:104-177) for U utterances x
 * `beam` hypothesis rows (row = u*beam + i) with NO device-to-host copy.
 *   asr_beam_candidates : candidates (rows,C) = att_logp.topk(C) per row (the CTC scorer's candidates, :129), descending.
 *   asr_ctc_prefix_{init,score}_batched : the prefix scorer over a batch: row n belongs to utterance n / rows_per_utt with
 *       log-probs logp[utt] (Tmax,V) and tlen[utt] valid frames; r (rows,Tmax,2), r_out (N,C,Tmax,2).
 *   asr_beam_step : score fusion (1-w)*att + w*(psi - ctc_prob) on the candidates / LOG_ZERO elsewhere, blank excluded
 *       (:131-141), + lm_weight*lm (:152); per live hypothesis top-`beam` and the <eos> rule of Hypothesis.addTopk
 *       (att[eos] > eos_threshold * max(att[2:]) ends it with that score, :235-242); children pruned to the `beam` best by
 *       average token score in stable order (:175-177); finished hypotheses kept as the `beam` best per utterance, sorted
 *       (:179-183, incl. the survivors when t+1 reaches max_len[u], and the beam-1 early return).  State is double
 *       buffered (in -> out); outputs for the next step: last_token (rows), parent (rows: source row of each new row),
 *       ctc_index (rows: parent*C + candidate slot, row index into r_out viewed (N*C, Tmax*2)), and column t+1 of the
 *       decoder's token table.  beam <= 16, V <= 2048, one wave per utterance.  Every pointer but lm_logp, psi and
 *       candidates is required (ctcp_in / ctcp_out too without CTC: they are read and written as 0); psi and candidates come
 *       together; anything else returns ASR_E_ARG and launches nothing. */
typedef struct {
    const float *att_logp, *lm_logp, *psi;  /* (R,V); (R,V) or NULL; (R,C) or NULL */
    const int* candidates;                  /* (R,C) or NULL */
    const int* alive_in; const float* sum_in; const float* ctcp_in; const int* len_in; const int* seq_in; const float* score_in;
    int* alive_out; float* sum_out; float* ctcp_out; int* len_out; int* seq_out; float* score_out;   /* seq/score: (R,Lmax) */
    int* last_token; int64_t* parent; int64_t* ctc_index;
    int64_t* tokens; long tokens_ld;        /* decoder token table (R, tokens_ld) */
    const int *min_len, *max_len; int* done;                   /* (U) */
    int* fin_n; int* fin_len; float* fin_avg; int* fin_seq; float* fin_score;   /* (U), (U,beam), (U,beam), (U,beam,Lmax+1) x2 */
    int U, beam, V, C, Lmax, t;
    float ctc_weight, lm_weight, eos_threshold;
} asr_beam_step_t;
/* Scheduled sampling (src/asr.py:151-158): out[row*out_ld] ~ Categorical(softmax(logits[row*ld : row*ld+V])), one Philox
 * uniform per (seed, row). */
int asr_sample_tokens(const float* logits, long ld, int64_t* out, long out_ld, int rows, int V, uint64_t seed, asr_stream_t stream);
int asr_beam_candidates(const float* att_logp, int* candidates, int rows, int V, int C, asr_stream_t stream);
int asr_beam_step(const asr_beam_step_t* args, asr_stream_t stream);
/* The same two steps for word and subword vocabularies, 2 <= V <= 65536 (csrc/beam_step.hip, "wide"): a multi-wave workgroup owns
 * a row and strides over V.
 *   asr_beam_candidates_wide : att_logp.topk(C) per row (src/decode.py:129), 1 <= C <= min(V, 32), in asr_beam_candidates' order
 *       (descending, the lower token first among equals, token 0 where fewer than C entries are above -inf).
 *   asr_beam_step_wide : asr_beam_step's argument block and rules (src/decode.py:131-183, Hypothesis.addTopk :214-263), the
 *       fused score in the same fp32 operation order.  Phase A reduces every live row to its `beam` best (token, score) pairs,
 *       att[<eos>] and max(att[2:]) in `workspace` (asr_beam_step_wide_workspace_bytes(U, beam) bytes, contents need not
 *       survive between calls); phase B, one wave per utterance, is asr_beam_step behind its picks.  beam <= 16, C <= 32.
 * V > 65536 returns ASR_E_UNSUPPORTED; null pointers, other bad dims, psi without candidates and a workspace that is too
 * small return ASR_E_ARG; nothing is launched then. */
int asr_beam_candidates_wide(const float* att_logp, int* candidates, int rows, int V, int C, asr_stream_t stream);
size_t asr_beam_step_wide_workspace_bytes(int U, int beam);
int asr_beam_step_wide(const asr_beam_step_t* args, void* workspace, size_t workspace_bytes, asr_stream_t stream);
int asr_ctc_prefix_init_batched(const float* logp, const int* tlen, float* r, int rows, int rows_per_utt, int Tmax, int V,
                                asr_stream_t stream);
int asr_ctc_prefix_score_batched(const float* logp, const int* tlen, const float* r_prev, const int* candidates,
                                 const int* prefix_len, const int* last_token, float* psi, float* r_out,
                                 int N, int C, int Tmax, int V, int rows_per_utt, asr_stream_t stream);

/* CTC prefix beam search of a CTC-only model (csrc/ctc_decode.hip): the decoder the reference does not have (`# ToDo :
 * implement pure ctc decode`, src/decode.py:26), behind the BeamDecoder.forward contract (src/decode.py:65-183: at most `beam`
 * hypotheses per utterance, best first).  ONE launch for all U utterances and all their frames, one workgroup per utterance,
 * the beam in LDS; blank = 0.  logp (U,Tmax,V) fp32 log-probabilities (the CTC head's output), tlen (U) valid frames: frames at
 * and past tlen[u] are never read.  Per frame every beam prefix stays (blank / repeated last token) and is extended by every
 * allowed non-blank token; an extension that is a beam member itself accumulates into that member; the K entries with the
 * largest logaddexp(p_blank, p_nonblank) survive, ties to the smaller (parent slot, token), entries at -inf never.  cand = 0:
 * every non-blank token extends; cand > 0: the `cand` tokens with the largest logp of the frame (ties: lower index).
 * Outputs per utterance, best first: out_tokens (U,K,Lcap) collapsed token ids (0 behind the end), out_len (U,K),
 * out_score (U,K) = log-probability of the token sequence under the pruned search (-inf in unused rows), out_n (U) = number of
 * hypotheses (tlen[u] = 0: the empty one, score 0).  Lcap >= Tmax.  workspace: asr_ctc_beam_search_workspace_bytes(U,Tmax,K)
 * (the prefix trie, 1 + K*Tmax nodes per utterance; need not be cleared).  Any V > 1, any Tmax > 0,
 * 1 <= K <= ASR_CTC_BEAM_MAX; anything else returns ASR_E_ARG and launches nothing.  No language-model fusion: that is the
 * resumable search below. */
#define ASR_CTC_BEAM_MAX 16
size_t asr_ctc_beam_search_workspace_bytes(int U, int Tmax, int K);
int asr_ctc_beam_search(const float* logp, const int* tlen, int U, int Tmax, int V, int K, int cand, int Lcap,
                        int* out_tokens, int* out_len, float* out_score, int* out_n,
                        void* workspace, size_t workspace_bytes, asr_stream_t stream);

/* The same search with RNN-LM shallow fusion, resumable (csrc/ctc_decode.hip; the frame body is the one of asr_ctc_beam_search).
 * A prefix l_1..l_n is ranked, at every frame and in the result, by
 *   log P_ctc(l | frames so far) + lm_weight * sum_j log P_lm(l_j | <sos>, l_1..l_{j-1}) + len_bonus * n
 * where log P_ctc = logaddexp(p_blank, p_nonblank) stays pure CTC and the LM part is one additive value per beam entry: a stay
 * inherits it, the extension of slot i by c gets lms_i + lm_weight * lm_logp[row_i, c] + len_bonus, an extension that is a beam
 * member keeps the member's value.  The allowed tokens stay the `cand` largest CTC log-probs of the frame; ties, the never-keep
 * -inf rule and the slot order are those of asr_ctc_beam_search; with lm_weight = len_bonus = 0 and a finite table the result
 * equals it bit for bit.  A new prefix needs an LM step (GEMMs) before it can be extended, so the beam and the trie live in the
 * workspace between launches (asr_ctc_beam_lm_workspace_bytes; need not be cleared, _init fills what is read):
 *   _init    : every utterance at the empty prefix, score 0.
 *   _advance : per utterance, loads the beam and runs frames until the first frame whose survivors include an extension
 *              (c != 0: some slot needs a new LM row), the utterance's last frame, or max_frames frames (max_frames > 0); at
 *              least one frame of every unfinished utterance.  lm_logp (U*K,V): row u*K + r = the LM's log-probs after the
 *              prefix of slot r.  Writes per slot src_row (U*K) int64 = the global row the slot inherits its LM state and
 *              distribution from (stays permute the slots by rank; identity for dead slots and finished utterances), step_tok
 *              (U*K) int64 = the slot's last token, need (U*K) int32 = 1 where the slot is an extension: the caller gathers
 *              state and table rows by src_row, steps the LM with step_tok and keeps the stepped rows where need.  Per
 *              utterance frame (U) = frames consumed so far, done (U) = 1 once all tlen[u] frames are.  A finished utterance
 *              is a no-op.
 *   _readout : out_tokens / out_len / out_n as asr_ctc_beam_search (same layout and padding), out_score (U,K) the fused score,
 *              out_ctc_score (U,K) its CTC part; -inf in unused rows.  May be called after any launch.
 * Null pointers, bad dims, K outside 1..ASR_CTC_BEAM_MAX and a short workspace return ASR_E_ARG and launch nothing. */
size_t asr_ctc_beam_lm_workspace_bytes(int U, int Tmax, int K);
int asr_ctc_beam_lm_init(int U, int Tmax, int K, void* workspace, size_t workspace_bytes, asr_stream_t stream);
int asr_ctc_beam_lm_advance(const float* logp, const int* tlen, const float* lm_logp, int U, int Tmax, int V, int K, int cand,
                            float lm_weight, float len_bonus, int max_frames, int64_t* src_row, int64_t* step_tok, int* need,
                            int* frame, int* done, void* workspace, size_t workspace_bytes, asr_stream_t stream);
int asr_ctc_beam_lm_readout(int U, int Tmax, int K, int Lcap, int* out_tokens, int* out_len, float* out_score,
                            float* out_ctc_score, int* out_n, const void* workspace, size_t workspace_bytes, asr_stream_t stream);

/* Two-pass decoding of a joint model (csrc/rescore.hip): the n-best list of the CTC prefix beam search above, scored by the
 * attention decoder teacher-forced in one batched pass and re-ranked.  No reference counterpart (the reference has the joint
 * search of src/decode.py:65-183 only).  Row r = u*K + i is beam slot i of utterance u.
 *   asr_rescore_pack  : the first pass's result -> the decoder's teacher table.  tokens (U,K,Lcap), len (U,K), n (U) int32 as
 *     asr_ctc_beam_search / asr_ctc_beam_lm_readout write them; enc_len (U) int64.  teacher (R,Lr) int64 = the hypothesis, `eos`
 *     appended when its last token is not `eos` already, zero-padded to Lr; tgt_len (R) int32 = the tokens to score (an empty
 *     hypothesis scores the one `eos`); row_utt (R) int64 = u (the index asr_gather_rows expands the encoder output with);
 *     row_enc_len (R) int64 = enc_len[u]; max_len (1) int32 = the largest tgt_len.  A slot i >= n[u] is unused: tgt_len 0, an
 *     all-zero teacher row, row_utt and row_enc_len as its utterance's (a valid row to read).  len is clamped to 0..Lcap.
 *     Lr >= Lcap + 1 (so no tgt_len exceeds Lr); one workgroup per utterance, every one finds max_len for itself from len and n.
 *   asr_rescore_nbest : logits fp32, element (r,t,v) at r*row_stride + t*pos_stride + v, both strides >= V (R,L,V of the decoder
 *     pass); teacher (R,teacher_ld) int64, tgt_len (R) int32 (clamped to 0..L); ctc_score, first_score (U,K) fp32 = the pure CTC
 *     log-probability and what the first pass ranked by (equal without an LM); n (U) int32.  Writes, all (U,K):
 *       att_score = sum_{t < tgt_len} log_softmax(logits[r,t,:])[teacher[r,t]]      (fp32, max subtracted, added in order of t)
 *       total     = (1 - ctc_weight) * att_score + ctc_weight * ctc_score + (first_score - ctc_score)
 *       order     int32, rank -> slot: descending total, ties to the lower slot; unused slots last, their att_score = total = -inf.
 *     A -inf logit is legal: a target at -inf (or outside 0..V-1) gives att_score = total = -inf, never NaN.  Nothing at or past
 *     tgt_len along L or past V along a row is read.  One workgroup per utterance, one wave per slot; the result does not depend
 *     on U, K or the launch shape.  Any V > 1, L >= 1, 1 <= K <= ASR_CTC_BEAM_MAX.
 * Null pointers, bad dims, K outside 1..ASR_CTC_BEAM_MAX, Lr < Lcap + 1 and a stride below V return ASR_E_ARG and launch nothing. */
int asr_rescore_pack(const int* tokens, const int* len, const int* n, const int64_t* enc_len, int U, int K, int Lcap, int Lr,
                     int eos, int64_t* teacher, int* tgt_len, int64_t* row_utt, int64_t* row_enc_len, int* max_len,
                     asr_stream_t stream);
int asr_rescore_nbest(const float* logits, long row_stride, long pos_stride, const int64_t* teacher, long teacher_ld,
                      const int* tgt_len, const float* ctc_score, const float* first_score, const int* n, int U, int K, int L,
                      int V, float ctc_weight, float* att_score, float* total, int* order, asr_stream_t stream);

/* The RNN-LM in the second pass (csrc/rescore.hip): the LM scores the same n-best list teacher-forced, so the first pass runs
 * without it.  Between asr_rescore_lm_input and asr_rescore_token_logp the caller runs the LM's full-sequence forward,
 * lm_in (R,L) -> logits (R,L,V), over chunks of rows if it likes.  For beam slot i of utterance u with the hypothesis l_1..l_n,
 * n = len[u,i] (the <eos> that asr_rescore_pack appends is not counted):
 *     lm_score = sum_{j=1..n} log_softmax(LM(sos, l_1..l_{j-1}))[l_j]                      (0 for the empty hypothesis)
 *     total    = (1 - ctc_weight) * att_score + ctc_weight * ctc_score + lm_weight * lm_score + len_bonus * n
 *   asr_rescore_lm_input  : lm_in (R,L) int64 contiguous from teacher (R,teacher_ld) int64, teacher_ld >= L:
 *     lm_in[r,0] = sos, lm_in[r,t] = teacher[r,t-1] for 1 <= t < L.  Every value written is `sos` or a value of the teacher table
 *     (token ids; its padding and its unused rows are 0), so an embedding gather over lm_in reads valid rows only.  sos >= 0.
 *   asr_rescore_token_logp: logits fp32, element (r,t,v) at r*row_stride + t*pos_stride + v, both strides >= V; target
 *     (R,target_ld) int64 = the teacher table as asr_rescore_pack wrote it, not shifted; len (R) int32 = the first pass's len
 *     (U,K) as it stands (0 in its unused slots), clamped here to 0..L.  out (R,out_ld) fp32, out_ld >= L:
 *       out[r,t] = log_softmax(logits[r,t,:])[target[r,t]]   for t < min(max(len[r],0), L)     (fp32, the max subtracted)
 *       out[r,t] = 0                                          for the other t < L
 *     A -inf logit is legal: a target at -inf or outside 0..V-1 gives -inf, a position whose every logit is -inf gives -inf, never
 *     NaN.  Nothing is read at or past len[r] along L, past V along a row or from the padding between strides; nothing is
 *     written past column L of out.  One wave per (r,t), four per workgroup, the grid covers R*L: the bound is one read of the
 *     logit block, and no logit is loaded twice: the wave takes the row in blocks of 1024 columns held in registers, max and
 *     then sum of each block, and carries the max m so far and the sum of exp(x - m) across blocks (a block with a larger max
 *     scales the sum by exp(m - max) first; up to 1024 columns that is max, then sum, with no scaling).  Lane c adds the columns
 *     c, c+64, .. in order: a value does not depend on R, on the chunk of rows a launch covers or on the launch shape.  V <= 2^30.
 *   asr_rescore_rank_lm   : att_score, ctc_score (U,K) fp32 (att_score from asr_rescore_nbest, whose own total and order are not
 *     used then); tok_logp (R,tok_ld) fp32 = out above, tok_ld >= L; len (U,K) int32, clamped to 0..L; n (U) int32.  Writes, (U,K):
 *       lm_score = sum_{t < len} tok_logp[r,t]   (fp32; lane c of the slot's wave adds positions c, c+64, .. in order, then one
 *                  butterfly over the lanes: one fixed order whatever U, K and the grid are)
 *       total    as defined above, in this order: (1-w)*att + w*ctc, + lm_weight*lm_score (left out when lm_weight == 0), + len_bonus*len
 *       order    int32, rank -> slot, the rule of asr_rescore_nbest: a count over the K totals in LDS, ties to the lower slot.
 *     att_score, ctc_score or (with lm_weight > 0) lm_score at -inf give total = -inf, never NaN; unused slots (i >= n[u]) get
 *     lm_score = total = -inf and rank last.  One workgroup per utterance, one wave per slot.  lm_weight >= 0.
 * Null pointers, bad dims, K outside 1..ASR_CTC_BEAM_MAX, a stride below V or a leading dimension below L return ASR_E_ARG and
 * launch nothing. */
int asr_rescore_lm_input(const int64_t* teacher, long teacher_ld, int R, int L, int64_t sos, int64_t* lm_in, asr_stream_t stream);
int asr_rescore_token_logp(const float* logits, long row_stride, long pos_stride, const int64_t* target, long target_ld,
                           const int* len, int R, int L, int V, float* out, long out_ld, asr_stream_t stream);
int asr_rescore_rank_lm(const float* att_score, const float* ctc_score, const float* tok_logp, long tok_ld, const int* len,
                        const int* n, int U, int K, int L, float ctc_weight, float lm_weight, float len_bonus, float* lm_score,
                        float* total, int* order, asr_stream_t stream);

/* CTC forced alignment (csrc/ctc_align.hip): the most probable alignment (Viterbi) of a KNOWN transcript to the CTC
 * log-probabilities - token and word timestamps, cutting long recordings, finding bad transcripts by their score.  No reference
 * counterpart.  ONE launch for all B utterances, one workgroup per utterance, one thread per lattice state; nothing is copied
 * to the host.  logp (B,T,V) fp32 log-probabilities, batch-major like asr_ctc_loss (the `ctc_output` of ASR.forward); targets
 * (B,L) padded; input_len, target_len (B), clamped to 0..T and 0..L: frames at and past input_len[b] and targets at and past
 * target_len[b] are never read.  Lattice of the loss, l' = (0, y1, 0, ..., yL, 0), S = 2L+1 states, blank = 0:
 *   d[t][s] = logp[t][l'_s] + max(d[t-1][s], d[t-1][s-1], d[t-1][s-2])     (s-2 only when l'_s != 0 and l'_s != l'_{s-2})
 * from d[0][0] and d[0][1], ending at the better of d[Tb-1][S-1] and d[Tb-1][S-2]; all fp32.
 * Tie rules (deterministic): among predecessors a tie goes to the smaller move - stay, then s-1, then s-2; at the end a tie
 * goes to S-1; -inf never wins over a finite value.  A row whose end value is -inf (too few frames for the target, or every
 * alignment runs through a -inf entry), a row with a target token outside 1..V-1, and a row with no frames and a non-empty
 * target have no alignment: ok = 0.  A row with no frames and an empty target is aligned (ok = 1, score 0).
 * Outputs, all fully written by the call:
 *   frame_token (B,T) token emitted at frame t, 0 = blank; -1 for t >= input_len[b] and in rows that are not ok
 *   frame_pos   (B,T) index into the target of that token; -1 where frame_token <= 0
 *   tok_start, tok_end (B,L) first / last frame of target token j, inclusive; -1 for j >= target_len[b] and in rows not ok
 *   tok_score   (B,L) sum of logp[t, y_j] over the frames of token j, added in frame order; 0 where tok_start is -1
 *   score       (B)   log-probability of the best alignment; -inf when not ok
 *   ok          (B)   1 aligned, 0 no alignment exists
 * L = 0 is legal (every frame blank; targets and the three tok_* pointers may then be NULL).  workspace:
 * asr_ctc_align_workspace_bytes(B,T,L) bytes, 4-byte aligned, need not be cleared (the moves: 2 bits per frame and state).
 * A null pointer, B, T <= 0, V <= 1, L < 0 or a too-small workspace return ASR_E_ARG, 2L+1 > 1024 states (the limit of
 * asr_ctc_loss) returns ASR_E_UNSUPPORTED; either way nothing is launched and no output is touched. */
size_t asr_ctc_align_workspace_bytes(int B, int T, int L);
int asr_ctc_align(const float* logp, const int64_t* targets, const int64_t* input_len, const int64_t* target_len,
                  int B, int T, int V, int L, int* frame_token, int* frame_pos, int* tok_start, int* tok_end,
                  float* tok_score, float* score, int* ok, void* workspace, size_t workspace_bytes, asr_stream_t stream);

/* Beam-search attention of the model variants (csrc/decode_variants.hip; src/decode_variants.py): one output position of
 * BeamDecoder.forward's attention (src/decode.py:107-110 -> src/asr.py:331-364, ScaleDotAttention / LocationAwareAttention
 * src/module.py:1121-1189) for U utterances x rows_per_utt hypothesis rows (row r belongs to utterance u = r / rows_per_utt),
 * forward only.  Keys and values are held once per utterance, not per row.  Per row r and head n:
 *   dot: e[t] = q[r,n,:] . key[u,n,t,:]
 *   loc: e[t] = wg . tanh(key[u,n,t,:] + q[r,n,:] + loc[r,t,:]) + bg[0]     (loc = tanh(loc_proj(loc_conv(prev_att))), shared by heads)
 *   attn[r, n*Tp + t] = softmax_t(e / temperature) over t < enc_len[u], exactly 0 for t >= enc_len[u] (row stride attn_ld);
 *   ctx[r*ctx_ld + n*Dv + c] = sum_t attn[r,n,t] value[u, NHv == 1 ? 0 : n, t, c].
 * key (U,NH,Tp,ld_k) and value (U,NHv,Tp,ld_v) are fp32 or, kv_bf16 = 1, bf16; q (R,NH,A), loc (R,Tp,ld_l), wg (A), bg (1),
 * attn and ctx are fp32.  Contiguous row strides that are a multiple of 16 bytes get 16-byte loads.  rows_per_utt <=
 * ASR_BEAM_ATTEND_MAX_ROWS and Tp <= ASR_BEAM_ATTEND_MAX_T, else ASR_E_UNSUPPORTED.  The energies stay in LDS while
 * rows_per_utt * Tp <= asr_beam_attend_resident_max_t(1) and are staged in the attn rows above that.  No reference
 * counterpart as one call: the reference runs its attention once per hypothesis. */
#define ASR_ATT_DOT 0
#define ASR_ATT_LOC 1
#define ASR_BEAM_ATTEND_MAX_ROWS 16
#define ASR_BEAM_ATTEND_MAX_T 8192
typedef struct {
    const void* key; const void* value;     /* (U,NH,Tp,ld_k), (U,NHv,Tp,ld_v): fp32 or bf16 (kv_bf16) */
    const float* q;                         /* (R,NH,A) */
    const float* loc;                       /* (R,Tp,ld_l) or NULL (dot) */
    const float* wg; const float* bg;       /* (A), (1) or NULL (dot) */
    const int64_t* enc_len;                 /* (U) */
    float* attn; long attn_ld;              /* (R, attn_ld >= NH*Tp) */
    float* ctx; long ctx_ld;                /* (R, ctx_ld >= NH*Dv) */
    long ld_k, ld_v, ld_l;
    int U, rows_per_utt, NH, NHv, Tp, A, Dv, mode, kv_bf16;
    float temperature;
} asr_beam_attend_t;
int asr_beam_attend(const asr_beam_attend_t* args, asr_stream_t stream);
/* largest Tp whose energies stay in LDS for `rows_per_utt` rows */
int asr_beam_attend_resident_max_t(int rows_per_utt);

/* Test support: keeps `workgroups` compute units busy (one 64-thread workgroup each holding `lds_bytes` of LDS) for
 * `seconds` (<= 20) on `stream`; tests/test_persist_abort.py uses it to starve a persistent launch of co-residency. */
int asr_debug_occupy(int workgroups, int lds_bytes, double seconds, asr_stream_t stream);

/* ---- CU-masked streams --------------------------------------------------------------------------------------------
 * The persistent recurrences keep 40 of the 256 CUs busy; the parameter-gradient contractions of the layer above are off
 * the critical path and can run beside them - but only if they never land on the recurrence's CUs (a shared CU stretches
 * every hand-off of the chain).  asr_stream_create_cu_mask creates a HIP stream restricted to `count` compute units PER XCD
 * starting at per-XCD unit `first` (0..31).  Mask layout measured on MI355X (tools/probe/cumask.hip): mask bit i = XCD i % 8,
 * unit i / 8 of that XCD (shader engine (i / 8) % 4); a mask that leaves an XCD empty is ignored by the driver.
 * (No reference counterpart: the reference trains on one CUDA stream.) */
/* Zero a hand-off work area from EVERY XCD with L2-local stores (whenever an area of the caller's hand-off pool changes hands):
 * see csrc/core.hip.  `tickets`: 64 bytes of device memory private to the calling stream (per-XCD chunk counters, cleared
 * by the call; word 15 is set when an XCD received no workgroup - register it like an abort word).  Placement-independent:
 * workgroups draw chunks from the counter of the XCD they find themselves on.  No reference counterpart. */
int asr_scrub_workspace(void* ptr, size_t bytes, void* tickets, asr_stream_t stream);
int asr_stream_create_cu_mask(int first, int count, asr_stream_t* stream);
int asr_stream_destroy(asr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ASR_HIP_H */
