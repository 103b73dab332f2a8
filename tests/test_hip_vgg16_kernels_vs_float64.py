"""The eleven entry points of the bf16 bordered VGG front-end (csrc/vgg16.hip; the CONV instantiation of gemm16_nt_kernel and
the nine-tap mode of gemm16_tn_kernel in csrc/gemm16.hip), each called through the C ABI and held to the float64 restatements
of tests/test_vgg16_kernels_reference.py, which also owns the case tables and the input recipes.

Conditions on every case: fully written outputs start as NaN (bf16 / fp32) or 0xAB bytes (pooling indices), accumulated outputs
(dw of the weight gradient, .grad of the fold, dw / db / dconv_bias of LayerNorm) start from random values and must equal
init + contribution, every output buffer carries a 64-element sentinel tail, and border pixels of every image output must be
exactly zero although the buffer was prefilled.

Contractions (asr_conv3x3_16 implicit and explicit, asr_conv3x3_16_wgrad) - nothing is measured, both rules are arithmetic:
  integer recipe  every partial sum is an integer below 2^24: the fp32 result equals float64 EXACTLY, the bf16 result equals
                  bf16(reference) bit for bit.
  random recipe   fp32: |err| <= n 2^-23 sum|terms| per element (n = 9C + 1 terms of a convolution with its bias, R + 1 for the
                  weight gradient over R pixel rows and its starting value; any order, atomics included);
                  bf16: |err| <= 2^-8 |ref| + 1.01 x that bound (one rounding of a value that far from the reference).
  The input gradient is the same kernel on the mode-1 packing of asr_conv_weight_pack16, against the autograd input gradient.
  asr_conv3x3_16_wgrad CONTRACT: `img` and `dout` both have zero borders - a shifted row that leaves the image lands on a border
  pixel of one of the two, which is how the nine row shifts need no bounds test.
asr_vgg16_im2col, asr_conv_weight_pack16, asr_conv_weight_fold, pooling forward (values and index bytes) and backward,
asr_vgg16_output[_bwd]: bit for bit.

LayerNorm over frequency (asr_ln_freq16_fwd / _bwd) follows tests/test_hip_glue_kernels_vs_float64.py: each case measures
e32 = max |the same formula in torch float32 on the CPU - float64| on ITS inputs and bounds the kernel by
K_LN * e32 + 4 * 2^-23 * scale, scale = max(1, max |reference|); bf16 outputs (y, dx) add 2^-8 |ref|; the sums dw / db add
n 2^-24 sum|terms| (n = B T C terms per f, plus the start value); dconv_bias is analytically zero and is judged against
n 2^-24 sum|terms| alone, its terms being the three addends rstd (g w), rstd s1, rstd xh s2 of every dx it sums (n = 3 B T F + 1).
An element whose float64 pre-activation lies within 1e-5 * scale of zero may gate either way: it is left out (at most 0.1 % of a
case, asserted on the CPU by the reference module), and what its gate can change in dx of its row and in dw / db of its f is
added to their bounds.  The backward reads the float64 statistics rounded to fp32, so it does not depend on the forward.
The borders of the fp32 input hold 1e30: one read of them would show in every statistic.

K_LN is the smallest power of two that clears the worst measured ratio by 2x over the cases whose e32 exceeds one ulp of scale,
capped at 4.  Measured on the MI355X (worst err_kernel / e32 per output over the 24 case x relu combinations):
  output   runs  above   worst ratio at                       | incl. runs below one ulp
  y          12     10    0.22  B8 T127 F2 C512 relu1          |  0.22
  mean       12      4    1.97  B2 T4 F40 C64                  |  2.06  B1 T2 F128 C8
  rstd       12      0     -                                   |  2.39  B1 T2 F128 C8
  dx         24     10    0.53  B8 T127 F2 C512 relu0          |  0.53                      (was infinite at B1 T1 F1 C8, see below)
  dw         24     18    0.00  (inside n 2^-24 sum|terms|)    |  0.00
  db         24      4    0.00  (inside n 2^-24 sum|terms|)    |  0.00
  dconv_bias 12           largest err / bound 0.0051 (B2 T3 F5 C6 relu0)
"above" counts the runs whose e32 exceeds one ulp of scale; the ratios are taken after the derived allowances (bf16 rounding, sum
bound, gate slack) have been subtracted from the error.  The kernel sums the F values of a row one after the other where torch sums
pairwise, which is the 1.97 on the mean at F = 40; 2 x 1.97 <= 4  ->  K_LN = 4.
The contraction bounds are arithmetic, not measured; for the record the largest err / bound seen was 0.07 for fp32 outputs and 0.995 for
bf16 ones (2^-8 |ref| is the half-ulp of a bf16 value just above a power of two, so that rule is tight by construction).

One finding of this module, fixed in csrc/vgg16.hip.  asr_ln_freq16_bwd summed s1 = sum_f round(g w) in its first loop and evaluated
rstd (g w - s1 / F - xh s2) in the second, where the compiler fused g w into the subtraction: the unrounded product minus the rounded
one.  At F = 1 the gradient is exactly zero (torch float32 gives 0, so e32 = 0), rstd = 1 / sqrt(eps) = 316, and the kernel returned
dx = 1.86e-05 (B1 T1 F1 C8 relu0: err 1.860e-05 against a bound of 4.8e-07).  The product is now rounded on its own in both loops
(a multiply under `#pragma clang fp contract(off)`; __fmul_rn is a plain contractable product in HIP): err 0 on that case, every
other ratio unchanged.
"""
import math

import pytest
import torch

import test_vgg16_kernels_reference as R
from test_vgg16_kernels_reference import ACT_NONE, ACT_RELU, F32, F64, bf16, border, border_is_zero, interior

gpu = pytest.mark.gpu

ULP32 = 2.0 ** -23
FLOOR = 4 * ULP32
U24 = 2.0 ** -24
K_LN = 4
TAIL = 64
SENT = -776.0                       # a bf16 value
E_ARG, E_UNSUPPORTED = -1, -3
BF = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------------
def _dev16(x):
    """float64 / float32 tensor of bf16 values -> contiguous bf16 device tensor (exact)."""
    y = x.to(F32).to(BF)
    assert torch.equal(y.to(F64), x.to(F64)), 'input is not a bf16 value'
    return y.contiguous().cuda()


def _out(shape, dtype=F32, init=None):
    """Device buffer for an output of `shape`: NaN (the kernel must write all of it) or `init` (it accumulates), followed by TAIL
    sentinel elements.  uint8 buffers start as 0xAB with a 0xCD tail."""
    n = math.prod(shape)
    if dtype == torch.uint8:
        t = torch.full((n + TAIL,), 0xCD, dtype=torch.uint8)
        t[:n] = 0xAB
        return t.cuda()
    t = torch.full((n + TAIL,), SENT, dtype=dtype)
    t[:n] = float('nan') if init is None else init.reshape(-1).to(dtype)
    return t.cuda()


def _back(buf, shape):
    """-> the output as float64 (int64 for index bytes), after checking the sentinel tail.  NaN left anywhere fails."""
    n = math.prod(shape)
    c = buf.cpu()
    if c.dtype == torch.uint8:
        assert bool((c[n:] == 0xCD).all()), 'the sentinel tail behind the output was overwritten'
        return c[:n].view(shape).to(torch.int64)
    assert bool((c[n:].to(F64) == SENT).all()), 'the sentinel tail behind the output was overwritten'
    got = c[:n].view(shape).to(F64)
    assert not bool(torch.isnan(got).any()), 'NaN left in an output the kernel must write'
    return got


def _bits(x64):
    """bf16 bit patterns of float64 values that are bf16 values."""
    return x64.to(F32).to(BF).view(torch.int16)


def _same_bits16(got64, want64):
    return torch.equal(_bits(got64), _bits(want64))


def _H():
    from src import hipabi as H
    return H


def _rc(name, *args):
    """The raw return code (H.call raises on anything but 0)."""
    H = _H()
    return getattr(H.lib(), name)(*args)


def _off(t, nbytes):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + nbytes)


# ---------------------------------------------------------------------------------------------------------------------
# convolution
# ---------------------------------------------------------------------------------------------------------------------
def _conv_call(img, w16, bias, B, T, Fq, C, N, K, implicit, act, out_f32):
    H = _H()
    shape = (B, T + 2, Fq + 2, N)
    out = _out(shape, F32 if out_f32 else BF)
    H.call('asr_conv3x3_16', H.ptr(img), H.ptr(w16), H.ptr(out), H.ptr(bias), B, T, Fq, C, N, K, implicit, act, out_f32, H.stream_ptr())
    torch.cuda.synchronize()
    return _back(out, shape)


def _judge_contraction(name, what, got, ref, abs_terms, n, recipe, is_bf16, image=True):
    """The two rules of the module docstring; `image`: the output is a bordered image whose border must be exactly zero."""
    if image:
        assert border_is_zero(got), '%s %s: a border pixel is not zero' % (name, what)
    err = (got - ref).abs()
    if recipe == 'integer':
        want = bf16(ref) if is_bf16 else ref
        bad = int((got != want).sum())
        print('EXACT %-44s %-10s wrong elements %d of %d, largest |err| %.3e' % (name, what, bad, got.numel(), float((got - want).abs().max())))
        assert bad == 0, (name, what, bad)
        if is_bf16:
            assert _same_bits16(got, want), (name, what, 'bit patterns differ (a signed zero)')
        return
    bound = n * ULP32 * abs_terms
    if is_bf16:
        bound = 2.0 ** -8 * ref.abs() + 1.01 * bound
    ratio = float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0
    print('RATIO %-44s %-10s err %.3e worst err / bound %.4f (n = %d)' % (name, what, float(err.max()), ratio, n))
    assert bool((err <= bound).all()), (name, what, float(err.max()), ratio)


@gpu
@pytest.mark.parametrize('recipe', R.RECIPES)
@pytest.mark.parametrize('case', R.CONV_CASES, ids=lambda c: 'B%d_T%d_F%d_C%d_N%d' % c)
def test_conv3x3_16_implicit(case, recipe):
    """asr_conv3x3_16(implicit = 1): act none / ReLU with bf16 output, out_f32 with act none, bias given and NULL; then the input
    gradient: the same kernel shape on dout (C channels) and asr_conv_weight_pack16(mode 1) of a (C, N, 3, 3) weight."""
    H = _H()
    B, T, Fq, C, N = case
    name = 'conv16 B%d T%d F%d C%d N%d %s' % (B, T, Fq, C, N, recipe)
    c = R.conv_inputs(case, recipe)
    K = 9 * C
    img = _dev16(c['x'])
    w16 = _dev16(R.pack_ref(c['w'], 0, K))
    bias_d = c['bias'].to(F32).cuda()
    for bias in (c['bias'], None):
        bias64 = None if bias is None else bias.to(F32).to(F64)
        terms = R.conv_abs_terms(c['x'], c['w'], bias64)
        for act, out_f32 in ((ACT_NONE, 0), (ACT_RELU, 0), (ACT_NONE, 1)):
            ref = R.conv_ref(c['x'], c['w'], bias64, act)
            got = _conv_call(img, w16, None if bias is None else bias_d, B, T, Fq, C, N, K, 1, act, out_f32)
            what = '%s%s%s' % ('f32' if out_f32 else 'bf16', ' relu' if act else '', '' if bias is None else ' +b')
            _judge_contraction(name, what, got, ref, terms, K + 1, recipe, not out_f32)
    # input gradient
    wg32 = c['wg'].to(F32).cuda()
    wd = _out((N, K), BF)
    H.call('asr_conv_weight_pack16', H.ptr(wg32), H.ptr(wd), C, N, K, 1, H.stream_ptr())
    torch.cuda.synchronize()
    packed = R.pack_ref(c['wg'], 1, K)
    assert _same_bits16(_back(wd, (N, K)), packed), name + ': asr_conv_weight_pack16 mode 1'
    dx_ref, _ = R.conv_grads_ref(border(torch.zeros(B, T, Fq, N, dtype=F64)), c['wg'], c['dout'])
    terms = R.conv_abs_terms(c['dout'], R.unpack_mode0(packed, N, C))
    dimg = _dev16(c['dout'])
    for out_f32 in (0, 1):
        got = _conv_call(dimg, wd[:N * K], None, B, T, Fq, C, N, K, 1, ACT_NONE, out_f32)
        _judge_contraction(name, 'dx ' + ('f32' if out_f32 else 'bf16'), got, dx_ref, terms, K + 1, recipe, not out_f32)


@gpu
@pytest.mark.parametrize('recipe', R.RECIPES)
@pytest.mark.parametrize('case', R.FIRST_CASES, ids=lambda c: 'B%d_T%d_F%d_Cin%d_Co%d_Kp%d' % c)
def test_first_layer_chain(case, recipe):
    """asr_vgg16_im2col -> asr_conv_weight_pack16(mode 0, Kp) -> asr_conv3x3_16(implicit = 0).  The two layout kernels are judged
    on their own, bit for bit (pad columns and border rows zero, values on bf16 rounding ties among the random inputs); the
    convolution then reads THEIR outputs and is judged by the contraction rules against conv_ref on the bordered bf16 image."""
    H = _H()
    B, T, Fq, Cin, Co, Kp = case
    name = 'first B%d T%d F%d Cin%d Co%d Kp%d %s' % (B, T, Fq, Cin, Co, Kp, recipe)
    c = R.first_inputs(case, recipe)
    feat, w = c['feat'].cuda(), c['w'].cuda()
    M = B * (T + 2) * (Fq + 2)
    x1, w16 = _out((M, Kp), BF), _out((Co, Kp), BF)
    H.call('asr_vgg16_im2col', H.ptr(feat), H.ptr(x1), B, T, Fq, Cin, Kp, H.stream_ptr())
    H.call('asr_conv_weight_pack16', H.ptr(w), H.ptr(w16), Co, Cin, Kp, 0, H.stream_ptr())
    torch.cuda.synchronize()
    got_x1 = _back(x1, (B, T + 2, Fq + 2, Kp))
    assert border_is_zero(got_x1) and bool((got_x1[..., 9 * Cin:] == 0).all()), name + ': im2col border rows / pad columns'
    assert _same_bits16(got_x1, R.im2col_ref(c['feat'], B, T, Fq, Cin, Kp)), name + ': im2col'
    got_w = _back(w16, (Co, Kp))
    assert bool((got_w[:, 9 * Cin:] == 0).all()), name + ': pack16 pad columns'
    assert _same_bits16(got_w, R.pack_ref(c['w'].double(), 0, Kp)), name + ': pack16 mode 0'
    xb, w64 = R.feature_image(c['feat'], B, T, Fq, Cin), bf16(c['w'].double())
    bias_d = c['bias'].to(F32).cuda()
    for bias in (c['bias'], None):
        bias64 = None if bias is None else bias.to(F32).to(F64)
        terms = R.conv_abs_terms(xb, w64, bias64)
        for act, out_f32 in ((ACT_NONE, 0), (ACT_RELU, 0), (ACT_NONE, 1)):
            ref = R.conv_ref(xb, w64, bias64, act)
            got = _conv_call(x1[:M * Kp], w16[:Co * Kp], None if bias is None else bias_d, B, T, Fq, Cin, Co, Kp, 0, act, out_f32)
            what = '%s%s%s' % ('f32' if out_f32 else 'bf16', ' relu' if act else '', '' if bias is None else ' +b')
            _judge_contraction(name, what, got, ref, terms, 9 * Cin + 1, recipe, not out_f32)


@gpu
@pytest.mark.parametrize('recipe', R.RECIPES)
@pytest.mark.parametrize('case', R.WGRAD_CASES, ids=lambda c: 'B%d_T%d_F%d_C%d_N%d_s%d_x%d' % c)
def test_conv3x3_16_wgrad_and_fold(case, recipe):
    """asr_conv3x3_16_wgrad: dw (N, ldw)[n][tap*C+ci] += sum over the bordered pixel rows of dout[row, n] img[row + shift(tap), ci].
    CONTRACT: img and dout have zero borders (asserted on the inputs here).  R = 288 rows with 3 splits leaves a short last slice,
    64 splits are clipped to the 18 k-steps, 0 splits count as 1, and with ldw = 9C + 8 the extra columns keep their bits.
    Then asr_conv_weight_fold adds the result into a non-zero (N,C,3,3) gradient: one fp32 add per element, exact."""
    H = _H()
    B, T, Fq, C, N, splits, extra = case
    name = 'wgrad B%d T%d F%d C%d N%d splits%d ldw+%d %s' % (B, T, Fq, C, N, splits, extra, recipe)
    c = R.wgrad_inputs(case, recipe)
    assert border_is_zero(c['img']) and border_is_zero(c['dout'])
    ldw, rows = 9 * C + extra, B * (T + 2) * (Fq + 2)
    img, dout = _dev16(c['img']), _dev16(c['dout'])
    dw = _out((N, ldw), F32, c['init'])
    H.call('asr_conv3x3_16_wgrad', H.ptr(img), H.ptr(dout), H.ptr(dw), B, T, Fq, C, N, ldw, splits, H.stream_ptr())
    torch.cuda.synchronize()
    got = _back(dw, (N, ldw))
    init64 = c['init'].to(F64)
    assert torch.equal(got[:, 9 * C:], init64[:, 9 * C:]), name + ': columns past 9C were touched'
    _, dw_ref = R.conv_grads_ref(c['img'], torch.zeros(N, C, 3, 3, dtype=F64), c['dout'])
    terms = R.wgrad_abs_terms(c['img'], c['dout']) + init64[:, :9 * C].abs()
    _judge_contraction(name, 'dw', got[:, :9 * C], init64[:, :9 * C] + dw_ref, terms, rows + 1, recipe, False, image=False)
    grad = _out((N, C, 3, 3), F32, c['grad0'])
    H.call('asr_conv_weight_fold', H.ptr(dw), H.ptr(grad), N, C, ldw, H.stream_ptr())
    torch.cuda.synchronize()
    folded = _back(grad, (N, C, 3, 3))
    want = R.fold_ref(got.to(F32), c['grad0']).to(F64)
    bad = int((folded != want).sum())
    print('EXACT %-44s %-10s wrong elements %d of %d' % (name, 'fold', bad, want.numel()))
    assert bad == 0


# ---------------------------------------------------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('kind', R.POOL_KINDS)
@pytest.mark.parametrize('case', R.POOL_CASES, ids=lambda c: 'B%d_T%d_F%d_C%d' % c)
def test_maxpool2x2_16(case, kind):
    """Ceil and floor output sizes (floor is left out where it gives no output).  Values bit-equal, index bytes EQUAL to the
    reference's (scan order (0,0),(0,1),(1,0),(1,1), strictly greater wins; post-ReLU images are mostly ties) with border bytes
    0, backward bit-equal, and in floor mode the rows and columns no window covers get zero."""
    H = _H()
    B, T, Fq, C = case
    c = R.pool_inputs(case, kind)
    xd = _dev16(c['x'])
    for ceil in (True, False):
        T2, F2 = R.pool_sizes(T, Fq, ceil)
        if T2 == 0 or F2 == 0:
            continue
        name = 'pool B%d T%d F%d C%d %s %s' % (B, T, Fq, C, kind, 'ceil' if ceil else 'floor')
        shape2 = (B, T2 + 2, F2 + 2, C)
        y, idx = _out(shape2, BF), _out(shape2, torch.uint8)
        H.call('asr_maxpool2x2_16_fwd', H.ptr(xd), H.ptr(y), H.ptr(idx), B, T, Fq, C, T2, F2, H.stream_ptr())
        torch.cuda.synchronize()
        y_ref, idx_ref = R.pool_ref(c['x'], T2, F2)
        got_y, got_idx = _back(y, shape2), _back(idx, shape2)
        print('EXACT %-44s values wrong %d, index bytes wrong %d of %d' % (name, int((got_y != y_ref).sum()), int((got_idx != idx_ref).sum()), y_ref.numel()))
        assert border_is_zero(got_y) and border_is_zero(got_idx), name + ': border pixels / border index bytes'
        assert _same_bits16(got_y, y_ref), name + ': values'
        assert torch.equal(got_idx, idx_ref), name + ': index bytes'
        g = border(c['g'][:, :T2, :F2])
        gd, idx_d = _dev16(g), idx_ref.to(torch.uint8).contiguous().cuda()          # the reference's bytes: independent of the forward
        dx = _out(c['x'].shape, BF)
        H.call('asr_maxpool2x2_16_bwd', H.ptr(gd), H.ptr(idx_d), H.ptr(dx), B, T, Fq, C, T2, F2, H.stream_ptr())
        torch.cuda.synchronize()
        got_dx = _back(dx, c['x'].shape)
        assert border_is_zero(got_dx), name + ': backward border'
        assert _same_bits16(got_dx, R.pool_bwd_ref(g, idx_ref, T, Fq)), name + ': backward'
        assert bool((interior(got_dx)[:, 2 * T2:] == 0).all()) and bool((interior(got_dx)[:, :, 2 * F2:] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm over frequency
# ---------------------------------------------------------------------------------------------------------------------
_LN_REF = {}


def _ln_refs(case, relu):
    """float64 and float32 CPU results of a case, computed once."""
    if (case, relu) not in _LN_REF:
        c = R.ln_inputs(case)
        _LN_REF[(case, relu)] = (c, R.ln_ref(c['x'], c['w'], c['b'], c['dy'], relu, F64), R.ln_ref(c['x'], c['w'], c['b'], c['dy'], relu, F32))
    return _LN_REF[(case, relu)]


def _judge_ln(name, what, got, ref64, ref32, keep=None, slack=None, k=K_LN):
    keep = torch.ones_like(ref64, dtype=torch.bool) if keep is None else keep
    scale = max(1.0, float(ref64.abs().max()))
    e32 = float((ref32.double() - ref64)[keep].abs().max())
    excess = (got - ref64).abs() - (0.0 if slack is None else slack)
    err = max(0.0, float(excess[keep].max()))
    print('RATIO %-36s %-6s err %.3e e32 %.3e ratio %7.2f scale %.3g%s'
          % (name, what, err, e32, err / max(e32, 1e-300), scale, '' if e32 > ULP32 * scale else '  (e32 below one ulp of scale)'))
    assert err <= k * e32 + FLOOR * scale, (name, what, err, e32, scale)


@gpu
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('case', R.LN_CASES, ids=lambda c: 'B%d_T%d_F%d_C%d' % c)
def test_ln_freq16_fwd_bwd(case, relu):
    """One thread per (b, t, c) walking f.  F = 1 (constant rows), F = 128 (the LDS limit of the backward), C = 512 (its column
    array), and B (T+2) C = 528384 > 2048 x 256 so that the backward's grid-stride loop takes a second trip.  The backward runs
    with dconv_bias given and NULL; dw / db / dconv_bias are accumulated onto random values."""
    H = _H()
    B, T, Fq, C = case
    name = 'ln16 B%d T%d F%d C%d relu%d' % (B, T, Fq, C, relu)
    c, r64, r32 = _ln_refs(case, relu)
    amb = R.ln_ambiguous(r64['pre64']) if relu else torch.zeros(B, T, Fq, C, dtype=torch.bool)
    assert int(amb.sum()) <= R.GATE_CAP * amb.numel()
    keep_b = border(amb.to(F64)) == 0                                             # border pixels are judged (they must be zero)
    xin = c['x'].clone()
    xin[border(torch.ones(B, T, Fq, C)) == 0] = 1e30                              # the kernel must not read a border pixel of x
    xd, wd, bd, dyd = xin.cuda(), c['w'].cuda(), c['b'].cuda(), _dev16(c['dy'])
    shape = (B, T + 2, Fq + 2, C)
    y, stats = _out(shape, BF), _out((B, T + 2, C, 2), F32)
    H.call('asr_ln_freq16_fwd', H.ptr(xd), H.ptr(wd), H.ptr(bd), H.ptr(y), H.ptr(stats), B, T, Fq, C, R.LN_EPS, relu, H.stream_ptr())
    st64 = torch.zeros(B, T + 2, C, 2, dtype=F64)
    st64[:, 1:-1, :, 0], st64[:, 1:-1, :, 1] = r64['mean'], r64['rstd']
    std = st64.to(F32).cuda()                                                     # the float64 statistics rounded to fp32
    outs = []
    for with_dcb in (True, False):
        dx, dw, db = _out(shape, BF), _out((Fq,), F32, c['dw0']), _out((Fq,), F32, c['db0'])
        dcb = _out((C,), F32, c['dcb0']) if with_dcb else None
        H.call('asr_ln_freq16_bwd', H.ptr(dyd), H.ptr(xd), H.ptr(wd), H.ptr(bd), H.ptr(std), H.ptr(dx), H.ptr(dw), H.ptr(db), H.ptr(dcb),
               B, T, Fq, C, relu, H.stream_ptr())
        outs.append((dx, dw, db, dcb))
    torch.cuda.synchronize()
    # forward
    got_y, got_st = _back(y, shape), _back(stats, (B, T + 2, C, 2))
    assert border_is_zero(got_y), name + ': y border'
    assert bool((got_st[:, 0] == 0).all()) and bool((got_st[:, -1] == 0).all()), name + ': statistics of the border rows'
    _judge_ln(name, 'y', got_y, r64['y'], r32['y'], keep_b, 2.0 ** -8 * r64['y'].abs())
    _judge_ln(name, 'mean', got_st[:, 1:-1, :, 0], r64['mean'], r32['mean'])
    _judge_ln(name, 'rstd', got_st[:, 1:-1, :, 1], r64['rstd'], r32['rstd'])
    # backward: what the gate of an ambiguous element i can change - g_i in db[f_i], g_i xh_i in dw[f_i], and through the two
    # row sums rstd (|g_i w_i| + |xh_j| |g_i w_i xh_i|) / F in dx of every j of its row
    x64, g64 = interior(c['x']).double(), interior(c['dy']).double()
    w64 = c['w'].double().view(1, 1, Fq, 1)
    mean, rstd = r64['mean'].unsqueeze(2), r64['rstd'].unsqueeze(2)
    xh = (x64 - mean) * rstd
    a = amb.double()
    s_dx = rstd * ((a * (g64 * w64).abs()).sum(2, keepdim=True) + xh.abs() * (a * (g64 * w64 * xh).abs()).sum(2, keepdim=True)) / Fq
    gate = (r64['pre64'] > 0).double() if relu else torch.ones_like(x64)
    gg = g64 * gate
    n_f = B * T * C + 1
    t_dw = n_f * U24 * ((gg * xh).abs().sum((0, 1, 3)) + c['dw0'].double().abs()) + (a * (g64 * xh).abs()).sum((0, 1, 3))
    t_db = n_f * U24 * (gg.abs().sum((0, 1, 3)) + c['db0'].double().abs()) + (a * g64.abs()).sum((0, 1, 3))
    # dconv_bias: every dx it sums is rstd (g w - s1 - xh s2); those three addends are its terms
    all_g = gg.abs() + a * g64.abs()                                              # an ambiguous gate may admit its g
    cb_terms = (rstd * ((all_g * w64.abs()) + (all_g * w64.abs()).mean(2, keepdim=True)
                        + xh.abs() * (all_g * w64.abs() * xh.abs()).mean(2, keepdim=True))).sum((0, 1, 2))
    n_cb = 3 * B * T * Fq + 1
    for with_dcb, (dx, dw, db, dcb) in zip((True, False), outs):
        tag = name + (' +dcb' if with_dcb else ' NULL')
        got_dx = _back(dx, shape)
        assert border_is_zero(got_dx), tag + ': dx border'
        _judge_ln(tag, 'dx', got_dx, r64['dx'], r32['dx'], keep_b, border(s_dx) + 2.0 ** -8 * r64['dx'].abs())
        _judge_ln(tag, 'dw', _back(dw, (Fq,)), c['dw0'].double() + r64['dw'], (c['dw0'] + r32['dw']), None, t_dw)
        _judge_ln(tag, 'db', _back(db, (Fq,)), c['db0'].double() + r64['db'], (c['db0'] + r32['db']), None, t_db)
        if with_dcb:
            got_cb = _back(dcb, (C,))
            bound = n_cb * U24 * (cb_terms + c['dcb0'].double().abs())
            err = (got_cb - c['dcb0'].double()).abs()
            print('SUM   %-36s %-6s err %.3e smallest bound %.3e worst err / bound %.4f' % (tag, 'dcb', float(err.max()), float(bound.min()), float((err / bound).max())))
            assert bool((err <= bound).all()), (tag, 'dcb', float(err.max()), float(bound.min()))


# ---------------------------------------------------------------------------------------------------------------------
# layout changes at the end of the stack
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('case', R.OUTPUT_CASES, ids=lambda c: 'B%d_T%d_F%d_C%d' % c)
def test_vgg16_output_and_bwd(case):
    H = _H()
    B, T, Fq, C = case
    c = R.output_inputs(case)
    xd, dd = _dev16(c['x']), _dev16(c['d'])
    out, g = _out((B, T, C * Fq), BF), _out(c['x'].shape, BF)
    H.call('asr_vgg16_output', H.ptr(xd), H.ptr(out), B, T, Fq, C, H.stream_ptr())
    H.call('asr_vgg16_output_bwd', H.ptr(dd), H.ptr(g), B, T, Fq, C, H.stream_ptr())
    torch.cuda.synchronize()
    assert _same_bits16(_back(out, (B, T, C * Fq)), R.output_ref(c['x']))
    got_g = _back(g, c['x'].shape)
    assert border_is_zero(got_g) and _same_bits16(got_g, R.output_bwd_ref(c['d'], Fq, C))


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def _untouched(buf):
    c = buf.cpu()
    if c.dtype == torch.uint8:
        return bool((c[:-TAIL] == 0xAB).all()) and bool((c[-TAIL:] == 0xCD).all())
    return bool(torch.isnan(c[:-TAIL]).all()) and bool((c[-TAIL:].to(F64) == SENT).all())


@gpu
def test_refusals_leave_the_output_untouched():
    """Each call returns its documented code and writes nothing."""
    H = _H()
    st = H.stream_ptr()
    B, T, Fq = 1, 2, 2
    M = B * (T + 2) * (Fq + 2)

    def conv(C, N, K, implicit=1, act=ACT_NONE, out_f32=0, img_off=0, w_off=0, out_off=0, bias_off=None, null=None):
        img = torch.zeros(M * max(C, K) + 8, dtype=BF).cuda()
        w16 = torch.zeros(N * K + 8, dtype=BF).cuda()
        bias = torch.zeros(N + 8, dtype=F32).cuda()
        out = _out((M * N + 8,), F32 if out_f32 else BF)
        args = [_off(img, img_off), _off(w16, w_off), _off(out, out_off), None if bias_off is None else _off(bias, bias_off)]
        if null is not None:
            args[null] = None
        rc = _rc('asr_conv3x3_16', *args, B, T, Fq, C, N, K, implicit, act, out_f32, st)
        torch.cuda.synchronize()
        assert rc == 0 or _untouched(out), ('asr_conv3x3_16 wrote its output although it refused', C, N, K)
        return rc

    assert conv(64, 8, 576) == 0                                                  # the shape the refusals below depart from
    assert conv(32, 8, 288) == E_UNSUPPORTED                                      # C % 64
    assert conv(64, 12, 576) == E_UNSUPPORTED                                     # N % 8
    assert conv(64, 8, 512) == E_UNSUPPORTED and conv(64, 8, 584) == E_UNSUPPORTED          # K != 9C
    assert conv(64, 8, 576, act=ACT_RELU, out_f32=1) == E_UNSUPPORTED
    assert conv(4, 8, 36, implicit=0) == E_UNSUPPORTED                            # explicit patch matrix: K % 8
    for k in ('img_off', 'w_off', 'out_off'):
        assert conv(64, 8, 576, **{k: 2}) == E_UNSUPPORTED, k                     # 2 bytes off a 16-byte boundary
    assert conv(64, 8, 576, bias_off=4) == E_UNSUPPORTED
    for null in (0, 1, 2):
        assert conv(64, 8, 576, null=null) == E_ARG
    last = H.lib().asr_last_error().decode()
    assert 'asr_conv3x3_16' in last

    # weight gradient: NULL pointers, C % 8, ldw < 9C, a misaligned operand
    img, dout = torch.zeros(M * 8 + 8, dtype=BF).cuda(), torch.zeros(M * 8 + 8, dtype=BF).cuda()
    for args, code in ((dict(), 0), (dict(null=0), E_ARG), (dict(null=1), E_ARG), (dict(null=2), E_ARG), (dict(C=12), E_ARG),
                       (dict(ldw=64), E_ARG), (dict(off=2), E_UNSUPPORTED)):
        dw = _out((8, 72), F32)
        ptrs = [_off(img, args.get('off', 0)), H.ptr(dout), H.ptr(dw)]
        if 'null' in args:
            ptrs[args['null']] = None
        C = args.get('C', 8)
        rc = _rc('asr_conv3x3_16_wgrad', *ptrs, B, T, Fq, C, 8, args.get('ldw', 72), 1, st)
        torch.cuda.synchronize()
        assert rc == code, (args, rc)
        assert code == 0 or _untouched(dw), args

    # LayerNorm backward beyond its LDS arrays; pooling with more windows than ceil(T/2) x ceil(F/2), forward and backward
    for (Fl, Cl) in ((129, 8), (2, 513)):
        n = 1 * 3 * (Fl + 2) * Cl
        x, dy = torch.zeros(n, dtype=F32).cuda(), torch.zeros(n, dtype=BF).cuda()
        w, b, stats = torch.ones(Fl).cuda(), torch.zeros(Fl).cuda(), torch.zeros(3 * Cl * 2).cuda()
        dx, dw, db, dcb = _out((n,), BF), _out((Fl,), F32), _out((Fl,), F32), _out((Cl,), F32)
        rc = _rc('asr_ln_freq16_bwd', H.ptr(dy), H.ptr(x), H.ptr(w), H.ptr(b), H.ptr(stats), H.ptr(dx), H.ptr(dw), H.ptr(db), H.ptr(dcb),
                 1, 1, Fl, Cl, 1, st)
        torch.cuda.synchronize()
        assert rc == E_UNSUPPORTED and all(_untouched(t) for t in (dx, dw, db, dcb)), (Fl, Cl, rc)
    Tp, Fp, Cp = 5, 7, 8
    x = torch.zeros(1 * (Tp + 2) * (Fp + 2) * Cp, dtype=BF).cuda()
    for (T2, F2) in ((4, 4), (3, 5), (0, 4), (3, 0)):
        n2 = (T2 + 2) * (F2 + 2) * Cp
        y, idx = _out((n2,), BF), _out((n2,), torch.uint8)
        rc = _rc('asr_maxpool2x2_16_fwd', H.ptr(x), H.ptr(y), H.ptr(idx), 1, Tp, Fp, Cp, T2, F2, st)
        torch.cuda.synchronize()
        assert rc == E_ARG and _untouched(y) and _untouched(idx), (T2, F2, rc)
        dy, idx_in = torch.zeros(n2, dtype=BF).cuda(), torch.zeros(n2, dtype=torch.uint8).cuda()
        dx = _out((x.numel(),), BF)
        rc = _rc('asr_maxpool2x2_16_bwd', H.ptr(dy), H.ptr(idx_in), H.ptr(dx), 1, Tp, Fp, Cp, T2, F2, st)
        torch.cuda.synchronize()
        assert rc == E_ARG and _untouched(dx), ('asr_maxpool2x2_16_bwd', T2, F2, rc)
