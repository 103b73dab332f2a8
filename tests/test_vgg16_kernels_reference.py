"""The yardstick of the bf16 VGG front-end (csrc/vgg16.hip and the CONV / tap instantiations of csrc/gemm16.hip): plain float64
torch restatements of every operation on BORDERED CHANNEL-LAST IMAGES P(T, F, C) = (B, T+2, F+2, C) whose border pixels are
zero, the input recipes, the case tables, and the CPU checks of all three.  tests/test_hip_vgg16_kernels_vs_float64.py imports
them; nothing here imports the code under test.

Operations
  conv_ref        float64 F.conv2d(padding=1) on the interior, returned bordered; bias and ReLU optional.  conv_rows_ref says the
                  same thing the way the kernel sees it - tap (dt, df) is the row shift (dt-1)(F+2) + (df-1) of the pixel-row
                  matrix against the packed weight [n][tap*C + ci], tap = 3 dt + df - and the two are checked against each other.
  conv_grads_ref  input gradient (bordered) and weight gradient [n][tap*C + ci] by float64 autograd.
  im2col_ref      feature (B, T, Cin*F) channel-major -> patch matrix (B, T+2, F+2, Kp), [tap*Cin + ci], zero pad columns and borders.
  pack_ref        (Co,Ci,3,3) -> mode 0 (Co, Kp)[co][tap*Ci+ci]; mode 1 (Ci, Kp)[ci][tap*Co+co] = src[co][ci][8-tap]; bf16 values.
  fold_ref        (Co,Ci,3,3) += (Co, ld)[tap*Ci+ci] in float32, one add per element.
  pool_ref        2x2 / stride 2 max pooling with T2 x F2 output windows (ceil or floor sizes), values AND the index byte 2 dt + df.
                  Tie rule: candidates are scanned in the order (0,0), (0,1), (1,0), (1,1) from -inf, and a candidate replaces
                  the best so far only when it is STRICTLY greater - the first of equal maxima keeps the index.  Candidates
                  outside the image (ceil mode, odd sizes) do not take part.
  pool_bwd_ref    the gradient of a window goes to the input its index byte names; inputs no window covers get zero.
  ln_ref          LayerNorm over the F interior pixels of every (b, t, c), biased variance, affine per f, optional ReLU;
                  y, mean, rstd, pre-activation, and by autograd dx, dw, db and the per-channel sum of dx.
  output_ref / output_bwd_ref   P(T,F,C) <-> (B, T, C*F) channel-major.

Recipes for the contractions
  integer   x, w, dout uniform integers in [-4, 4] (about half of x exactly zero), bias in [-8, 8], accumulator start values
            in [-64, 64]: every product and partial sum is an integer below 2^24 (asserted for every case), so fp32 accumulation
            is EXACT in any order, atomics included, and the kernel must reproduce float64 exactly.
  random    bf16-rounded normals, x ~ N(0,1), w ~ N(0,1) / sqrt(9 C); bias fp32 N(0,1).

bf16(x) rounds through float32; every value it is applied to where exactness matters is a float32 value already.
"""
import math

import pytest
import torch
import torch.nn.functional as F

F64, F32 = torch.float64, torch.float32
ACT_NONE, ACT_RELU = 0, 2
LN_EPS = 1e-5
GATE_BAND = 1e-5
GATE_CAP = 1e-3
TAPS = [(dt, df) for dt in range(3) for df in range(3)]          # tap = 3 dt + df
POOL_SCAN = [(0, 0), (0, 1), (1, 0), (1, 1)]                      # index byte = 2 dt + df = position in this list


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def border(x):
    """(B, T, F, C) -> (B, T+2, F+2, C) with a zero border."""
    return F.pad(x, (0, 0, 1, 1, 1, 1))


def interior(p):
    return p[:, 1:-1, 1:-1, :]


def border_is_zero(p):
    q = p.clone()
    q[:, 1:-1, 1:-1, :] = 0
    return bool((q == 0).all())


def bf16(x):
    """Round to nearest even onto bfloat16, back as float64."""
    return x.to(F32).to(torch.bfloat16).to(F64)


# ---------------------------------------------------------------------------------------------------------------------
# convolution
# ---------------------------------------------------------------------------------------------------------------------
def conv_ref(xb, w, bias=None, act=ACT_NONE):
    """xb (B,T+2,F+2,C) bordered, w (N,C,3,3), bias (N) or None -> (B,T+2,F+2,N) bordered."""
    y = F.conv2d(interior(xb).permute(0, 3, 1, 2), w, bias, padding=1)
    if act == ACT_RELU:
        y = torch.relu(y)
    return border(y.permute(0, 2, 3, 1))


def unpack_mode0(p, rows, inner):
    """(rows, >= 9*inner)[r][tap*inner + c] -> conv weight (rows, inner, 3, 3)."""
    return p[:, :9 * inner].reshape(rows, 3, 3, inner).permute(0, 3, 1, 2).contiguous()


def conv_rows_ref(xb, packed, bias=None):
    """The kernel's view: rows of the bordered pixel matrix shifted by the tap, against packed (N, 9C); border rows zeroed."""
    B, T2, F2, C = xb.shape
    N = packed.shape[0]
    rows = xb.reshape(B * T2 * F2, C)
    M = rows.shape[0]
    out = torch.zeros(M, N, dtype=xb.dtype)
    for tap, (dt, df) in enumerate(TAPS):
        sh = (dt - 1) * F2 + (df - 1)
        src = torch.zeros_like(rows)
        lo, hi = max(0, -sh), min(M, M - sh)
        src[lo:hi] = rows[lo + sh:hi + sh]
        out += src @ packed[:, tap * C:(tap + 1) * C].t()
    if bias is not None:
        out = out + bias
    return border(interior(out.view(B, T2, F2, N)))


def conv_abs_terms(xb, w, bias=None):
    """Sum of |terms| of every output element: sum |x||w| + |bias|, bordered."""
    return conv_ref(xb.abs(), w.abs(), None if bias is None else bias.abs())


def conv_grads_ref(xb, w, doutb):
    """-> (dx bordered (B,T+2,F+2,C), dw (N, 9C)[n][tap*C+ci]) of sum(conv(x, w) * dout) by autograd."""
    x = interior(xb).clone().requires_grad_(True)
    wl = w.clone().requires_grad_(True)
    y = F.conv2d(x.permute(0, 3, 1, 2), wl, None, padding=1).permute(0, 2, 3, 1)
    (y * interior(doutb)).sum().backward()
    N, C = w.shape[0], w.shape[1]
    return border(x.grad), wl.grad.permute(0, 2, 3, 1).reshape(N, 9 * C)


def wgrad_abs_terms(xb, doutb):
    """Sum of |dout||img| behind every element of the weight gradient, (N, 9C)."""
    ones = torch.zeros(doutb.shape[-1], xb.shape[-1], 3, 3, dtype=xb.dtype)
    return conv_grads_ref(xb.abs(), ones, doutb.abs())[1]


def im2col_ref(feat, B, T, Fq, Cin, Kp):
    img = feat.to(F64).view(B, T, Cin, Fq).permute(0, 1, 3, 2)          # (B, T, F, Cin)
    p2 = F.pad(img, (0, 0, 2, 2, 2, 2))
    out = torch.zeros(B, T + 2, Fq + 2, Kp, dtype=F64)
    for tap, (dt, df) in enumerate(TAPS):
        out[:, 1:T + 1, 1:Fq + 1, tap * Cin:(tap + 1) * Cin] = p2[:, 1 + dt:1 + dt + T, 1 + df:1 + df + Fq, :]
    return bf16(out)


def feature_image(feat, B, T, Fq, Cin):
    """The bordered bf16 image the first layer convolves: feature (B, T, Cin*F) channel-major -> (B, T+2, F+2, Cin)."""
    return border(bf16(feat.to(F64).view(B, T, Cin, Fq).permute(0, 1, 3, 2)))


def pack_ref(w, mode, Kp):
    Co, Ci = w.shape[0], w.shape[1]
    if mode == 0:
        p = w.permute(0, 2, 3, 1).reshape(Co, 9 * Ci)
    else:
        p = w.flip(2, 3).permute(1, 2, 3, 0).reshape(Ci, 9 * Co)
    out = torch.zeros(p.shape[0], Kp, dtype=F64)
    out[:, :p.shape[1]] = bf16(p)
    return out


def pack_unrounded(w, mode):
    """The packing rule alone, values untouched (the fp32 asr_conv_weight_permute): mode 0 (Co, 9 Ci)[co][tap*Ci+ci], mode 1
    (Ci, 9 Co)[ci][tap*Co+co] = w[co][ci][8-tap]."""
    Co, Ci = w.shape[0], w.shape[1]
    if mode == 0:
        return w.permute(0, 2, 3, 1).reshape(Co, 9 * Ci)
    return w.flip(2, 3).permute(1, 2, 3, 0).reshape(Ci, 9 * Co)


def fold_ref(src, dst):
    """dst (Co,Ci,3,3) fp32 + src (Co, ld)[tap*Ci+ci] fp32: one float32 add per element."""
    Co, Ci = dst.shape[0], dst.shape[1]
    assert src.dtype == F32 and dst.dtype == F32
    return dst + src[:, :9 * Ci].reshape(Co, 9, Ci).permute(0, 2, 1).reshape(Co, Ci, 3, 3)


# ---------------------------------------------------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------------------------------------------------
def pool_sizes(T, Fq, ceil):
    return ((T + 1) // 2, (Fq + 1) // 2) if ceil else (T // 2, Fq // 2)


def pool_ref(xb, T2, F2):
    """-> (values bordered (B,T2+2,F2+2,C), index bytes bordered, int64; border bytes 0)."""
    x = interior(xb)
    B, T, Fq, C = x.shape
    assert T2 > 0 and F2 > 0 and 2 * T2 - 1 <= T and 2 * F2 - 1 <= Fq
    best = torch.full((B, T2, F2, C), float('-inf'), dtype=x.dtype)
    idx = torch.zeros((B, T2, F2, C), dtype=torch.int64)
    for k, (dt, df) in enumerate(POOL_SCAN):
        sub = x[:, dt:2 * T2:2, df:2 * F2:2, :]
        cand = torch.full_like(best, float('-inf'))
        cand[:, :sub.shape[1], :sub.shape[2], :] = sub
        win = cand > best                                            # strictly greater: the first of equal maxima stays
        best = torch.where(win, cand, best)
        idx = torch.where(win, torch.full_like(idx, k), idx)
    return border(best), border(idx)


def pool_bwd_ref(gb, idxb, T, Fq):
    g, idx = interior(gb), interior(idxb)
    B, T2, F2, C = g.shape
    dx = torch.zeros(B, T, Fq, C, dtype=g.dtype)
    for k, (dt, df) in enumerate(POOL_SCAN):
        view = dx[:, dt:2 * T2:2, df:2 * F2:2, :]
        nt, nf = view.shape[1], view.shape[2]
        view.copy_(torch.where(idx[:, :nt, :nf, :] == k, g[:, :nt, :nf, :], torch.zeros((), dtype=g.dtype)))          # +0, never g * 0 = -0
    return border(dx)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm over frequency
# ---------------------------------------------------------------------------------------------------------------------
def ln_pre(x, w, b):
    """x (B,T,F,C) interior -> pre-activation, mean (B,T,C), rstd (B,T,C); the formula, in the dtype of x."""
    mean = x.mean(2, keepdim=True)
    var = ((x - mean) ** 2).mean(2, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    pre = (x - mean) * rstd * w.view(1, 1, -1, 1) + b.view(1, 1, -1, 1)
    return pre, mean.squeeze(2), rstd.squeeze(2)


def ln_ref(xb, w, b, dyb, relu, dtype=F64):
    """Forward and backward in `dtype`.  The ReLU gate is the float64 one in either dtype (a 0 / 1 factor), so the float32
    run measures arithmetic and not gates that flipped.  Borders of xb are not read."""
    pre64, _, _ = ln_pre(interior(xb).to(F64), w.to(F64), b.to(F64))
    x = interior(xb).to(dtype).clone().requires_grad_(True)
    wl, bl = w.to(dtype).clone().requires_grad_(True), b.to(dtype).clone().requires_grad_(True)
    pre, mean, rstd = ln_pre(x, wl, bl)
    y = pre * (pre64 > 0).to(dtype) if relu else pre
    (y * interior(dyb).to(dtype)).sum().backward()
    return dict(y=border(y.detach()), mean=mean.detach(), rstd=rstd.detach(), dx=border(x.grad), dw=wl.grad, db=bl.grad,
                dcb=x.grad.sum((0, 1, 2)), pre64=pre64)


def ln_ambiguous(pre64):
    return pre64.abs() <= GATE_BAND * max(1.0, float(pre64.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------
# layout changes at the end of the stack
# ---------------------------------------------------------------------------------------------------------------------
def output_ref(xb):
    x = interior(xb)
    B, T, Fq, C = x.shape
    return x.permute(0, 1, 3, 2).reshape(B, T, C * Fq)


def output_bwd_ref(d, Fq, C):
    B, T = d.shape[0], d.shape[1]
    return border(d.view(B, T, C, Fq).permute(0, 1, 3, 2))


# ---------------------------------------------------------------------------------------------------------------------
# case tables and input recipes
# ---------------------------------------------------------------------------------------------------------------------
# implicit convolution (B, T, F, C, N)
CONV_CASES = [(1, 1, 1, 64, 8),            # one interior pixel, M = 9
              (2, 3, 5, 64, 72),           # M = 70 < one tile, partial N tile
              (3, 6, 10, 128, 136),        # 3 M tiles with a 32-row tail, 2 N tiles the second 8 wide, two k-steps per tap
              (2, 22, 22, 64, 136),        # 9 x 2 = 18 tiles: the XCD remap has rr = 2, qq = 2
              (1, 4, 4, 256, 128)]         # the real 36-k-step depth
# first layer (B, T, F, Cin, Co, Kp)
FIRST_CASES = [(2, 4, 5, 4, 64, 40), (1, 8, 40, 4, 64, 40), (3, 5, 7, 1, 72, 16), (2, 6, 9, 3, 128, 32), (2, 4, 5, 4, 64, 48)]
# weight gradient (B, T, F, C, N, splits, extra columns of ldw)
WGRAD_CASES = [(1, 1, 1, 8, 8, 1, 0), (2, 5, 6, 40, 24, 2, 0), (2, 3, 5, 64, 72, 1, 8), (3, 6, 10, 128, 136, 3, 0),
               (2, 22, 22, 64, 64, 64, 0), (2, 3, 5, 64, 72, 0, 0)]
POOL_CASES = [(1, 1, 1, 8), (1, 2, 2, 16), (2, 5, 7, 8), (3, 9, 10, 72), (2, 4, 40, 64)]
LN_CASES = [(1, 1, 1, 8), (2, 3, 5, 6), (2, 4, 40, 64), (1, 2, 128, 8), (3, 5, 20, 128), (8, 127, 2, 512)]
OUTPUT_CASES = [(1, 1, 1, 64), (2, 3, 5, 8), (3, 7, 10, 128)]
RECIPES = ['integer', 'random']


def _ints(g, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=g).to(F64)


def _image(g, recipe, shape, half_zero=False):
    """A bordered image of bf16 values, float64."""
    if recipe == 'integer':
        x = _ints(g, shape, 4)
        if half_zero:
            x = x * (torch.rand(shape, generator=g) < 0.5)
    else:
        x = bf16(torch.randn(shape, generator=g))
    return border(x)


def _weight(g, recipe, Co, Ci):
    if recipe == 'integer':
        return _ints(g, (Co, Ci, 3, 3), 4)
    return bf16(torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci))


def _bias(g, recipe, N):
    return _ints(g, (N,), 8) if recipe == 'integer' else torch.randn(N, generator=g).to(F64)


def conv_inputs(case, recipe):
    """Forward: x (C channels), w (N,C,3,3), bias (N).  Input gradient, the SAME kernel shape: a layer with Co = C, Ci = N,
    weight wg (C,N,3,3), its output gradient dout with C channels and its input xg with N channels (autograd needs only its
    shape); the kernel convolves dout with pack16(wg, mode 1) = (N, 9C)."""
    B, T, Fq, C, N = case
    g = gen(4100 + 7 * CONV_CASES.index(case) + RECIPES.index(recipe))
    return dict(x=_image(g, recipe, (B, T, Fq, C), True), w=_weight(g, recipe, N, C), bias=_bias(g, recipe, N),
                dout=_image(g, recipe, (B, T, Fq, C)), wg=_weight(g, recipe, C, N))


def first_inputs(case, recipe):
    """feature (B, T, Cin*F) fp32 and w (Co,Cin,3,3) fp32.  The random recipe is NOT rounded to bf16 beforehand and carries
    values on bf16 rounding ties (1 + 2^-8 rounds down to even, 1 + 3 2^-8 up to even, both signs)."""
    B, T, Fq, Cin, Co, Kp = case
    g = gen(4200 + 7 * FIRST_CASES.index(case) + RECIPES.index(recipe))
    if recipe == 'integer':
        feat = (_ints(g, (B, T, Cin * Fq), 4) * (torch.rand(B, T, Cin * Fq, generator=g) < 0.5)).to(F32)
        w, bias = _ints(g, (Co, Cin, 3, 3), 4).to(F32), _ints(g, (Co,), 8)
    else:
        feat = torch.randn(B, T, Cin * Fq, generator=g)
        w, bias = torch.randn(Co, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin), torch.randn(Co, generator=g).to(F64)
        ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 2.0 ** -9 + 2.0 ** -17])
        feat.view(-1)[:5] = ties
        w.view(-1)[:5] = ties
        w.view(-1)[-5:] = ties
    return dict(feat=feat, w=w, bias=bias)


def wgrad_inputs(case, recipe):
    B, T, Fq, C, N, splits, extra = case
    g = gen(4300 + 7 * WGRAD_CASES.index(case) + RECIPES.index(recipe))
    ldw = 9 * C + extra
    init = _ints(g, (N, ldw), 64) if recipe == 'integer' else torch.randn(N, ldw, generator=g).to(F64)
    grad0 = _ints(g, (N, C, 3, 3), 64) if recipe == 'integer' else torch.randn(N, C, 3, 3, generator=g).to(F64)
    return dict(img=_image(g, recipe, (B, T, Fq, C), True), dout=_image(g, recipe, (B, T, Fq, N)), init=init.to(F32), grad0=grad0.to(F32))


POOL_KINDS = ['post_relu', 'negative']


def pool_inputs(case, kind):
    """post_relu: relu of bf16 normals, more than half of the elements exactly zero, so most windows hold ties;
    negative: every element below zero (a maximum that starts from 0 instead of -inf would show)."""
    B, T, Fq, C = case
    g = gen(4400 + 7 * (POOL_CASES + [POOL_CASE_STRIDE]).index(case) + POOL_KINDS.index(kind))
    x = bf16(torch.randn(B, T, Fq, C, generator=g))
    x = torch.relu(x - 0.25) if kind == 'post_relu' else -(x.abs() + 0.125)
    x = bf16(x)
    T2, F2 = pool_sizes(T, Fq, True)
    return dict(x=border(x), g=bf16(torch.randn(B, T2, F2, C, generator=g)))


# further pooling inputs on one odd-sized image: 'tie0' .. 'tie3' - in every window the maximum stands at scan position k and at
# every later one, smaller values before it, so the index byte must be k wherever position k lies inside the image; 'neg_inf' - a
# third of the elements are -inf, whole windows among them (their index byte stays 0)
POOL_EXTRA_CASE = (2, 5, 7, 8)
POOL_EXTRA_KINDS = ['tie0', 'tie1', 'tie2', 'tie3', 'neg_inf']


def pool_extra_inputs(kind):
    B, T, Fq, C = POOL_EXTRA_CASE
    g = gen(4450 + POOL_EXTRA_KINDS.index(kind))
    T2, F2 = pool_sizes(T, Fq, True)
    if kind == 'neg_inf':
        x = bf16(torch.randn(B, T, Fq, C, generator=g))
        x[torch.rand(B, T, Fq, C, generator=g) < 0.33] = float('-inf')
        x[0, 0:2, 0:2, :] = float('-inf')
        x[1, 4, 6, :] = float('-inf')                                 # the one-element corner window of the ceil sizes
    else:
        first = int(kind[3])
        top = bf16(torch.randn(B, T2, F2, C, generator=g))
        x = torch.zeros(B, 2 * T2, 2 * F2, C, dtype=F64)
        for k, (dt, df) in enumerate(POOL_SCAN):
            x[:, dt::2, df::2, :] = top if k >= first else top - 1.0 - k
        x = bf16(x[:, :T, :Fq, :].contiguous())
    return dict(x=border(x), g=bf16(torch.randn(B, T2, F2, C, generator=g)))


# fp32 kernels only (tests/test_hip_vgg_kernels_vs_float64.py): their grids are capped, and these sizes run past the caps.
#   LN_CASE_BWD_STRIDE  B T C = 527352 > 512 x 1024 thread slots of asr_ln_freq_bwd: a second pass of its loop by 3 workgroups, the
#                       last of them with 1016 of its 1024 lanes in range.  F = 8, not 2: dw / db are sums of 527352 terms each,
#                       torch's float32 error on ONE such sum varies 16-fold with the data (7e-5 .. 1.2e-3 seen on F = 2), and e32
#                       is the maximum over the F outputs - with two of them the yardstick itself is a lottery
#   LN_CASE_FWD_STRIDE  B T C = 4198400 > 16384 x 256 threads of asr_ln_freq_fwd (forward only)
#   POOL_CASE_STRIDE    4259840 outputs and 17039360 inputs against the 16384 x 256 threads of the pooling forward / backward
LN_CASE_BWD_STRIDE = (8, 129, 8, 511)
LN_CASE_FWD_STRIDE = (8, 1025, 2, 512)
POOL_CASE_STRIDE = (16, 130, 64, 128)
LN_SEEDS = {case: 4500 + 7 * i for i, case in enumerate(LN_CASES + [LN_CASE_BWD_STRIDE, LN_CASE_FWD_STRIDE])}


def ln_inputs(case):
    """x fp32 with a per-channel offset and scale (pre-activations of a convolution), dy bf16 values, w / b per f, and the
    random starting values of the three accumulated outputs."""
    B, T, Fq, C = case
    g = gen(LN_SEEDS[case])
    x = torch.randn(B, T, Fq, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
    return dict(x=border(x), w=1.0 + 0.5 * torch.randn(Fq, generator=g), b=0.5 * torch.randn(Fq, generator=g),
                dy=border(bf16(torch.randn(B, T, Fq, C, generator=g))).to(F32), dw0=torch.randn(Fq, generator=g),
                db0=torch.randn(Fq, generator=g), dcb0=torch.randn(C, generator=g))


def output_inputs(case):
    B, T, Fq, C = case
    g = gen(4600 + OUTPUT_CASES.index(case))
    return dict(x=border(bf16(torch.randn(B, T, Fq, C, generator=g))), d=bf16(torch.randn(B, T, C * Fq, generator=g)))


# ---------------------------------------------------------------------------------------------------------------------
# CPU checks of the references, the recipes and the conditions the GPU module relies on
# ---------------------------------------------------------------------------------------------------------------------
def test_helpers():
    x = torch.arange(2 * 3 * 4 * 5, dtype=F64).view(2, 3, 4, 5) + 1
    p = border(x)
    assert p.shape == (2, 5, 6, 5) and torch.equal(interior(p), x) and border_is_zero(p)
    q = p.clone()
    q[1, 4, 5, 4] = 1e-30
    assert not border_is_zero(q)
    v = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, -3.0, 36864.0, 36865.0], dtype=F64)
    assert bf16(v).tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -3.0, 36864.0, 36864.0]


@pytest.mark.parametrize('recipe', RECIPES)
@pytest.mark.parametrize('case', CONV_CASES[:3] + CONV_CASES[4:])
def test_conv_ref_is_conv2d_and_shifted_rows(case, recipe):
    B, T, Fq, C, N = case
    c = conv_inputs(case, recipe)
    raw = interior(c['x']).permute(0, 3, 1, 2)
    want = F.conv2d(raw, c['w'], c['bias'], padding=1).permute(0, 2, 3, 1)
    got = conv_ref(c['x'], c['w'], c['bias'])
    assert border_is_zero(got) and torch.equal(interior(got), want)
    assert torch.equal(interior(conv_ref(c['x'], c['w'], c['bias'], ACT_RELU)), torch.relu(want))
    rows = conv_rows_ref(c['x'], pack_ref(c['w'], 0, 9 * C), c['bias'])
    tol = 0.0 if recipe == 'integer' else 1e-12 * float(conv_abs_terms(c['x'], c['w'], c['bias']).max())
    assert float((rows - got).abs().max()) <= tol
    assert torch.equal(unpack_mode0(pack_ref(c['w'], 0, 9 * C + 8), N, C), c['w'])
    # the weight gradient layout: d/dw of <conv(x, w), dout'> against the shifted-row contraction written out
    dout = _image(gen(1), recipe, (B, T, Fq, N))
    _, dw = conv_grads_ref(c['x'], c['w'], dout)
    xr, dr = c['x'].reshape(-1, C), dout.reshape(-1, N)
    M, F2 = xr.shape[0], Fq + 2
    for tap in (0, 4, 5, 8):
        dt, df = TAPS[tap]
        sh = (dt - 1) * F2 + (df - 1)
        src = torch.zeros_like(xr)
        lo, hi = max(0, -sh), min(M, M - sh)
        src[lo:hi] = xr[lo + sh:hi + sh]
        assert float((dr.t() @ src - dw[:, tap * C:(tap + 1) * C]).abs().max()) <= 1e-12 * max(1.0, float(dw.abs().max()))


@pytest.mark.parametrize('recipe', RECIPES)
@pytest.mark.parametrize('case', CONV_CASES[:3] + CONV_CASES[4:])
def test_mode1_packing_gives_the_input_gradient(case, recipe):
    """conv_ref(dout, unpack(pack_ref(wg, mode 1))) == autograd input gradient of the layer with weight wg."""
    B, T, Fq, C, N = case
    c = conv_inputs(case, recipe)
    xg = border(torch.zeros(B, T, Fq, N, dtype=F64))
    dx, _ = conv_grads_ref(xg, c['wg'], c['dout'])
    got = conv_ref(c['dout'], unpack_mode0(pack_ref(c['wg'], 1, 9 * C), N, C))
    assert float((got - dx).abs().max()) <= (0.0 if recipe == 'integer' else 1e-12 * max(1.0, float(dx.abs().max())))
    p = pack_ref(c['wg'], 1, 9 * C)
    assert p[3, 2 * C + 5] == c['wg'][5, 3, 2, 0] and p[0, 8 * C + 1] == c['wg'][1, 0, 0, 0]          # [ci][tap*Co+co] = w[co][ci][8-tap]


def test_integer_recipe_is_exact_in_fp32():
    """max sum |terms| < 2^24 for every committed contraction case, and every input is a bf16 value."""
    lim = 2.0 ** 24
    for case in CONV_CASES:
        c = conv_inputs(case, 'integer')
        assert float(conv_abs_terms(c['x'], c['w'], c['bias']).max()) < lim
        assert float(conv_abs_terms(c['dout'], unpack_mode0(pack_ref(c['wg'], 1, 9 * case[3]), case[4], case[3])).max()) < lim
        assert float((interior(c['x']) == 0).double().mean()) > 0.4
        for k in ('x', 'w', 'dout', 'wg'):
            assert torch.equal(bf16(c[k]), c[k]) and float(c[k].abs().max()) <= 4
        assert float(c['bias'].abs().max()) <= 8
    for case in FIRST_CASES:
        B, T, Fq, Cin, Co, Kp = case
        c = first_inputs(case, 'integer')
        assert float(conv_abs_terms(feature_image(c['feat'], B, T, Fq, Cin), c['w'].double(), c['bias']).max()) < lim
        assert Kp % 8 == 0 and Kp >= 9 * Cin
    assert [c[5] for c in FIRST_CASES[:4]] == [8 * ((9 * c[3] + 7) // 8) for c in FIRST_CASES[:4]]
    for case in WGRAD_CASES:
        c = wgrad_inputs(case, 'integer')
        assert float(wgrad_abs_terms(c['img'], c['dout']).max()) + 64 < lim
        assert border_is_zero(c['img']) and border_is_zero(c['dout'])


def test_random_recipe_is_bf16():
    for case in CONV_CASES[:2]:
        c = conv_inputs(case, 'random')
        for k in ('x', 'w', 'dout', 'wg'):
            assert torch.equal(bf16(c[k]), c[k])
    c = first_inputs(FIRST_CASES[0], 'random')
    assert not torch.equal(bf16(c['w'].double()), c['w'].double())
    assert bf16(c['w'].double()).view(-1)[:4].tolist() == [1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6)]


@pytest.mark.parametrize('case', FIRST_CASES)
def test_im2col_and_pack_feed_the_same_convolution(case):
    """X1 @ pack(w, 0)^T over the patch matrix == conv_ref on the bordered feature image (interior rows)."""
    B, T, Fq, Cin, Co, Kp = case
    c = first_inputs(case, 'integer')
    x1 = im2col_ref(c['feat'], B, T, Fq, Cin, Kp)
    assert bool((x1[..., 9 * Cin:] == 0).all()) and border_is_zero(x1)
    w16 = pack_ref(c['w'].double(), 0, Kp)
    assert bool((w16[:, 9 * Cin:] == 0).all())
    got = (x1.view(-1, Kp) @ w16.t()).view(B, T + 2, Fq + 2, Co)
    want = conv_ref(feature_image(c['feat'], B, T, Fq, Cin), c['w'].double())
    assert torch.equal(got, want)


def test_fold_ref():
    src = torch.arange(2 * 30, dtype=F32).view(2, 30)
    got = fold_ref(src, torch.ones(2, 3, 3, 3))
    assert got[1, 2, 1, 0] == 1 + src[1, 3 * 3 + 2] and got[0, 0, 2, 2] == 1 + src[0, 8 * 3]


@pytest.mark.parametrize('kind', POOL_KINDS)
@pytest.mark.parametrize('case', POOL_CASES)
def test_pool_ref(case, kind):
    B, T, Fq, C = case
    c = pool_inputs(case, kind)
    x = interior(c['x'])
    assert bool((x < 0).all()) if kind == 'negative' else (B * T * Fq * C < 64 or float((x == 0).double().mean()) > 0.5)
    for ceil in (True, False):
        T2, F2 = pool_sizes(T, Fq, ceil)
        if T2 == 0 or F2 == 0:
            continue
        y, idx = pool_ref(c['x'], T2, F2)
        want = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2, ceil_mode=ceil).permute(0, 2, 3, 1)
        assert torch.equal(interior(y), want) and border_is_zero(y) and border_is_zero(idx)
        assert 0 <= int(idx.min()) and int(idx.max()) <= 3
        # the index names an element that holds the maximum, and no earlier candidate of the scan holds it too
        for k, (dt, df) in enumerate(POOL_SCAN):
            sub = x[:, dt:2 * T2:2, df:2 * F2:2, :]
            yi, ii = interior(y)[:, :sub.shape[1], :sub.shape[2]], interior(idx)[:, :sub.shape[1], :sub.shape[2]]
            assert bool((sub[ii == k] == yi[ii == k]).all()) and not bool((sub[ii > k] == yi[ii > k]).any())
        # adjoint identity <pool(x), g> == <x, pool_bwd(g)>
        g = border(interior(border(c['g']))[:, :T2, :F2])
        dx = pool_bwd_ref(g, idx, T, Fq)
        assert border_is_zero(dx) and dx.shape == c['x'].shape
        assert not bool(torch.signbit(dx[dx == 0]).any())               # zeros are +0: the kernel's bit pattern
        assert abs(float((y * g).sum() - (c['x'] * dx).sum())) <= 1e-12 * max(1.0, float((y * g).abs().sum()))
        if not ceil:
            assert bool((interior(dx)[:, 2 * T2:] == 0).all()) and bool((interior(dx)[:, :, 2 * F2:] == 0).all())
    # the tie rule on a window of four equal values, and on a maximum that appears twice
    t = border(torch.tensor([[5.0, 5.0], [5.0, 5.0]], dtype=F64).view(1, 2, 2, 1))
    assert int(interior(pool_ref(t, 1, 1)[1])) == 0
    t = border(torch.tensor([[1.0, 7.0], [7.0, 2.0]], dtype=F64).view(1, 2, 2, 1))
    assert int(interior(pool_ref(t, 1, 1)[1])) == 1


def test_pool_extra_inputs():
    B, T, Fq, C = POOL_EXTRA_CASE
    assert T % 2 == 1 and Fq % 2 == 1
    for kind in POOL_EXTRA_KINDS:
        c = pool_extra_inputs(kind)
        x = interior(c['x'])
        assert torch.equal(bf16(x), x)
        for ceil in (True, False):
            T2, F2 = pool_sizes(T, Fq, ceil)
            y, idx = pool_ref(c['x'], T2, F2)
            yi, ii = interior(y), interior(idx)
            if kind == 'neg_inf':
                assert bool((x == float('-inf')).any()) and bool((yi == float('-inf')).any()) and bool((yi > float('-inf')).any())
                assert bool((ii[yi == float('-inf')] == 0).all())
                assert not bool(torch.isnan(interior(pool_bwd_ref(border(c['g'][:, :T2, :F2]), idx, T, Fq))).any())
                continue
            first = int(kind[3])
            full = ii[:, :T // 2, :Fq // 2]                             # windows that lie inside the image
            assert bool((full == first).all()), kind
            dt, df = POOL_SCAN[first]
            sub = x[:, dt:2 * T2:2, df:2 * F2:2, :]
            assert torch.equal(yi[:, :sub.shape[1], :sub.shape[2]], sub)
            # a scan from the last position down would name the last of the equal maxima instead
            assert first == 3 or bool((x[:, 1:2 * (T // 2):2, 1:2 * (Fq // 2):2, :] == yi[:, :T // 2, :Fq // 2]).all())


def test_pack_unrounded_is_pack_ref_before_rounding():
    g = gen(5)
    w = torch.randn(3, 2, 3, 3, generator=g).to(F64)
    for mode in (0, 1):
        u = pack_unrounded(w, mode)
        assert torch.equal(bf16(u), pack_ref(w, mode, u.shape[1])) and not torch.equal(bf16(u), u)
    assert pack_unrounded(w, 0)[2, 5 * 2 + 1] == w[2, 1, 1, 2] and pack_unrounded(w, 1)[1, 2 * 3 + 2] == w[2, 1, 2, 0]
    wf = w.to(F32)
    back = fold_ref(pack_unrounded(wf, 0), torch.zeros(3, 2, 3, 3))
    assert torch.equal(back, wf)                                       # mode 2 undoes mode 0


def test_stride_cases_pass_the_grid_caps():
    B, T, Fq, C = LN_CASE_BWD_STRIDE
    assert 512 * 1024 < B * T * C < 2 * 512 * 1024 and (B * T * C) % 1024 == 1016 and 8 <= Fq <= 128
    B, T, Fq, C = LN_CASE_FWD_STRIDE
    assert B * T * C > 16384 * 256
    B, T, Fq, C = POOL_CASE_STRIDE
    T2, F2 = pool_sizes(T, Fq, True)
    assert B * T2 * F2 * C > 16384 * 256 and B * T * Fq * C > 16384 * 256
    # the largest case of the common table stays below the fp32 backward's cap: it is the bordered bf16 form that passes it
    B, T, Fq, C = LN_CASES[-1]
    assert B * T * C < 512 * 1024 < B * (T + 2) * C


@pytest.mark.parametrize('case', LN_CASES + [LN_CASE_BWD_STRIDE])
def test_ln_ref_and_gate_band(case):
    """ln_ref against F.layer_norm + autograd in float64; the share of pre-activations within 1e-5 * scale of zero is at most
    0.1 % for the committed seed (elements whose ReLU gate fp32 arithmetic may decide either way), and float32 torch flips a gate
    only inside that band."""
    B, T, Fq, C = case
    c = ln_inputs(case)
    assert B * (T + 2) * C > 2048 * 256 or case != LN_CASES[-1]
    amb = ln_ambiguous(ln_ref(c['x'], c['w'], c['b'], c['dy'], 1)['pre64'])
    assert int(amb.sum()) <= GATE_CAP * amb.numel(), (case, int(amb.sum()))
    pre32 = ln_pre(interior(c['x']), c['w'], c['b'])[0]
    pre64 = ln_pre(interior(c['x']).double(), c['w'].double(), c['b'].double())[0]
    assert not bool((((pre32 > 0) != (pre64 > 0)) & ~amb).any())
    if B * T * Fq * C > 200000:
        return
    for relu in (0, 1):
        r = ln_ref(c['x'], c['w'], c['b'], c['dy'], relu)
        x = interior(c['x']).double().permute(0, 1, 3, 2).clone().requires_grad_(True)          # (B,T,C,F)
        wl, bl = c['w'].double().requires_grad_(True), c['b'].double().requires_grad_(True)
        y = F.layer_norm(x, (Fq,), wl, bl, LN_EPS)
        y = torch.relu(y) if relu else y
        (y * interior(c['dy']).double().permute(0, 1, 3, 2)).sum().backward()
        assert float((interior(r['y']).permute(0, 1, 3, 2) - y.detach()).abs().max()) < 1e-12
        assert float((interior(r['dx']).permute(0, 1, 3, 2) - x.grad).abs().max()) < 1e-9 * max(1.0, float(x.grad.abs().max()))
        assert float((r['dw'] - wl.grad).abs().max()) < 1e-9 and float((r['db'] - bl.grad).abs().max()) < 1e-9
        assert float(r['dcb'].abs().max()) < 1e-9 * max(1.0, float(r['dx'].abs().sum()))          # analytically zero
        m, rs = r['mean'], r['rstd']
        xi = interior(c['x']).double()
        assert float((m - xi.mean(2)).abs().max()) < 1e-12
        assert float((rs - 1 / torch.sqrt(xi.var(2, unbiased=False) + LN_EPS)).abs().max()) < 1e-9 * float(rs.max())


@pytest.mark.parametrize('case', OUTPUT_CASES)
def test_output_ref(case):
    B, T, Fq, C = case
    c = output_inputs(case)
    o = output_ref(c['x'])
    nchw = interior(c['x']).permute(0, 3, 1, 2)                    # the reference model: (B,C,T,F) -> transpose(1,2) -> view(B,T,C*F)
    assert torch.equal(o, nchw.transpose(1, 2).reshape(B, T, C * Fq))
    gb = output_bwd_ref(c['d'], Fq, C)
    assert border_is_zero(gb) and gb.shape == c['x'].shape
    assert torch.equal(output_ref(gb), c['d'])
    assert abs(float((o * c['d']).sum() - (c['x'] * gb).sum())) <= 1e-12 * float((o * c['d']).abs().sum())
