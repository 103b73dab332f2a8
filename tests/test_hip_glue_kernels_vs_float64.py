"""The fp32 glue kernels of the encoder layers and heads (csrc/elementwise.hip: log-softmax and its fused backward, LayerNorm,
activation backward, column sums) and the embedding gradient (asr_embedding_bwd, csrc/decoder.hip) against float64 references.

References (float64 torch / numpy on the CPU, written out below from the kernels' header comments; backward = autograd)
  log-softmax        (x - max) - log sum exp(x - max)                                         pinned to F.log_softmax
  its fused backward autograd of log_softmax(relu(pre)); the kernel is handed act = relu(pre) with exact zeros
  LayerNorm          (x - mean) rstd w + b, biased variance, rstd = 1 / sqrt(var + eps)        pinned to F.layer_norm
  activation bwd     the float32 expression g (1 - o o) / (o > 0 ? g : 0) itself
  column sums        math.fsum per column (float64 numpy sums for the one large case, pinned to fsum)
  embedding gradient float64 index_add_

Conditions on every case: fully written outputs start as NaN, accumulated outputs (dw / db, out / out2, demb) start from random
values and must equal init + contribution, every output buffer carries a 64-element sentinel tail, out2 is also passed as NULL.

Tolerances.  Pointwise kernels: each case measures e32 = max |torch float32 on the CPU - float64| on ITS inputs and bounds the
kernel by K * e32 + FLOOR * scale, FLOOR = 4 * 2^-23, scale = max(1, max |reference|); every case prints a RATIO line before it
asserts.  K is the smallest power of two that clears the worst measured ratio by 2x over the cases whose e32 exceeds one ulp of
scale, capped at 4.  Pure sums: n * 2^-24 * sum |terms| per output element (any summation order of n terms).  asr_act_bwd: 2 ulp
of the float32 expression, where the compiler may or may not contract 1 - o * o into one fused operation (both roundings are
the float32 expression).  ReLU gates of LayerNorm: an element whose float64 pre-activation lies within 1e-5 * scale of zero may
gate either way; it is left out (at most 0.1 % of a case), and what its gate can change in the sums of its row and column
(dx of the row, dw / db of the column) is added to their bounds.

Measured on the MI355X (worst err_kernel / e32 per family over the cases with e32 above one ulp of scale):
  family / output            cases  above   worst ratio at                                   | incl. cases below one ulp
  log_softmax     logp          48      0     -                            (was 43.76, see below) |  3.30
  logsoftmax_relu_bwd dpre      48     16    1.00  R4 V31 x30                                    |  1.67
  layernorm       y             20      7    1.23  n320 R5 offset relu1                          |  1.76
                  mean          20      0     -                                                  |  1.28
                  rstd          20      2    0.02  n320 R5 offset                                |  1.00
                  dx            20      8    0.72  n1024 R5 unit relu1                           |  2.40
                  dw            20     11    1.43  n63 R77 unit relu1      (was 2.48 at n2049)   |  1.43
                  db            20      1    0.60  n2049 R77 unit relu0    (was 1.62)            |  1.90
  act_bwd tanh / relu: 0 ulp from the float32 expression at every n.  Column sums and the embedding gradient stay inside their
  derived bounds (largest error 5.9e-05 on a column of 8193 terms against a bound of 3.1).
"above" counts the cases whose e32 exceeds one ulp of scale; log-probabilities are judged on the scale of the largest |logp| of the
case, so none of the log-softmax cases rises above one ulp there and FLOOR decides.  -> K_LOGSOFTMAX = 2, K_LAYERNORM = 4.

Two findings of this module, fixed in csrc/elementwise.hip; the "was" figures are the same cases before the change:
  log-softmax      x - (m + log(sum)) rounds at ulp(|m|): with unit logits on an offset of 100 the kernel was 43.76x torch's float32
                   error at V = 2 (2.6e-06 against 5.9e-08; 10 - 23x at the other V) and missed its bound at V = 2; the x1 / x30 /
                   x80 cases do not show it, their largest |logp| is as large as |m|.  Now (x - m) - log(sum): 3.30 at worst.
  LayerNorm dw/db  one atomic per row and column: 2.48 on dw at R = 77, which K = 4 does not clear by 2x.  Now the four rows of a
                   workgroup are summed in LDS before one atomic per column.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

ULP32 = 2.0 ** -23
FLOOR = 4 * ULP32
U24 = 2.0 ** -24
K_LOGSOFTMAX = 2
K_LAYERNORM = 4
TAIL = 64
SENT = -777.25
LN_EPS = 1e-5
GATE_BAND = 1e-5
GATE_CAP = 1e-3
ACT_TANH, ACT_RELU = 1, 2
F64, F32 = torch.float64, torch.float32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _out(shape, init=None):
    """Device buffer for an output of `shape`: NaN (the kernel must write all of it) or `init` (the kernel accumulates),
    followed by TAIL sentinel elements."""
    n = math.prod(shape)
    t = torch.full((n + TAIL,), SENT, dtype=F32)
    t[:n] = float('nan') if init is None else init.reshape(-1)
    return t.cuda()


def _back(buf, shape, dtype=F64):
    n = math.prod(shape)
    c = buf.cpu()
    assert (c[n:] == SENT).all(), 'the sentinel tail behind the output was overwritten'
    return c[:n].view(shape).to(dtype)


def _judge(name, what, got, ref64, ref32, K, keep=None, slack=None):
    """keep: elements that are judged (default all); slack: a derived allowance per element added to the bound."""
    keep = torch.ones_like(ref64, dtype=torch.bool) if keep is None else keep
    scale = max(1.0, float(ref64.abs().max()))
    e32 = float((ref32.double() - ref64)[keep].abs().max()) if bool(keep.any()) else 0.0
    assert not torch.isnan(got).any(), '%s %s: NaN left in an output the kernel must write' % (name, what)
    excess = (got - ref64).abs() - (0.0 if slack is None else slack)
    err = max(0.0, float(excess[keep].max())) if bool(keep.any()) else 0.0
    print('RATIO %-36s %-6s err %.3e e32 %.3e ratio %7.2f scale %.3g%s'
          % (name, what, err, e32, err / max(e32, 1e-300), scale, '' if e32 > ULP32 * scale else '  (e32 below one ulp of scale)'))
    assert err <= K * e32 + FLOOR * scale, (name, what, err, e32, scale)


def _judge_sum(name, what, got, ref64, abs_terms, n):
    """A pure sum of n terms in any order: |error| <= n * 2^-24 * sum |terms| per output element (n: a number or one per row)."""
    bound = n * U24 * abs_terms
    err = (got - ref64).abs()
    assert not torch.isnan(got).any(), (name, what)
    print('SUM   %-36s %-6s err %.3e smallest bound %.3e (n <= %d)' % (name, what, float(err.max()), float(bound.min()), int(torch.as_tensor(n).max())))
    assert (err <= bound).all(), (name, what, float(err.max()), float(bound.min()))


# ---------------------------------------------------------------------------------------------------------------------
# log-softmax and the backward of log_softmax(relu(.))
# ---------------------------------------------------------------------------------------------------------------------
def _lsm_ref(x):
    m = x.max(-1, keepdim=True).values.detach()
    return (x - m) - torch.log(torch.exp(x - m).sum(-1, keepdim=True))


LSM_SHAPES = [(1, 1), (3, 2), (4, 31), (5, 63), (77, 64), (1, 65), (3, 1000), (77, 5000), (77, 2), (4, 65), (5, 1000), (5, 5000)]
# logits x 1, x 30, x 80, and unit logits on a common offset of 100 (log-softmax does not depend on the offset; fp32 may)
LSM_SCALES = ['x1', 'x30', 'x80', 'x1+100']


def _lsm_inputs(R, V, scale):
    g = _gen(201)
    x = torch.randn(R, V, generator=g) * {'x1': 1.0, 'x30': 30.0, 'x80': 80.0, 'x1+100': 1.0}[scale]
    if scale == 'x1+100':
        x = x + 100.0
    return x, torch.randn(R, V, generator=g)


@gpu
@pytest.mark.parametrize('scale', LSM_SCALES)
@pytest.mark.parametrize('R,V', LSM_SHAPES)
def test_log_softmax_fwd(R, V, scale):
    """One wave per row, four rows per workgroup (R % 4 of every kind), lanes striding V by 64."""
    from src import hipabi as H
    name = 'log_softmax R%d V%d %s' % (R, V, scale)
    x, _ = _lsm_inputs(R, V, scale)
    xd, out = x.cuda(), _out((R, V))
    H.call('asr_log_softmax', H.ptr(xd), H.ptr(out), R, V, H.stream_ptr())
    torch.cuda.synchronize()
    _judge(name, 'logp', _back(out, (R, V)), _lsm_ref(x.double()), F.log_softmax(x, -1), K_LOGSOFTMAX)


@gpu
@pytest.mark.parametrize('scale', LSM_SCALES)
@pytest.mark.parametrize('R,V', LSM_SHAPES)
def test_logsoftmax_relu_bwd(R, V, scale):
    """dpre = (act > 0) ? dlogp - exp(logp) * rowsum(dlogp) : 0 with act = relu(pre) holding exact zeros; logp is the float64
    log-softmax rounded to fp32, so the case does not depend on the forward kernel."""
    from src import hipabi as H
    name = 'logsoftmax_relu_bwd R%d V%d %s' % (R, V, scale)
    pre, g = _lsm_inputs(R, V, scale)
    if scale == 'x1+100':
        pre = pre - 100.0 * (torch.rand(R, V, generator=_gen(202)) < 0.3)          # a third of the units off
    act = torch.relu(pre)
    assert V < 31 or (bool((act == 0).any()) and bool((act > 0).any()))
    want = []
    for dtype in (F64, F32):
        p = pre.to(dtype).clone().requires_grad_(True)
        lp = _lsm_ref(torch.relu(p)) if dtype == F64 else F.log_softmax(torch.relu(p), -1)
        lp.backward(g.to(dtype))
        want.append((lp.detach(), p.grad))
    gd, lpd, ad = g.cuda(), want[0][0].float().cuda(), act.cuda()
    dpre = _out((R, V))
    H.call('asr_logsoftmax_relu_bwd', H.ptr(gd), H.ptr(lpd), H.ptr(ad), H.ptr(dpre), R, V, H.stream_ptr())
    torch.cuda.synchronize()
    got = _back(dpre, (R, V))
    assert (got[act == 0] == 0).all(), name + ': the gate reads the stored activation, so it is exact'
    _judge(name, 'dpre', got, want[0][1], want[1][1], K_LOGSOFTMAX)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def _ln_ref(x, w, b):
    """float64 LayerNorm over the last axis: pre-activation, mean, rstd."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    return (x - mean) * rstd * w + b, mean, rstd


# (n, R, kind): kind 'unit' = unit-normal rows, 'offset' = row mean 100, standard deviation 0.1
LN_CASES = [(1, 4, 'unit'), (2, 5, 'unit'), (63, 77, 'unit'), (64, 1, 'unit'), (65, 4, 'unit'), (320, 77, 'unit'), (1024, 5, 'unit'),
            (2049, 77, 'unit'), (2049, 1, 'unit'), (320, 5, 'offset')]


def _ln_inputs(n, R, kind):
    g = _gen(203)
    x = torch.randn(R, n, generator=g)
    if kind == 'offset':
        x = x * 0.1 + 100.0
    return dict(x=x, w=1.0 + 0.5 * torch.randn(n, generator=g), b=0.5 * torch.randn(n, generator=g), dy=torch.randn(R, n, generator=g),
                dw0=torch.randn(n, generator=g), db0=torch.randn(n, generator=g))


def _ln_all(c, relu, dtype):
    """Forward and backward in `dtype`; float64 by _ln_ref, float32 by torch's own layer_norm.  The ReLU gate is the float64
    one in both (a 0 / 1 factor), so e32 measures arithmetic and not gates that flipped in float32."""
    x, w, b = [c[k].to(dtype).clone().requires_grad_(True) for k in ('x', 'w', 'b')]
    pre64, mean64, rstd64 = _ln_ref(c['x'].double(), c['w'].double(), c['b'].double())
    if dtype == F64:
        pre, mean, rstd = _ln_ref(x, w, b)
    else:
        pre, mean, rstd = torch.native_layer_norm(x, (x.shape[-1],), w, b, LN_EPS)
    y = pre * (pre64 > 0).to(dtype) if relu else pre
    y.backward(c['dy'].to(dtype))
    stats = torch.cat([mean.detach().view(-1, 1), rstd.detach().view(-1, 1)], 1)
    return dict(y=y.detach(), stats=stats, dx=x.grad, dw=c['dw0'].to(dtype) + w.grad, db=c['db0'].to(dtype) + b.grad, pre64=pre64)


def _ln_ambiguous(pre64):
    amb = pre64.abs() <= GATE_BAND * max(1.0, float(pre64.abs().max()))
    return amb


@gpu
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('n,R,kind', LN_CASES)
def test_layernorm_fwd_bwd(n, R, kind, relu):
    """One wave per row, lanes striding n by 64 (n = 1 and 2: constant and two-point rows; n around one stride; several
    strides), four rows per workgroup.  dw / db are accumulated into non-zero buffers; stats = (mean, rstd) is an output."""
    from src import hipabi as H
    name = 'layernorm n%d R%d %s relu%d' % (n, R, kind, relu)
    c = _ln_inputs(n, R, kind)
    r64, r32 = _ln_all(c, relu, F64), _ln_all(c, relu, F32)
    amb = _ln_ambiguous(r64['pre64']) if relu else torch.zeros(R, n, dtype=torch.bool)
    assert int(amb.sum()) <= GATE_CAP * R * n, (name, int(amb.sum()))
    keep = ~amb
    xd, wd, bd, dyd = [c[k].cuda() for k in ('x', 'w', 'b', 'dy')]
    y, stats = _out((R, n)), _out((R, 2))
    H.call('asr_layernorm_fwd', H.ptr(xd), H.ptr(wd), H.ptr(bd), H.ptr(y), H.ptr(stats), R, n, LN_EPS, relu, H.stream_ptr())
    std = r64['stats'].float().cuda()                      # the backward reads the float64 statistics rounded to fp32
    dx, dw, db = _out((R, n)), _out((n,), c['dw0']), _out((n,), c['db0'])
    H.call('asr_layernorm_bwd', H.ptr(dyd), H.ptr(xd), H.ptr(wd), H.ptr(bd), H.ptr(std), H.ptr(dx), H.ptr(dw), H.ptr(db), R, n, relu,
           H.stream_ptr())
    torch.cuda.synchronize()
    _judge(name, 'y', _back(y, (R, n)), r64['y'], r32['y'], K_LAYERNORM, keep)
    got_stats = _back(stats, (R, 2))
    _judge(name, 'mean', got_stats[:, 0], r64['stats'][:, 0], r32['stats'][:, 0], K_LAYERNORM)
    _judge(name, 'rstd', got_stats[:, 1], r64['stats'][:, 1], r32['stats'][:, 1], K_LAYERNORM)
    # what the gate of an ambiguous element i can change: g_i in db[i], g_i xh_i in dw[i], and through the two row sums
    # rstd (g_i w_i + xh_j g_i w_i xh_i) / n in dx[row, j]
    x64, w64, g64 = c['x'].double(), c['w'].double(), c['dy'].double()
    mean, rstd = r64['stats'][:, :1], r64['stats'][:, 1:]
    xh = (x64 - mean) * rstd
    a = amb.double()
    s_dx = rstd * ((a * (g64 * w64).abs()).sum(-1, keepdim=True) + xh.abs() * (a * (g64 * w64 * xh).abs()).sum(-1, keepdim=True)) / n
    _judge(name, 'dx', _back(dx, (R, n)), r64['dx'], r32['dx'], K_LAYERNORM, keep, s_dx)
    _judge(name, 'dw', _back(dw, (n,)), r64['dw'], r32['dw'], K_LAYERNORM, None, (a * (g64 * xh).abs()).sum(0))
    _judge(name, 'db', _back(db, (n,)), r64['db'], r32['db'], K_LAYERNORM, None, (a * g64.abs()).sum(0))


# ---------------------------------------------------------------------------------------------------------------------
# activation backward
# ---------------------------------------------------------------------------------------------------------------------
def _ulps_apart(a, b):
    """Distance in units in the last place between two float32 arrays (same sign or zero)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def _act_bwd_inputs(n):
    g = _gen(204)
    o = torch.tanh(torch.randn(n, generator=g) * 3)           # outputs of tanh, saturated ones among them
    o[::7] = 0.0
    if n > 2:
        o[1], o[2] = 1.0, -1.0
    return torch.randn(n, generator=g), o


def _act_bwd_allowed(gr, o):
    """g (1 - o o) in float32, with the product o o rounded (three roundings) or fused into the subtraction (two)."""
    g_, o_ = gr.numpy(), o.numpy()
    plain = g_ * (np.float32(1) - o_ * o_)
    fused = g_ * (1.0 - o_.astype(np.float64) ** 2).astype(np.float32)          # o o and 1 - o o are exact in float64
    return plain, fused


@gpu
@pytest.mark.parametrize('n', [1, 255, 257, 4096 * 256 + 3])
def test_act_bwd(n):
    """Grid-stride loop with the grid capped at 4096 workgroups of 256: the last n needs a second trip for three elements."""
    from src import hipabi as H
    gr, o = _act_bwd_inputs(n)
    gd, od = gr.cuda(), o.cuda()
    for act in (ACT_TANH, ACT_RELU):
        dpre = _out((n,))
        H.call('asr_act_bwd', H.ptr(gd), H.ptr(od), H.ptr(dpre), n, act, H.stream_ptr())
        torch.cuda.synchronize()
        got = _back(dpre, (n,), F32).numpy()
        assert not np.isnan(got).any()
        if act == ACT_RELU:
            assert np.array_equal(got, np.where(o.numpy() > 0, gr.numpy(), np.float32(0)))
        else:
            plain, fused = _act_bwd_allowed(gr, o)
            d = np.minimum(_ulps_apart(got, plain), _ulps_apart(got, fused))
            print('ULP   act_bwd tanh n %d: worst distance %d ulp' % (n, int(d.max())))
            assert int(d.max()) <= 2


# ---------------------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------------------
def _colsum_inputs(M, N, lda):
    g = _gen(205)
    A = torch.randn(M, lda, generator=g)
    A[:, N:] = 1.0e6                                          # columns past N belong to somebody else
    return A, torch.randn(N, generator=g), torch.randn(N, generator=g)


def _colsum_run(A, M, N, lda, o1, o2, fn):
    from src import hipabi as H
    Ad = A.cuda()
    b1, b2 = _out((N,), o1), (_out((N,), o2) if o2 is not None else None)
    if fn == 'asr_colsum':
        H.call('asr_colsum', H.ptr(Ad), lda, M, N, H.ptr(b1), H.stream_ptr())
    else:
        H.call('asr_colsum2', H.ptr(Ad), lda, M, N, H.ptr(b1), H.ptr(b2), H.stream_ptr())
    torch.cuda.synchronize()
    return _back(b1, (N,)), (_back(b2, (N,)) if b2 is not None else None)


def _colsum_check(name, A, M, N, lda, exact):
    A_, o1, o2 = A
    a64 = A_[:, :N].double()
    if exact:
        col = torch.tensor([math.fsum(a64[:, j].tolist()) for j in range(N)], dtype=F64)
    else:
        col = torch.from_numpy(a64.numpy().sum(0))
    absum = a64.abs().sum(0)
    for fn, second in (('asr_colsum', None), ('asr_colsum2', o2), ('asr_colsum2', None)):
        g1, g2 = _colsum_run(A_, M, N, lda, o1, second, fn)
        what = fn[4:] + ('' if second is None else '+out2')
        _judge_sum(name, what, g1, o1.double() + col, absum + o1.double().abs(), M + 1)
        if second is not None:
            _judge_sum(name, 'out2', g2, o2.double() + col, absum + o2.double().abs(), M + 1)


@gpu
@pytest.mark.parametrize('M,N', [(1, 1), (3, 63), (16, 64), (17, 65), (33, 200), (513, 65), (513, 1), (17, 200)])
def test_colsum(M, N):
    """Four row groups per workgroup, 16 rows per unrolled trip (M around 16 and 32), 64 columns per workgroup, lda > N;
    out / out2 are accumulated into non-zero vectors, out2 may be NULL."""
    lda = N + 5
    _colsum_check('colsum M%d N%d' % (M, N), _colsum_inputs(M, N, lda), M, N, lda, exact=True)


@gpu
def test_colsum_full_row_blocks():
    """M = 8193, N = 4096: 64 x 17 = 1088 workgroups keep rows_per_block at 512, so every wave runs the four-way unrolled loop
    for 32 trips, and the last row block holds a single row."""
    M, N, lda = 8193, 4096, 4096 + 8
    assert (N + 63) // 64 * ((M + 511) // 512) >= 1024 and (N + 63) // 64 * ((M - 1 + 511) // 512) >= 1024
    _colsum_check('colsum M%d N%d' % (M, N), _colsum_inputs(M, N, lda), M, N, lda, exact=False)


# ---------------------------------------------------------------------------------------------------------------------
# embedding gradient
# ---------------------------------------------------------------------------------------------------------------------
EMB_CASES = [(1, 1, 1, 'same'), (3, 63, 31, 'uniform'), (4, 64, 31, 'absent'), (5, 65, 300, 'uniform'), (257, 200, 31, 'uniform'),
             (257, 64, 31, 'same'), (14336, 65, 31, 'same'), (14336, 63, 300, 'uniform'), (14337, 64, 31, 'same'), (14337, 1, 300, 'absent'),
             (30000, 200, 300, 'uniform'), (30000, 65, 31, 'same'), (30000, 64, 31, 'absent')]


def _emb_inputs(rows, width, V, dist):
    g = _gen(206)
    ld = width + 3
    dy = torch.randn(rows, ld, generator=g)
    dy[:, width:] = 1.0e6                                     # columns past `width` are not part of the rows
    if dist == 'same':
        idx = torch.full((rows,), V - 1, dtype=torch.long)
    else:
        idx = torch.randint(0, V, (rows,), generator=g)
        if dist == 'absent':
            idx[idx == 7] = 8
    return dy, idx, torch.randn(V, width, generator=g), ld


@gpu
@pytest.mark.parametrize('rows,width,V,dist', EMB_CASES)
def test_embedding_bwd(rows, width, V, dist):
    """rows around the four waves' interleave, around 4 x 3584 (the last size with one chunk of position lists - with every row
    on one token the lists are full - and the first with two) and at three chunks; width around one 64-column workgroup;
    dy_ld > width.  demb is accumulated; a token that never occurs leaves its row bit for bit; two runs agree bit for bit."""
    from src import hipabi as H
    name = 'embedding_bwd rows%d w%d V%d %s' % (rows, width, V, dist)
    dy, idx, d0, ld = _emb_inputs(rows, width, V, dist)
    want = d0.double().index_add_(0, idx, dy[:, :width].double())
    absterms = d0.double().abs().index_add_(0, idx, dy[:, :width].double().abs())
    count = torch.bincount(idx, minlength=V)
    dyd, idd = dy.cuda(), idx.cuda()
    runs = []
    for _ in range(2):
        demb = _out((V, width), d0)
        H.call('asr_embedding_bwd', H.ptr(dyd), ld, H.ptr(idd), H.ptr(demb), rows, width, V, H.stream_ptr())
        torch.cuda.synchronize()
        runs.append(_back(demb, (V, width), F32))
    assert torch.equal(runs[0], runs[1]), name + ': two runs on the same inputs must agree bit for bit'
    got = runs[0].double()
    absent = count == 0
    if dist == 'absent':
        assert bool(absent[7]) if V > 7 else True
    assert torch.equal(runs[0][absent], d0[absent]), name + ': the row of a token that does not occur must be unchanged'
    _judge_sum(name, 'demb', got, want, absterms, (count + 1).view(V, 1))          # row v: its count[v] rows of dy and the initial value


# ---------------------------------------------------------------------------------------------------------------------
# the references themselves (CPU, runs everywhere)
# ---------------------------------------------------------------------------------------------------------------------
def test_glue_references_agree():
    # log-softmax against F.log_softmax (float64), its fused backward against the formula the kernel states
    for (R, V) in LSM_SHAPES:
        for scale in LSM_SCALES:
            x, g = _lsm_inputs(R, V, scale)
            assert float((_lsm_ref(x.double()) - F.log_softmax(x.double(), -1)).abs().max()) < 1e-12
            p = (x - 100.0 if scale == 'x1+100' else x).double().requires_grad_(True)
            lp = _lsm_ref(torch.relu(p))
            lp.backward(g.double())
            act = torch.relu(p.detach())
            want = torch.where(act > 0, g.double() - torch.exp(lp.detach()) * g.double().sum(-1, keepdim=True), torch.zeros_like(act))
            assert float((p.grad - want).abs().max()) < 1e-12 * max(1.0, float(want.abs().max()))
    # LayerNorm against F.layer_norm, statistics against torch.native_layer_norm; float32 torch alone flips fewer gates than the cap
    for (n, R, kind) in LN_CASES:
        c = _ln_inputs(n, R, kind)
        x, w, b = [c[k].double() for k in ('x', 'w', 'b')]
        pre, mean, rstd = _ln_ref(x, w, b)
        ref, m2, r2 = torch.native_layer_norm(x, (n,), w, b, LN_EPS)
        assert float((pre - F.layer_norm(x, (n,), w, b, LN_EPS)).abs().max()) < 1e-12
        assert float((mean - m2).abs().max()) < 1e-12 and float(((rstd - r2) / rstd).abs().max()) < 1e-12
        if kind == 'offset':
            assert float((x.mean(-1) - 100).abs().max()) < 0.05 and float((x.std(-1) - 0.1).abs().max()) < 0.02
        pre32 = F.layer_norm(c['x'], (n,), c['w'], c['b'], LN_EPS)
        flips = int(((pre32 > 0) != (pre > 0)).sum())
        amb = _ln_ambiguous(pre)
        assert flips <= GATE_CAP * R * n and int(amb.sum()) <= GATE_CAP * R * n, (n, R, kind, flips, int(amb.sum()))
        assert not bool((((pre32 > 0) != (pre > 0)) & ~amb).any())          # float32 flips only inside the band
        for relu in (0, 1):
            r64 = _ln_all(c, relu, F64)
            xl, wl, bl = [c[k].double().clone().requires_grad_(True) for k in ('x', 'w', 'b')]
            y = F.layer_norm(xl, (n,), wl, bl, LN_EPS)
            y = torch.relu(y) if relu else y
            y.backward(c['dy'].double())
            assert float((r64['y'] - y.detach()).abs().max()) < 1e-12
            assert float((r64['dx'] - xl.grad).abs().max()) < 1e-9 * max(1.0, float(xl.grad.abs().max()))
            assert float((r64['dw'] - c['dw0'].double() - wl.grad).abs().max()) < 1e-10
            assert float((r64['db'] - c['db0'].double() - bl.grad).abs().max()) < 1e-10
    # activation backward: the float32 expression against autograd of tanh / relu in float64
    gr, o = _act_bwd_inputs(257)
    plain, fused = _act_bwd_allowed(gr, o)
    xs = torch.atanh(o.double().clamp(-1 + 1e-12, 1 - 1e-12)).requires_grad_(True)
    torch.tanh(xs).backward(gr.double())
    inner = (o.abs() < 1).numpy()
    for v in (plain, fused):
        assert np.abs(v.astype(np.float64) - xs.grad.numpy())[inner].max() < 4 * 2.0 ** -24 * 4
    assert _ulps_apart(np.float32([1.0, -1.0, 0.0]), np.float32([1.0 + 2.0 ** -23, -1.0 - 2.0 ** -22, -0.0])).tolist() == [1, 2, 0]
    # column sums: float64 numpy sums against fsum; embedding gradient: index_add_ against a loop
    A, _, _ = _colsum_inputs(513, 65, 70)
    a64 = A[:, :65].double()
    fs = np.array([math.fsum(a64[:, j].tolist()) for j in range(65)])
    assert np.abs(a64.numpy().sum(0) - fs).max() < 1e-12
    for (rows, width, V, dist) in [(257, 64, 31, 'same'), (257, 200, 31, 'uniform'), (4, 64, 31, 'absent'), (14337, 1, 300, 'absent')]:
        dy, idx, d0, ld = _emb_inputs(rows, width, V, dist)
        want = d0.double().index_add_(0, idx, dy[:, :width].double())
        loop = d0.double().clone()
        for r in range(rows):
            loop[idx[r]] += dy[r, :width].double()
        assert float((want - loop).abs().max()) < 1e-11
        assert ld > width and (dist != 'absent' or not bool((idx == 7).any())) and (dist != 'same' or bool((idx == V - 1).all()))
    assert 4 * 3584 == 14336
