"""The variant kernels (csrc/variants.hip: masked softmax, location-aware energy and convolution, LSTM / GRU cells, the GRU
sequence kernels) against float64 references, at the sizes where their strided loops, chunks and clamps change behaviour.

References (float64 torch on the CPU, written out below from the kernels' header comments; backward = autograd of the forward)
  masked softmax   exp(e / temp - max) / sum over t < min(len, T), 0 beyond          pinned to torch.softmax on -inf-masked rows
  location energy  sum_d wg[d] tanh(key + q + tanh(loc_pre)) + bg
  location conv    sum_h sum_j W[k, h, j] prev[b, h, t + j - Ks] over an unfolded, zero-padded prev      pinned to F.conv1d
  cells            oracle.lstm_cell / gru_cell; the two pre-activation halves go in as its two biases (zero weights), so the
                   oracle sees exactly the fp32 numbers the kernel does                    pinned to nn.LSTMCell / nn.GRUCell
  GRU sequence     y: oracle.bigru on float64 parameters (identity input weights, so gi is its input projection); saved
                   activations and gradients: _gru_seq_ref, which must reproduce the oracle's y          pinned to nn.GRU

Conditions on every case: fully written outputs start as NaN, accumulated outputs start from random values and must equal
init + contribution, every output buffer carries a 64-element sentinel tail, optional pointers are also passed as NULL.

Tolerances.  Each case measures e32 = max |torch float32 on the CPU - float64| on ITS inputs and bounds the kernel by
K * e32 + FLOOR * scale, FLOOR = 4 * 2^-23, scale = max(1, max |reference|); every case prints a RATIO line (err_kernel / e32)
before it asserts.  K is one constant per kernel family: the smallest power of two that clears the worst measured ratio by
2x over the cases whose e32 exceeds one ulp of scale, capped at 4 for single-step kernels and at 8 for the GRU sequence and
asr_loc_energy_bwd.  Pure sums (dbg, dW of the convolution) get a derived bound instead: n * 2^-24 * sum |terms| per element.

Measured on the MI355X (worst err_kernel / e32 per family over the cases with e32 above one ulp of scale; cases / worst case):
  family / output            cases  above   worst ratio at                                   | incl. cases below one ulp
  masked softmax  attn          16      1    0.32  T700 NH4 temp8 x30                            |  2.09
                  denergy       16      2    0.69  T257 NH1 temp0.5 x30                          |  3.14
  loc_energy_fwd  energy         8      0     -                                                  |  1.10
  loc_energy_bwd  dkey           8      0     -                                                  |  1.05
                  dq             8      4    1.75  T70 D300 NH1                                  |  1.75
                  dloc_pre       8      0     -                                                  |  1.29
                  dwg            8      2    1.64  T33 D257 NH3                                  |  2.32
  loc_conv        out           10      3    1.13  Ks50 T65 Kn1 NH2 B2     (was 3.04, see below) |  1.13
                  dprev         10      3    0.72  Ks50 T130 Kn10 NH2 B1   (was 3.94)            |  2.14
  lstm_cell       h / c / act   48      1    1.00  N5 D257 x1 (c)                                | 15.54
                  dg / dc_prev  96      8    1.00  N3 D85 x1                                     |  7.48
  gru_cell        h / saved     32      1    0.75  N2 D1024 x1                                   |  2.29
                  dgi/dgh/dh_p  48      1    1.00  N5 D257 x1 (dgh)                              |  1.36
  gru_seq         y             12      7    0.80  H100 T9 ND2 B3          (was 2.95 at H2048)   |  6.54
                  saved         12      7    0.88  H100 T9 ND2 B3          (was 3.26 at H1025)   |  9.12
                  dgi           12      9    1.91  H2048 T3 ND2 B1         (was 12.99)           |  7.54
                  dgh           12      7    1.57  H2048 T3 ND2 B1         (was 8.17 at H1024)   |  6.47
"above" counts the cases whose e32 exceeds one ulp of scale; the last column is the worst ratio over all cases, where a kernel
error far below one ulp is divided by whatever smaller fraction of an ulp torch's float32 landed on (15.54: 1.6e-08 against 1.0e-09) and
FLOOR decides.  -> K_SOFTMAX = 2, K_LOC_ENERGY_FWD = 1, K_LOC_ENERGY_BWD = 4, K_LOC_CONV = 4, K_CELL = 2, K_GRU_SEQ = 4.

Two findings of this module, fixed in csrc/variants.hip; the "was" figures are the same cases before the change:
  GRU sequence     h W_hh^T (H terms) and dgh W_hh (3H terms) were summed in ONE fp32 accumulator: 12.99 on dgi at H = 2048
                   (7.7e-06 against 5.9e-07), above the cap of 8.  Now blocks of 64 terms on four accumulators (dot_blocked).
  location conv    the taps of all filter rows went through one accumulator: 3.94 on dprev at 101 taps x 10 filters, which K = 4
                   does not clear by 2x.  Now one partial sum per filter row on four accumulators (taps_sum).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import asr_oracle as O

gpu = pytest.mark.gpu

ULP32 = 2.0 ** -23
FLOOR = 4 * ULP32
U24 = 2.0 ** -24
K_SOFTMAX = 2
K_LOC_ENERGY_FWD = 1
K_LOC_ENERGY_BWD = 4
K_LOC_CONV = 4
K_CELL = 2
K_GRU_SEQ = 4
TAIL = 64
SENT = -777.25
INF = float('inf')
F64, F32 = torch.float64, torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# buffers and the judge
# ---------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _out(shape, init=None):
    """Device buffer for an output of `shape`: NaN (the kernel must write all of it) or `init` (the kernel accumulates),
    followed by TAIL sentinel elements."""
    n = math.prod(shape)
    t = torch.full((n + TAIL,), SENT, dtype=F32)
    t[:n] = float('nan') if init is None else init.reshape(-1)
    return t.cuda()


def _back(buf, shape):
    n = math.prod(shape)
    c = buf.cpu()
    assert (c[n:] == SENT).all(), 'the sentinel tail behind the output was overwritten'
    return c[:n].view(shape).double()


def _judge(name, what, got, ref64, ref32, K):
    scale = max(1.0, float(ref64.abs().max()))
    e32 = float((ref32.double() - ref64).abs().max())
    assert not torch.isnan(got).any(), '%s %s: NaN left in an output the kernel must write' % (name, what)
    err = float((got - ref64).abs().max())
    print('RATIO %-34s %-9s err %.3e e32 %.3e ratio %7.2f scale %.3g%s'
          % (name, what, err, e32, err / max(e32, 1e-300), scale, '' if e32 > ULP32 * scale else '  (e32 below one ulp of scale)'))
    assert err <= K * e32 + FLOOR * scale, (name, what, err, e32, scale)


def _judge_sum(name, what, got, ref64, abs_terms, n):
    """A pure sum of n terms in any order: |error| <= n * 2^-24 * sum |terms| per output element."""
    bound = n * U24 * abs_terms
    err = (got - ref64).abs()
    assert not torch.isnan(got).any(), (name, what)
    print('SUM   %-34s %-9s err %.3e bound %.3e (n = %d)' % (name, what, float(err.max()), float(bound.min()), n))
    assert (err <= bound).all(), (name, what, float(err.max()), float(bound.min()))


# ---------------------------------------------------------------------------------------------------------------------
# masked softmax
# ---------------------------------------------------------------------------------------------------------------------
def _msm_ref(e, lens, NH, temp, dtype):
    """(leaf energies, attn) : attn[r, t] = softmax_t(e[r, t] / temp) over t < min(len[r / NH], T), 0 beyond; a row of
    length 0 is all zeros."""
    x = e.to(dtype).clone().requires_grad_(True)
    R, T = x.shape
    L = lens.clamp(max=T).repeat_interleave(NH)
    mask = torch.arange(T).view(1, T) < L.view(R, 1)
    xs = (x / temp).masked_fill(~mask, -INF)
    m = xs.detach().max(-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    w = torch.exp(xs - m)
    s = w.sum(-1, keepdim=True)
    return x, w / torch.where(s > 0, s, torch.ones_like(s)), mask


MSM_CASES = [(1, 1, 1.0, 1), (37, 2, 0.5, 1), (256, 4, 8.0, 30), (257, 1, 0.5, 30), (700, 2, 1.0, 1), (700, 4, 8.0, 30),
             (257, 4, 1.0, 1), (256, 1, 0.5, 1)]


def _msm_lens(T, which):
    return torch.tensor([T, 1, 0] if which == 'full_one_zero' else [T + 9, 0, max(1, T // 2)])


def _msm_inputs(T, NH, scale):
    g = _gen(101)
    return torch.randn(3 * NH, T, generator=g) * scale, torch.randn(3 * NH, T, generator=g)


@gpu
@pytest.mark.parametrize('lens', ['full_one_zero', 'above_zero_half'])
@pytest.mark.parametrize('T,NH,temp,scale', MSM_CASES)
def test_masked_softmax_fwd_bwd(T, NH, temp, scale, lens):
    """T on both sides of the 256-thread stride and past two trips of it; lengths T, 1, 0 and above T; rows of every head
    share their utterance's length."""
    from src import hipabi as H
    name = 'masked_softmax T%d NH%d temp%g x%d %s' % (T, NH, temp, scale, lens[:4])
    ln = _msm_lens(T, lens)
    e, dattn = _msm_inputs(T, NH, scale)
    R = 3 * NH
    x64, a64, mask = _msm_ref(e, ln, NH, temp, F64)
    x32, a32, _ = _msm_ref(e, ln, NH, temp, F32)
    a64.backward(dattn.double())
    a32.backward(dattn)
    ed, ld = e.cuda(), ln.cuda()
    attn = _out((R, T))
    H.call('asr_masked_softmax_fwd', H.ptr(ed), H.ptr(ld), R, NH, T, temp, H.ptr(attn), H.stream_ptr())
    de = _out((R, T))
    gd = dattn.cuda()
    H.call('asr_masked_softmax_bwd', H.ptr(attn), H.ptr(gd), R, T, temp, H.ptr(de), H.stream_ptr())
    torch.cuda.synchronize()
    got_a, got_de = _back(attn, (R, T)), _back(de, (R, T))
    assert (got_a[~mask] == 0).all(), name + ': attention beyond the length must be exactly 0'
    assert (got_de[~mask] == 0).all(), name + ': d energy beyond the length must be exactly 0'
    for b in range(3):
        if int(ln[b]) == 0:
            assert (got_a[b * NH:(b + 1) * NH] == 0).all() and (a64[b * NH:(b + 1) * NH] == 0).all()
    _judge(name, 'attn', got_a, a64.detach(), a32.detach(), K_SOFTMAX)
    _judge(name, 'denergy', got_de, x64.grad, x32.grad, K_SOFTMAX)


# ---------------------------------------------------------------------------------------------------------------------
# location-aware energy
# ---------------------------------------------------------------------------------------------------------------------
def _le_fwd(key, q, loc, wg, bg, NH):
    """energy[r, t] = sum_d wg[d] tanh(key[r, t, d] + q[r, d] + tanh(loc_pre[r / NH, t, d])) + bg"""
    u = torch.tanh(key + q.unsqueeze(1) + torch.tanh(loc).repeat_interleave(NH, 0))
    return (u * wg).sum(-1) + bg


def _le_inputs(B, NH, T, D):
    g = _gen(102)
    R = B * NH
    return dict(key=torch.randn(R, T, D, generator=g), q=torch.randn(R, D, generator=g), loc=torch.randn(B, T, D, generator=g),
                wg=torch.randn(D, generator=g) / math.sqrt(D), bg=torch.randn(1, generator=g), de=torch.randn(R, T, generator=g),
                dkey0=torch.randn(R, T, D, generator=g), dwg0=torch.randn(D, generator=g), dbg0=torch.randn(1, generator=g))


def _le_leaves(c, dtype):
    return [c[k].to(dtype).clone().requires_grad_(True) for k in ('key', 'q', 'loc', 'wg', 'bg')]


LE_FWD_CASES = [(1, 1, 1), (3, 63, 3), (4, 64, 1), (5, 65, 3), (33, 300, 1), (33, 64, 3), (5, 300, 3), (4, 1, 3)]


@gpu
@pytest.mark.parametrize('T,D,NH', LE_FWD_CASES)
def test_loc_energy_fwd(T, D, NH):
    """One wave per (row, frame), four frames per workgroup (T % 4 of every kind), lanes striding D by 64 (D below, at and
    above one stride, and several)."""
    from src import hipabi as H
    B = 2
    name = 'loc_energy_fwd T%d D%d NH%d' % (T, D, NH)
    c = _le_inputs(B, NH, T, D)
    with torch.no_grad():
        e64, e32 = _le_fwd(*_le_leaves(c, F64), NH), _le_fwd(*_le_leaves(c, F32), NH)
    d = {k: c[k].cuda() for k in ('key', 'q', 'loc', 'wg', 'bg')}
    en = _out((B * NH, T))
    H.call('asr_loc_energy_fwd', H.ptr(d['key']), H.ptr(d['q']), H.ptr(d['loc']), H.ptr(d['wg']), H.ptr(d['bg']), B, NH, T, D, H.ptr(en),
           H.stream_ptr())
    torch.cuda.synchronize()
    _judge(name, 'energy', _back(en, (B * NH, T)), e64, e32, K_LOC_ENERGY_FWD)


LE_BWD_CASES = [(1, 1, 1), (31, 255, 3), (32, 256, 1), (33, 257, 3), (70, 300, 1), (70, 256, 3), (32, 1, 3), (33, 300, 1)]


@gpu
@pytest.mark.parametrize('T,D,NH', LE_BWD_CASES)
def test_loc_energy_bwd(T, D, NH):
    """Chunks of 32 frames (T below, at, above one chunk and three chunks), 256 threads striding D.  dkey / dwg / dbg are
    accumulated into non-zero buffers, dq is zeroed by the callee, dloc_pre is written as the sum over the heads."""
    from src import hipabi as H
    B = 2
    R = B * NH
    name = 'loc_energy_bwd T%d D%d NH%d' % (T, D, NH)
    c = _le_inputs(B, NH, T, D)
    grads = {}
    for dtype in (F64, F32):
        leaves = _le_leaves(c, dtype)
        _le_fwd(*leaves, NH).backward(c['de'].to(dtype))
        gk, gq, gl, gw, gb = [t.grad for t in leaves]
        grads[dtype] = dict(dkey=c['dkey0'].to(dtype) + gk, dq=gq, dloc=gl, dwg=c['dwg0'].to(dtype) + gw, dbg=c['dbg0'].to(dtype) + gb)
    d = {k: c[k].cuda() for k in ('key', 'q', 'loc', 'wg', 'de')}
    dkey, dq, dloc = _out((R, T, D), c['dkey0']), _out((R, D)), _out((B, T, D))
    dwg, dbg = _out((D,), c['dwg0']), _out((1,), c['dbg0'])
    H.call('asr_loc_energy_bwd', H.ptr(d['key']), H.ptr(d['q']), H.ptr(d['loc']), H.ptr(d['wg']), H.ptr(d['de']), B, NH, T, D,
           H.ptr(dkey), H.ptr(dq), H.ptr(dloc), H.ptr(dwg), H.ptr(dbg), H.stream_ptr())
    torch.cuda.synchronize()
    g64, g32 = grads[F64], grads[F32]
    _judge(name, 'dkey', _back(dkey, (R, T, D)), g64['dkey'], g32['dkey'], K_LOC_ENERGY_BWD)
    _judge(name, 'dq', _back(dq, (R, D)), g64['dq'], g32['dq'], K_LOC_ENERGY_BWD)
    _judge(name, 'dloc_pre', _back(dloc, (B, T, D)), g64['dloc'], g32['dloc'], K_LOC_ENERGY_BWD)
    _judge(name, 'dwg', _back(dwg, (D,)), g64['dwg'], g32['dwg'], K_LOC_ENERGY_BWD)
    terms = c['de'].double().abs().sum() + c['dbg0'].double().abs()
    _judge_sum(name, 'dbg', _back(dbg, (1,)), g64['dbg'], terms, R * T + 1)


# ---------------------------------------------------------------------------------------------------------------------
# location convolution
# ---------------------------------------------------------------------------------------------------------------------
def _lc_windows(prev, Ks):
    """(B, NH, T, 2 Ks + 1): windows[b, h, t, j] = prev[b, h, t + j - Ks], 0 outside [0, T)."""
    return F.pad(prev, (Ks, Ks)).unfold(-1, 2 * Ks + 1, 1)


def _lc_fwd(prev, W, Ks):
    """out[b, t, k] = sum_h sum_j W[k, h, j] prev[b, h, t + j - Ks]"""
    return torch.einsum('bhtj,khj->btk', _lc_windows(prev, Ks), W)


def _lc_inputs(Ks, T, Kn, NH, B):
    g = _gen(103)
    taps = 2 * Ks + 1
    return dict(prev=torch.rand(B, NH, T, generator=g), W=torch.randn(Kn, NH, taps, generator=g) / math.sqrt(NH * min(taps, T)),
                dout=torch.randn(B, T, Kn, generator=g), dW0=torch.randn(Kn, NH, taps, generator=g))


# (Ks, T, Kn, NH, B): B*T*Kn / B*NH*T = 257/257, 280/56, 133/266, 640/64, 130/260, 2600/260, 2600/260, 1920/384, 130/26, 260/260
LC_CASES = [(0, 1, 1, 1, 257), (1, 7, 10, 2, 4), (50, 7, 1, 2, 19), (50, 64, 10, 1, 1), (50, 65, 1, 2, 2), (1, 130, 10, 1, 2),
            (50, 130, 10, 2, 1), (0, 64, 10, 2, 3), (50, 1, 10, 2, 13), (1, 65, 1, 1, 4)]


@gpu
@pytest.mark.parametrize('Ks,T,Kn,NH,B', LC_CASES)
def test_loc_conv_fwd_bwd(Ks, T, Kn, NH, B):
    """A single tap, the shipped 101 taps and T < Ks (every tap clamp active at once); element counts on both sides of one
    256-thread workgroup; T on both sides of the weight gradient's 64-frame stride.  dW is accumulated; dprev may be NULL."""
    from src import hipabi as H
    taps = 2 * Ks + 1
    name = 'loc_conv Ks%d T%d Kn%d NH%d B%d' % (Ks, T, Kn, NH, B)
    c = _lc_inputs(Ks, T, Kn, NH, B)
    res = {}
    for dtype in (F64, F32):
        prev, W = [c[k].to(dtype).clone().requires_grad_(True) for k in ('prev', 'W')]
        out = _lc_fwd(prev, W, Ks)
        out.backward(c['dout'].to(dtype))
        res[dtype] = (out.detach(), prev.grad, c['dW0'].to(dtype) + W.grad)
    pd, Wd, dod = c['prev'].cuda(), c['W'].cuda(), c['dout'].cuda()
    out = _out((B, T, Kn))
    H.call('asr_loc_conv_fwd', H.ptr(pd), H.ptr(Wd), B, NH, T, Kn, Ks, H.ptr(out), H.stream_ptr())
    dprev, dW, dW_only = _out((B, NH, T)), _out((Kn, NH, taps), c['dW0']), _out((Kn, NH, taps), c['dW0'])
    H.call('asr_loc_conv_bwd', H.ptr(dod), H.ptr(pd), H.ptr(Wd), B, NH, T, Kn, Ks, H.ptr(dprev), H.ptr(dW), H.stream_ptr())
    H.call('asr_loc_conv_bwd', H.ptr(dod), H.ptr(pd), H.ptr(Wd), B, NH, T, Kn, Ks, None, H.ptr(dW_only), H.stream_ptr())
    torch.cuda.synchronize()
    _judge(name, 'out', _back(out, (B, T, Kn)), res[F64][0], res[F32][0], K_LOC_CONV)
    _judge(name, 'dprev', _back(dprev, (B, NH, T)), res[F64][1], res[F32][1], K_LOC_CONV)
    # dW[k, h, j] = dW0 + sum over (b, t) of dout * prev: B * T + 1 terms in some order, each product rounded once more
    absterms = torch.einsum('bhtj,btk->khj', _lc_windows(c['prev'].double(), Ks), c['dout'].double().abs()) + c['dW0'].double().abs()
    got_dW = _back(dW, (Kn, NH, taps))
    _judge_sum(name, 'dW', got_dW, res[F64][2], absterms, B * T + 2)
    assert torch.equal(_back(dW_only, (Kn, NH, taps)), got_dW), name + ': dW must not depend on dprev being NULL'


# ---------------------------------------------------------------------------------------------------------------------
# LSTM / GRU cells
# ---------------------------------------------------------------------------------------------------------------------
CELL_SHAPES = [(1, 1), (3, 85), (5, 257), (2, 1024)]


def _cell_inputs(N, D, gates, sat):
    g = _gen(104)
    gx, gh = torch.randn(N, gates * D, generator=g), torch.randn(N, gates * D, generator=g)
    if sat:                                                   # saturated gates: pre-activations around +-30
        gh = gh + 30.0 * (torch.randint(0, 2, (N, gates * D), generator=g) * 2 - 1)
    return dict(gx=gx, gh=gh, prev=torch.randn(N, D, generator=g), dh=torch.randn(N, D, generator=g), dc=torch.randn(N, D, generator=g))


def _lstm_cell_ref(gx, gh, c_prev, dtype):
    """h, c and the gate activations (i | f | g | o) of nn.LSTM's cell on the pre-activation halves gx + gh.  h and c come from
    oracle.lstm_cell, row by row, with gx[n] / gh[n] as its two biases and zero weights."""
    N, D4 = gx.shape
    D = D4 // 4
    bx, bh = gx.to(dtype).clone().requires_grad_(True), gh.to(dtype).clone().requires_grad_(True)
    cp = (c_prev.to(dtype) if c_prev is not None else torch.zeros(N, D, dtype=dtype)).clone().requires_grad_(True)
    zx, zh, x0, h0 = torch.zeros(D4, 1, dtype=dtype), torch.zeros(D4, D, dtype=dtype), torch.zeros(1, 1, dtype=dtype), torch.zeros(1, D, dtype=dtype)
    hs, cs = zip(*[O.lstm_cell(x0, h0, cp[n:n + 1], zx, zh, bx[n], bh[n]) for n in range(N)])
    i, f, gg, o = (bx + bh).detach().chunk(4, -1)
    act = torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)], -1)
    return bx, bh, cp, torch.cat(hs), torch.cat(cs), act


def _gru_cell_ref(gi, gh, h_prev, dtype):
    """h and the saved activations (r | z | n | gh_n) of nn.GRU's cell; h from oracle.gru_cell with gi[n] / gh[n] as its biases
    and zero weights (so only the direct z * h_prev path reaches h_prev, which is what dh_prev of the kernel is)."""
    N, D3 = gi.shape
    D = D3 // 3
    bx, bh = gi.to(dtype).clone().requires_grad_(True), gh.to(dtype).clone().requires_grad_(True)
    hp = (h_prev.to(dtype) if h_prev is not None else torch.zeros(N, D, dtype=dtype)).clone().requires_grad_(True)
    zx, zh, x0 = torch.zeros(D3, 1, dtype=dtype), torch.zeros(D3, D, dtype=dtype), torch.zeros(1, 1, dtype=dtype)
    h = torch.cat([O.gru_cell(x0, hp[n:n + 1], zx, zh, bx[n], bh[n]) for n in range(N)])
    xr, xz, xn = bx.detach().chunk(3, -1)
    hr, hz, hn = bh.detach().chunk(3, -1)
    r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
    saved = torch.cat([r, z, torch.tanh(xn + r * hn), hn], -1)
    return bx, bh, hp, h, saved


@gpu
@pytest.mark.parametrize('with_prev', [True, False])
@pytest.mark.parametrize('sat', [False, True])
@pytest.mark.parametrize('N,D', CELL_SHAPES)
def test_lstm_cell_fwd_bwd(N, D, sat, with_prev):
    """One thread per (n, d), 256 per workgroup: one element, sizes that are no multiple of 256, more than one workgroup.  The
    backward runs with dh alone, dc alone and both; c_prev may be NULL."""
    from src import hipabi as H
    name = 'lstm_cell N%d D%d %s %s' % (N, D, 'sat' if sat else 'x1', 'prev' if with_prev else 'null')
    c = _cell_inputs(N, D, 4, sat)
    prev = c['prev'] if with_prev else None
    gxd, ghd, pd = c['gx'].cuda(), c['gh'].cuda(), (prev.cuda() if with_prev else None)
    act, h, cn = _out((N, 4 * D)), _out((N, D)), _out((N, D))
    H.call('asr_lstm_cell_fwd', H.ptr(gxd), H.ptr(ghd), H.ptr(pd), N, D, H.ptr(act), H.ptr(h), H.ptr(cn), H.stream_ptr())
    torch.cuda.synchronize()
    r64, r32 = _lstm_cell_ref(c['gx'], c['gh'], prev, F64), _lstm_cell_ref(c['gx'], c['gh'], prev, F32)
    _judge(name, 'h', _back(h, (N, D)), r64[3].detach(), r32[3].detach(), K_CELL)
    _judge(name, 'c', _back(cn, (N, D)), r64[4].detach(), r32[4].detach(), K_CELL)
    _judge(name, 'act', _back(act, (N, 4 * D)), r64[5], r32[5], K_CELL)
    for mode in ('dh', 'dc', 'both'):
        want = []
        for dtype in (F64, F32):
            bx, bh, cp, hh, cc, _ = _lstm_cell_ref(c['gx'], c['gh'], prev, dtype)
            loss = (hh * c['dh'].to(dtype)).sum() * (mode != 'dc') + (cc * c['dc'].to(dtype)).sum() * (mode != 'dh')
            loss.backward()
            assert torch.equal(bx.grad, bh.grad)
            want.append((bx.grad, cp.grad))
        dhd = c['dh'].cuda() if mode != 'dc' else None
        dcd = c['dc'].cuda() if mode != 'dh' else None
        dg, dcp = _out((N, 4 * D)), _out((N, D))
        H.call('asr_lstm_cell_bwd', H.ptr(act), H.ptr(pd), H.ptr(cn), H.ptr(dhd), H.ptr(dcd), N, D, H.ptr(dg), H.ptr(dcp), H.stream_ptr())
        torch.cuda.synchronize()
        _judge(name, 'dg/' + mode, _back(dg, (N, 4 * D)), want[0][0], want[1][0], K_CELL)
        _judge(name, 'dc_prev/' + mode, _back(dcp, (N, D)), want[0][1], want[1][1], K_CELL)


@gpu
@pytest.mark.parametrize('with_prev', [True, False])
@pytest.mark.parametrize('sat', [False, True])
@pytest.mark.parametrize('N,D', CELL_SHAPES)
def test_gru_cell_fwd_bwd(N, D, sat, with_prev):
    from src import hipabi as H
    name = 'gru_cell N%d D%d %s %s' % (N, D, 'sat' if sat else 'x1', 'prev' if with_prev else 'null')
    c = _cell_inputs(N, D, 3, sat)
    prev = c['prev'] if with_prev else None
    gid, ghd, pd, dhd = c['gx'].cuda(), c['gh'].cuda(), (prev.cuda() if with_prev else None), c['dh'].cuda()
    saved, h = _out((N, 4 * D)), _out((N, D))
    H.call('asr_gru_cell_fwd', H.ptr(gid), H.ptr(ghd), H.ptr(pd), N, D, H.ptr(saved), H.ptr(h), H.stream_ptr())
    dgi, dgh, dhp = _out((N, 3 * D)), _out((N, 3 * D)), _out((N, D))
    H.call('asr_gru_cell_bwd', H.ptr(saved), H.ptr(pd), H.ptr(dhd), N, D, H.ptr(dgi), H.ptr(dgh), H.ptr(dhp), H.stream_ptr())
    torch.cuda.synchronize()
    want = []
    for dtype in (F64, F32):
        bx, bh, hp, hh, sv = _gru_cell_ref(c['gx'], c['gh'], prev, dtype)
        hh.backward(c['dh'].to(dtype))
        want.append((hh.detach(), sv, bx.grad, bh.grad, hp.grad))
    for i, (what, buf, shape) in enumerate((('h', h, (N, D)), ('saved', saved, (N, 4 * D)), ('dgi', dgi, (N, 3 * D)), ('dgh', dgh, (N, 3 * D)),
                                            ('dh_prev', dhp, (N, D)))):
        _judge(name, what, _back(buf, shape), want[0][i], want[1][i], K_CELL)


# ---------------------------------------------------------------------------------------------------------------------
# GRU over a sequence
# ---------------------------------------------------------------------------------------------------------------------
def _gru_seq_inputs(H_, T, ND, B):
    g = _gen(105)
    k = 1.0 / math.sqrt(H_)
    return dict(gi=torch.randn(B, T, ND, 3 * H_, generator=g), whh=(torch.rand(ND, 3 * H_, H_, generator=g) * 2 - 1) * k,
                bhh=(torch.rand(ND, 3 * H_, generator=g) * 2 - 1) * k, dy=torch.randn(B, T, ND * H_, generator=g))


def _gru_seq_ref(gi, whh, bhh, dtype):
    """nn.GRU (batch_first, zero initial state, direction 1 reversed) on the input projections gi (B, T, ND, 3H):
    gh_t = h_{t-1} W_hh^T + b_hh, r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n), h_t = (1 - z) n + z h_{t-1}.
    Returns the leaves (gi, eh) - eh is a zero added to gh, so its gradient is d loss / d gh - and y (B, T, ND*H), saved
    (B, T, ND, 4H) = r | z | n | gh_n."""
    B, T, ND, G = gi.shape
    Hd = G // 3
    x = gi.to(dtype).clone().requires_grad_(True)
    eh = torch.zeros(B, T, ND, G, dtype=dtype, requires_grad=True)
    W, bias = whh.to(dtype), bhh.to(dtype)
    ys, svs = [], []
    for d in range(ND):
        h = torch.zeros(B, Hd, dtype=dtype)
        out, sv = [None] * T, [None] * T
        for t in (range(T - 1, -1, -1) if d else range(T)):
            gh = h @ W[d].t() + bias[d] + eh[:, t, d]
            xr, xz, xn = x[:, t, d].chunk(3, -1)
            hr, hz, hn = gh.chunk(3, -1)
            r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
            n = torch.tanh(xn + r * hn)
            h = (1 - z) * n + z * h
            out[t], sv[t] = h, torch.cat([r, z, n, hn], -1)
        ys.append(torch.stack(out, 1))
        svs.append(torch.stack(sv, 1))
    return x, eh, torch.cat(ys, -1), torch.stack(svs, 2)


def _gru_oracle_y(gi, whh, bhh):
    """oracle.bigru on float64 parameters: identity input weights and a zero input bias make gi its input projection."""
    B, T, ND, G = gi.shape
    eye, zero = torch.eye(G, dtype=F64), torch.zeros(G, dtype=F64)
    P, ys = {}, []
    for d in range(ND):
        sfx = '_reverse' if d else ''
        P.update({'weight_ih_l0' + sfx: eye, 'weight_hh_l0' + sfx: whh[d].double(), 'bias_ih_l0' + sfx: zero, 'bias_hh_l0' + sfx: bhh[d].double()})
    if ND == 1:
        return O.bigru(gi[:, :, 0].double(), P, '', bidirection=False)
    # the two directions of the kernel have inputs of their own (gi[:, :, d]); bigru feeds one x to both
    return torch.cat([O.gru_direction(gi[:, :, d].double(), P['weight_ih_l0' + s], P['weight_hh_l0' + s], P['bias_ih_l0' + s], P['bias_hh_l0' + s], bool(d))
                      for d, s in ((0, ''), (1, '_reverse'))], -1)


# (H, T, ND, B)
GRU_SEQ_CASES = [(1, 1, 1, 1), (1, 9, 2, 3), (16, 2, 2, 3), (16, 9, 1, 1), (100, 9, 2, 3), (100, 1, 1, 3), (1024, 3, 1, 1), (1024, 3, 2, 3),
                 (1025, 3, 2, 1), (1025, 3, 1, 3), (2048, 3, 2, 1), (2048, 3, 1, 3)]


@gpu
@pytest.mark.parametrize('Hd,T,ND,B', GRU_SEQ_CASES)
def test_gru_sequence_fwd_bwd(Hd, T, ND, B):
    """1024 threads own one or two hidden units each: H = 1024 is the last size with one, 1025 has a single thread in its second
    trip, 2048 every thread (and is the limit).  T = 1 has no recurrence, T >= 2 carries h forward and dh backward; the carried
    gradient shows in dgi / dgh of the earlier frames."""
    from src import hipabi as H
    name = 'gru_seq H%d T%d ND%d B%d' % (Hd, T, ND, B)
    c = _gru_seq_inputs(Hd, T, ND, B)
    want = []
    for dtype in (F64, F32):
        x, eh, y, sv = _gru_seq_ref(c['gi'], c['whh'], c['bhh'], dtype)
        y.backward(c['dy'].to(dtype))
        want.append((y.detach(), sv.detach(), x.grad, eh.grad))
    with torch.no_grad():
        y_oracle = _gru_oracle_y(c['gi'], c['whh'], c['bhh'])
    assert float((y_oracle - want[0][0]).abs().max()) < 1e-13
    gid, whhd, whhTd, bhhd, dyd = c['gi'].cuda(), c['whh'].cuda(), c['whh'].transpose(1, 2).contiguous().cuda(), c['bhh'].cuda(), c['dy'].cuda()
    y, saved = _out((B, T, ND * Hd)), _out((B, T, ND, 4 * Hd))
    H.call('asr_gru_fwd', H.ptr(gid), H.ptr(whhTd), H.ptr(bhhd), B, T, Hd, ND, H.ptr(y), H.ptr(saved), H.stream_ptr())
    dgi, dgh = _out((B, T, ND, 3 * Hd)), _out((B, T, ND, 3 * Hd))
    H.call('asr_gru_bwd', H.ptr(dyd), H.ptr(y), H.ptr(saved), H.ptr(whhd), B, T, Hd, ND, H.ptr(dgi), H.ptr(dgh), H.stream_ptr())
    torch.cuda.synchronize()
    _judge(name, 'y', _back(y, (B, T, ND * Hd)), y_oracle, want[1][0], K_GRU_SEQ)
    for i, (what, buf, shape) in enumerate((('saved', saved, (B, T, ND, 4 * Hd)), ('dgi', dgi, (B, T, ND, 3 * Hd)), ('dgh', dgh, (B, T, ND, 3 * Hd)))):
        _judge(name, what, _back(buf, shape), want[0][i + 1], want[1][i + 1], K_GRU_SEQ)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: argument checks that return before any launch
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_before_launch():
    from src import hipabi as H
    t = torch.full((64,), 3.0, device='cuda')
    ln = torch.zeros(4, dtype=torch.long, device='cuda')
    p, sp = H.ptr(t), H.stream_ptr()
    bad = [('asr_gru_fwd', (p, p, p, 1, 1, 2049, 1, p, p, sp), 'above 2048'),
           ('asr_gru_bwd', (p, p, p, p, 1, 1, 2049, 1, p, p, sp), 'above 2048'),
           ('asr_masked_softmax_fwd', (p, H.ptr(ln), 3, 2, 4, 1.0, p, sp), 'bad args'),          # rows % NH != 0
           ('asr_masked_softmax_fwd', (p, H.ptr(ln), 4, 2, 4, 0.0, p, sp), 'bad args'),          # temperature <= 0
           ('asr_masked_softmax_fwd', (p, H.ptr(ln), 4, 2, 4, -1.0, p, sp), 'bad args'),
           ('asr_masked_softmax_bwd', (p, p, 4, 4, 0.0, p, sp), 'bad args')]
    for fn, args, msg in bad:
        assert getattr(H.lib(), fn)(*args) != 0, fn
        assert msg in H.lib().asr_last_error().decode(), (fn, H.lib().asr_last_error())
        with pytest.raises(RuntimeError):
            H.call(fn, *args)
    torch.cuda.synchronize()
    assert (t == 3.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# the references themselves (CPU, runs everywhere)
# ---------------------------------------------------------------------------------------------------------------------
def test_variant_references_agree():
    g = _gen(7)
    # masked softmax against torch.softmax on -inf-masked energies, rows with len >= 1; a row of length 0 is zeros
    for (T, NH, temp, scale) in MSM_CASES:
        for which in ('full_one_zero', 'above_zero_half'):
            ln = _msm_lens(T, which)
            e, dattn = _msm_inputs(T, NH, scale)
            x, a, mask = _msm_ref(e, ln, NH, temp, F64)
            a.backward(dattn.double())
            x2 = e.double().clone().requires_grad_(True)
            rows = mask.any(-1)
            a2 = torch.softmax((x2 / temp).masked_fill(~mask, -INF)[rows], -1)
            a2.backward(dattn.double()[rows])
            assert float((a.detach()[rows] - a2.detach()).abs().max()) < 1e-15
            assert float((x.grad[rows] - x2.grad[rows]).abs().max()) < 1e-14
            assert (a.detach()[~rows] == 0).all() and (x.grad[~rows] == 0).all() and (x.grad[~mask] == 0).all()
        both = set(_msm_lens(T, 'full_one_zero').tolist()) | set(_msm_lens(T, 'above_zero_half').tolist())
        assert {T, 1, 0} <= both and max(both) > T
    # location energy against oracle.loc_attention_step's energy expression written with a matrix product
    c = _le_inputs(2, 3, 5, 65)
    k, q, l, w, b = [c[n].double() for n in ('key', 'q', 'loc', 'wg', 'bg')]
    u = torch.tanh(k + q.unsqueeze(1) + torch.tanh(l).repeat_interleave(3, 0))
    assert float((_le_fwd(k, q, l, w, b, 3) - ((u @ w.view(-1, 1)).squeeze(-1) + b)).abs().max()) < 1e-14
    # location convolution against F.conv1d(padding=Ks), T < Ks included
    for (Ks, T, Kn, NH, B) in LC_CASES:
        c = _lc_inputs(Ks, T, Kn, NH, B)
        prev, W = c['prev'].double().requires_grad_(True), c['W'].double().requires_grad_(True)
        p2, W2 = c['prev'].double().requires_grad_(True), c['W'].double().requires_grad_(True)
        out, out2 = _lc_fwd(prev, W, Ks), F.conv1d(p2, W2, padding=Ks).transpose(1, 2)
        out.backward(c['dout'].double())
        out2.backward(c['dout'].double())
        assert out.shape == (B, T, Kn) and float((out - out2).detach().abs().max()) < 1e-13
        assert float((prev.grad - p2.grad).abs().max()) < 1e-13 and float((W.grad - W2.grad).abs().max()) < 1e-12
    # cells: oracle.lstm_cell / gru_cell against nn.LSTMCell / nn.GRUCell in float64, then the bias-fed form used above
    N, D, Din = 3, 5, 4
    x, h0, c0 = [torch.randn(N, n, generator=g, dtype=F64) for n in (Din, D, D)]
    lstm, gru = torch.nn.LSTMCell(Din, D).double(), torch.nn.GRUCell(Din, D).double()
    with torch.no_grad():
        hn, cn = lstm(x, (h0, c0))
        ho, co = O.lstm_cell(x, h0, c0, lstm.weight_ih, lstm.weight_hh, lstm.bias_ih, lstm.bias_hh)
        assert float((hn - ho).abs().max()) < 1e-15 and float((cn - co).abs().max()) < 1e-15
        assert float((gru(x, h0) - O.gru_cell(x, h0, gru.weight_ih, gru.weight_hh, gru.bias_ih, gru.bias_hh)).abs().max()) < 1e-15
        gx, gh = x @ lstm.weight_ih.t() + lstm.bias_ih, h0 @ lstm.weight_hh.t() + lstm.bias_hh
    _, _, _, hr, cr, act = _lstm_cell_ref(gx, gh, c0, F64)
    assert float((hr - hn).abs().max()) < 1e-15 and float((cr - cn).abs().max()) < 1e-15
    assert float((act[:, 3 * D:] * torch.tanh(cr) - hr).abs().max()) < 1e-15          # h = o tanh(c): the saved gates are the cell's
    assert float((act[:, D:2 * D] * c0 + act[:, :D] * act[:, 2 * D:3 * D] - cr).abs().max()) < 1e-15
    with torch.no_grad():
        gi, gh = x @ gru.weight_ih.t() + gru.bias_ih, h0 @ gru.weight_hh.t() + gru.bias_hh
        hn = gru(x, h0)
    _, _, _, hr, sv = _gru_cell_ref(gi, gh, h0, F64)
    assert float((hr - hn).abs().max()) < 1e-15
    assert float(((1 - sv[:, D:2 * D]) * sv[:, 2 * D:3 * D] + sv[:, D:2 * D] * h0 - hr).abs().max()) < 1e-15
    assert torch.equal(sv[:, 3 * D:], gh[:, 2 * D:])
    # GRU sequence: _gru_seq_ref against nn.GRU (float64, bidirectional) and against the oracle
    for (Hd, T, ND, B) in [(16, 9, 2, 3), (5, 4, 1, 2), (1, 3, 2, 1)]:
        rnn = torch.nn.GRU(Din, Hd, batch_first=True, bidirectional=(ND == 2)).double()
        x = torch.randn(B, T, Din, generator=g, dtype=F64)
        sfx = ['', '_reverse'][:ND]
        with torch.no_grad():
            gi = torch.stack([x @ getattr(rnn, 'weight_ih_l0' + s).t() + getattr(rnn, 'bias_ih_l0' + s) for s in sfx], 2)
            whh = torch.stack([getattr(rnn, 'weight_hh_l0' + s) for s in sfx])
            bhh = torch.stack([getattr(rnn, 'bias_hh_l0' + s) for s in sfx])
            want = rnn(x)[0]
            P = {k: v.detach() for k, v in rnn.named_parameters()}
            assert float((O.bigru(x, P, '', ND == 2) - want).abs().max()) < 1e-14
            assert float((_gru_oracle_y(gi, whh, bhh) - want).abs().max()) < 1e-14
        xl, eh, y, sv = _gru_seq_ref(gi, whh, bhh, F64)
        assert float((y - want).abs().max()) < 1e-14
        dy = torch.randn(B, T, ND * Hd, generator=g, dtype=F64)
        y.backward(dy)
        # d loss / d gh differs from d loss / d gi in the n block alone, by the factor r
        r = sv[..., :Hd].detach()
        assert float((eh.grad[..., :2 * Hd] - xl.grad[..., :2 * Hd]).abs().max()) < 1e-15
        assert float((eh.grad[..., 2 * Hd:] - xl.grad[..., 2 * Hd:] * r).abs().max()) < 1e-15
        # and d loss / d gi reaches nn.GRU's input gradient through the input projection
        x2 = x.clone().requires_grad_(True)
        rnn(x2)[0].backward(dy)
        dx = sum(xl.grad[:, :, d] @ getattr(rnn, 'weight_ih_l0' + s).detach() for d, s in enumerate(sfx))
        assert float((dx - x2.grad).abs().max()) < 1e-13
