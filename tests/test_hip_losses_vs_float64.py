"""The kernels that turn model outputs into a loss, its gradient and a parameter update (csrc/ctc.hip, csrc/xent.hip,
csrc/optim.hip) against float64 references, at the shapes and edges where they can go wrong.

References
  CTC            torch.nn.functional.ctc_loss on float64 log-probs (reduction='none') + autograd; the small edge cases also
                 against oracle.asr_oracle.ctc_nll_restated (textbook lattice), and the two against each other on the CPU.
  sequence loss  F.cross_entropy(ignore_index=0) / oracle label_smoothing_loss on float64 logits.
  optimizer      clip_grad_norm_ + torch.optim.Adadelta written out in float64; math.fsum for the sum of squares.

Tolerances.  fp32 log-space has an error floor that grows with |nll|, so no constant fits every case.  Each case measures
e32 = max |torch float32 - float64| on ITS inputs (a reference-only quantity) and bounds the kernel by K * e32 + FLOOR, FLOOR =
4 ulp of 1.0 in fp32; gradients are compared with their normalisation removed (CTC: grad * B * max(tl,1) / gscale, sequence
loss: dlogits * counted rows / gscale) so every case lives on the [-1, 1] scale.  NLL / loss: relative error, same form.
K covers the kernel's arithmetic (CTC: __expf / __logf and the three-way log-sum-exp) set against libm.  Every case prints a
RATIO line with err_kernel / e32 before it asserts.  K is the smallest power of two that clears the worst measured ratio by 2x,
within the caps K_CTC <= 8 and K_XENT <= 4 - a ratio that needs more is a finding about the kernel, not a reason to widen.

Measured on the MI355X (err_kernel / e32; gradient on the unit scale | nll relative):
  CTC case                  grad err   e32        ratio | nll err    e32        ratio
  multichunk_ragged         5.539e-03  5.555e-03  1.00  | 7.883e-07  7.883e-07  1.00
  multichunk_single         1.690e-03  1.508e-03  1.12  | 5.880e-07  5.880e-07  1.00
  large_vocab_V1918         6.266e-03  6.146e-03  1.02  | 6.648e-07  5.934e-07  1.12
  large_vocab_V1919         7.045e-03  6.975e-03  1.01  | 1.093e-06  1.093e-06  1.00
  large_vocab_V2046         3.258e-03  3.278e-03  0.99  | 4.169e-07  4.169e-07  1.00
  large_vocab_V2047         5.306e-03  5.166e-03  1.03  | 9.790e-07  9.790e-07  1.00
  large_vocab_V5000         6.591e-03  6.459e-03  1.02  | 1.469e-06  1.469e-06  1.00
  vocab_limit_V15333        6.722e-06  8.546e-06  0.79  | 7.757e-08  7.757e-08  1.00
  launch_limit_L511         1.355e-03  1.542e-03  0.88  | 2.928e-07  3.014e-07  0.97
  edges (both references)   1.530e-05  1.786e-05  0.86  | 1.310e-07  1.310e-07  1.00
  all_repeat (both)         3.859e-06  4.521e-06  0.85  | 9.647e-08  9.647e-08  1.00
  medium_gscale0.3          1.161e-04  1.325e-04  0.88  | 1.055e-07  1.055e-07  1.00
  edges_gscale0.3           1.529e-05  1.786e-05  0.86  | 1.310e-07  1.310e-07  1.00
  multichunk_gscale0.3      5.539e-03  5.555e-03  1.00  | 7.883e-07  7.883e-07  1.00
  loss_fn_gout2.5           1.161e-04  1.325e-04  0.88  | (nll not returned by the wrapper)
Worst CTC ratio 1.12 -> K_CTC = 4.

  sequence loss (160 cases)  grad err max  e32 range          ratio max | loss err max  ratio max
  mode 0, logits x 1         1.33e-07      4.1e-08..1.3e-07   2.69      | 6.74e-08      11.35
  mode 0, logits x 30        2.77e-07      6.4e-08..2.7e-07   1.30      | 7.68e-08       1.02
  mode 0, logits x 80        1.52e-07      3.5e-08..1.5e-07   1.33      | 5.08e-08       1.14
  mode 1, logits x 1         1.66e-07      4.3e-08..1.4e-07   3.04      | 1.21e-07      56.42
  mode 1, logits x 30        8.41e-07      5.0e-08..4.8e-06   1.98      | 1.16e-07       2.00
  mode 1, logits x 80        5.99e-07      6.6e-08..4.8e-06   1.42      | 5.19e-08       1.35
Most of these cases live inside FLOOR: the kernel's error is about one ulp of 1.0 (the loss is a float32 number: 1.2e-07 relative is
one rounding) and the ratio divides it by whatever fraction of an ulp torch's float32 happened to land on (1.8e-09 in the 56.42
case), which says nothing about either side.  Over the cases whose e32 exceeds one ulp of 1.0 - where the ratio does measure
arithmetic - the worst is 1.30 on the gradient (56 cases) and 1.00 on the loss (17 cases) -> K_XENT = 4, the cap.
Before the kernel formed log-softmax as (x - m) - log(sum) it measured 26.3 on the gradient at V = 2, logits x 30 (1.7e-06 against
6.4e-08): m + log(sum) rounded at ulp(|m|).  That was a finding of this module and is fixed in csrc/xent.hip.

Optimizer tolerances are derived, not measured: see _adadelta_tol and test_sumsq_vs_fsum.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import asr_oracle as O

gpu = pytest.mark.gpu

ULP32 = 2.0 ** -23
FLOOR = 4 * ULP32
K_CTC = 4
K_XENT = 4
INF = float('inf')


# ---------------------------------------------------------------------------------------------------------------------
# CTC
# ---------------------------------------------------------------------------------------------------------------------
def _sweep_chunk_frames(L, V):
    """CF of asr_ctc_loss: frames of log-probs staged per chunk beside the lattice buffers in 60 KB."""
    smax = 2 * L + 1
    fixed = (smax + 2) * 4 + 2 * (smax + 6) * 4 + 16
    return (60 * 1024 - fixed) // (4 * V)


def _sweep_waves(L):
    return (L + 1 + 63) // 64 + (L + 63) // 64


def _grad_boundary_vocab(L, budget=64 * 1024):
    """Largest V whose 8 frames of class sums (+ per-wave blank sums) fit `budget` bytes of dynamic LDS: 64 KiB is what a launch
    can get, 60 KB is where asr_ctc_loss starts to halve the frames per workgroup."""
    return budget // (8 * 4) - _sweep_waves(L)


def _labels(g, n, V, repeats=()):
    t = torch.randint(1, V, (n,), generator=g)
    for i in repeats:
        t[i + 1] = t[i]
    return t


def _n_repeats(lab):
    return int((lab[1:] == lab[:-1]).sum()) if len(lab) > 1 else 0


def _ctc_inputs(seed, B, T, V, L, tl, il, scale=1.0, repeats=None):
    g = torch.Generator().manual_seed(seed)
    lp = torch.log_softmax(torch.randn(B, T, V, generator=g) * scale, -1)
    txt = torch.zeros(B, L, dtype=torch.long)
    for b in range(B):
        txt[b, :tl[b]] = _labels(g, tl[b], V, (repeats or {}).get(b, ()))
    return dict(lp=lp, txt=txt, il=torch.tensor(il), tl=torch.tensor(tl))


def _case_multichunk(tail):
    B, T, V, L = 4, 1500, 31, 400
    CF = _sweep_chunk_frames(L, V)
    assert 1 < CF < T // 3
    tl = [400, 1, 200, 0]
    # 'ragged': ~4 chunks forward, ragged ends backward; 'single': the last chunk of every row is one frame
    il = [1500, 900, 1499, 700] if tail == 'ragged' else [2 * CF + 1, CF + 1, 3 * CF + 1, CF + 1]
    c = _ctc_inputs(21, B, T, V, L, tl, il)
    c['CF'] = CF
    return c


def _case_large_vocab(V):
    return _ctc_inputs(22, 3, 700, V, 60, [60, 17, 33], [700, 300, 650])


def _case_launch_limit():
    return _ctc_inputs(23, 3, 1023, 31, 511, [511, 300, 511], [1023, 640, 900])


def _case_medium():
    return _ctc_inputs(24, 3, 120, 31, 40, [40, 7, 25], [120, 60, 100], scale=2.0, repeats={0: (3, 4, 20)})


# rows of the mixed edge batch (V = 5, T = 44, L = 19)
EDGE_ROWS = ['tl0', 'tl0_il0', 'il0', 'minimal', 'plain', 'infeasible', 'short', 'one_frame']


def _case_edges():
    B, T, V, L = len(EDGE_ROWS), 44, 5, 19
    tl = [0, 0, 4, 6, 10, 10, 3, 1]
    c = _ctc_inputs(25, B, T, V, L, tl, [0] * B, scale=1.5, repeats={3: (1, 3), 5: (2,)})
    rep = [_n_repeats(c['txt'][b, :tl[b]]) for b in range(B)]
    assert rep[3] >= 2
    # 'minimal': exactly tl + repeats frames, one valid path; 'infeasible': one frame fewer than that
    c['il'] = torch.tensor([30, 0, 0, tl[3] + rep[3], 44, tl[5] + rep[5] - 1, 20, 1])
    return c


def _case_all_repeat():
    """V = 2: every label is 1, so every label-to-label move needs the blank between.  tl = 19: il = 37 is the single path."""
    B, T, V, L = 3, 40, 2, 19
    c = _ctc_inputs(26, B, T, V, L, [19, 19, 0], [37, 40, 40])
    assert (c['txt'][:2] == 1).all()
    return c


def _ctc_torch(c, dtype):
    """(nll (B), d nll_b / d lp (B,T,V)) from torch on the CPU in `dtype`."""
    lp = c['lp'].detach().to(dtype).clone().requires_grad_(True)
    nll = F.ctc_loss(lp.transpose(0, 1), c['txt'], c['il'], c['tl'], blank=0, reduction='none', zero_infinity=False)
    nll.sum().backward()
    return nll.detach().double(), lp.grad.double()


def _ctc_restated(c):
    B, T, V = c['lp'].shape
    nll, grad = torch.zeros(B, dtype=torch.float64), torch.zeros(B, T, V, dtype=torch.float64)
    for b in range(B):
        il, tl = int(c['il'][b]), int(c['tl'][b])
        if il == 0:
            nll[b] = 0.0 if tl == 0 else INF
            continue
        n, g = O.ctc_nll_restated(c['lp'][b, :il].double().numpy(), c['txt'][b, :tl].numpy())
        nll[b] = float(n)
        grad[b, :il] = torch.from_numpy(g)
    return nll, grad


def _feasible(nll64):
    return torch.isfinite(nll64)


def _max_abs(a, b, rows):
    return float((a[rows] - b[rows]).abs().max()) if bool(rows.any()) else 0.0


def _max_rel(a, b, rows):
    rows = rows & (b != 0)
    return float(((a[rows] - b[rows]).abs() / b[rows].abs()).max()) if bool(rows.any()) else 0.0


def _ctc_kernel(c, gscale=1.0):
    from src import hipabi as Hh
    lp, txt = c['lp'], c['txt']
    B, T, V = lp.shape
    L = txt.shape[1]
    assert int(txt.min()) >= 0 and int(txt.max()) < V
    nll = torch.empty(B, device='cuda')
    loss = torch.empty((), device='cuda')
    grad = torch.full((B, T, V), 7.0, device='cuda')
    nb = Hh.lib().asr_ctc_loss_workspace_bytes(B, T, L)
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    lpd, txd, ild, tld = lp.contiguous().cuda(), txt.cuda(), c['il'].cuda(), c['tl'].cuda()
    Hh.call('asr_ctc_loss', Hh.ptr(lpd), Hh.ptr(txd), Hh.ptr(ild), Hh.ptr(tld), Hh.ptr(nll), Hh.ptr(loss), Hh.ptr(grad),
            B, T, V, L, gscale, Hh.ptr(ws), nb, Hh.stream_ptr())
    torch.cuda.synchronize()
    return nll.cpu().double(), float(loss), grad.cpu().double()


def _unit(grad, c, gscale):
    B = grad.shape[0]
    return grad * (B * c['tl'].clamp(min=1).double() / gscale).view(B, 1, 1)


def _judge_ctc(name, c, nll_k, loss_k, unit_k, ref=None):
    """Kernel results (gradient on the unit scale) against float64, bounded by K_CTC x torch float32's own error."""
    nll64, g64 = ref if ref is not None else _ctc_torch(c, torch.float64)
    nll32, g32 = _ctc_torch(c, torch.float32)
    ok = _feasible(nll64)
    B, T, V = g64.shape
    # structure first: which rows are infeasible, what lies past the input length
    assert torch.equal(torch.isinf(nll_k) & (nll_k > 0), ~ok), (name, nll_k, nll64)
    past = torch.arange(T).view(1, T) >= c['il'].view(B, 1)
    assert (unit_k[past] == 0).all(), name + ': gradient past input_len must be exactly 0'
    assert (g64[past] == 0).all()
    for b in range(B):
        il = int(c['il'][b])
        if not ok[b]:
            assert torch.isnan(unit_k[b, :il]).all(), name + ': infeasible row %d: NaN for t < input_len' % b
            assert torch.isnan(g64[b, :il]).all()
    zero = ok & (nll64 == 0)
    assert (nll_k[zero] == 0).all()
    e32_g, e32_n = _max_abs(g32, g64, ok), _max_rel(nll32, nll64, ok)
    err_g, err_n = _max_abs(unit_k, g64, ok), _max_rel(nll_k, nll64, ok)
    print('RATIO ctc %-28s grad err %.3e e32 %.3e ratio %6.2f | nll rel err %.3e e32 %.3e ratio %6.2f'
          % (name, err_g, e32_g, err_g / max(e32_g, 1e-300), err_n, e32_n, err_n / max(e32_n, 1e-300)))
    assert err_g <= K_CTC * e32_g + FLOOR, (name, err_g, e32_g)
    assert err_n <= K_CTC * e32_n + FLOOR, (name, err_n, e32_n)
    # scalar loss = mean_b nll_b / max(tl_b, 1)
    want = float((nll64 / c['tl'].clamp(min=1).double()).mean())
    if math.isfinite(want):
        w32 = float((nll32 / c['tl'].clamp(min=1).double()).mean())
        assert abs(loss_k - want) <= (K_CTC * abs(w32 - want) / max(abs(want), 1e-300) + FLOOR) * abs(want), (name, loss_k, want)
    else:
        assert loss_k == want, (name, loss_k, want)
    return err_g, e32_g


@gpu
@pytest.mark.parametrize('tail', ['ragged', 'single'])
def test_ctc_multichunk_both_sweeps(tail):
    """T = 1500 with 801 states: ~4 staged chunks in each sweep.  The loss comes from the alpha sweep alone; only the gradient
    sees the beta sweep's chunk arithmetic (reversed frame order, ragged first chunk)."""
    c = _case_multichunk(tail)
    assert int(c['il'].max()) > 2 * c['CF']
    if tail == 'single':
        assert all(int(i) % c['CF'] == 1 for i in c['il'])
    nll, loss, grad = _ctc_kernel(c)
    _judge_ctc('multichunk_' + tail, c, nll, loss, _unit(grad, c, 1.0))


@gpu
@pytest.mark.parametrize('which', ['switch_below', 'switch_above', 'below', 'above', '5000'])
def test_ctc_large_vocab(which):
    """Word / subword vocabularies: on both sides of the V where the gradient kernel goes from 8 to 4 frames per workgroup, on
    both sides of the V where 8 frames of class sums pass 64 KiB, and far past it (2 frames)."""
    vb, vs = _grad_boundary_vocab(60), _grad_boundary_vocab(60, 60 * 1024)
    V = {'switch_below': vs, 'switch_above': vs + 1, 'below': vb, 'above': vb + 1, '5000': 5000}[which]
    c = _case_large_vocab(V)
    nll, loss, grad = _ctc_kernel(c)
    _judge_ctc('large_vocab_V%d' % V, c, nll, loss, _unit(grad, c, 1.0))


@gpu
def test_ctc_vocab_limit():
    """The largest V the sweep can stage (one frame beside the lattice buffers in 60 KB) is served and matches float64; one more
    class comes back as ASR_E_UNSUPPORTED with the limit in the message."""
    L = 1
    vmax = (60 * 1024 - ((2 * L + 3) * 4 + 2 * (2 * L + 7) * 4 + 16)) // 4
    assert _sweep_chunk_frames(L, vmax) == 1 and _sweep_chunk_frames(L, vmax + 1) == 0
    c = _ctc_inputs(27, 2, 6, vmax, L, [1, 1], [6, 3])
    nll, loss, grad = _ctc_kernel(c)
    _judge_ctc('vocab_limit_V%d' % vmax, c, nll, loss, _unit(grad, c, 1.0))
    for V in (vmax + 1, 20000):
        c = _ctc_inputs(27, 1, 2, V, L, [1], [2])
        with pytest.raises(RuntimeError) as ei:
            _ctc_kernel(c)
        msg = str(ei.value)
        assert 'asr_ctc_loss failed (-3)' in msg and 'V=%d' % V in msg and 'at most V=%d' % vmax in msg, msg


@gpu
def test_ctc_launch_limit():
    """L = 511: 1023 states, 16 waves, the largest workgroup the sweep can launch."""
    c = _case_launch_limit()
    nll, loss, grad = _ctc_kernel(c)
    _judge_ctc('launch_limit_L511', c, nll, loss, _unit(grad, c, 1.0))


@gpu
@pytest.mark.parametrize('case', ['edges', 'all_repeat'])
def test_ctc_edge_rows(case):
    """Empty targets, empty inputs, frames past input_len, a single valid path, an infeasible row between feasible ones, and the
    V = 2 all-repeat target - each row against BOTH float64 references."""
    c = _case_edges() if case == 'edges' else _case_all_repeat()
    ref = _ctc_torch(c, torch.float64)
    nll_r, g_r = _ctc_restated(c)
    ok = _feasible(ref[0])
    assert torch.equal(ok, _feasible(nll_r))
    assert _max_abs(g_r, ref[1], ok) < 1e-12 and _max_rel(nll_r, ref[0], ok) < 1e-13
    nll, loss, grad = _ctc_kernel(c)
    if case == 'edges':
        assert [bool(x) for x in ok] == [r != 'il0' and r != 'infeasible' for r in EDGE_ROWS]
        assert nll[EDGE_ROWS.index('tl0_il0')] == 0 and nll[EDGE_ROWS.index('il0')] == INF
        assert loss == INF
    _judge_ctc(case, c, nll, loss, _unit(grad, c, 1.0), ref)
    _judge_ctc(case + '_vs_restated', c, nll, loss, _unit(grad, c, 1.0), (nll_r, g_r))


@gpu
@pytest.mark.parametrize('case', ['medium', 'edges', 'multichunk'])
def test_ctc_gscale(case):
    c = {'medium': _case_medium, 'edges': _case_edges, 'multichunk': lambda: _case_multichunk('ragged')}[case]()
    nll, loss, grad = _ctc_kernel(c, gscale=0.3)
    _judge_ctc(case + '_gscale0.3', c, nll, loss, _unit(grad, c, 0.3))


@gpu
def test_ctc_loss_fn_upstream_scale():
    """CTCLossFn under a non-unit upstream gradient that lives on the device (the loss mix: total = w * ctc + ...)."""
    from src import functions as F_hip
    c = _case_medium()
    w = torch.tensor(2.5, device='cuda')
    lpd = c['lp'].cuda().requires_grad_(True)
    out = F_hip.CTCLossFn.apply(lpd, c['txt'].cuda(), c['il'].cuda(), c['tl'].cuda())
    (out * w).backward()
    torch.cuda.synchronize()
    nll64, _ = _ctc_torch(c, torch.float64)
    # nll is not returned by the wrapper: judge the gradient and the scalar loss, with the float64 nll standing in
    unit = _unit(lpd.grad.cpu().double(), c, 2.5)
    _judge_ctc('loss_fn_gout2.5', c, nll64.clone(), float(out.detach()), unit)


# ---------------------------------------------------------------------------------------------------------------------
# sequence losses
# ---------------------------------------------------------------------------------------------------------------------
def _xent_inputs(seed, B, L, ld, V, scale, all_pad=False):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B * L, V, generator=g) * scale
    tgt = torch.randint(1, V, (B, ld), generator=g)           # columns >= L hold other labels: wrong addressing shows
    tgt[:, :L][torch.rand(B, L, generator=g) < 0.3] = 0       # pad targets interleaved
    tgt[0, 0] = V - 1                                         # the last class is used
    if all_pad:
        tgt[:, :L] = 0
    return logits, tgt


def _xent_classes(V):
    return 31 if V in (31, 1000) else V


def _xent_ref(logits, tgt, L, mode, classes, dtype):
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    t = tgt[:, :L].reshape(-1)
    loss = F.cross_entropy(x, t, ignore_index=0) if mode == 0 else O.label_smoothing_loss(x, t, classes, 0.1)
    loss.backward()
    return float(loss.detach()), x.grad.double()


def _xent_kernel(logits, tgt, B, L, V, mode, classes, gscale=1.0):
    from src import hipabi as Hh
    ld = tgt.shape[1]
    xd, td = logits.contiguous().cuda(), tgt.contiguous().cuda()
    dl = torch.full((B * L, V), 7.0, device='cuda')
    loss = torch.empty((), device='cuda')
    acc = torch.empty(4, device='cuda')
    Hh.call('asr_xent', Hh.ptr(xd), Hh.ptr(td), ld, Hh.ptr(dl), Hh.ptr(loss), Hh.ptr(acc), B, L, V, mode, classes, 0.1, gscale,
            Hh.stream_ptr())
    torch.cuda.synchronize()
    return loss.cpu(), dl.cpu().double()


def _xent_cases():
    out = []
    for (B, L, ld) in [(1, 77, 77), (5, 13, 13), (5, 13, 40)]:
        for V in (2, 31, 64, 65, 1000, 5003):
            for scale in (1, 30, 80):
                out.append((B, L, ld, V, scale, 1.0))
            out.append((B, L, ld, V, 1, 0.7))
    for V in (2, 31, 64, 65):
        out.append((64, 400, 401, V, 1, 1.0))
        out.append((64, 400, 401, V, 30, 0.7))
    return out


@gpu
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('B,L,ld,V,scale,gscale', _xent_cases())
def test_xent_vs_float64(B, L, ld, V, scale, gscale, mode):
    """asr_xent directly: target_ld > L addressing, V past one wave's stride and not a multiple of 64, partial last workgroups
    (R % 16 = 13, 1, 0), label smoothing with classes != V, large logits, gscale."""
    classes = _xent_classes(V)
    logits, tgt = _xent_inputs(31, B, L, ld, V, scale)
    loss64, g64 = _xent_ref(logits, tgt, L, mode, classes, torch.float64)
    loss32, g32 = _xent_ref(logits, tgt, L, mode, classes, torch.float32)
    cnt = int((tgt[:, :L] != 0).sum()) if mode == 0 else B * L
    assert cnt > 0
    loss_k, dl = _xent_kernel(logits, tgt, B, L, V, mode, classes, gscale)
    err_g, e32_g = float((dl * cnt / gscale - g64 * cnt).abs().max()), float((g32 * cnt - g64 * cnt).abs().max())
    err_l, e32_l = abs(float(loss_k) - loss64) / abs(loss64), abs(loss32 - loss64) / abs(loss64)
    print('RATIO xent mode %d B %2d L %3d ld %3d V %4d scale %2d gscale %.1f: grad err %.3e e32 %.3e ratio %6.2f | loss rel err %.3e '
          'e32 %.3e ratio %6.2f' % (mode, B, L, ld, V, scale, gscale, err_g, e32_g, err_g / max(e32_g, 1e-300), err_l, e32_l,
                                    err_l / max(e32_l, 1e-300)))
    assert err_g <= K_XENT * e32_g + FLOOR
    assert err_l <= K_XENT * e32_l + FLOOR
    if mode == 0:
        pad = (tgt[:, :L].reshape(-1) == 0)
        assert (dl[pad] == 0).all()


@gpu
def test_xent_all_pad_batch():
    """No counted row: loss NaN (0/0) and an exactly zero gradient, as torch."""
    B, L, ld, V = 5, 13, 40, 31
    logits, tgt = _xent_inputs(32, B, L, ld, V, 1, all_pad=True)
    loss64, g64 = _xent_ref(logits, tgt, L, 0, V, torch.float64)
    assert math.isnan(loss64) and (g64 == 0).all()
    loss_k, dl = _xent_kernel(logits, tgt, B, L, V, 0, V, 0.7)
    assert math.isnan(float(loss_k)) and (dl == 0).all()


@gpu
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('V', [31, 1000])
def test_xent_loss_bits_do_not_depend_on_grouping(V, mode):
    """The loss is summed in 64-bit fixed point: the same R rows give the same bits on every call and however they are
    factorised into (B, L, target_ld)."""
    R = 65
    logits, tgt = _xent_inputs(33, 1, R, R, V, 3)
    rows = tgt.view(-1)
    seen = []
    for (B, L, ld) in [(1, 65, 65), (1, 65, 65), (5, 13, 13), (13, 5, 5), (65, 1, 1), (5, 13, 40), (13, 5, 6)]:
        t = torch.full((B, ld), V - 1, dtype=torch.long)
        t[:, :L] = rows.view(B, L)
        loss_k, dl = _xent_kernel(logits, t, B, L, V, mode, _xent_classes(V))
        seen.append((loss_k.view(torch.int32).item(), dl))
    assert math.isfinite(float(loss_k))
    assert all(s[0] == seen[0][0] for s in seen), [hex(s[0] & 0xffffffff) for s in seen]
    assert all(torch.equal(s[1], seen[0][1]) for s in seen)


@gpu
@pytest.mark.parametrize('mode', [0, 1])
def test_seq_loss_fn_upstream_scale(mode):
    from src import functions as F_hip
    R, V = 77, 65
    logits, tgt = _xent_inputs(34, 1, R, R, V, 2)
    loss64, g64 = _xent_ref(logits, tgt, R, mode, V, torch.float64)
    loss32, g32 = _xent_ref(logits, tgt, R, mode, V, torch.float32)
    cnt = int((tgt != 0).sum()) if mode == 0 else R
    xd = logits.cuda().requires_grad_(True)
    out = F_hip.SeqLossFn.apply(xd, tgt.view(-1).cuda(), mode, V, 0.1)
    (out * torch.tensor(0.7, device='cuda')).backward()
    torch.cuda.synchronize()
    err_g, e32_g = float((xd.grad.cpu().double() * cnt / 0.7 - g64 * cnt).abs().max()), float((g32 * cnt - g64 * cnt).abs().max())
    print('RATIO xent SeqLossFn mode %d: grad err %.3e e32 %.3e ratio %6.2f' % (mode, err_g, e32_g, err_g / max(e32_g, 1e-300)))
    assert err_g <= K_XENT * e32_g + FLOOR
    assert abs(float(out) - loss64) <= (K_XENT * abs(loss32 - loss64) / abs(loss64) + FLOOR) * abs(loss64)


# ---------------------------------------------------------------------------------------------------------------------
# optimizer
# ---------------------------------------------------------------------------------------------------------------------
LR, RHO, EPS = 1.0, 0.9, 1e-8


def _adadelta_ref(p, g, sq, ad, wd, clip, normsq, gmul):
    """clip_grad_norm_ (on gmul * g) + torch.optim.Adadelta, float64 numpy.  normsq None: no clipping (the kernel's NULL)."""
    coef = float(gmul)
    if normsq is not None and clip > 0:
        c = clip / (math.sqrt(normsq) * gmul + 1e-6)
        if c < 1.0:
            coef *= c
    gi = g * coef
    if wd != 0:
        gi = gi + wd * p
    sq = RHO * sq + (1 - RHO) * gi * gi
    delta = np.sqrt(ad + EPS) / np.sqrt(sq + EPS) * gi
    ad = RHO * ad + (1 - RHO) * delta * delta
    return p - LR * delta, sq, ad


def _adadelta_tol(ref):
    """Every element goes through ~12 fp32 roundings per step (sqrtf and the division up to 2.5 ulp, the constants rho, eps, wd
    and the clip coefficient rounded to fp32 once more), three steps: <= 64 x 2^-24 relative to the operands.  Two subtractions
    (g * coef + wd * p, p - lr * delta) make the error relative to the operands, not to the result, so the largest magnitude
    of the tensor joins |ref| in the bound."""
    return 64 * 2.0 ** -24 * (np.abs(ref) + np.abs(ref).max())


def _adadelta_inputs(n, step):
    g = torch.Generator().manual_seed(41)
    p0 = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g) * 0.1 * (step + 1)
    return p0, gr


@gpu
@pytest.mark.parametrize('n', [1, 3, 255, 257, 100003])
@pytest.mark.parametrize('gmul', [1.0, 0.25])
@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('clipmode', ['active', 'inactive', 'zero', 'null'])
def test_adadelta_vs_float64(clipmode, wd, gmul, n):
    from src import hipabi as Hh
    p0, _ = _adadelta_inputs(n, 0)
    norm0 = float(_adadelta_inputs(n, 0)[1].double().norm()) * gmul          # the smallest of the three steps' norms
    clip = {'active': 0.5 * norm0, 'inactive': 12.0 * norm0, 'zero': 0.0, 'null': 5.0}[clipmode]
    pd, sqd, add = p0.cuda(), torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    nsq = torch.zeros(1, dtype=torch.float64, device='cuda')
    pr, sqr, adr = p0.double().numpy(), np.zeros(n), np.zeros(n)
    for step in range(3):
        gr = _adadelta_inputs(n, step)[1]
        gd = gr.cuda()
        Hh.call('asr_sumsq', Hh.ptr(gd), n, Hh.ptr(nsq), Hh.stream_ptr())
        Hh.call('asr_adadelta_step', Hh.ptr(pd), Hh.ptr(gd), Hh.ptr(sqd), Hh.ptr(add), n, LR, RHO, EPS, wd, clip,
                None if clipmode == 'null' else Hh.ptr(nsq), gmul, None, Hh.stream_ptr())
        torch.cuda.synchronize()
        g64 = gr.double().numpy()
        normsq = math.fsum((g64 * g64).tolist())
        nrm = math.sqrt(normsq) * gmul
        if clipmode == 'active':
            assert clip < nrm
        if clipmode == 'inactive':
            assert clip > nrm + 1e-6
        pr, sqr, adr = _adadelta_ref(pr, g64, sqr, adr, wd, clip, None if clipmode == 'null' else normsq, gmul)
    for name, got, want in (('param', pd, pr), ('square_avg', sqd, sqr), ('acc_delta', add, adr)):
        err = np.abs(got.cpu().double().numpy() - want)
        assert (err <= _adadelta_tol(want)).all(), (name, float(err.max()), float(_adadelta_tol(want).min()))
    assert float(np.abs(pr - p0.double().numpy()).min()) > 0          # every parameter moved: the comparison is not vacuous


@gpu
@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 1023, 4 * 512 * 256 * 4 + 3, 3_000_001])
def test_sumsq_vs_fsum(n):
    """n < 4 and every n % 4 (scalar tail only / float4 body + tail), one full trip of the 4-way unrolled loop for every thread
    (4 * 512 * 256 float4) and a size that leaves a remainder loop.  Products of two floats are exact in double; the sum is a
    tree of depth < 600 (24 adds per chain, 4 chains, 6 shuffles, 4 waves, 512 atomics in any order) of positive terms, so
    the relative error is below 600 * 2^-53 = 7e-14 < 1e-12."""
    from src import hipabi as Hh
    g = torch.Generator().manual_seed(42)
    x = torch.randn(n, generator=g) * 3
    want = math.fsum((x.double() * x.double()).tolist())
    xd = x.cuda()
    out = torch.full((1,), -1.0, dtype=torch.float64, device='cuda')
    Hh.call('asr_sumsq', Hh.ptr(xd), n, Hh.ptr(out), Hh.stream_ptr())
    torch.cuda.synchronize()
    assert abs(float(out) - want) <= 1e-12 * want, (float(out), want)


@gpu
@pytest.mark.parametrize('n', [1, 255, 100003, 2048 * 256 + 77])
def test_scale_kernels_exact(n):
    """asr_scale / asr_scale_dev: one fp32 multiplication per element, so the host's float32 product bit for bit (the last n is
    past one grid-stride trip)."""
    from src import hipabi as Hh
    g = torch.Generator().manual_seed(43)
    x = torch.randn(n, generator=g)
    k = 0.3
    want = torch.from_numpy(x.numpy() * np.float32(k))
    xd = x.cuda()
    Hh.call('asr_scale', Hh.ptr(xd), n, k, Hh.stream_ptr())
    assert torch.equal(xd.cpu(), want)
    a = torch.tensor([np.float32(-1.7)], device='cuda')
    src, out = x.cuda(), torch.full((n,), 7.0, device='cuda')
    Hh.call('asr_scale_dev', Hh.ptr(src), Hh.ptr(out), n, Hh.ptr(a), Hh.stream_ptr())
    assert torch.equal(out.cpu(), torch.from_numpy(x.numpy() * np.float32(-1.7)))
    assert torch.equal(src.cpu(), x)


@gpu
def test_loss_mix_exact():
    """out = a * wa (+ b * wb).  One term: the float32 product.  Two terms: the float32 sum of the products, where the compiler may
    fuse either product into the addition - exactly one of those three roundings of the exact value."""
    from src import hipabi as Hh
    g = torch.Generator().manual_seed(44)
    f32 = lambda v: float(np.float32(v))
    for _ in range(20):
        a, wa, b, wb = [float(v) for v in (torch.randn(4, generator=g) * torch.tensor([30.0, 1.0, 5.0, 1.0])).tolist()]
        ad, wad, bd, wbd = [torch.tensor([v], dtype=torch.float32, device='cuda') for v in (a, wa, b, wb)]
        out = torch.full((1,), 7.0, device='cuda')
        Hh.call('asr_loss_mix', Hh.ptr(ad), Hh.ptr(wad), None, None, Hh.ptr(out), Hh.stream_ptr())
        assert float(out) == f32(a * wa)                       # doubles hold the product of two floats exactly
        Hh.call('asr_loss_mix', Hh.ptr(ad), Hh.ptr(wad), Hh.ptr(bd), Hh.ptr(wbd), Hh.ptr(out), Hh.stream_ptr())
        allowed = {f32(f32(a * wa) + f32(b * wb)), f32(a * wa + f32(b * wb)), f32(f32(a * wa) + b * wb)}
        assert float(out) in allowed, (float(out), allowed)


# ---------------------------------------------------------------------------------------------------------------------
# the references themselves (CPU, runs everywhere)
# ---------------------------------------------------------------------------------------------------------------------
def test_float64_references_agree():
    # CTC: torch float64 against the textbook lattice on every edge row, and the structure the GPU tests rely on
    for c in (_case_edges(), _case_all_repeat(), _case_medium()):
        nll_t, g_t = _ctc_torch(c, torch.float64)
        nll_r, g_r = _ctc_restated(c)
        ok = _feasible(nll_t)
        assert torch.equal(ok, _feasible(nll_r))
        assert _max_rel(nll_r, nll_t, ok) < 1e-13 and _max_abs(g_r, g_t, ok) < 1e-12
        B, T, V = g_t.shape
        past = torch.arange(T).view(1, T) >= c['il'].view(B, 1)
        assert (g_t[past] == 0).all()
        for b in range(B):
            il, tl = int(c['il'][b]), int(c['tl'][b])
            if not ok[b]:
                assert nll_t[b] == INF and nll_r[b] == INF
                assert torch.isnan(g_t[b, :il]).all() and (il == 0 or torch.isnan(g_r[b, :il]).all())
            if il == 0:
                assert nll_t[b] == (0.0 if tl == 0 else INF)
    e = _case_edges()
    nll_t, g_t = _ctc_torch(e, torch.float64)
    assert [bool(x) for x in _feasible(nll_t)] == [r != 'il0' and r != 'infeasible' for r in EDGE_ROWS]
    # a single valid path (a blank only between repeated labels): nll = -sum of its log-probs, gradient = softmax - onehot
    b = EDGE_ROWS.index('minimal')
    lab = e['txt'][b, :int(e['tl'][b])].tolist()
    path = [lab[0]]
    for prev, cur in zip(lab, lab[1:]):
        path += [0, cur] if cur == prev else [cur]
    assert len(path) == int(e['il'][b])
    assert abs(float(nll_t[b]) + float(sum(e['lp'][b, t, v].double() for t, v in enumerate(path)))) < 1e-10
    onehot = F.one_hot(torch.tensor(path), 5).double()
    assert float((g_t[b, :len(path)] - (e['lp'][b, :len(path)].double().exp() - onehot)).abs().max()) < 1e-12
    a = _case_all_repeat()
    nll_a, g_a = _ctc_torch(a, torch.float64)
    path = [1 if t % 2 == 0 else 0 for t in range(37)]
    assert abs(float(nll_a[0]) + float(sum(a['lp'][0, t, v].double() for t, v in enumerate(path)))) < 1e-10
    # the size formulas of the test match the cases they are meant to build
    assert _grad_boundary_vocab(60) == 2046 and _grad_boundary_vocab(60, 60 * 1024) == 1918 and _sweep_chunk_frames(400, 31) == 417 and _sweep_chunk_frames(511, 31) == 395
    assert sorted({(B * L) % 16 for B, L, _ in [(1, 77, 77), (5, 13, 13), (64, 400, 401)]}) == [0, 1, 13]

    # sequence losses against a numpy restatement
    for mode in (0, 1):
        for V, classes in ((31, 31), (1000, 31), (65, 65)):
            logits, tgt = _xent_inputs(31, 5, 13, 40, V, 30)
            loss, grad = _xent_ref(logits, tgt, 13, mode, classes, torch.float64)
            x, t = logits.double().numpy(), tgt[:, :13].reshape(-1).numpy()
            m = x.max(-1, keepdims=True)
            lsm = x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))
            if mode == 0:
                rows = np.nonzero(t)[0]
                want = -lsm[rows, t[rows]].mean()
                gw = np.zeros_like(x)
                gw[rows] = np.exp(lsm[rows])
                gw[rows, t[rows]] -= 1
                gw /= len(rows)
            else:
                true = np.full_like(x, 0.1 / (classes - 1))
                true[np.arange(len(t)), t] = 0.9
                want = -(true * lsm).sum(-1).mean()
                gw = (true.sum(-1, keepdims=True) * np.exp(lsm) - true) / len(t)
            assert abs(loss - want) < 1e-12 * abs(want) and np.abs(grad.numpy() - gw).max() < 1e-14
    logits, tgt = _xent_inputs(32, 5, 13, 40, 31, 1, all_pad=True)
    loss, grad = _xent_ref(logits, tgt, 13, 0, 31, torch.float64)
    assert math.isnan(loss) and (grad == 0).all()

    # the float64 Adadelta restatement against torch.optim.Adadelta + clip_grad_norm_ on float64 parameters
    for clipmode, wd, gmul in (('active', 0.0, 1.0), ('inactive', 0.01, 0.25), ('active', 0.01, 0.25), ('zero', 0.01, 1.0)):
        n = 257
        p0 = _adadelta_inputs(n, 0)[0].double()
        norm0 = float(_adadelta_inputs(n, 0)[1].double().norm()) * gmul
        clip = {'active': 0.5 * norm0, 'inactive': 12.0 * norm0, 'zero': 0.0}[clipmode]
        pt = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Adadelta([pt], lr=LR, rho=RHO, eps=EPS, weight_decay=wd)
        pr, sqr, adr = p0.numpy().copy(), np.zeros(n), np.zeros(n)
        for step in range(3):
            g64 = _adadelta_inputs(n, step)[1].double()
            pt.grad = g64.clone() * gmul
            if clip > 0:
                torch.nn.utils.clip_grad_norm_([pt], clip)
            opt.step()
            pr, sqr, adr = _adadelta_ref(pr, g64.numpy(), sqr, adr, wd, clip, float((g64 * g64).sum()), gmul)
        st = opt.state[pt]
        for got, want in ((pr, pt.data), (sqr, st['square_avg']), (adr, st['acc_delta'])):
            assert np.abs(got - want.numpy()).max() <= 1e-13 * np.abs(got).max()
    x = torch.randn(1023, generator=torch.Generator().manual_seed(42)).double()
    assert abs(math.fsum((x * x).tolist()) - float((x * x).sum())) < 1e-12 * float((x * x).sum())
