"""The single-direction GRU recurrence of csrc/gru_rec.hip (asr_gru_rec_fwd / _bwd) and the LM layer built on it (GRULayerFn)
against float64 torch: nn.GRU's cell unrolled by hand, so that gi, gh and h0 are leaves whose gradients autograd reports.

Shapes: H in {16, 64, 320, 1024, 2048} plus ragged sizes (37, 3: H % 4 != 0 takes the scalar-load path of dot_rows), B in
{1, 5, 37} (one and three 16-row batch tiles, partial tiles), T in {1, 7, 50}, zero and given h0.  fp32 (ASR_F32: exact fp32
MFMA inputs) is held to 1e-4 relative to each tensor's largest magnitude.

bf16 bounds (ASR_BF16: h, W_hh and dgh rounded to bf16, unit roundoff u = 2^-9, fp32 accumulation), per tensor, relative to
the tensor's largest magnitude:
  - gh = h W_hh^T: each product carries a relative error of at most 2u; with nn.GRU's W ~ U(-1/sqrt(H), 1/sqrt(H)) and |h| <= 1
    the rounding errors of the H products add like a random walk, |err(gh)| ~ 2u * sqrt(sum_k h_k^2 W_jk^2) <= 2u / sqrt(3)
    ~ 2.3e-3 in absolute terms, independent of H.  Gates are Lipschitz-1 (sigmoid' <= 1/4, tanh' <= 1), so one step moves h by
    at most ~2 * 2.3e-3; the recurrence contracts (z in (0,1)), so the error stays at a few steps' worth over T = 50:
    Y_BOUND = 2e-2 (about 4x the accumulated estimate).
  - dgi / dgh: the cell backward multiplies dh by factors <= 1 and adds the carried dgh_{t+1} W_hh term, which has the same
    2u random-walk error relative to |dgh| plus the inherited error of the saved gates (<= Y_BOUND): GRAD_BOUND = 4e-2.
  - dh0 collects the same chain once more: GRAD_BOUND.
A wrong row, column, gate or time step moves these tensors by O(1) of their magnitude, far above either bound."""

import pytest
import torch

FP32_BOUND = 1e-4
Y_BOUND = 2e-2
GRAD_BOUND = 4e-2

# (H, B, T, given h0)
SHAPES = [
    (16, 1, 1, False), (16, 5, 7, True), (64, 37, 50, False), (64, 5, 7, True), (320, 5, 50, True), (320, 37, 7, False),
    (1024, 37, 7, False), (1024, 5, 50, True), (2048, 5, 7, False), (2048, 1, 1, True), (37, 5, 7, True), (37, 37, 50, False),
    (3, 5, 7, True), (1, 1, 1, False),
]


def _inputs(Hd, B, T, h0, seed):
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / Hd ** 0.5
    gi = torch.randn(B, T, 3 * Hd, generator=g, dtype=torch.float64) * 0.7
    whh = (torch.rand(3 * Hd, Hd, generator=g, dtype=torch.float64) * 2 - 1) * k
    bhh = (torch.rand(3 * Hd, generator=g, dtype=torch.float64) * 2 - 1) * k
    hz = (torch.rand(B, Hd, generator=g, dtype=torch.float64) * 2 - 1) * 0.8 if h0 else None
    dy = torch.randn(B, T, Hd, generator=g, dtype=torch.float64)
    return gi, whh, bhh, hz, dy


def reference(gi, whh, bhh, h0, dy):
    """float64 nn.GRU recurrence (torch.nn.GRU's equations, gate order r, z, n) with gh_t retained: y, saved, dgi, dgh, dh0."""
    B, T, G = gi.shape
    Hd = G // 3
    dev = 'cuda'
    gi = gi.to(dev).clone().requires_grad_(True)
    h = (torch.zeros(B, Hd, dtype=torch.float64, device=dev) if h0 is None else h0.to(dev).clone()).requires_grad_(True)
    h_init = h
    W, b = whh.to(dev), bhh.to(dev)
    ys, ghs, saved = [], [], []
    for t in range(T):
        gh = h @ W.t() + b
        gh.retain_grad()
        ghs.append(gh)
        r = torch.sigmoid(gi[:, t, :Hd] + gh[:, :Hd])
        z = torch.sigmoid(gi[:, t, Hd:2 * Hd] + gh[:, Hd:2 * Hd])
        n = torch.tanh(gi[:, t, 2 * Hd:] + r * gh[:, 2 * Hd:])
        h = (1 - z) * n + z * h
        ys.append(h)
        saved.append(torch.cat([r, z, n, gh[:, 2 * Hd:]], -1))
    y = torch.stack(ys, 1)
    (y * dy.to(dev)).sum().backward()
    dgh = torch.stack([g_.grad for g_ in ghs], 1)
    return {'y': y.detach(), 'saved': torch.stack(saved, 1).detach(), 'dgi': gi.grad, 'dgh': dgh,
            'dh0': h_init.grad if h0 is not None else None}


def run_kernel(gi, whh, bhh, h0, dy, prec, with_saved=True, want_dh0=True):
    from src import hipabi as H
    B, T, G = gi.shape
    Hd = G // 3
    f = lambda t: None if t is None else t.float().cuda().contiguous()
    gi_, whh_, bhh_, h0_, dy_ = f(gi), f(whh), f(bhh), f(h0), f(dy)
    y = torch.full((B, T, Hd), float('nan'), device='cuda')
    saved = torch.full((B, T, 4 * Hd), float('nan'), device='cuda') if with_saved else None
    st = H.stream_ptr()
    H.call('asr_gru_rec_fwd', H.ptr(gi_), H.ptr(whh_), H.ptr(bhh_), H.ptr(h0_), B, T, Hd, prec, H.ptr(y), H.ptr(saved), st)
    out = {'y': y, 'saved': saved}
    if not with_saved:
        return out
    dgi = torch.full((B, T, G), float('nan'), device='cuda')
    dgh = torch.full((B, T, G), float('nan'), device='cuda')
    dh0 = torch.full((B, Hd), float('nan'), device='cuda') if want_dh0 else None
    nbytes = H.lib().asr_gru_rec_workspace_bytes(B, Hd)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    H.call('asr_gru_rec_bwd', H.ptr(dy_), H.ptr(y), H.ptr(saved), H.ptr(h0_), H.ptr(whh_), B, T, Hd, prec, H.ptr(dgi), H.ptr(dgh),
           H.ptr(dh0), H.ptr(ws), nbytes, st)
    torch.cuda.synchronize()
    out.update(dgi=dgi, dgh=dgh, dh0=dh0)
    return out


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize('Hd,B,T,h0', SHAPES)
def test_recurrence_matches_float64(Hd, B, T, h0):
    from src import hipabi as H
    gi, whh, bhh, hz, dy = _inputs(Hd, B, T, h0, seed=Hd * 1000 + B * 10 + T)
    ref = reference(gi, whh, bhh, hz, dy)
    for prec in (H.F32, H.BF16):
        got = run_kernel(gi, whh, bhh, hz, dy, prec)
        yb, gb = (FP32_BOUND, FP32_BOUND) if prec == H.F32 else (Y_BOUND, GRAD_BOUND)
        errs = {k: _rel(got[k], ref[k]) for k in ('y', 'saved', 'dgi', 'dgh')}
        if h0:
            errs['dh0'] = _rel(got['dh0'], ref['dh0'])
        for k, e in errs.items():
            assert e < (yb if k in ('y', 'saved') else gb), (Hd, B, T, h0, prec, k, errs)
        # inference (saved = NULL, as the decode step passes it) writes the same y, bit for bit
        inf = run_kernel(gi, whh, bhh, hz, dy, prec, with_saved=False)
        torch.cuda.synchronize()
        assert torch.equal(inf['y'], got['y'])


@pytest.mark.gpu
def test_zero_h0_equals_null_h0():
    from src import hipabi as H
    gi, whh, bhh, _, dy = _inputs(64, 5, 7, False, 3)
    for prec in (H.F32, H.BF16):
        a = run_kernel(gi, whh, bhh, None, dy, prec, want_dh0=False)
        b = run_kernel(gi, whh, bhh, torch.zeros(5, 64, dtype=torch.float64), dy, prec)
        for k in ('y', 'saved', 'dgi', 'dgh'):
            assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
def test_decode_step_chain_equals_sequence():
    """T steps of T = 1 (h0 = the previous output, saved = NULL: what RNNLM.step issues) give the sequence's y exactly."""
    from src import hipabi as H
    gi, whh, bhh, hz, dy = _inputs(320, 5, 7, True, 4)
    for prec in (H.F32, H.BF16):
        full = run_kernel(gi, whh, bhh, hz, dy, prec, with_saved=False)['y']
        h = hz
        for t in range(7):
            h = run_kernel(gi[:, t:t + 1], whh, bhh, h, None, prec, with_saved=False)['y'][:, 0]
            assert torch.equal(h, full[:, t]), (prec, t)
            h = h.double().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize('Hd,B,T,tying', [(64, 5, 7, True), (37, 37, 50, False), (1024, 5, 7, False)])
def test_layer_gradients_match_torch_gru(Hd, B, T, tying):
    """GRULayerFn (src/lm.py): y, dx, dW_ih, dW_hh, db_ih, db_hh against torch.nn.GRU in float64."""
    from src import hipabi as H
    from src.lm import GRULayerFn
    torch.manual_seed(Hd + B + T)
    Din = 24
    ref = torch.nn.GRU(Din, Hd, batch_first=True).double().cuda()
    x = torch.randn(B, T, Din, dtype=torch.float64, device='cuda', requires_grad=True)
    dy = torch.randn(B, T, Hd, dtype=torch.float64, device='cuda')
    y_r, _ = ref(x)
    (y_r * dy).sum().backward()

    class L(object):
        pass
    layer = L()
    layer.dim = Hd
    names = ('w_ih', 'w_hh', 'b_ih', 'b_hh')
    refp = (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0)
    for n, p in zip(names, refp):
        setattr(layer, n, p.detach().float().contiguous())
        setattr(layer, 'g_' + n, torch.zeros_like(p, dtype=torch.float32))
    for prec, bound in ((H.F32, FP32_BOUND), (H.BF16, GRAD_BOUND)):
        for n in names:
            getattr(layer, 'g_' + n).zero_()
        anchor = torch.zeros(1, device='cuda', requires_grad=True)
        xf = x.detach().float().requires_grad_(True)
        y = GRULayerFn.apply(anchor, xf, layer, prec)
        y.backward(dy.float())
        torch.cuda.synchronize()
        assert _rel(y, y_r) < (FP32_BOUND if prec == H.F32 else Y_BOUND)
        assert _rel(xf.grad, x.grad) < bound, ('dx', prec)
        for n, p in zip(names, refp):
            assert _rel(getattr(layer, 'g_' + n), p.grad) < bound, (n, prec, _rel(getattr(layer, 'g_' + n), p.grad))
