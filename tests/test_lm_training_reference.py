"""The yardstick of RNN-LM training (src/lm.py::RNNLM.forward with its autograd functions) and of the fused Adam step
(csrc/optim.hip::adam_kernel): float64 restatements, their pins, the case table and the input recipes.
tests/test_hip_lm_training_vs_float64.py runs the device path against them; the restatements import nothing of the code under
test (only test_rnnlm_refuses_untied_emb_dim_mismatch constructs an RNNLM, on the CPU).

lm_train_ref    the reference's training pass in float64 torch autograd, dropout given as explicit keep masks
lm_masks        the masks RNNLM.forward draws for one call: Philox keep masks (tests/test_encoder_glue_reference.py) over the
                (B,T,D) elements in memory order, which is the order asr_dropout_downsample_fwd numbers them at rate 1, style 0
                (downsample_ref and its GPU test: keep_mask(B T D, p, seed).reshape(B, T, D))
adam_ref        clip_grad_norm_ + torch.optim.Adam in float64 numpy, with the kernel's refusals
CASES           the LM training cases; the LSTM dims are chosen with test_lstm_recurrence_reference.route and every case records
                the route it names (test_case_table holds the table to that)

Bounds of the pins: float64 against float64 1e-12; the fixtures tests/golden/g12_lm_gru_train_*.npz were written by a float32 run
of the reference, so float64 agrees with them only to float32 round-off: 2^-24 per operation, contractions of K = 24 terms, 13
steps, 2 layers, counted linearly 24 * 13 * 2 * 2^-24 = 3.7e-5 -> FIXTURE_TOL = 4e-5 (relative to max(1, max |logit|), to the
loss and to each gradient's norm).  Measured: below 3e-7 everywhere.
"""
import collections
import functools
import glob
import math
import os
import time

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import test_lstm_recurrence_reference as R
from test_encoder_glue_reference import drop_scale, drop_thresh, keep_mask

F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURE_TOL = 4e-5
SEED0, SEED_STRIDE = 12345 + 7919, 7919          # the seed of a fresh model's first training call and the step to the next one


# ---------------------------------------------------------------------------------------------------------------------
# the training pass
# ---------------------------------------------------------------------------------------------------------------------
LMRef = collections.namedtuple('LMRef', 'logits loss grads emb_lookup emb_projection')


def lm_masks(B, T, emb_dim, dim, n_layers, p, seed):
    """-> [mask of the embedding (B,T,emb_dim), mask of layer 0's output (B,T,dim), ..., of layer n_layers-1's], bool, True =
    kept.  The embedding is drawn at `seed`, layer l at seed + 1 + l.  drop_thresh(p) == 0 (p <= 0) keeps everything."""
    masks = [keep_mask(B * T * emb_dim, p, seed).reshape(B, T, emb_dim)]
    for l in range(n_layers):
        masks.append(keep_mask(B * T * dim, p, seed + 1 + l).reshape(B, T, dim))
    if drop_thresh(p) == 0:
        assert all(m.all() for m in masks)
    return masks


def lm_train_ref(module, n_layers, tying, state_dict, x, y, masks, p, dtype=F64):
    """The reference's RNNLM training pass (its src/lm.py:27-38 and bin/train_lm.py:40-42) in torch autograd of `dtype`:
    embedding -> mask 0 -> n_layers single-layer nn.LSTM / nn.GRU from the zero state, mask l + 1 behind layer l -> tied
    (F.linear with emb.weight) or `trans` projection -> cross_entropy(ignore_index=0).

    One mask per layer output is the reference's own model: nn.LSTM(dropout=p) / nn.GRU(dropout=p) drop the output of every
    layer but the last, and the model's dp2 drops the last (reference src/lm.py:16-18, 28-37); dp1 is mask 0.  A dropped element
    is 0, a kept one is multiplied by drop_scale(p), the float32 quotient 1 / (1 - p) the kernel multiplies by.  masks None (or
    all True with p = 0): no dropout.  The reference packs by length; with one direction the outputs at valid positions do not
    depend on what follows them and the padded targets are ignored, so nothing is packed here (pinned against a packing model).

    state_dict: the reference's names (emb.weight, rnn.weight_ih_l0, ..., trans.weight, trans.bias); x, y (B,T) int64.
    -> LMRef(logits (B,T,V), loss (float), grads {name: tensor}, emb_lookup, emb_projection): the last two are the separate
    contributions of the embedding lookup and of the tied output projection to grads['emb.weight'] (None when untied)."""
    sd = {k: v.detach().to(dtype) for k, v in state_dict.items()}
    emb_in = sd['emb.weight'].clone().requires_grad_(True)
    emb_out = sd['emb.weight'].clone().requires_grad_(True) if tying else None
    scale = float(drop_scale(p)) if masks is not None else 1.0

    def drop(h, m):
        if masks is None:
            return h
        return h * (torch.from_numpy(np.array(m)).to(dtype) * scale)

    h = drop(F.embedding(x, emb_in), None if masks is None else masks[0])
    layers = []
    for l in range(n_layers):
        w_hh = sd['rnn.weight_hh_l%d' % l]
        rnn = getattr(nn, module)(h.shape[-1], w_hh.shape[1], num_layers=1, batch_first=True).to(dtype)
        with torch.no_grad():
            for k in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'):
                getattr(rnn, k + '_l0').copy_(sd['rnn.%s_l%d' % (k, l)])
        layers.append(rnn)
        h = drop(rnn(h)[0], None if masks is None else masks[l + 1])
    if tying:
        logits = F.linear(h, emb_out)
    else:
        tw, tb = sd['trans.weight'].clone().requires_grad_(True), sd['trans.bias'].clone().requires_grad_(True)
        logits = F.linear(h, tw, tb)
    V = logits.shape[-1]
    loss = F.cross_entropy(logits.reshape(-1, V), y.reshape(-1), ignore_index=0)
    loss.backward()
    grads = {}
    for l, rnn in enumerate(layers):
        for k in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'):
            grads['rnn.%s_l%d' % (k, l)] = getattr(rnn, k + '_l0').grad.detach()
    if tying:
        grads['emb.weight'] = emb_in.grad + emb_out.grad
    else:
        grads['emb.weight'] = emb_in.grad
        grads['trans.weight'], grads['trans.bias'] = tw.grad, tb.grad
    assert set(grads) == set(sd)
    return LMRef(logits.detach(), float(loss.detach()), grads, emb_in.grad if tying else None, emb_out.grad if tying else None)


class PackedRefLM(nn.Module):
    """A model built the way the reference builds its RNNLM (src/lm.py:7-21, 27-38), dropout 0: ONE multi-layer nn.LSTM / nn.GRU
    over the sequence packed by length."""

    def __init__(self, module, V, dim, n_layers, tying):
        super().__init__()
        self.emb = nn.Embedding(V, dim)
        self.rnn = getattr(nn, module)(dim, dim, num_layers=n_layers, dropout=0.0, batch_first=True)
        self.tying = tying
        if not tying:
            self.trans = nn.Linear(dim, V)

    def forward(self, x, lens):
        packed = nn.utils.rnn.pack_padded_sequence(self.emb(x), lens, batch_first=True, enforce_sorted=False)
        out, _ = nn.utils.rnn.pad_packed_sequence(self.rnn(packed)[0], batch_first=True, total_length=x.shape[1])
        return F.linear(out, self.emb.weight) if self.tying else self.trans(out)


# ---------------------------------------------------------------------------------------------------------------------
# errors, as tests/test_lm_gru.py measures them
# ---------------------------------------------------------------------------------------------------------------------
def valid_positions(y):
    return y != 0


def logits_error(got, ref, y):
    """largest |got - ref| over the valid positions, in units of max(1, largest |ref| there)"""
    v = valid_positions(y)
    return float((got[v] - ref[v]).abs().max()) / max(1.0, float(ref[v].abs().max()))


def loss_error(got, ref):
    return abs(got - ref) / max(1.0, abs(ref))


def rel_norm(a, b):
    return float((a - b).norm() / (b.norm() + 1e-12))


def grad_errors(got, ref):
    assert set(got) == set(ref)
    return {k: rel_norm(got[k].to(F64), ref[k]) for k in ref}


# ---------------------------------------------------------------------------------------------------------------------
# cases and inputs
# ---------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'module H layers tying p prec B T V fwd bwd')
FP32, BF16 = R.FP32, R.BF16
LSTM_MODE = 1                                    # asr_lstm_set_persistent's default, what the Solver trains under


def shipped_route_dim():
    """The smallest H above 512 whose forward and backward take the routes of H = 1024 (config/librispeech_lm.yaml) at every
    B <= 16 in both precisions."""
    def routes(H):
        return [R.route('lstm', LSTM_MODE, prec, B, H, 1, bwd) for prec in (FP32, BF16) for B in range(1, 17) for bwd in (False, True)]
    want = routes(1024)
    return next(H for H in range(513, 1025) if routes(H) == want)


H_BIG = 516
_GRU = 'gru_rec per step'                        # csrc/gru_rec.hip has one kernel per pass; its H edges: tests/test_gru_recurrence_reference.py
_L, _G = 'LSTM', 'GRU'
CASES = (
    # H = 64: the persistent plans in use today (second generation at bf16 and B <= 16, first generation otherwise)
    Case(_L, 64, 2, True, 0.5, BF16, 5, 23, 31, 'fwd2<NKS=2>', 'bwd2<NTO=1>'),
    Case(_L, 64, 1, False, 0.0, FP32, 5, 23, 31, 'fwd1<fp32,NKS=2,MT=1>', 'bwd1<fp32,NTO=1,NKS=8,NE=2>'),
    Case(_L, 64, 4, True, 0.3, FP32, 17, 7, 130, 'fwd1<fp32,NKS=2,MT=2>', 'bwd1<fp32,NTO=1,NKS=8,NE=8>'),
    Case(_L, 64, 2, False, 0.5, BF16, 17, 7, 31, 'fwd1<bf16,NKS=2,MT=2>', 'bwd1<bf16,NTO=1,NKS=8,NE=8>'),
    Case(_L, 64, 1, True, 0.5, BF16, 1, 1, 31, 'fwd2<NKS=2>', 'bwd2<NTO=1>'),
    # H = 40: a multiple of 4, not of 16 - first-generation forward, per-step backward with vector loads
    Case(_L, 40, 2, True, 0.5, FP32, 5, 7, 31, 'fwd1<fp32,NKS=2,MT=1>', 'bwd0<fp32,vec>'),
    Case(_L, 40, 1, False, 0.3, BF16, 17, 23, 130, 'fwd1<bf16,NKS=2,MT=2>', 'bwd0<bf16,vec>'),
    # H = 30: not a multiple of 4 - per-step backward with scalar loads
    Case(_L, 30, 2, False, 0.5, FP32, 5, 23, 31, 'fwd1<fp32,NKS=1,MT=1>', 'bwd0<fp32,scalar>'),
    Case(_L, 30, 4, True, 0.0, BF16, 1, 7, 31, 'fwd1<bf16,NKS=1,MT=1>', 'bwd0<bf16,scalar>'),
    # H = 516: the shipped LM's route (H = 1024), one launch per step in both passes
    Case(_L, H_BIG, 2, True, 0.5, BF16, 5, 7, 31, 'fwd0<bf16,vec>', 'bwd0<bf16,vec>'),
    Case(_L, H_BIG, 1, False, 0.3, FP32, 1, 23, 130, 'fwd0<fp32,vec>', 'bwd0<fp32,vec>'),
    Case(_L, H_BIG, 4, True, 0.5, FP32, 5, 7, 31, 'fwd0<fp32,vec>', 'bwd0<fp32,vec>'),
    # the GRU LM at the same four dims
    Case(_G, 64, 2, True, 0.5, BF16, 5, 23, 31, _GRU, _GRU),
    Case(_G, 64, 1, False, 0.0, FP32, 17, 7, 130, _GRU, _GRU),
    Case(_G, 64, 4, True, 0.3, FP32, 5, 7, 31, _GRU, _GRU),
    Case(_G, 40, 2, False, 0.5, BF16, 17, 7, 31, _GRU, _GRU),
    Case(_G, 40, 1, True, 0.5, FP32, 1, 1, 31, _GRU, _GRU),
    Case(_G, 40, 2, True, 0.0, FP32, 5, 7, 31, _GRU, _GRU),
    Case(_G, 30, 2, True, 0.3, BF16, 5, 23, 130, _GRU, _GRU),
    Case(_G, 30, 4, False, 0.5, FP32, 5, 7, 31, _GRU, _GRU),
    Case(_G, 30, 1, True, 0.0, BF16, 17, 23, 31, _GRU, _GRU),
    Case(_G, H_BIG, 2, True, 0.5, FP32, 5, 7, 31, _GRU, _GRU),
    Case(_G, H_BIG, 1, False, 0.3, BF16, 17, 7, 130, _GRU, _GRU),
    Case(_G, H_BIG, 4, True, 0.5, BF16, 5, 7, 31, _GRU, _GRU),
)


def case_id(c):
    return '%s-H%d-L%d-%s-p%g-%s-B%d-T%d-V%d' % (c.module.lower(), c.H, c.layers, 'tied' if c.tying else 'untied', c.p,
                                                 'bf16' if c.prec == BF16 else 'fp32', c.B, c.T, c.V)


def case_routes(c):
    if c.module != 'LSTM':
        return [_GRU, _GRU]
    return [R.route('lstm', LSTM_MODE, c.prec, c.B, c.H, 1, bwd) for bwd in (False, True)]


@functools.lru_cache(maxsize=None)
def case_inputs(c):
    """-> (state_dict, x, y), shared and never written.  Tokens as bin/train_lm.py::fetch_data makes them: a zero-padded batch
    `data` (B,T) of ragged rows, x = [<sos> = 0 | data[:, :-1]], y = data.  Row 0 has the full length, the last row of a batch
    of several has a single valid target.  Weights: PyTorch's default initialisation of the reference's modules, rounded to
    float32 (the device holds exactly these values), but see `gain`."""
    i = CASES.index(c)
    g = np.random.default_rng(9100 + i)
    lens = g.integers(1, c.T + 1, c.B)
    lens[0] = c.T
    if c.B > 1:
        lens[-1] = 1
    data = g.integers(1, c.V, (c.B, c.T))
    for b, n in enumerate(lens):
        data[b, n:] = 0
    y = torch.from_numpy(data.astype(np.int64))
    x = torch.cat([torch.zeros((c.B, 1), dtype=torch.int64), y[:, :-1]], 1)
    torch.manual_seed(9200 + i)
    ref = PackedRefLM(c.module, c.V, c.H, c.layers, c.tying)
    # a four-layer LSTM at that initialisation passes under 5 % of emb.weight.grad back to the lookup (measured 0.047 and 0.017 of
    # the norm): its weight matrices are doubled, which brings the lookup's share to 0.25 .. 0.8 (test_cases_are_quick_and_not_vacuous)
    gain = 2.0 if (c.module == 'LSTM' and c.layers == 4) else 1.0
    # nn.Linear's initialisation gives an untied model logits below 1, where the bf16 ceiling is absolute and dropout does not
    # move them by ten times as much: trans.weight is multiplied by 4 (logits of the size the tied models have)
    gains = {'rnn.weight': gain, 'trans.weight': 4.0}
    sd = {k: v.detach().float().double() * next((f for pre, f in gains.items() if k.startswith(pre)), 1.0) for k, v in ref.state_dict().items()}
    return sd, x, y


@functools.lru_cache(maxsize=None)
def case_ref(c, seed):
    """lm_train_ref of a case with the masks of a training call at `seed`; seed None: no dropout (eval(), or p = 0)."""
    sd, x, y = case_inputs(c)
    masks = None if seed is None else lm_masks(c.B, c.T, c.H, c.H, c.layers, c.p, seed)
    return lm_train_ref(c.module, c.layers, c.tying, sd, x, y, masks, c.p)


def tolerances(c):
    """(logits and loss, gradients): the ceilings of tests/test_lm_gru.py"""
    from test_lm_gru import BF16_GRAD, BF16_TOL, FP32_GRAD, FP32_TOL
    return (BF16_TOL, BF16_GRAD) if c.prec == BF16 else (FP32_TOL, FP32_GRAD)


# ---------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------
AdamState = collections.namedtuple('AdamState', 'p m v vmax applied')


def adam_init(p, amsgrad):
    z = np.zeros_like(p)
    return AdamState(p.copy(), z, z.copy(), z.copy() if amsgrad else None, 0)


def adam_ref(st, g, lr, b1, b2, eps, wd, clip, normsq, gmul, status=0, step=None):
    """One asr_adam_step in float64 numpy: clip_grad_norm_ on gmul * g (coefficient clip / (norm + 1e-6), applied only below 1),
    then torch.optim.Adam with L2 weight decay and, where st.vmax is given, amsgrad.  normsq: the squared norm of g, None for the
    kernel's NULL (no clipping, no guard).  The step number of the bias corrections is "applied updates + 1" (`step`, when given:
    the host-step mode's number instead).  A non-finite norm or a set status word leaves everything, st.applied included,
    untouched.  -> the new AdamState."""
    if status:
        return st
    coef = float(gmul)
    if normsq is not None:
        nrm = math.sqrt(normsq) * gmul if normsq >= 0 else float('nan')
        if not math.isfinite(nrm):
            return st
        if clip > 0:
            c = clip / (nrm + 1e-6)
            if c < 1.0:
                coef *= c
    t = st.applied + 1 if step is None else step
    gi = g * coef
    if wd != 0:
        gi = gi + wd * st.p
    m = b1 * st.m + (1 - b1) * gi
    v = b2 * st.v + (1 - b2) * gi * gi
    vmax = None if st.vmax is None else np.maximum(st.vmax, v)
    denom = np.sqrt(v if vmax is None else vmax) / math.sqrt(1 - b2 ** t) + eps
    return AdamState(st.p - lr / (1 - b1 ** t) * (m / denom), m, v, vmax, st.applied + 1)


ADAM_STEPS = 3
ADAM_K_STEP = 32
ADAM_K = ADAM_K_STEP * ADAM_STEPS


def adam_tol(ref, steps=ADAM_STEPS):
    """K 2^-24 (|ref| + max |ref|), the form of _adadelta_tol (tests/test_hip_losses_vs_float64.py).  fp32 roundings of adam_kernel
    on the longest chain of one element and one step, sqrtf and each division at 2.5:
        coef = gmul * (float)c               2    (the clip coefficient rounded once, the product)
        gi = g coef (+ wd p)                 4    (product; wd rounded once, product, sum)
        m = b1 m + (1 - b1) gi               4    (b1 rounded once, two products, sum; 1 - b1 is exact)
        v = b2 v + (1 - b2) gi gi            5    (b2 rounded once, three products, sum)
        denom = sqrtf(v) / bc2_sqrt + eps    7    (2.5 + 2.5, bc2_sqrt and eps rounded once, sum)
        step_size = lr / bc1                 4.5  (lr and bc1 rounded once, 2.5)
        p - step_size (m / denom)            4.5  (2.5, product, difference)
    = 31, taken as 32 per step; the moments carry their error into the next step, so K = 32 * steps (96 at three steps).  As
    there, the differences g coef + wd p and p - step make the error relative to the operands: max |ref| joins |ref|."""
    return ADAM_K_STEP * steps * 2.0 ** -24 * (np.abs(ref) + np.abs(ref).max())


def abi_float(v):
    """The value a `float` parameter of the C ABI holds.  The references are evaluated at these: the kernel computes 1 - b2 from
    the float it was given, and 1 - float32(0.999) differs from 0.001 by 1.3e-5 relative (216 x 2^-24) - a property of the
    argument, not a rounding of the kernel's."""
    return float(np.float32(v))


@functools.lru_cache(maxsize=None)
def adam_inputs(n):
    """p0 and the gradients of steps 0, 1, 2, ... (growing norms, as _adadelta_inputs), float32 tensors; shared, never written."""
    g = torch.Generator().manual_seed(43)
    p0 = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g) * 0.1
    return p0, tuple(gr * (s + 1) for s in range(5))


@functools.lru_cache(maxsize=None)
def adam_normsq(n, step):
    g64 = adam_inputs(n)[1][step].double()
    return math.fsum((g64 * g64).tolist())


# ---------------------------------------------------------------------------------------------------------------------
# CPU checks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('module', ['LSTM', 'GRU'])
@pytest.mark.parametrize('n_layers', [1, 2, 4])
@pytest.mark.parametrize('tying', [True, False])
def test_all_ones_masks_reproduce_the_packed_multilayer_model(module, n_layers, tying):
    V, dim, B, T = 29, 20, 4, 9
    torch.manual_seed(100 + n_layers)
    ref = PackedRefLM(module, V, dim, n_layers, tying).double()
    g = np.random.default_rng(5)
    lens = np.array([T, 5, 1, T - 1])
    data = g.integers(1, V, (B, T))
    for b, n in enumerate(lens):
        data[b, n:] = 0
    y = torch.from_numpy(data.astype(np.int64))
    x = torch.cat([torch.zeros((B, 1), dtype=torch.int64), y[:, :-1]], 1)
    out = ref(x, torch.from_numpy(lens))
    loss = F.cross_entropy(out.reshape(-1, V), y.reshape(-1), ignore_index=0)
    loss.backward()
    sd = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    for masks, p in ((None, 0.0), (lm_masks(B, T, dim, dim, n_layers, 0.0, 77), 0.0), ([np.ones((B, T, dim), dtype=bool)] * (n_layers + 1), 0.0)):
        r = lm_train_ref(module, n_layers, tying, sd, x, y, masks, p)
        assert logits_error(r.logits, out.detach(), y) < 1e-12
        assert loss_error(r.loss, float(loss.detach())) < 1e-12
        want = {k: v.grad for k, v in ref.named_parameters()}
        errs = grad_errors(r.grads, want)
        assert max(errs.values()) < 1e-12, errs
        if tying:
            assert rel_norm(r.emb_lookup + r.emb_projection, want['emb.weight']) < 1e-12


@pytest.mark.parametrize('path', sorted(glob.glob(os.path.join(GOLDEN, 'g12_lm_gru_train_*.npz'))), ids=os.path.basename)
def test_gru_reproduces_the_reference_fixtures(path):
    import yaml
    z = np.load(path)
    meta = yaml.safe_load(str(z['meta']))
    assert meta['module'] == 'GRU' and meta['dropout'] == 0.0
    sd = {k[2:]: torch.from_numpy(z[k]).double() for k in z.files if k.startswith('w:')}
    x, y = torch.from_numpy(z['tokens']), torch.from_numpy(z['targets'])
    r = lm_train_ref('GRU', meta['n_layers'], meta['emb_tying'], sd, x, y, None, 0.0)
    want = torch.from_numpy(z['logits']).double()
    figs = dict(logits=logits_error(r.logits, want, y), loss=loss_error(r.loss, float(z['loss'])))
    figs.update(grad_errors(r.grads, {k: torch.from_numpy(z['g:' + k]).double() for k in r.grads}))
    print(os.path.basename(path), {k: '%.2e' % v for k, v in figs.items()})
    assert max(figs.values()) < FIXTURE_TOL, figs
    assert [int(v) for v in (y != 0).sum(1)] == z['lens'].tolist()


@pytest.mark.parametrize('amsgrad', [False, True])
@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_adam_ref_is_torch_adam(amsgrad, wd):
    """ten steps, step 4 refused (NaN norm; torch's side leaves that step out), clipping active on some steps and not on others"""
    n, lr, b1, b2, eps, clip = 257, 1e-2, 0.9, 0.999, 1e-8, 2.4
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, generator=g, dtype=F64)
    pt = nn.Parameter(p0.clone())
    opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, amsgrad=amsgrad)
    st = adam_init(p0.numpy(), amsgrad)
    clipped = []
    for it in range(10):
        gr = torch.randn(n, generator=g, dtype=F64) * 0.05 * (it + 1)
        normsq = float((gr * gr).sum())
        if it == 4:
            before = st
            st = adam_ref(st, gr.numpy(), lr, b1, b2, eps, wd, clip, float('nan'), 1.0)
            assert st is before
            st = adam_ref(st, gr.numpy(), lr, b1, b2, eps, wd, clip, float('inf'), 1.0)
            st = adam_ref(st, gr.numpy(), lr, b1, b2, eps, wd, clip, normsq, 1.0, status=2)
            assert st is before and st.applied == 4
            continue
        pt.grad = gr.clone()
        clipped.append(float(nn.utils.clip_grad_norm_([pt], clip)) > clip)
        opt.step()
        st = adam_ref(st, gr.numpy(), lr, b1, b2, eps, wd, clip, normsq, 1.0)
    assert st.applied == 9 and True in clipped and False in clipped
    state = opt.state[pt]
    assert float(state['step']) == 9
    scale = lambda a: max(1.0, float(np.abs(a).max()))
    assert np.abs(st.p - pt.detach().numpy()).max() < 1e-12 * scale(st.p)
    assert np.abs(st.m - state['exp_avg'].numpy()).max() < 1e-12
    assert np.abs(st.v - state['exp_avg_sq'].numpy()).max() < 1e-12
    if amsgrad:
        assert np.abs(st.vmax - state['max_exp_avg_sq'].numpy()).max() < 1e-12
    # grad_mul scales the gradient and its norm alike; the host-step mode takes the number it is given
    a = adam_ref(adam_init(p0.numpy(), amsgrad), 4 * gr.numpy(), lr, b1, b2, eps, wd, clip, 16 * normsq, 0.25)
    b = adam_ref(adam_init(p0.numpy(), amsgrad), gr.numpy(), lr, b1, b2, eps, wd, clip, normsq, 1.0)
    assert np.abs(a.p - b.p).max() < 1e-12
    c = adam_ref(adam_init(p0.numpy(), amsgrad), gr.numpy(), lr, b1, b2, eps, wd, clip, normsq, 1.0, step=1000)
    assert np.abs(c.p - b.p).max() > 1e-4 and c.applied == 1
    # NULL norm: neither clip nor guard
    d = adam_ref(adam_init(p0.numpy(), amsgrad), gr.numpy(), lr, b1, b2, eps, wd, 1e-3, None, 1.0)
    e = adam_ref(adam_init(p0.numpy(), amsgrad), gr.numpy(), lr, b1, b2, eps, wd, 0.0, normsq, 1.0)
    assert np.array_equal(d.p, e.p)


def test_adam_constants_and_inputs():
    assert ADAM_K == 96
    # why the references take the ABI's float values: 1 - float32(0.999) is not 0.001 to within the bound
    assert abs((1 - abi_float(0.999)) / 0.001 - 1) > ADAM_K * 2.0 ** -24
    assert 1 - abi_float(0.999) == float(np.float32(1) - np.float32(0.999))          # the kernel's own 1.f - b2 is exact
    p0, grads = adam_inputs(257)
    assert p0.dtype == torch.float32 and len(grads) == 5
    n0, n2 = math.sqrt(adam_normsq(257, 0)), math.sqrt(adam_normsq(257, 2))
    assert abs(n2 / n0 - 3) < 1e-6


def test_masks_differ_between_sites_and_calls():
    B, T, D, NL = 5, 23, 64, 4
    for p in (0.3, 0.5):
        a = lm_masks(B, T, D, D, NL, p, SEED0)
        b = lm_masks(B, T, D, D, NL, p, SEED0 + SEED_STRIDE)
        assert len(a) == NL + 1 and all(m.shape == (B, T, D) and m.dtype == bool for m in a)
        allm = a + b
        for i in range(len(allm)):
            for j in range(i):
                # independent masks agree on a share p^2 + (1 - p)^2 of the elements; anything near 1 is a reused mask
                agree = float((allm[i] == allm[j]).mean())
                assert abs(agree - (p * p + (1 - p) ** 2)) < 0.05, (p, i, j, agree)
        n = B * T * D
        for m in allm:
            assert abs(float(m.mean()) - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n), (p, float(m.mean()))
    # the element order: memory order of (B,T,D), the site's seed
    m = lm_masks(2, 3, 8, 4, 2, 0.5, 99)
    assert np.array_equal(m[0].reshape(-1), keep_mask(48, 0.5, 99)) and np.array_equal(m[2].reshape(-1), keep_mask(24, 0.5, 101))
    assert m[0].shape == (2, 3, 8) and m[1].shape == (2, 3, 4)
    assert all(mm.all() for mm in lm_masks(2, 3, 8, 4, 2, 0.0, 99))
    assert drop_thresh(0.5) == 1 << 31 and float(drop_scale(0.3)) != 1 / 0.7


@pytest.mark.parametrize('module', ['LSTM', 'GRU'])
def test_rnnlm_refuses_untied_emb_dim_mismatch(module):
    """The reference's trans = nn.Linear(emb_dim, vocab) is applied to outputs of width dim: untied with emb_dim != dim it fails at
    its first forward.  The HIP path would contract over K = dim with the row stride emb_dim and return numbers; it refuses."""
    from src.lm import RNNLM
    for emb_dim, dim in ((48, 32), (32, 48)):
        with pytest.raises(NotImplementedError, match='reference'):
            RNNLM(31, False, emb_dim, module, dim, 2, 0.0)
        ref = nn.Linear(emb_dim, 31)
        with pytest.raises(RuntimeError):
            ref(torch.zeros(2, dim))
    lm = RNNLM(31, False, 32, module, 32, 2, 0.0)
    assert lm.trans.weight.shape == (31, 32)
    with pytest.raises(AssertionError):
        RNNLM(31, True, 48, module, 32, 2, 0.0)


def test_case_table():
    assert shipped_route_dim() == H_BIG
    assert len(CASES) == 24 and len({case_id(c) for c in CASES}) == 24
    for c in CASES:
        assert [c.fwd, c.bwd] == case_routes(c), (case_id(c), case_routes(c))
    for module in ('LSTM', 'GRU'):
        cs = [c for c in CASES if c.module == module]
        assert {c.H for c in cs} == {64, 40, 30, H_BIG}
        assert {c.layers for c in cs} == {1, 2, 4} and {c.tying for c in cs} == {True, False}
        assert {c.p for c in cs} == {0.0, 0.3, 0.5} and {c.prec for c in cs} == {FP32, BF16}
        assert {c.B for c in cs} == {1, 5, 17} and {c.T for c in cs} == {1, 7, 23} and {c.V for c in cs} == {31, 130}
        for H in (64, 40, 30, H_BIG):
            assert {c.prec for c in cs if c.H == H} == {FP32, BF16}
    lstm = [c for c in CASES if c.module == 'LSTM']
    # the persistent plan of today's tests, both per-step load forms, and the shipped LM's route in both precisions
    assert any(c.fwd.startswith('fwd2') and c.bwd.startswith('bwd2') for c in lstm)
    assert any(c.bwd.endswith('vec>') and c.H == 40 for c in lstm) and any(c.bwd.endswith('scalar>') for c in lstm)
    for prec in (FP32, BF16):
        want = [R.route('lstm', LSTM_MODE, prec, 5, 1024, 1, bwd) for bwd in (False, True)]
        assert any([c.fwd, c.bwd] == want and c.H == H_BIG for c in lstm if c.prec == prec)
    assert 64 % 16 == 0 and 40 % 4 == 0 and 40 % 16 != 0 and 30 % 4 != 0 and H_BIG > 512
    for c in CASES:
        _, x, y = case_inputs(c)
        assert x.shape == y.shape == (c.B, c.T) and bool((x[:, 0] == 0).all())
        assert bool((x[:, 1:] == y[:, :-1]).all()) and int(y.max()) < c.V
        lens = (y != 0).sum(1)
        assert int(lens[0]) == c.T and (c.B == 1 or int(lens[-1]) == 1) and int(lens.min()) >= 1
        for b in range(c.B):
            assert bool((y[b, :lens[b]] != 0).all())


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_cases_are_quick_and_not_vacuous(c):
    """Each case's float64 reference takes under two seconds.  A tied case gets at least 10 % of the norm of emb.weight.grad from
    each of its two writers, so losing either breaks the gradient bound; with p > 0 the pass without dropout misses the masked
    one by more than eleven times the bound, in the logits and in the worst gradient (ten for the device test, which also owns
    one bound of error itself; a gradient such as trans.bias's, or dW_hh at T = 1, which is 0, need not move)."""
    case_ref.cache_clear()
    t0 = time.perf_counter()
    r = case_ref(c, SEED0)
    dt = time.perf_counter() - t0
    print('%s: %.2f s' % (case_id(c), dt))
    assert dt < 2.0
    _, _, y = case_inputs(c)
    tol, gtol = tolerances(c)
    assert gtol <= 4e-2
    if c.tying:
        total = float(r.grads['emb.weight'].norm())
        shares = float(r.emb_lookup.norm()) / total, float(r.emb_projection.norm()) / total
        print('   emb.weight.grad shares: lookup %.2f projection %.2f' % shares)
        assert min(shares) >= 0.1, shares
    if c.p > 0:
        plain = case_ref(c, None)
        e_log = logits_error(plain.logits, r.logits, y)
        e_grad = grad_errors(plain.grads, r.grads)
        print('   without dropout: logits %.2f (bound %.0e) gradients %.2f .. %.2f (bound %.0e)' % (e_log, tol, min(e_grad.values()), max(e_grad.values()), gtol))
        assert e_log > 11 * tol and max(e_grad.values()) > 11 * gtol
        nxt = case_ref(c, SEED0 + SEED_STRIDE)
        assert logits_error(nxt.logits, r.logits, y) > 11 * tol
