"""RNNLM(module='GRU') on the GPU: training forward / backward against the genuine reference (tests/golden/g12_lm_gru_train_*.npz,
tests/golden/gen_lm_gru.py) and against torch.nn.GRU in float64, the one-token decode step against the full-sequence forward,
the fused Adam step, and the LM Solver end to end with reference-format checkpoints."""
import glob
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
TRAIN_FIXTURES = sorted(os.path.basename(p)[len('g12_lm_gru_train_'):-4] for p in glob.glob(os.path.join(GOLDEN, 'g12_lm_gru_train_*.npz')))
# bf16: logits and loss carry the recurrence's bf16 error (tests/test_hip_gru_rec.py: Y_BOUND) through the output projection,
# itself a bf16 contraction over dim; gradients the GRAD_BOUND of the recurrence plus the bf16 weight-gradient GEMMs.  Relative
# to each tensor's largest magnitude (logits) or norm (gradients), as in tests/test_lm_training.py.
FP32_TOL, BF16_TOL = 1e-4, 3e-2
FP32_GRAD, BF16_GRAD = 1e-4, 4e-2


class _RefLM(nn.Module):
    """What the reference builds for module 'GRU' (src/lm.py:7-21), dropout 0."""

    def __init__(self, V, dim, n_layers, tying):
        super().__init__()
        self.emb = nn.Embedding(V, dim)
        self.rnn = nn.GRU(dim, dim, num_layers=n_layers, batch_first=True)
        self.tying = tying
        if not tying:
            self.trans = nn.Linear(dim, V)

    def forward(self, x):
        h, _ = self.rnn(self.emb(x))
        return nn.functional.linear(h, self.emb.weight) if self.tying else self.trans(h)


def _lm(V, dim, n_layers, tying, prec, sd):
    from src import hipabi as H
    from src.lm import RNNLM
    lm = RNNLM(V, tying, dim, 'GRU', dim, n_layers, 0.0)
    lm.load_state_dict({k: v.float() for k, v in sd.items()})
    lm = lm.cuda()
    lm.prec = H.F32 if prec == 'fp32' else H.BF16
    lm.flatten()
    return lm


def _train_pass(lm, x, y, V):
    from src.util import CrossEntropyLoss
    lm.train()
    lm.flat_grad.zero_()
    out, _ = lm(x.cuda(), None)
    loss = CrossEntropyLoss(ignore_index=0)(out.reshape(-1, V), y.cuda().reshape(-1))
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().cpu().double(), float(loss.detach()), {n: p.grad.detach().cpu().double() for n, p in lm.named_parameters()}


def _rel_norm(a, b):
    return float((a - b).norm() / (b.norm() + 1e-12))


@pytest.mark.gpu
@pytest.mark.parametrize('name', TRAIN_FIXTURES)
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_training_pass_matches_reference_fixture(name, prec):
    z = np.load(os.path.join(GOLDEN, 'g12_lm_gru_train_%s.npz' % name))
    meta = yaml.safe_load(str(z['meta']))
    V = meta['V']
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('w:')}
    lm = _lm(V, meta['dim'], meta['n_layers'], meta['emb_tying'], prec, sd)
    out, loss, grads = _train_pass(lm, torch.from_numpy(z['tokens']), torch.from_numpy(z['targets']), V)
    want = torch.from_numpy(z['logits']).double()
    tol, gtol = (FP32_TOL, FP32_GRAD) if prec == 'fp32' else (BF16_TOL, BF16_GRAD)
    lens = z['lens']
    scale = max(1.0, float(want.abs().max()))
    for b, n in enumerate(lens):
        assert float((out[b, :n] - want[b, :n]).abs().max()) < tol * scale, (name, prec, b)
    assert abs(loss - float(z['loss'])) < tol * max(1.0, abs(float(z['loss'])))
    for k, g in grads.items():
        rel = _rel_norm(g, torch.from_numpy(z['g:' + k]).double())
        assert rel < gtol, (name, prec, k, rel)


@pytest.mark.gpu
@pytest.mark.parametrize('n_layers,tying', [(1, False), (2, True), (4, True)])
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_training_pass_matches_float64_torch(n_layers, tying, prec):
    V, dim, B, T = 31, 64, 5, 23
    torch.manual_seed(7 + n_layers)
    ref = _RefLM(V, dim, n_layers, tying).double()
    lm = _lm(V, dim, n_layers, tying, prec, ref.state_dict())
    g = torch.Generator().manual_seed(5)
    x = torch.randint(1, V, (B, T), generator=g)
    y = torch.randint(1, V, (B, T), generator=g)
    y[2, 15:] = 0
    out_r = ref(x)
    loss_r = nn.functional.cross_entropy(out_r.reshape(-1, V), y.reshape(-1), ignore_index=0)
    loss_r.backward()
    out, loss, grads = _train_pass(lm, x, y, V)
    tol, gtol = (FP32_TOL, FP32_GRAD) if prec == 'fp32' else (BF16_TOL, BF16_GRAD)
    out_r = out_r.detach()
    assert float((out - out_r).abs().max()) < tol * max(1.0, float(out_r.abs().max()))
    assert abs(loss - float(loss_r)) < tol * max(1.0, abs(float(loss_r)))
    rg = dict(ref.named_parameters())
    for n, gr in grads.items():
        rel = _rel_norm(gr, rg[n].grad)
        assert rel < gtol, (n_layers, tying, prec, n, rel)


@pytest.mark.gpu
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_step_reproduces_the_sequence_forward(prec):
    """step(), fed one token at a time from init_state, gives log_softmax(forward) at every position."""
    from src import hipabi as H
    V, dim, NL, B, T = 31, 48, 2, 6, 11
    torch.manual_seed(11)
    ref = _RefLM(V, dim, NL, False)
    lm = _lm(V, dim, NL, False, prec, ref.state_dict())
    x = torch.randint(1, V, (B, T), generator=torch.Generator().manual_seed(2)).cuda()
    lm.eval()
    with torch.no_grad():
        full, _ = lm(x, None)
    want = torch.log_softmax(full.double(), -1)
    state = lm.init_state(B, 'cuda')
    assert isinstance(state, torch.Tensor)
    tol = 1e-4 if prec == 'fp32' else 2e-2
    for t in range(T):
        lp, state = lm.step(x[:, t].contiguous(), state)
        assert state.shape == (NL, B, dim)
        err = float((lp.double() - want[:, t]).abs().max())
        assert err < tol, (prec, t, err)
    # the state reorders through gather_state (one tensor in, one tensor out)
    idx = torch.tensor([5, 0, 0, 3, 2, 1], dtype=torch.int64, device='cuda')
    g = lm.gather_state(state, idx)
    torch.cuda.synchronize()
    assert torch.equal(g, state[:, idx])


@pytest.mark.gpu
def test_adam_steps_follow_torch():
    from src.optim import Optimizer
    V, dim = 31, 32
    torch.manual_seed(4)
    ref = _RefLM(V, dim, 2, False)
    lm = _lm(V, dim, 2, False, 'fp32', ref.state_dict())
    opt_r = torch.optim.Adam(ref.parameters(), lr=1e-2, eps=1e-8)
    opt = Optimizer(lm.parameters(), 'Adam', 1e-2, 1e-8, 'fixed')
    g = torch.Generator().manual_seed(1)
    for it in range(5):
        grads = {n: torch.randn(p.shape, generator=g) * 0.1 for n, p in ref.named_parameters()}
        for n, p in ref.named_parameters():
            p.grad = grads[n].clone()
        opt_r.step()
        opt.pre_step(it)
        for n, p in lm.named_parameters():
            p.grad.copy_(grads[n])
        opt.opt.grad_norm()
        opt.step(clip=0.0, use_norm=True)
    torch.cuda.synchronize()
    rp = dict(ref.named_parameters())
    for n, p in lm.named_parameters():
        err = float((p.detach().cpu() - rp[n].detach()).abs().max())
        assert err < 2e-6, '%s differs by %g after 5 Adam steps' % (n, err)


@pytest.mark.gpu
def test_solver_trains_a_gru_lm_and_checkpoints_reference_keys(tmp_path):
    pkg = os.path.join(ROOT, 'e2e-asr-pytorch_amd')
    cwd = os.getcwd()
    os.chdir(pkg)
    try:
        from bin.train_lm import Solver
        config = yaml.safe_load(open(os.path.join(pkg, 'config', 'librispeech_lm.yaml')))
        config['model'].update(module='GRU', emb_dim=64, dim=64, n_layers=2, dropout=0.1)
        config['data']['corpus'].update(batch_size=16, subset=512)
        config['hparas'].update(lr=3e-3, valid_step=40, max_step=60)
        paras = types.SimpleNamespace(gpu=True, cuda=0, njobs=0, pin_memory=False, load=None, name='lmgru', verbose=False,
                                      logdir=str(tmp_path / 'log'), ckpdir=str(tmp_path / 'ckpt'), amp=False, seed=0, config='x.yaml',
                                      no_msg=True, reserve_gpu=0)
        s = Solver(config, paras, 'train')
        s.load_data()
        s.set_model()
        assert s.model.module == 'GRU'
        losses = []
        orig = s.backward

        def spy(loss, *a, **k):
            losses.append(float(loss))
            return orig(loss, *a, **k)
        s.backward = spy
        s.exec()
        assert len(losses) == 60 and all(np.isfinite(losses))
        assert np.mean(losses[-10:]) < 0.8 * np.mean(losses[:5]), 'GRU LM loss did not go down: %s ... %s' % (losses[:5], losses[-5:])
        ck = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path / 'ckpt')) for f in fs if f == 'best_ppx.pth']
        assert ck
        sd = torch.load(ck[0], map_location='cpu')['model']
        ref = _RefLM(s.vocab_size, 64, 2, True)
        ref.load_state_dict(sd)                             # the reference's module names: emb, rnn (nn.GRU)
        assert 'rnn.weight_hh_l1' in sd and tuple(sd['rnn.weight_hh_l1'].shape) == (192, 64)
    finally:
        os.chdir(cwd)
