"""The overlapped training step against its in-line order and against float64.

What is under test is the layer between the kernels (src/hipabi.py defer_side / flush_side / join_side / side_branch /
join_branch / on_rec_stream / on_side_stream / begin_forward / work_stream; src/functions.py layer_backward / prepack16 /
CTCHeadFn.backward / AttDecoderFn.backward; the side_ctc branch of src/asr.py; src/step.py and the Solver's use of the step
in bin/train_asr.py).  Families, shapes and the K = 3 schedule: tests/test_step_streams_reference.py.

In-line against float64 (test_inline_step_vs_float64).  ASR_OVERLAP=0, ASR_CTC_SIDE=0.  Before each step the device's
parameters and Adadelta state are read back, the step's dropout masks are regenerated with asr_dropout_mask from model.seed and
_drop_counter, and the oracle runs from exactly those; outputs, losses and gradients are held to test_hip_model.compare,
unchanged, the update to _adadelta_ref fed the device's own flat gradient within _adadelta_tol.  asr_adadelta_step takes the
gradient as `const float *` and does not rewrite it, so every run here steps through train_step(optimize=True) - the product's
path, in which the optimizer reads the gradient behind the joins with no host synchronisation in between - and the gradient is
cloned behind the step on the step's own stream.  `emb` is not in this part: the oracle has no plugin.

Every switch against the in-line run (test_switch_equals_inline).  Before each step the in-line run's parameters, optimizer
state and _drop_counter / _ss_counter are copied into the switched model.  Settings: a overlap on, default stream; b overlap on,
inside work_stream(); c overlap on, inside a fresh stream; d overlap on + ASR_CTC_SIDE=1; e overlap off + ASR_CTC_SIDE=1;
f overlap on + ASR_FAST16=0 against an in-line run with ASR_FAST16=0.  Bounds, the project's own (tests/test_bench_shape.py):
total_loss, ctc_output, att_output, att_align bitwise equal; every parameter's gradient within GRAD_BOUND = 1e-5 of its norm,
floored at 1e-3 of the largest gradient norm (the order of the fp32 atomics is the only admitted difference); parameters after
the step within PARAM_BOUND = 1e-5 max-abs.  Each case also proves the path it names (storage classes, plans, defer_side calls,
_pack16_ev from step 2 on, _asr_side, the stream a forward hook sees) and the _side invariants after every step.

A backward that raised (test_backward_that_raised_leaves_nothing_behind), the Solver's use of the step against train_step and an
eval pass between steps (test_solver_*): see the tests.

A defect found here and fixed in csrc/decoder.hip.  test_inline_step_vs_float64[base-bf16] first measured 1 - cos = 2.18e-2 .. 2.63e-2
(bound 1e-2) on attention.att_layer.gen_energy.weight and attention.proj_k.weight, and [vgg1-bf16] 1.64e-2 on ctc_layer.0.weight
at step 2; both passed with the decoder's single-launch forward switched off.  Both backward loops take the dot of the softmax
backward from the SAVED context, dot = dctx . ctx, which holds only if ctx = sum attn * enc over the operands the backward reads;
the single-launch forward forms its context from other roundings (0.5 % of ctx, coherent when the attention row is flat), so
sum_tau de[tau] != 0 and every gradient of the energy path carried a bias.  asr_att_decoder_bwd now restates the context columns
of xin from the saved attention behind such a forward (ctx_from_saved_att_kernel).  With it base/bf16 measures 0.045 of
compare's tolerance (worst: ctc_output) and vgg1/bf16 0.38.

Worst measured ratios on MI355X, over all families and settings (RATIO lines of a run with -s):
    switch against in-line   forward bitwise equal in all 60 cases (and in the three steps behind the backward that raised);
                             gradient: 1.7e-6 of the norm in every family but `emb` (base/fp32/d, gen_energy.bias), bound 1e-5;
                             `emb` 1.81e-5 (emb/bf16/d step 0, attention.proj_q.weight), bound GRAD_BOUNDS['emb'] = 1e-4: settings
                             b, c and e measure the same 8.995e-6 there, and e takes the in-line path launch for launch, so
                             this is what two runs of ONE order differ by (dq is summed with fp32 atomics) on a gradient whose
                             norm sits at the floor; the forward is asserted bitwise equal first;
                             parameters after the step 2.98e-8 max-abs, bound 1e-5
    in-line against float64  fp32: 0.06 of compare's tolerance (base/fp32 step 2, grad.ctc_layer.0.weight);
                             bf16: worst 0.69 of the tolerance (sampled step 0, gradient cosine of
                             encoder.layers.1.layer.weight_hh_l0)
    update against _adadelta_ref   0.058 of _adadelta_tol (dec_plan step 0, acc_delta)
    Solver (debug.yaml model, joint)   losses bitwise equal at every step; gradients 4.95e-4 of the norm against train_step and 8.15e-4
                             between two Solvers (attention.proj_k.weight; SOLVER_GRAD_BOUND); parameters after one step 1.0e-6
                             (1.12e-5 on the attention-only model; SOLVER_PARAM_BOUND); every update 0.06 of _adadelta_tol from
                             its own gradient
    Solver (debug_emb.yaml model, joint, fusing plugin)   totals bitwise equal at every step - also when the Solver still summed the
                             plugin's term first and with torch arithmetic (4.53065777, 4.48111534, 4.43938971 on both sides);
                             gradients, the plugin's included, 8.65e-4 of the norm (attention.proj_k.weight), parameters 1.94e-6
"""
import contextlib
import os
import sys
import math

import numpy as np
import pytest
import torch
import yaml

from test_checkpoint_interop import _paras
from test_dp_hooks import _recording_reducer
from test_hip_emb_plugin import _Tokens, _vector_file
from test_hip_losses_vs_float64 import _adadelta_ref, _adadelta_tol
from test_hip_model import compare, finish
from test_step_streams_reference import (CASES, FAMILIES, V, batches, build_model, decisions_for, encoder_frames, mask_shapes,
                                         oracle_step, plans_of, storage_of)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'e2e-asr-pytorch_amd')
GRAD_BOUND, PARAM_BOUND = 1e-5, 1e-5
GRAD_BOUNDS = {'emb': 1e-4}      # measured above 1e-5 with the forward bitwise equal: module docstring
# The Solver's shape (config/debug.yaml: B*T' > 512 rows, split reductions) measured 1.05e-5 to 1.12e-5 after ONE step from the same state
# with the step's loss bitwise equal: partial sums of the decoder's bias gradients reach ~100 (ulp 7.6e-6) while the element
# itself is ~1e-4, where Adadelta's first steps move a parameter by about its gradient.  With the forward shown bitwise equal
# first, the bound goes up to the 1e-4 that tests/test_dp_hooks.py grants bf16, and no further.
SOLVER_PARAM_BOUND = 1e-4
# Gradients at the Solver's shape, in the part-3 measure.  The reference here is ONE order run twice: eight in-line runs
# (ASR_OVERLAP=0, one stream) of one step of this model from one state, losses bitwise equal, differ from the first by up to
# 6.2e-4 (attention.proj_k.weight; 5.8e-4, 2.3e-4 and 2.1e-4 recur: a handful of summation orders of the split reductions), 7.2e-5
# on an encoder weight and 3e-6 .. 1.2e-5 elsewhere; with the overlap on the same figures.  The bound is K = 8 times that, the
# project's convention for a bound taken from the reference's own error (tests/test_hip_emb_plugin.py); a branch left out or a
# wrong scale moves a gradient by its own size.
SOLVER_GRAD_BOUND = 8 * 6.2e-4
OUT_KEYS = ('total_loss', 'ctc_output', 'att_output', 'att_align')

# name -> (environment, stream the step is called on)
SETTINGS = {
    'inline': ({'ASR_OVERLAP': '0', 'ASR_CTC_SIDE': '0'}, 'default'),
    'a': ({'ASR_OVERLAP': '1', 'ASR_CTC_SIDE': '0'}, 'default'),
    'b': ({'ASR_OVERLAP': '1', 'ASR_CTC_SIDE': '0'}, 'work'),
    'c': ({'ASR_OVERLAP': '1', 'ASR_CTC_SIDE': '0'}, 'fresh'),
    'd': ({'ASR_OVERLAP': '1', 'ASR_CTC_SIDE': '1'}, 'work'),
    'e': ({'ASR_OVERLAP': '0', 'ASR_CTC_SIDE': '1'}, 'default'),
    'f': ({'ASR_OVERLAP': '1', 'ASR_CTC_SIDE': '0', 'ASR_FAST16': '0'}, 'work'),
}
_INLINE = {}          # (family, precision, fast16) -> the in-line run, made once and left unchanged


def _setenv(monkeypatch, env):
    for k in ('ASR_OVERLAP', 'ASR_CTC_SIDE', 'ASR_FAST16', 'ASR_OVERLAP_DP'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@contextlib.contextmanager
def _on(kind, fresh=None):
    """The caller's stream of a setting: the default stream, work_stream() as the Solver and bench.py use it, or `fresh`."""
    from src import hipabi as H
    cur = torch.cuda.current_stream()
    if kind == 'default':
        yield cur
        return
    s = H.work_stream() if kind == 'work' else fresh
    s.wait_stream(cur)
    with torch.cuda.stream(s):
        yield s
    cur.wait_stream(s)


class _Run(object):
    """One model of a family with its optimizer(s) and the probes of part 4."""

    def __init__(self, fid, prec, monkeypatch, tmp_path):
        from src import functions as F
        from src import hipabi as H
        from src.module import RNNLayer
        from src.optim import Optimizer
        self.fid, self.prec = fid, prec
        self.fam, self.cfg, self.sd, model = build_model(fid, prec)
        self.model = model.cuda().train()
        self.opt = Optimizer(self.model.parameters(), 'Adadelta', 1.0, 1e-8)
        self.plugin = self.eopt = None
        if self.fam['emb']:
            from src.plugin import EmbeddingRegularizer
            g = torch.Generator().manual_seed(21)
            vec = _vector_file(tmp_path / ('vec_%d.txt' % id(self)), torch.randn(V, 16, generator=g))
            torch.manual_seed(22)
            self.plugin = EmbeddingRegularizer(_Tokens(V), self.model.dec_dim, True, vec, 'CosEmb', 0.5, 0, 1.0, prec=prec).cuda().train()
            assert not self.plugin.apply_fuse
            self.eopt = Optimizer(self.plugin.trainable_parameters(), 'Adadelta', 1.0, 1e-8)
        self.layers = [m for m in self.model.encoder.layers if isinstance(m, RNNLayer)]
        self.deferred, self.packed, self.streams = [0], [], []
        defer, prepack = H.defer_side, F.prepack16

        def count_defer(fn, *keep):
            self.deferred[0] += 1
            return defer(fn, *keep)

        def watch_prepack(layers, B, p):
            r = prepack(layers, B, p)
            if layers and layers[0] is self.layers[0]:
                self.packed.append(['_pack16_ev' in l.__dict__ for l in layers])     # before the layers pop them
            return r
        monkeypatch.setattr(H, 'defer_side', count_defer)
        monkeypatch.setattr(F, 'prepack16', watch_prepack)
        self.model.encoder.register_forward_hook(lambda m, i, o: self.streams.append(torch.cuda.current_stream()))

    def state(self):
        o = self.opt.opt
        st = {'p': self.model.flat_param.clone(), 'sq': o.square_avg.clone(), 'ad': o.acc_delta.clone(),
              'drop': self.model._drop_counter, 'ss': getattr(self.model, '_ss_counter', 0)}
        if self.plugin is not None:
            e = self.eopt.opt
            st.update(ep=self.plugin.flat_param.clone(), esq=e.square_avg.clone(), ead=e.acc_delta.clone())
        return st

    def load(self, st):
        o = self.opt.opt
        self.model.flat_param.copy_(st['p']), o.square_avg.copy_(st['sq']), o.acc_delta.copy_(st['ad'])
        self.model._drop_counter, self.model._ss_counter = st['drop'], st['ss']
        if self.plugin is not None:
            e = self.eopt.opt
            self.plugin.flat_param.copy_(st['ep']), e.square_avg.copy_(st['esq']), e.acc_delta.copy_(st['ead'])

    def step(self, batch, k):
        """One train_step on the current stream; everything read here is cloned behind the step on that stream (no host sync)."""
        from src.step import train_step
        from src.util import CTCLoss, CrossEntropyLoss
        feat, lens, txt = batch
        if self.fam['tf_rate'] != 1:
            self.model._tf_decisions = decisions_for(txt.shape[1], k)
        out = train_step(self.model, self.opt, CTCLoss(), CrossEntropyLoss(), feat, lens, txt, int(txt.shape[1]), tf_rate=self.fam['tf_rate'],
                         clip=self.fam['clip'], emb_decoder=self.plugin, emb_optimizer=self.eopt)
        res = {k_: (out[k_].detach().clone() if out.get(k_) is not None else None) for k_ in OUT_KEYS + ('ctc_loss', 'att_loss', 'encode_len')}
        res['side'] = bool(getattr(out['ctc_output'], '_asr_side', False)) if out['ctc_output'] is not None else False
        res['grad'] = self.model.flat_grad.clone()
        if self.plugin is not None:
            res['egrad'] = self.plugin.flat_grad.clone()
        if self.fam['tf_rate'] != 1:
            res['tokens'] = self.model._last_tokens.clone()
        res['after'] = self.state()
        return res


def _side_invariants(run, where):
    from src import hipabi as H
    s = H._side
    assert s['deferred'] == [] and s['keep'] == [] and not s['pending'] and not s.get('callback'), (where, len(s['deferred']), len(s['keep']),
                                                                                                     s['pending'], s.get('callback'))
    assert not any('_pack16_ev' in l.__dict__ for l in run.layers), where
    H.raise_if_aborted()


def _schedule(run, setting, follow=None):
    """The family's K steps under a setting; `follow`: the in-line run whose state every step starts from."""
    env, kind = SETTINGS[setting]
    fresh = torch.cuda.Stream() if kind == 'fresh' else None
    steps = []
    for k, batch in enumerate(batches(run.fid)):
        batch = tuple(t.cuda() for t in batch)
        if follow is not None:
            run.load(follow[k]['before'])
        before = run.state()
        with _on(kind, fresh) as s:
            res = run.step(batch, k)
        torch.cuda.synchronize()
        res['before'], res['caller'] = before, s
        _side_invariants(run, '%s/%s step %d' % (run.fid, setting, k))
        steps.append(res)
    return steps


def _inline(fid, prec, fast16, monkeypatch, tmp_path):
    key = (fid, prec, fast16)
    if key not in _INLINE:
        env = dict(SETTINGS['inline'][0])
        if not fast16:
            env['ASR_FAST16'] = '0'
        _setenv(monkeypatch, env)
        run = _Run(fid, prec, monkeypatch, tmp_path)
        steps = _schedule(run, 'inline')
        assert run.deferred[0] == 0, 'defer_side was called with the overlap off'
        assert all(not any(p) for p in run.packed)
        assert all(s == torch.cuda.default_stream() for s in run.streams)
        _INLINE[key] = (run, steps)
        monkeypatch.undo()
    return _INLINE[key]


def _params(model):
    return [(k, model._offsets[id(p)], p.numel()) for k, p in model.named_parameters()]


def device_masks(model, cfg, B, T, counter):
    """The masks a step drew whose _drop_counter stood at `counter` before it: layer l takes seed model.seed * 1000003 +
    counter + l + 1 (src/asr._RunCtx.next_seed), over the LSTM output's frames (test_hip_model, test_bench_shape._dropout_masks)."""
    from src import hipabi as H
    masks = []
    for l, (shape, p) in enumerate(zip(mask_shapes(cfg, B, T), cfg.enc_dropout)):
        seed = (model.seed * 1000003 + counter + l + 1) & 0xFFFFFFFFFFFF
        m = torch.empty(int(np.prod(shape)), device='cuda')
        H.call('asr_dropout_mask', H.ptr(m), m.numel(), float(p), seed, H.stream_ptr())
        masks.append(m.view(shape).cpu().double())
    return masks


# ---------------------------------------------------------------------------------------------------------------------
# part 2: the in-line step against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fid,prec', [c for c in CASES if not FAMILIES[c[0]]['emb']])
def test_inline_step_vs_float64(fid, prec, monkeypatch, tmp_path):
    run, steps = _inline(fid, prec, True, monkeypatch, tmp_path)
    fam, cfg, model = run.fam, run.cfg, run.model
    names = _params(model)
    every = []                 # the reports of all steps: judged together at the end, so that a run prints every figure
    for k, (batch, st) in enumerate(zip(batches(fid), steps)):
        b4 = st['before']
        p0 = b4['p'].cpu()
        P = {n: p0[o:o + c].view(tuple(run.sd[n].shape)).double() for n, o, c in names}
        masks = device_masks(model, cfg, fam['B'], batch[0].shape[1], b4['drop'])
        for m, p in zip(masks, cfg.enc_dropout):
            assert abs(float(m.mean()) - (1 - p)) < 0.1
        assert st['after']['drop'] == b4['drop'] + len(cfg.enc_dim)
        fed = None
        if fam['tf_rate'] != 1:
            tok = st['tokens'].cpu()
            dec = decisions_for(batch[2].shape[1], k)
            assert bool((tok[:, 0] == 0).all())
            for t, keep in enumerate(dec):             # the teacher's token where the decision says so
                if keep:
                    assert torch.equal(tok[:, t + 1], batch[2][:, t])
            assert st['after']['ss'] == b4['ss'] + sum(1 for d in dec if not d)
            fed = torch.cat([tok[:, 1:], torch.zeros_like(tok[:, :1])], 1)
        ref_out, ref_grads, ok = oracle_step(cfg, P, batch, masks, fed)
        assert ok, 'the case must be CTC-feasible'
        assert np.array_equal(st['encode_len'].cpu().numpy(), ref_out['enc_len'])
        res = dict(st, att_seq=st['att_align'])
        g = st['grad'].cpu()
        shim = type('M', (), {'named_parameters': staticmethod(
            lambda: [(n, type('P', (), {'grad': g[o:o + c].view(tuple(run.sd[n].shape))})()) for n, o, c in names])})()
        report = []
        compare(shim, res, ref_out, ref_grads, prec, report)
        worst = max(report, key=lambda r: r[1] / r[2])
        print('RATIO float64 %s/%s step %d: worst %s err %.3e tol %.3e ratio %.3f' % (fid, prec, k, worst[0], worst[1], worst[2], worst[1] / worst[2]))
        for r in report:
            if r[1] > 0.5 * r[2]:
                print('RATIO float64 %s/%s step %d: %s err %.3e tol %.3e' % (fid, prec, k, r[0], r[1], r[2]))
        every += [('step %d %s' % (k, r[0]),) + tuple(r[1:]) for r in report]
        # the update from the device's own gradient
        g64 = g.double().numpy()
        want = _adadelta_ref(p0.double().numpy(), g64, b4['sq'].cpu().double().numpy(), b4['ad'].cpu().double().numpy(), 0.0, fam['clip'],
                             math.fsum((g64 * g64).tolist()), 1.0)
        gn = math.sqrt(math.fsum((g64 * g64).tolist()))
        assert (gn > fam['clip']) == (fid == 'base'), gn
        for name, got, w in zip(('param', 'square_avg', 'acc_delta'), (st['after'][x] for x in ('p', 'sq', 'ad')), want):
            err, tol = np.abs(got.cpu().double().numpy() - w), _adadelta_tol(w)
            print('RATIO update %s/%s step %d %s: %.3f of its bound' % (fid, prec, k, name, float((err / tol).max())))
            assert (err <= tol).all(), (name, float(err.max()))
        assert float((st['after']['p'] - b4['p']).abs().max()) > 0
    finish(every)


# ---------------------------------------------------------------------------------------------------------------------
# parts 3 and 4: every switch against the in-line run, and the proof of the path
# ---------------------------------------------------------------------------------------------------------------------
def _own_update(tag, before, grad, after, clip, keys=('p', 'sq', 'ad'), normsq=None):
    """The state a step left is _adadelta_ref of the state before it and of the step's OWN final gradient, within _adadelta_tol:
    an optimizer that read the flat gradient before a deferred contraction had landed, or with a wrong scale, misses this whatever
    the parameters did.  normsq: the norm the clip and the NaN guard read (default: of `grad`; the plugin's step reads the model's)."""
    g64 = grad.cpu().double().numpy()
    if normsq is None:
        normsq = float(np.dot(g64, g64))
    p0, sq0, ad0 = (before[k].cpu().double().numpy() for k in keys)
    want = _adadelta_ref(p0, g64, sq0, ad0, 0.0, clip, normsq, 1.0)
    worst = 0.0
    for k, w in zip(keys, want):
        err, tol = np.abs(after[k].cpu().double().numpy() - w), _adadelta_tol(w)
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (tag, k, float(err.max()))
    print('RATIO %s update from its own gradient (%s): %.3f of _adadelta_tol' % (tag, '/'.join(keys), worst))
    return normsq


def _grad_ratio(a_, b_, spans, what='grad'):
    """Worst per-parameter ||a - b|| / max(||b||, 1e-3 of the largest gradient norm): the part-3 measure."""
    gmax = max(float(b_[o:o + n].double().norm()) for _, o, n in spans)
    assert gmax > 0
    worst = (0.0, '')
    for name, o, n in spans:
        a, b = a_[o:o + n].double(), b_[o:o + n].double()
        worst = max(worst, (float((a - b).norm() / max(float(b.norm()), 1e-3 * gmax)), what + '.' + name))
    return worst


def _hold_to_inline(tag, model, got, want, clip, grad_bound=GRAD_BOUND):
    """Part-3 bounds between two runs of one step, and the run's own update; returns (worst gradient ratio, worst parameter
    difference)."""
    for key in OUT_KEYS:
        if want[key] is None:
            assert got[key] is None, key
            continue
        same = torch.equal(got[key], want[key])
        print('RATIO %s %s bitwise %s (max diff %.3e)' % (tag, key, same, float((got[key].double() - want[key].double()).abs().max())))
        assert same, (tag, key)
    worst_g = _grad_ratio(got['grad'], want['grad'], _params(model))
    if 'egrad' in want:
        worst_g = max(worst_g, _grad_ratio(got['egrad'], want['egrad'], [('emb_decoder', 0, want['egrad'].numel())], 'emb grad'))
    print('RATIO %s gradient: worst %.3e of the norm (%s), bound %.0e' % (tag, worst_g[0], worst_g[1], grad_bound))
    assert worst_g[0] <= grad_bound, (tag, worst_g)
    worst_p = max(float((got['after'][k] - want['after'][k]).abs().max()) for k in ('p', 'ep') if k in want['after'])
    print('RATIO %s parameters after the step: max-abs %.3e, bound %.0e' % (tag, worst_p, PARAM_BOUND))
    assert worst_p <= PARAM_BOUND, (tag, worst_p)
    # the optimizer state: each run's p, square_avg and acc_delta follow from its own final gradient
    normsq = _own_update(tag, got['before'], got['grad'], got['after'], clip)
    if 'egrad' in got:
        _own_update(tag + ' plugin', got['before'], got['egrad'], got['after'], 0.0, keys=('ep', 'esq', 'ead'), normsq=normsq)
    assert got['after']['drop'] == want['after']['drop'] and got['after']['ss'] == want['after']['ss']
    return worst_g[0], worst_p


def _expected_storage(fam, prec, fast16):
    return fam['storage'] if (prec == 'bf16' and fast16) else ['f32'] * len(fam['storage'])


@pytest.mark.parametrize('setting', ['a', 'b', 'c', 'd', 'e', 'f'])
@pytest.mark.parametrize('fid,prec', CASES)
def test_switch_equals_inline(fid, prec, setting, monkeypatch, tmp_path):
    from src import hipabi as H
    env, kind = SETTINGS[setting]
    fast16 = env.get('ASR_FAST16', '1') != '0'
    overlap = env['ASR_OVERLAP'] == '1'
    _, base = _inline(fid, prec, fast16, monkeypatch, tmp_path)
    _setenv(monkeypatch, env)
    run = _Run(fid, prec, monkeypatch, tmp_path)
    fam, cfg, model = run.fam, run.cfg, run.model
    # the row of the table: storage classes, plans, decoder kind
    storage = _expected_storage(fam, prec, fast16)
    assert storage_of(H, model, fam['B'], prec) == storage
    if prec == 'bf16':
        assert plans_of(H, model, fam['B'], encoder_frames(cfg, fam['T']), fam['L']) == fam['plans']
    if model.enable_att:
        assert (model.decoder.fast and model.attention.fast) == fam['dec_fast']
    steps = _schedule(run, setting, follow=base)
    for k, (got, want) in enumerate(zip(steps, base)):
        _hold_to_inline('%s/%s/%s step %d' % (fid, prec, setting, k), model, got, want, fam['clip'], grad_bound=GRAD_BOUNDS.get(fid, GRAD_BOUND))
        if 'tokens' in want:
            assert torch.equal(got['tokens'], want['tokens'])
    # the path the case names
    assert (run.deferred[0] >= 1) if overlap else (run.deferred[0] == 0), run.deferred
    assert len(run.packed) == len(steps)
    ahead = [overlap and s == 'bf16' and i >= 1 for i, s in enumerate(storage)]
    assert run.packed[0] == [False] * len(storage), run.packed
    for k in range(1, len(steps)):
        assert run.packed[k] == ahead, (k, run.packed[k], ahead)
    if fid == 'base' and prec == 'bf16' and overlap and fast16:
        assert ahead == [False, True, True]
    for got in steps:
        assert got['side'] == (setting == 'd' and fam['joint']), (setting, got['side'])
    assert len(run.streams) == len(steps)
    for got, seen in zip(steps, run.streams):
        if kind == 'default':
            assert seen == (H.work_stream() if overlap else torch.cuda.default_stream())
        else:
            assert seen == got['caller'] and (kind != 'work' or seen == H.work_stream())
            assert kind != 'fresh' or seen not in (H.work_stream(), torch.cuda.default_stream())


def test_ctc_side_stays_off_under_data_parallel(monkeypatch, tmp_path):
    """ASR_CTC_SIDE=1 with a reducer attached: the CTC branch stays on the step's stream (the gradient buckets are signalled in
    backward order), and the step leaves nothing behind."""
    _setenv(monkeypatch, SETTINGS['d'][0])
    run = _Run('base', 'bf16', monkeypatch, tmp_path)
    from src.step import train_step
    from src.util import CTCLoss, CrossEntropyLoss
    dp = run.model.attach_data_parallel(reducer_cls=_recording_reducer())
    feat, lens, txt = (t.cuda() for t in batches('base')[0])
    out = train_step(run.model, run.opt, CTCLoss(), CrossEntropyLoss(), feat, lens, txt, int(txt.shape[1]), dp=dp, clip=0.05)
    torch.cuda.synchronize()
    assert not getattr(out['ctc_output'], '_asr_side', False)
    assert dp.order == list(range(len(dp.buckets)))
    assert run.deferred[0] == 0                  # data parallel without ASR_OVERLAP_DP: everything in line
    _side_invariants(run, 'dp')


# ---------------------------------------------------------------------------------------------------------------------
# part 5: a backward that raised
# ---------------------------------------------------------------------------------------------------------------------
class _Boom(Exception):
    pass


def test_backward_that_raised_leaves_nothing_behind(monkeypatch, tmp_path):
    """A Python exception from a tensor hook on the encoder output's gradient: by then CTCHeadFn.backward and AttDecoderFn.backward
    have deferred their parameter gradients and the engine callback is registered, and neither runs.  begin_forward drops what is
    stale at the next forward (its docstring records the defect this repairs: wrong gradients in the step after a failing one):
    the next three steps of the same model equal those of a model that never failed."""
    from src import hipabi as H
    _, base = _inline('base', 'bf16', True, monkeypatch, tmp_path)
    _setenv(monkeypatch, SETTINGS['a'][0])
    run = _Run('base', 'bf16', monkeypatch, tmp_path)
    armed, seen = [True], []

    def raiser(g):
        if armed[0]:
            raise _Boom('from the hook')

    def arm(m, i, o):
        s = H._side
        seen.append((len(s['deferred']), bool(s.get('callback')), len(s['keep'])))      # behind begin_forward and the encoder
        if armed[0]:
            o[0].register_hook(raiser)
    run.model.encoder.register_forward_hook(arm)
    batch = tuple(t.cuda() for t in batches('base')[0])
    with pytest.raises(_Boom):
        run.step(batch, 0)
    torch.cuda.synchronize()
    assert run.deferred[0] >= 2, 'the head and the decoder deferred their parameter gradients before the hook'
    print('RATIO raised: left behind deferred %d keep %d pending %s callback %s' % (len(H._side['deferred']), len(H._side['keep']),
                                                                                     H._side['pending'], H._side.get('callback')))
    assert len(H._side['deferred']) > 0 and H._side.get('callback'), 'the test must reach the state that begin_forward repairs'
    armed[0] = False
    steps = _schedule(run, 'a', follow=base)
    assert seen[1] == (0, False, 0), seen           # the first forward after the failure starts clean
    for k, (got, want) in enumerate(zip(steps, base)):
        _hold_to_inline('raised/a step %d' % k, run.model, got, want, run.fam['clip'])


# ---------------------------------------------------------------------------------------------------------------------
# part 6: the Solver's use of the step
# ---------------------------------------------------------------------------------------------------------------------
def _solver_config(emb=False):
    cfg = yaml.safe_load(open(os.path.join(PKG, 'config', 'debug_emb.yaml' if emb else 'debug.yaml')))
    cfg['data']['corpus'].update(batch_size=4, subset=12)
    cfg['data']['text']['vocab_file'] = os.path.join(PKG, cfg['data']['text']['vocab_file'])
    if emb:
        cfg['emb']['src'] = os.path.join(PKG, cfg['emb']['src'])
    cfg['hparas'].update(max_step=3, valid_step=1000)          # the Solver validates behind step 1 whatever valid_step says
    cfg['model']['ctc_weight'] = 0.5       # both files are attention-only: a JOINT model, or the CTC branch of the step (side_branch,
    return cfg                             # the loss on the side stream, join_branch: src/step.py) would never run under the Solver


def _count_side_branches(monkeypatch):
    """Every `with H.side_branch(...)` entered from here on: the forward's (src/asr.py) and the loss's (src/step.py)."""
    from src import hipabi as H
    n = [0]

    class Counting(H.side_branch):
        def __enter__(self):
            n[0] += 1
            return super().__enter__()
    monkeypatch.setattr(H, 'side_branch', Counting)
    return n


def _solver_run(tmp_path, name, validate=True, force=None, emb=False):
    """Three steps of bin/train_asr.Solver with its fetch_data, backward and validate wrapped: the initial state_dict, the fetched
    batches, the per-step losses and gradients, the state (parameters, Adadelta state, _drop_counter) before and after every step,
    whether a step's CTC output carried _asr_side, and what the eval pass left.  Every step's update is held to its own gradient
    (_own_update).  force: states to load before each step (step-forced, as everywhere in this file).  emb: config/debug_emb.yaml's
    model and plugin; the plugin's parameters, Adadelta state and gradient are then recorded, loaded and held beside the model's."""
    sys.path.insert(0, PKG)
    from bin.train_asr import Solver
    from src import hipabi as H
    from src.module import RNNLayer
    torch.manual_seed(0)
    solver = Solver(_solver_config(emb), _paras(tmp_path, name=name), 'train')
    solver.load_data()
    solver.set_model()
    assert solver.model.enable_ctc and solver.model.enable_att and (solver.emb_decoder is not None) == emb
    r = {'init': {k: v.detach().clone() for k, v in solver.model.state_dict().items()}, 'fetched': [], 'losses': [], 'grads': [], 'pre': [],
         'post': [], 'side': [], 'eval': [], 'solver': solver, 'egrads': []}
    if emb:
        r['init_emb'] = {k: v.detach().clone() for k, v in solver.emb_decoder.state_dict().items()}
    fetch, backward, val = solver.fetch_data, solver.backward, solver.validate

    def snap():
        o = solver.optimizer.opt
        st = {'p': solver.model.flat_param.clone(), 'sq': o.square_avg.clone(), 'ad': o.acc_delta.clone(), 'drop': solver.model._drop_counter}
        if emb:
            e = solver.emb_optimizer.opt
            st.update(ep=solver.emb_decoder.flat_param.clone(), esq=e.square_avg.clone(), ead=e.acc_delta.clone())
        return st

    def record_fetch(data, train=False):
        out = fetch(data, train=train)
        if train:
            if force is not None:
                _load_solver_state(solver.model, solver.optimizer, force[len(r['pre'])], solver.emb_decoder, solver.emb_optimizer)
            r['fetched'].append(tuple(t.clone() for t in out))
            r['pre'].append(snap())
        return out

    def record_forward(m, inp, out):
        if m.training:
            r['side'].append(bool(getattr(out[0], '_asr_side', False)))
    solver.model.register_forward_hook(record_forward)

    def record_backward(loss, *a, **kw):
        r['losses'].append(loss.detach().clone())
        out = backward(loss, *a, **kw)
        r['grads'].append(solver.model.flat_grad.clone())
        if emb:
            r['egrads'].append(solver.emb_decoder.flat_grad.clone())
        r['post'].append(snap())
        return out

    def watch_validate(*a):
        if not validate:
            r['eval'].append(None)
            return None
        b4 = snap()
        out = val(*a)
        torch.cuda.synchronize()
        now, s = snap(), H._side
        layers = [m for m in solver.model.encoder.layers if isinstance(m, RNNLayer)]
        r['eval'].append({'state_kept': all(torch.equal(b4[k], now[k]) for k in ('p', 'sq', 'ad')) and b4['drop'] == now['drop'],
                          'side_clean': s['deferred'] == [] and s['keep'] == [] and not any('_pack16_ev' in l.__dict__ for l in layers),
                          'training': solver.model.training})
        return out
    solver.fetch_data, solver.backward, solver.validate = record_fetch, record_backward, watch_validate
    solver.exec()
    torch.cuda.synchronize()
    H.raise_if_aborted()
    assert solver.step == 3 and len(r['losses']) == 3 and len(r['eval']) == 1 and len(r['side']) == 3
    for k in range(3):
        assert bool(torch.isfinite(r['losses'][k])), 'the batch must be CTC-feasible'
        normsq = _own_update('solver %s step %d' % (name, k), r['pre'][k], r['grads'][k], r['post'][k], solver.GRAD_CLIP)
        if emb:
            _own_update('solver %s step %d plugin' % (name, k), r['pre'][k], r['egrads'][k], r['post'][k], 0.0, keys=('ep', 'esq', 'ead'),
                        normsq=normsq)
    return r


def _load_solver_state(model, optimizer, st, plugin=None, emb_optimizer=None):
    o = optimizer.opt
    model.flat_param.copy_(st['p']), o.square_avg.copy_(st['sq']), o.acc_delta.copy_(st['ad'])
    model._drop_counter = st['drop']
    if plugin is not None:             # as _Run.load
        e = emb_optimizer.opt
        plugin.flat_param.copy_(st['ep']), e.square_avg.copy_(st['esq']), e.acc_delta.copy_(st['ead'])


@pytest.mark.parametrize('ctc_side,emb', [('0', False), ('1', False), ('0', True)], ids=['0', '1', 'emb'])
def test_solver_step_equals_train_step(ctc_side, emb, monkeypatch, tmp_path):
    """bin/train_asr.Solver._exec runs the step of src/step.py in two halves (forward_losses, then backward_update inside
    BaseSolver.backward) with its own zeroing of the gradients, the continuation of the CTC side branch included.  Three steps
    of it on config/debug.yaml's model made joint (ctc_weight 0.5; synthetic corpus, batches of 4, T up to 2450) against
    train_step over the same fetched batches, from the same initial state_dict and seeds.  Under ASR_CTC_SIDE=1 both take the
    side branch in every step (two `with H.side_branch` per step: the head in ASR.forward, the loss in the step; _asr_side on the
    CTC output), under 0 neither does.  Per-step losses bitwise equal; then gradients within SOLVER_GRAD_BOUND of their norm,
    parameters within SOLVER_PARAM_BOUND, and each side's p / square_avg / acc_delta held to its own gradient (_own_update).

    `emb`: config/debug_emb.yaml's model made joint in the same way, with its fusing plugin: the Solver hands the plugin, its
    optimizer and the zeroing of its gradient to the shared step.  The total (the plugin's term included) is bitwise equal, the
    plugin's gradient and parameters are held by the same two bounds as the model's, and its update to its own gradient under the
    model's norm.

    Step-forced: before each step the Solver's parameters, Adadelta state and _drop_counter are copied into the train_step model.
    A free-running loop cannot be held to equal bits at this shape, and neither can two runs of the Solver itself: measured on
    MI355X (attention-only model), two identical Solver runs agree bitwise in the loss of step 1 and then read
    3.38223815 / 3.38224387 and 3.37456298 / 3.37450767, with parameters 1.6e-5 apart after three steps.  The weight-gradient
    reductions over B * T' > 512 rows add their slices with fp32 atomics in no fixed order
    (tests/test_bench_shape.py::test_step_repeatability), and a parameter that differs in its last bit can round to the
    neighbouring bf16 operand (2^-9 relative) in the next forward."""
    from src import hipabi as H
    from src.asr import ASR
    from src.optim import Optimizer
    from src.step import train_step
    from src.util import CTCLoss, LabelSmoothingLoss
    _setenv(monkeypatch, {'ASR_CTC_SIDE': ctc_side})
    entered = _count_side_branches(monkeypatch)
    r = _solver_run(tmp_path, 'solver' + ctc_side + ('emb' if emb else ''), emb=emb)
    solver = r['solver']
    # the path: the continuation of the side branch ran under the Solver in every step, or in none
    assert r['side'] == [ctc_side == '1'] * 3, r['side']
    assert entered[0] == (6 if ctc_side == '1' else 0), entered
    cfg = solver.config
    model = ASR(solver.feat_dim, solver.vocab_size, cfg['data']['corpus']['batch_size'] // 2, prec=cfg['hip']['prec'], seed=solver.paras.seed,
                **cfg['model']).cuda()
    model.load_state_dict(r['init'])
    model.train()
    opt = Optimizer(model.parameters(), **dict(cfg['hparas']))
    assert torch.equal(model.flat_param, r['pre'][0]['p'])
    plugin = eopt = None
    if emb:
        from src.plugin import EmbeddingRegularizer
        plugin = EmbeddingRegularizer(solver.tokenizer, model.dec_dim, prec=cfg['hip']['prec'], seed=solver.paras.seed, **cfg['emb']).cuda()
        plugin.load_state_dict(r['init_emb'])
        plugin.train()
        assert plugin.apply_fuse and torch.equal(plugin.flat_param, r['pre'][0]['ep'])
        eopt = Optimizer(plugin.trainable_parameters(), **dict(cfg['hparas']))
    mine, after, grads, sides, egrads = [], [], [], [], []
    ws = H.work_stream()
    ws.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(ws):
        for k, (feat, flen, txt, tl) in enumerate(r['fetched']):
            _load_solver_state(model, opt, r['pre'][k], plugin, eopt)
            out = train_step(model, opt, CTCLoss(), LabelSmoothingLoss(31, 0.1), feat, flen, txt, int(txt.shape[1]), tf_rate=1.0,
                             clip=solver.GRAD_CLIP, txt_len=tl, emb_decoder=plugin, emb_optimizer=eopt)
            mine.append(out['total_loss'].clone())
            grads.append(model.flat_grad.clone())
            o = opt.opt
            after.append({'p': model.flat_param.clone(), 'sq': o.square_avg.clone(), 'ad': o.acc_delta.clone()})
            if emb:
                egrads.append(plugin.flat_grad.clone())
                after[-1].update(ep=plugin.flat_param.clone(), esq=eopt.opt.square_avg.clone(), ead=eopt.opt.acc_delta.clone())
            sides.append(bool(getattr(out['ctc_output'], '_asr_side', False)))
    torch.cuda.current_stream().wait_stream(ws)
    torch.cuda.synchronize()
    H.raise_if_aborted()
    assert sides == r['side'] and entered[0] == (12 if ctc_side == '1' else 0), (sides, entered)
    tag = ctc_side + (' emb' if emb else '')
    diffs = [max(float((a[x] - post[x]).abs().max()) for x in ('p', 'ep') if x in a) for a, post in zip(after, r['post'])]
    ratios = [_grad_ratio(g, gs, _params(model)) for g, gs in zip(grads, r['grads'])]
    if emb:
        ratios = [max(x, _grad_ratio(g, gs, [('emb_decoder', 0, g.numel())], 'emb grad')) for x, g, gs in zip(ratios, egrads, r['egrads'])]
    for k, (a, b) in enumerate(zip(r['losses'], mine)):
        print('RATIO solver ctc_side=%s step %d: loss %.9g train_step %.9g (apart %.3e), gradient %.3e of the norm (%s, bound %.0e), parameters after the '
              'step max-abs %.3e (bound %.0e), moved %.3e' % (tag, k, float(a), float(b), abs(float(a) - float(b)), ratios[k][0], ratios[k][1], SOLVER_GRAD_BOUND,
                                                              diffs[k], SOLVER_PARAM_BOUND, float((r['post'][k]['p'] - r['pre'][k]['p']).abs().max())))
    for k, (a, b) in enumerate(zip(r['losses'], mine)):
        assert torch.equal(a.reshape(()), b.reshape(())), (k, float(a), float(b))
        assert ratios[k][0] <= SOLVER_GRAD_BOUND, (k, ratios[k])
        assert diffs[k] <= SOLVER_PARAM_BOUND, (k, diffs[k])
        assert float((r['post'][k]['p'] - r['pre'][k]['p']).abs().max()) > 0
        normsq = _own_update('train_step ctc_side=%s step %d' % (tag, k), r['pre'][k], grads[k], after[k], solver.GRAD_CLIP)
        if emb:
            assert float((r['post'][k]['ep'] - r['pre'][k]['ep']).abs().max()) > 0
            _own_update('train_step ctc_side=%s step %d plugin' % (tag, k), r['pre'][k], egrads[k], after[k], 0.0,
                        keys=('ep', 'esq', 'ead'), normsq=normsq)
    assert solver.model._drop_counter == model._drop_counter == 3


def test_solver_eval_pass_between_steps_leaves_nothing_behind(monkeypatch, tmp_path):
    """The Solver as it is runs an eval pass on the work stream behind step 1.  The pass leaves the parameters, the optimizer state
    and _drop_counter bit for bit as they were, nothing in the _side bookkeeping and the model back in training mode; and a
    Solver whose `validate` is a no-op, started before each step from the as-is Solver's state (step-forced, for the reason given
    in test_solver_step_equals_train_step), computes the same training losses bit for bit, gradients within SOLVER_GRAD_BOUND and
    parameters within SOLVER_PARAM_BOUND; every step's p / square_avg / acc_delta follow from its own gradient (_solver_run)."""
    _setenv(monkeypatch, {})
    a = _solver_run(tmp_path, 'eval1', validate=True)
    assert a['eval'][0] == {'state_kept': True, 'side_clean': True, 'training': True}, a['eval']
    b = _solver_run(tmp_path, 'eval0', validate=False, force=a['pre'])
    for x, y in zip(a['fetched'], b['fetched']):
        assert all(torch.equal(u, v) for u, v in zip(x, y))
    diffs = [float((x['p'] - y['p']).abs().max()) for x, y in zip(a['post'], b['post'])]
    ratios = [_grad_ratio(y, x, _params(a['solver'].model)) for x, y in zip(a['grads'], b['grads'])]
    for k, (x, y) in enumerate(zip(a['losses'], b['losses'])):
        print('RATIO solver eval pass: step %d loss with %.9g without %.9g, gradient %.3e of the norm (%s), parameters after the step '
              'max-abs %.3e' % (k, float(x), float(y), ratios[k][0], ratios[k][1], diffs[k]))
    for k, (x, y) in enumerate(zip(a['losses'], b['losses'])):
        assert torch.equal(x, y), (k, float(x), float(y))
        assert ratios[k][0] <= SOLVER_GRAD_BOUND, (k, ratios[k])
        assert diffs[k] <= SOLVER_PARAM_BOUND and a['post'][k]['drop'] == b['post'][k]['drop']
