"""The encoder layer stack as the model composes it, against float64, in both storages at their edges.

Each case of tests/test_encoder_layer_reference.py::CASES builds src.asr.ASR with the case's encoder block from
seeded_state_dict (bf16 mode: weights and x rounded to bf16 before either side sees them), calls model.encoder(x, lens,
_RunCtx(model)) in train or eval mode as the case says, then to_f32_fn and backward from (out * dout).sum().  The dropout masks
are regenerated with asr_dropout_mask from model.seed and _drop_counter (the rule of
test_hip_model.py::test_training_mode_dropout_vs_oracle) and fed to the float64 side, layers_f64.  Per layer it asserts the
storage class taken (rnn_fast_ok), LayerF32's recurrence plan (asr_lstm_plan) and that no abort word is set; out, dx and every
parameter gradient of every layer are held to the case's own bounds (8 x the rounded restatement's error E0, computed on the
CPU: the reference file's docstring), under the relative Frobenius and `proj` metrics.  The device runs seed 0 once; ASR_OVERLAP=0
for the matrix, and the two-step stack case again with the overlap on, where step 2 must take the weights prepack16 packed on
the side stream (_pack16_ev) and both steps the cached recurrence workspace at epochs 1 and 2.

Every run prints `RATIO <case> <precision> step <k>: worst metric / bound (metric value, bound)`.

Measured on MI355X: 36 cases x 2 precisions = 72 case runs (74 steps) + the overlapped two-step run, every one run and none
skipped; one refusal (below).  Worst metric / bound per storage and precision:
    LayerBF16, bf16 mode            0.247  stack4_T33, proj of layers.2 weight_ih_l0_reverse (3.41e-3, bound 1.38e-2)
    LayerF32, bf16 mode             0.199  all_on, proj of layers.0 pj.bias (6.31e-4, bound 3.17e-3)
    both storages in one stack      0.219  stack_concat_then_bf16, proj of layers.0 weight_ih_l0_reverse (1.75e-3, bound 7.97e-3)
    LayerF32, fp32 mode             0.351  stack_bf16x2_p25 step 1, proj of layers.0 weight_hh_l0_reverse (3.31e-7, bound 9.44e-7)
    two steps, overlap on (bf16)    0.134 / 0.155  the same figures as with the overlap off, step for step

Found on the way:
  * A `proj` behind 'concat' down-sampling at rate > 1 (case concat2_proj of REFUSED).  The float64 side raised on the case (the
    projection is D x D, the layer's output rate * D wide, and the reference's own forward fails there); the library built the
    layer and LayerF32.out_proj would have contracted over rate * D columns of a D-column weight and left (rate - 1) * D columns
    of `out` unwritten.  src/module.RNNLayer now raises ValueError when such a layer is built (test_refused); every 'concat'
    case of the table runs without the projection.  No figure before the fix: the shape was never launched.
  * x_bf16 / x_bf16_ln in fp32 mode first measured dx 1.69e-3 / 1.88e-3 against a bound of 7.6e-6.  Not a defect: a bf16 input
    takes its gradient back as bf16 (CastF32Fn.backward, src/functions.py) and the rounded restatement did not state that
    rounding point; with it stated (one bf16 rounding of dx) the bound is 1.4e-2 / 1.5e-2 and dx measures 0.12 of it.
"""
import types

import pytest
import torch

import test_encoder_layer_reference as R

pytestmark = pytest.mark.gpu

SEED = 5                       # model.seed of the dropout cases


def _setenv(monkeypatch, overlap):
    for k in ('ASR_OVERLAP', 'ASR_CTC_SIDE', 'ASR_FAST16', 'ASR_OVERLAP_DP'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('ASR_OVERLAP', '1' if overlap else '0')
    monkeypatch.setenv('ASR_CTC_SIDE', '0')


def _device_masks(H, model, c, counter):
    """Layer l's mask over its LSTM output's frames; a layer draws a seed only when it drops (src/module.RNNLayer.forward):
    (model.seed * 1000003 + the running _drop_counter) & 0xFFFFFFFFFFFF."""
    masks = []
    for (T, T2, Din, Dz), l in zip(R.frames(c), c['layers']):
        if not (c['train'] and l['p'] > 0):
            masks.append(None)
            continue
        counter += 1
        seed = (model.seed * 1000003 + counter) & 0xFFFFFFFFFFFF
        m = torch.empty(c['B'] * T * c['ND'] * c['H'], device='cuda')
        H.call('asr_dropout_mask', H.ptr(m), m.numel(), float(l['p']), seed, H.stream_ptr())
        masks.append(m.view(c['B'], T, c['ND'] * c['H']).cpu().double())
        assert 0.5 < float(m.mean()) < 0.95
    return masks, counter


def _run(c, prec, monkeypatch, overlap=False):
    """Every step of one case: [(step, report)]; asserts storage, plans, dtypes, counters and the abort words on the way."""
    _setenv(monkeypatch, overlap)
    from src import functions as F
    from src import hipabi as H
    from src.asr import ASR, _RunCtx
    from src.module import RNNLayer
    precflag = H.BF16 if prec == 'bf16' else H.F32
    sd, x, dout, _ = R.inputs(c, 0, prec, masks=None)
    model = ASR(c['Din'], R.V, c['B'], prec=prec, seed=SEED, **R.model_cfg(c))
    assert list(model.state_dict().keys()) == list(sd.keys())
    model.load_state_dict(sd)
    model = model.cuda()
    model = model.train() if c['train'] else model.eval()
    model._drop_counter = 0
    layers = [m for m in model.encoder.layers if isinstance(m, RNNLayer)]
    storage = c['storage'][prec]
    for m, (T, T2, Din, Dz), st in zip(layers, R.frames(c), storage):
        took = F.rnn_fast_ok(m, types.SimpleNamespace(shape=(c['B'], T, Din)), precflag)
        assert took == (st == 'bf16'), '%s %s: layer storage %s, table %s' % (c['id'], prec, took, st)
    for l, B, T, Hd, ND in R.f32_layers(c, prec):
        assert int(H.lib().asr_lstm_plan(B, T, Hd, ND, precflag)) == R.F32_PLANS[(B, Hd, ND, prec)]
    packed = []
    hooks = [m.register_forward_pre_hook(lambda mod, args: packed.append('_pack16_ev' in mod.__dict__)) for m in layers[1:]]
    bound = R.bounds(c, prec)
    lens = torch.full((c['B'],), c['T'], dtype=torch.int64, device='cuda')
    reports = []
    try:
        for step in range(1, c['steps'] + 1):
            del packed[:]
            masks, after = _device_masks(H, model, c, model._drop_counter)
            model.zero_grad()
            xd = x.to('cuda', torch.bfloat16 if c['x_bf16'] else torch.float32).requires_grad_(c['need_dx'])
            out, out_len = model.encoder(xd, lens, _RunCtx(model))
            assert model._drop_counter == after
            assert out.dtype == (torch.bfloat16 if storage[-1] == 'bf16' else torch.float32)
            assert tuple(out.shape) == (c['B'],) + R.frames(c)[-1][1::2]
            out32 = F.to_f32_fn(out)
            (out32 * dout.to('cuda', torch.float32)).sum().backward()
            H.join_side()
            torch.cuda.synchronize()
            H.raise_if_aborted()
            # the path the step took
            want_packed = [bool(overlap and c['train'] and prec == 'bf16' and step >= 2 and st == 'bf16') for st in storage[1:]]
            assert packed == want_packed, (step, packed, want_packed)
            assert not any('_pack16_ev' in m.__dict__ for m in layers)
            for m, st in zip(layers, storage):
                if st == 'bf16':
                    assert [m.__dict__['_ws16_cache'][(c['B'], b)][1] for b in (0, 1)] == [step, step]     # launch epoch of the cached workspace
            if c['need_dx']:
                assert xd.grad.dtype == xd.dtype
                dx = xd.grad.double().cpu()
            else:
                assert xd.grad is None
                dx = None
            got = {'out': out32.detach().double().cpu(), 'dx': dx}
            for k, p in model.named_parameters():
                if k.startswith('encoder.'):
                    got['grad.' + k] = p.grad.detach().double().cpu().clone()
            ref = R.layers_f64(c, sd, x, masks, dout)
            # frames the reference defines as exact zeros are exact zeros
            assert bool((got['out'][ref['out'] == 0] == 0).all())
            reports.append((step, R.check(got, ref, bound)))
    finally:
        for h in hooks:
            h.remove()
    return reports


def _judge(c, prec, reports, tag=''):
    bad = []
    for step, rep in reports:
        worst = max(rep, key=lambda r: r[1] / r[2])
        print('RATIO %s %s%s step %d: %.3f (%s %.3e, bound %.3e)' % (c['id'], prec, tag, step, worst[1] / worst[2], worst[0], worst[1], worst[2]))
        if not all(r[3] for r in rep):
            bad.append('step %d\n' % step + '\n'.join('%-60s %.3e bound %.3e %s' % (k, v, b, 'ok' if ok else 'FAIL') for k, v, b, ok in rep))
    assert not bad, '%s %s%s storage %s\n' % (c['id'], prec, tag, c['storage'][prec]) + '\n'.join(bad)


@pytest.mark.parametrize('prec', R.PRECS)
@pytest.mark.parametrize('case', R.CASES, ids=[c['id'] for c in R.CASES])
def test_encoder_layers_vs_float64(case, prec, monkeypatch):
    _judge(case, prec, _run(case, prec, monkeypatch))


def test_two_steps_with_overlap(monkeypatch):
    """The two-step stack case with the overlap on: step 1 packs layer 1's weights in line, step 2 takes the copies prepack16 made
    on the side stream (asserted in _run), parameter gradients deferred beside the backward recurrence; both steps against float64."""
    c = R.BY_ID['stack_bf16x2_two_steps']
    _judge(c, 'bf16', _run(c, 'bf16', monkeypatch, overlap=True), tag=' overlap')


@pytest.mark.parametrize('case,error', R.REFUSED, ids=[c['id'] for c, _ in R.REFUSED])
def test_refused(case, error):
    """What the table lists as refused raises on the host, in either precision, before a model exists or a kernel is launched."""
    from src.asr import ASR
    for prec in R.PRECS:
        with pytest.raises(error):
            ASR(case['Din'], R.V, case['B'], prec=prec, **R.model_cfg(case))
    torch.cuda.synchronize()
