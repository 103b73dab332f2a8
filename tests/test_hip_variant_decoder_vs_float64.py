"""The variant decoder loop and the GRU encoder layers as the model composes them, against float64, at their edges.

Each case of tests/test_variant_decoder_reference.py::CASES builds src.asr.ASR with the case's attention and decoder block from
seeded_state_dict (bf16 mode: weights and encoder output rounded to bf16 before either side sees them), asserts that the model
leaves the fast path, calls src.variants.variant_decoder on a synthetic encoder output in train or eval mode as the case says,
then runs backward from (logits * dlogits).sum() + (att * watt).sum().  The dropout masks are regenerated with asr_dropout_mask
from model.seed and _drop_counter (the rule of tests/test_variants.py::test_decoder_and_embedding_dropout_vs_oracle) and fed to
the float64 side, which is teacher-forced with the tokens the device fed (model._last_tokens).  Logits, attention rows, states,
d enc and every attention / decoder / embedding parameter gradient are held to the case's own bounds (8 x the rounded twin's
error E0, computed on the CPU: the reference file's docstring) under the relative Frobenius and `proj` metrics; attention past
enc_len is exactly 0, rows sum to 1 within the attention bound, everything is finite and a second, backward-free forward is
bit-equal to the first.  Greedy cases: every token the device chose is an argmax of the float64 logits up to the logits bound.
Sampled cases: the decisions are fixed (model._tf_decisions; torch.rand is made to raise), teacher tokens stand where the decision
says teacher, at least one sampled token differs from the teacher's, all lie in [0, V).

The GRU encoder layer cases (GRU_CASES) go through model.encoder(x, lens, _RunCtx(model)) with ASR_OVERLAP=0; the whole-model
case (ctc_weight 0.5, GRU encoder layer, dot attention with 2 heads) runs model.forward in training mode with the overlap and
the CTC side branch on, inside work_stream(): the CTC head runs on the side stream beside the variant loop (one side_branch
entered), the encoder output's gradient has both consumers, and every parameter gradient - the encoder layer's among them - is
held to the float64 gradient of the summed loss.

Every run prints `RATIO <case> <precision>: worst metric / bound (metric, value, bound)`.

Which contractions run in bf16: all of them in bf16 mode, none in fp32 mode - asr_gemm's MFMA follows `prec` alone, M = 1 rows,
K = 1 outer products and seqT / bshift only choose the loader (reference file's docstring; test_plan_takes_the_odd_shapes).

Measured on MI355X: 46 decoder cases x 2 precisions = 92 case runs, 14 GRU encoder layer cases x 2 = 28, the whole-model case
x 2; every one run and none skipped; two refusals (test_refused).  The longest case takes 0.6 s (the first, which loads the
library), the rest 0.05 - 0.2 s.  Worst metric / bound per group (bf16 mode unless said):
    dot                 0.133  dot_mh_sampled, grad of attention.proj_q.weight (4.96e-3, bound 3.73e-2)
    loc                 0.276  loc_greedy, grad of att_layer.loc_proj.weight (1.27e-2, bound 4.60e-2)
    multi-head          0.133  dot_mh_sampled, as above
    GRU decoder         0.276  loc_greedy, as above
    dropout             0.134  loc_embdrop_sampled, grad of decoder.layers.bias_hh_l0 (2.56e-3, bound 1.91e-2)
    greedy              0.276  loc_greedy, as above; dot_greedy 0.120
    sampled             0.134  loc_embdrop_sampled, as above
    GRU encoder         0.404  g_all_on, proj of layers.0 ln.bias (1.75e-3, bound 4.33e-3)
    whole model         0.125  grad of attention.proj_k.bias (2.41e-2, bound 1.93e-1); fp32 0.179
    fp32 mode, all      0.281  loc_len1, grad of att_layer.gen_energy.bias (4.46e-5, bound 1.59e-4)
The device sits at 0.1 - 0.4 of 8 x E0 everywhere, i.e. at about E0 itself: the twin's rounding points are the device's.

Found on the way:
  * No defect of the chain: every metric of every case is within its bound on the first run, in both precisions.
  * Scheduled sampling on the variant path could not be tested (the loop drew torch.rand and recorded nothing): variant_decoder
    now honours model._tf_decisions where tf_rate != 1, as att_decoder_forward_sampled does, and leaves the fed tokens in
    model._last_tokens; draws and their order are unchanged when no decisions are set.
  * gen_energy.bias's gradient is analytically zero (the softmax Jacobian's rows sum to zero) and the device's value is fp32
    cancellation noise, 4e-5 of the 1e-3 x largest-gradient floor of the metric.  A float64 twin has no such noise (E0 = 1e-17)
    and would have left this metric to the 2^-24 floor; the twin therefore runs in float32 between its bf16 rounding points in
    bf16 mode as well ("everything else is fp32"), which is stated in the reference file and was fixed before the first device
    run.
  * Not every mutant is visible at every case: the initial prev_att over T' instead of enc_len changes nothing for an utterance of
    one frame beside a full one (its softmax has one entry); mutant 4 is judged at loc_2_F (lengths 9, 4, 7).
  * A GRU layer below an LSTM layer cannot be stated: the encoder block names one module for all layers and a list is refused
    with NotImplementedError (GRU_REFUSED).
"""
import ctypes

import pytest
import torch

import test_variant_decoder_reference as R

pytestmark = pytest.mark.gpu

SEED = 5                       # model.seed of the dropout and sampling cases


def _setenv(monkeypatch, overlap, ctc_side=False):
    for k in ('ASR_OVERLAP', 'ASR_CTC_SIDE', 'ASR_FAST16', 'ASR_OVERLAP_DP'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('ASR_OVERLAP', '1' if overlap else '0')
    monkeypatch.setenv('ASR_CTC_SIDE', '1' if ctc_side else '0')


def _mask(H, shape, p, seed):
    m = torch.empty(shape, dtype=torch.float32, device='cuda')
    H.call('asr_dropout_mask', H.ptr(m), m.numel(), float(p), int(seed), H.stream_ptr())
    return m.cpu().double()


def _seed(model, k):
    return (model.seed * 1000003 + k) & 0xFFFFFFFFFFFF


def _decoder_masks(H, model, c):
    """The masks variant_decoder draws from _drop_counter = 0, in its order: the teacher embeddings' (B, L, dim) once, then per
    step the inter-layer masks, the final one and, where the step samples its token, that token's embedding's (B, dim) - which
    takes the place of the teacher's row in the mask the float64 side reads.  Returns (masks or None, the counter afterwards)."""
    if not c['train'] or (c['dec_p'] == 0 and c['emb_p'] == 0):
        return None, 0
    B, L, NL, k = c['B'], c['L'], c['NL'], 0
    masks = {'emb': None, 'layer': [], 'final': []}
    if c['emb_p'] > 0:
        k += 1
        masks['emb'] = _mask(H, (B, L, R.DIM), c['emb_p'], _seed(model, k))
    for t in range(L):
        lm = []
        if c['dec_p'] > 0:
            for l in range(NL - 1):
                k += 1
                lm.append(_mask(H, (B, R.DIM), c['dec_p'], _seed(model, k)))
            k += 1
            masks['final'].append(_mask(H, (B, R.DIM), c['dec_p'], _seed(model, k)))
        masks['layer'].append(lm)
        if c['feed'] == 'sampled' and not c['decisions'][t] and c['emb_p'] > 0:
            k += 1
            masks['emb'][:, t] = _mask(H, (B, R.DIM), c['emb_p'], _seed(model, k))
    return masks, k


def _judge(cid, prec, rep, tag=''):
    worst = max(rep, key=lambda r: r[1] / r[2])
    print('RATIO %s %s%s: %.3f (%s %.3e, bound %.3e)' % (cid, prec, tag, worst[1] / worst[2], worst[0], worst[1], worst[2]))
    bad = '\n'.join('%-60s %.3e bound %.3e FAIL' % (k, v, b) for k, v, b, ok in rep if not ok)
    assert not bad, '%s %s%s\n%s' % (cid, prec, tag, bad)


def _run_decoder(c, prec, monkeypatch):
    _setenv(monkeypatch, overlap=False)
    from src import hipabi as H
    from src.asr import ASR, _RunCtx
    from src.variants import variant_decoder
    assert H.MAX_DEC_LAYERS == R.MAX_DEC_LAYERS
    inp = R.inputs(c, c['run_seed'], prec, masks=None)
    sd = inp['sd']
    model = ASR(R.EIN, R.V, c['B'], prec=prec, seed=SEED, **R.model_cfg(c))
    assert list(model.state_dict().keys()) == list(sd.keys())
    model.load_state_dict(sd)
    model = model.cuda()
    model = model.train() if c['train'] else model.eval()
    # the model takes the variant path (the choice of ASR.forward)
    assert not (model.decoder.fast and model.attention.fast and model.emb_drop == 0.0) and R.leaves_fast_path(c)
    sampled, greedy = c['feed'] == 'sampled', c['feed'] == 'greedy'
    if sampled:
        model._tf_decisions = list(c['decisions'])

        def no_draw(*a, **k):
            raise AssertionError('torch.rand drawn although the decisions are fixed')
        monkeypatch.setattr(torch, 'rand', no_draw)
    B, L, Tp = c['B'], c['L'], c['Tp']
    lens = inp['lens'].to(torch.int32 if c['len_dtype'] == 'int32' else torch.int64).cuda()
    teacher = None if greedy else inp['teacher'].cuda()

    def forward(grad):
        model._drop_counter, model._ss_counter = 0, 0
        enc = inp['enc'].to('cuda', torch.float32).requires_grad_(grad and c['need_denc'])
        ctx = _RunCtx(model)
        with torch.set_grad_enabled(grad):
            logits, att, states = variant_decoder(model, ctx.anchor, enc, lens, L, teacher, 0.5 if sampled else 1.0, ctx)
        return enc, logits, att, states, model._last_tokens.clone()

    masks, after = _decoder_masks(H, model, c)
    model.zero_grad()
    enc, logits, att, states, fed = forward(True)
    assert model._drop_counter == after
    assert tuple(logits.shape) == (B, L, R.V) and tuple(att.shape) == (B, c['NH'], L, Tp) and tuple(states.shape) == (B, L, R.DIM)
    ((logits * inp['dl'].to('cuda', torch.float32)).sum() + (att * inp['wa'].to('cuda', torch.float32)).sum()).backward()
    H.join_side()
    torch.cuda.synchronize()
    H.raise_if_aborted()
    # ---- the tokens that were fed
    fed = fed.cpu()
    assert tuple(fed.shape) == (B, L) and fed.dtype == torch.int64 and bool((fed[:, 0] == 0).all())
    assert int(fed.min()) >= 0 and int(fed.max()) < R.V
    if c['feed'] == 'teacher':
        assert torch.equal(fed, inp['fed'])
    if sampled:
        differs = 0
        for t, use_teacher in enumerate(c['decisions'][:L - 1]):
            if use_teacher:
                assert torch.equal(fed[:, t + 1], inp['teacher'][:, t]), t
            else:
                differs += int((fed[:, t + 1] != inp['teacher'][:, t]).sum())
        assert differs >= 1
        assert model._ss_counter == sum(1 for d in c['decisions'] if not d)
    # ---- float64, teacher := fed tokens, the device's masks
    ref_inp = dict(inp, fed=fed, masks=masks)
    ref = R.dec_f64(c, ref_inp)
    if c['need_denc']:
        denc = enc.grad.double().cpu()
    else:
        assert enc.grad is None
        denc = None
    got = {'logits': logits.detach().double().cpu(), 'att': att.detach().double().cpu(), 'states': states.detach().double().cpu(), 'denc': denc}
    for k, p in model.named_parameters():
        if not k.startswith('encoder.'):
            got['grad.' + k] = p.grad.detach().double().cpu().clone()
    for k, v in got.items():
        assert v is None or bool(torch.isfinite(v).all()), k
    bound = R.bounds(c, prec)
    a = got['att']
    for b, n in enumerate(c['lens']):
        assert float(a[b, :, :, n:].abs().sum()) == 0.0                      # attention past enc_len is exactly 0
    assert float((a.sum(-1) - 1).abs().max()) <= bound['att']
    if greedy:
        d = R.greedy_delta(c, prec, ref['logits'])
        r = ref['logits']
        chosen = r.gather(-1, got['logits'].argmax(-1, keepdim=True)).squeeze(-1)
        assert bool((chosen >= r.max(-1).values - 2 * d).all())
        assert torch.equal(fed[:, 1:], got['logits'].argmax(-1)[:, :-1])    # what was fed is what the device's own logits chose
        assert torch.equal(fed, inp['fed'])                                  # and, by the margin of the run seed, the float64 greedy tokens
    rep = R.check(got, ref, bound)
    # ---- a second, backward-free forward is bit-equal
    _, logits2, att2, states2, fed2 = forward(False)
    torch.cuda.synchronize()
    assert torch.equal(logits2, logits) and torch.equal(att2, att) and torch.equal(states2, states) and torch.equal(fed2.cpu(), fed)
    return rep


@pytest.mark.parametrize('prec', R.PRECS)
@pytest.mark.parametrize('case', R.CASES, ids=[c['id'] for c in R.CASES])
def test_variant_decoder_vs_float64(case, prec, monkeypatch):
    _judge(case['id'], prec, _run_decoder(case, prec, monkeypatch))


def test_nothing_of_the_decoder_table_is_refused():
    """Every decoder case is launched: the host refuses none of the table's shapes (the refusals of the encoder table: below)."""
    assert R.REFUSED == []


# ----------------------------------------------------------------------------------------------------------------------
# GRU encoder layers
# ----------------------------------------------------------------------------------------------------------------------
def _run_gru(c, prec, monkeypatch):
    _setenv(monkeypatch, overlap=False)
    from src import functions as F
    from src import hipabi as H
    from src.asr import ASR, _RunCtx
    from src.module import RNNLayer
    inp = R.gru_inputs(c, 0, prec, masks=None)
    sd = inp['sd']
    model = ASR(c['Din'], R.V, c['B'], prec=prec, seed=SEED, **R.gru_model_cfg(c))
    assert list(model.state_dict().keys()) == list(sd.keys())
    model.load_state_dict(sd)
    model = model.cuda()
    model = model.train() if c['train'] else model.eval()
    model._drop_counter = 0
    assert all(isinstance(m, RNNLayer) and m.module == 'GRU' for m in model.encoder.layers)
    masks, k = [], 0
    for (T, T2, Din, Dz), l in zip(R.gru_frames(c), c['layers']):
        if c['train'] and l['p'] > 0:
            k += 1
            masks.append(_mask(H, (c['B'], T, c['ND'] * c['H']), l['p'], _seed(model, k)))
            assert 0.5 < float(masks[-1].mean()) < 0.95
        else:
            masks.append(None)
    model.zero_grad()
    xd = inp['x'].to('cuda', torch.float32).requires_grad_(True)
    lens = inp['lens'].cuda()
    out, out_len = model.encoder(xd, lens, _RunCtx(model))
    assert model._drop_counter == k
    rate = 1
    for l in c['layers']:
        rate *= l['rate']
    fr = R.gru_frames(c)
    assert out.dtype == torch.float32 and tuple(out.shape) == (c['B'],) + fr[-1][1::2]
    want_len = inp['lens']
    for l in c['layers']:
        want_len = want_len // l['rate']
    assert torch.equal(out_len.cpu(), want_len)
    (F.to_f32_fn(out) * inp['dout'].to('cuda', torch.float32)).sum().backward()
    H.join_side()
    torch.cuda.synchronize()
    H.raise_if_aborted()
    got = {'out': out.detach().double().cpu(), 'dx': xd.grad.double().cpu()}
    for kk, p in model.named_parameters():
        if kk.startswith('encoder.'):
            got['grad.' + kk] = p.grad.detach().double().cpu().clone()
    for kk, v in got.items():
        assert bool(torch.isfinite(v).all()), kk
    ref = R.gru_f64(c, dict(inp, masks=masks if c['train'] else None))
    assert bool((got['out'][ref['out'] == 0] == 0).all())                    # dropped units are exact zeros
    return R.check(got, ref, R.gru_bounds(c, prec))


@pytest.mark.parametrize('prec', R.PRECS)
@pytest.mark.parametrize('case', R.GRU_CASES, ids=[c['id'] for c in R.GRU_CASES])
def test_gru_encoder_layers_vs_float64(case, prec, monkeypatch):
    _judge(case['id'], prec, _run_gru(case, prec, monkeypatch))


@pytest.mark.parametrize('case,over,error', R.GRU_REFUSED, ids=[c['id'] for c, _, _ in R.GRU_REFUSED])
def test_refused(case, over, error):
    """What the table lists as refused raises on the host, in either precision, before a model exists or a kernel is launched."""
    from src.asr import ASR
    for prec in R.PRECS:
        cfg = R.gru_model_cfg(case)
        cfg['encoder'].update(over)
        with pytest.raises(error):
            ASR(case['Din'], R.V, case['B'], prec=prec, **cfg)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# the whole model: CTC head on the side stream beside the variant loop
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', R.PRECS)
def test_whole_model_ctc_beside_variant_loop(prec, monkeypatch):
    _setenv(monkeypatch, overlap=True, ctc_side=True)
    from src import hipabi as H
    from src.asr import ASR
    entered = [0]

    class Counting(H.side_branch):
        def __enter__(self):
            entered[0] += 1
            return super().__enter__()
    monkeypatch.setattr(H, 'side_branch', Counting)
    d, e = R.WHOLE['dec'], R.WHOLE['enc']
    inp = R.whole_inputs(0, prec)
    sd = inp['sd']
    model = ASR(R.EIN, R.V, d['B'], prec=prec, seed=SEED, **R.whole_model_cfg())
    assert list(model.state_dict().keys()) == list(sd.keys())
    model.load_state_dict(sd)
    model = model.cuda().train()
    assert model.enable_ctc and model.enable_att and not model.attention.fast
    ws = H.work_stream()
    ws.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(ws):
        model.zero_grad()
        feat, flen, teacher = inp['x'].to('cuda', torch.float32), inp['lens'].cuda(), inp['teacher'].cuda()
        ctc, enc_len, logits, att, _ = model(feat, flen, d['L'], tf_rate=1.0, teacher=teacher)
        assert entered[0] == 1                                               # the CTC head went to the side stream
        f32 = lambda t: t.to('cuda', torch.float32)
        ((ctc * f32(inp['dctc'])).sum() + (logits * f32(inp['dl'])).sum() + (att * f32(inp['wa'])).sum()).backward()
        H.join_side()
    torch.cuda.current_stream().wait_stream(ws)
    torch.cuda.synchronize()
    H.raise_if_aborted()
    assert torch.equal(enc_len.cpu(), inp['lens']) and torch.equal(model._last_tokens.cpu(), inp['fed'])
    got = {'ctc': ctc.detach().double().cpu(), 'logits': logits.detach().double().cpu(), 'att': att.detach().double().cpu()}
    for k, p in model.named_parameters():
        got['grad.' + k] = p.grad.detach().double().cpu().clone()
    ref = R.whole_f64(inp)
    assert {'grad.encoder.layers.0.pj.weight', 'grad.encoder.layers.0.layer.weight_hh_l0_reverse', 'grad.ctc_layer.0.weight'} <= set(ref)
    _judge(R.WHOLE['id'], prec, R.check(got, ref, R.whole_bounds(prec)))


# ----------------------------------------------------------------------------------------------------------------------
# the contraction shapes of the path, as the plan query sees them
# ----------------------------------------------------------------------------------------------------------------------
def _plan(H, A, B, C, M, N, K, lda, ldb, ldc, a_kc, b_kc, accum=0, splits=1, batch=1, sA=0, sB=0, sC=0, seqT=0, bshift=0, prec=None):
    out = (ctypes.c_int * 8)()
    rc = H.lib().asr_gemm_plan(H.ptr(A), H.ptr(B), H.ptr(C), None, M, N, K, lda, ldb, ldc, a_kc, b_kc, H.ACT_NONE, accum, splits,
                               batch, sA, sB, sC, seqT, bshift, prec, out)
    assert rc == 0, H.lib().asr_last_error()
    return dict(zip(('fastA', 'fastB', 'plain_order', 'nx', 'ny', 'nz', 'gx', 'ngx'), list(out)))


def test_plan_takes_the_odd_shapes():
    """The M = 1 batched rows of DotEnergyFn / AttendFn, their K = 1 outer-product accumulations and GRUSeqFn's seqT / bshift weight
    gradient are each ONE asr_gemm launch of `batch` (x splits) slices of one tile, planned identically in both precisions: `prec`
    selects the MFMA of that launch and nothing else, the shape only the loader (fast where the contiguous extent is a multiple
    of 4 and the rows are 16-byte aligned)."""
    from src import hipabi as H
    Rr, T, D, Dv = 6, 9, 8, 16
    q, key, e = (torch.zeros(s, device='cuda') for s in ((Rr, D), (Rr, T, D), (Rr, T)))
    val, ctxv = torch.zeros(Rr, T, Dv, device='cuda'), torch.zeros(Rr, Dv, device='cuda')
    B, Tg, Hd, ND = 3, 5, 16, 2
    G, Dy = ND * 3 * Hd, ND * Hd
    gh, y, gw = torch.zeros(B * Tg, G, device='cuda'), torch.zeros(B * Tg, Dy, device='cuda'), torch.zeros(ND, 3 * Hd, Hd, device='cuda')
    plans = {}
    for prec in (H.BF16, H.F32):
        plans[prec] = [
            _plan(H, q, key, e, 1, T, D, D, D, T, 1, 1, batch=Rr, sA=D, sB=T * D, sC=T, prec=prec),                 # energy = q . key
            _plan(H, e, key, q, 1, D, T, T, D, D, 1, 0, batch=Rr, sA=T, sB=T * D, sC=D, prec=prec),                 # dq
            _plan(H, e, q, key, T, D, 1, T, D, D, 0, 0, accum=1, batch=Rr, sA=T, sB=D, sC=T * D, prec=prec),        # key.grad += de (x) q
            _plan(H, e, val, ctxv, 1, Dv, T, T, Dv, Dv, 1, 0, batch=Rr, sA=T, sB=T * Dv, sC=Dv, prec=prec),         # context
            _plan(H, ctxv, val, e, 1, T, Dv, Dv, Dv, T, 1, 1, batch=Rr, sA=Dv, sB=T * Dv, sC=T, prec=prec),         # dattn
            _plan(H, e, ctxv, val, T, Dv, 1, T, Dv, Dv, 0, 0, accum=1, batch=Rr, sA=T, sB=Dv, sC=T * Dv, prec=prec),   # value.grad
            _plan(H, gh, y, gw[0], 3 * Hd, Hd, B * Tg, G, Dy, Hd, 0, 0, accum=1, splits=H.wgrad_splits(B * Tg, 3 * Hd, Hd), seqT=Tg,
                  bshift=-1, prec=prec),                                                                             # GRU dW_hh
        ]
    assert plans[H.BF16] == plans[H.F32]
    p = plans[H.BF16]
    for pl in p[:6]:
        assert (pl['nx'], pl['ny'], pl['nz']) == (1, 1, Rr)
    assert [(pl['fastA'], pl['fastB']) for pl in p[:6]] == [(1, 1), (0, 1), (0, 1), (0, 1), (1, 1), (0, 1)]
    assert (p[6]['nx'], p[6]['ny'], p[6]['nz']) == (1, 1, 1) and (p[6]['fastA'], p[6]['fastB']) == (1, 1)
    torch.cuda.synchronize()
