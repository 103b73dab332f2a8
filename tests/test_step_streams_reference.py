"""The family table and the float64 schedule behind tests/test_hip_step_streams.py, which holds the layer BETWEEN the kernels -
which stream a launch goes to, when a deferred closure runs, when the optimizer reads the flat gradient (src/hipabi.py
defer_side / flush_side / join_side / side_branch / begin_forward / work_stream, src/functions.py layer_backward / prepack16,
src/step.py, bin/train_asr.py) - to its in-line order and to float64.  Nothing here needs a GPU.

Base family: the model of smoke() and tests/test_dp_hooks.MC (D=40, V=31, B=4, T=50, L=8, bi-LSTM [32,32,32] with projections,
'drop' rates [1,2,1], dropout 0.1, location attention 24 / 4 x 5, LSTM decoder 24, ctc_weight 0.5): the smallest dims at which
every encoder layer still takes the bf16 storage (LayerBF16: H % 16 == 0, input width % 8 == 0).  Each other family changes one
thing (FAMILIES below; `what` says which code it reaches).

Every family runs K = 3 steps at the shapes (T, L), (T2 ~ 3T/4, L - 2), (T, L): step 1 takes the first-step path (prepack16
returns early, every work area is new), step 2 is the first with the weight copies packed on the side stream and the other
launch parity of the recurrence work areas, step 3 meets the first shape's work areas again.  T2 is rounded to a value that is
even behind the front-end, so that 'drop' and 'concat' agree with the oracle's x_len // rate.  Global-norm clip 0.05 (active,
as in test_dp_hooks) on `base`, 5.0 elsewhere.

`dec_plan`.  The host plan queries (asr_att_decoder_fwd_plan / _bwd_plan) report a persistent plan for the MID dims of
tests/test_decoder_dims_vs_oracle.py from T' = 1 on (PLAN_MIN_TP, asserted below): at these widths no T' is too short for a
plan.  What binds the shape from below is CTC: the shortest row of a batch keeps T'/2 frames and must hold L labels and their
repeats, so the family runs T' = 32 and 24 (both forward plans 1 = LDS-resident, backward plan 1).

Two families have no float64 schedule of their own forward: `emb` (the oracle has no plugin; the module is held by
tests/test_hip_emb_plugin.py) runs the oracle of the model alone here and is held to the in-line run on the GPU; `sampled` runs
the oracle teacher-forced on the tokens that were FED (labels at the teacher's positions, other tokens where a sample was taken).

CPU tests: the float64 schedule (O.asr_losses + _adadelta_ref) of every family is finite and CTC-feasible; a float32 CPU run,
held step by step to the float64 oracle started from the same parameters, passes test_hip_model.compare at its fp32 tolerances
and _adadelta_tol on the update - the same comparison the GPU file makes with the device in the float32 run's place; every
table entry builds and its storage classes and plans are the row's.
"""
import copy
import ctypes
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

from oracle import asr_oracle as O
from test_dp_hooks import MC
from test_hip_losses_vs_float64 import _adadelta_ref, _adadelta_tol
from test_hip_model import compare, finish

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from batchgen import make_batch      # noqa: E402

D, V, K_STEPS = 40, 31, 3
PLAN_MIN_TP = 1            # smallest T' at which both plan queries report a persistent plan at the dec_plan dims


def _mc(**over):
    mc = copy.deepcopy(MC)
    for path, v in over.items():
        sec, _, key = path.partition('.')
        if key:
            mc[sec][key] = v
        else:
            mc[sec] = v
    return mc


def _fam(mc, what, B=4, T=50, T2=38, L=8, precs=('bf16',), clip=5.0, tf_rate=1.0, emb=False, storage=None, plans=(1, 0), dec_fast=True,
         joint=True):
    return dict(mc=mc, what=what, B=B, T=T, T2=T2, L=L, precs=precs, clip=clip, tf_rate=tf_rate, emb=emb,
                storage=storage or ['bf16'] * len(mc['encoder']['dim']), plans=plans, dec_fast=dec_fast, joint=joint)


# storage: the class of every encoder LSTM layer in bf16 contraction mode ('bf16' LayerBF16, 'f32' LayerF32; all 'f32' in fp32 mode
# and under ASR_FAST16=0).  plans: (asr_att_decoder_fwd_plan, asr_att_decoder_bwd_plan) at the first shape, bf16 mode; 0 per-step,
# 1 LDS-resident, 2 streamed; None for a model without the shipped decoder.
FAMILIES = {
    'base': _fam(_mc(), 'all-LayerBF16 stack (bf16) / all-LayerF32 stack with deferred head and decoder gradients (fp32)',
                 precs=('bf16', 'fp32'), clip=0.05),
    'dec_plan': _fam(_mc(**{'encoder.dim': [128], 'encoder.dropout': [0.1], 'encoder.layer_norm': [False], 'encoder.proj': [True],
                            'encoder.sample_rate': [1], 'attention.dim': 128, 'attention.loc_kernel_num': 5,
                            'attention.loc_kernel_size': 20, 'decoder.dim': 128}),
                     'asr_att_decoder_bwd_params deferred behind a persistent backward; _DEC_WS met again after another shape',
                     B=8, T=32, T2=24, plans=(1, 1)),
    'mixed': _fam(_mc(**{'encoder.layer_norm': [False, True, False], 'encoder.sample_style': 'concat',
                         'encoder.proj': [True, False, True]}),      # the reference's projection is H x H: none behind a 'concat'
                  'a LayerF32 layer (LayerNorm, concat) between two LayerBF16 layers: closures deferred above it cross it',
                  storage=['bf16', 'f32', 'bf16']),
    'vgg1': _fam(_mc(**{'encoder.vgg': 1, 'encoder.dim': [32, 32], 'encoder.dropout': [0.1, 0.1], 'encoder.layer_norm': [False, False],
                        'encoder.proj': [True, True], 'encoder.sample_rate': [1, 1]}),
                 'front-end backward below deferred layers', T=48, T2=40, L=5, plans=(1, 0)),
    'variant': _fam(_mc(**{'decoder.module': 'GRU', 'decoder.layer': 2, 'attention.mode': 'dot', 'attention.num_head': 2}),
                    'variant_decoder above an overlapping encoder', plans=None, dec_fast=False),
    'ctc_only': _fam(_mc(ctc_weight=1.0), "the head's deferral alone; side_ctc must stay off", plans=None, joint=False),
    'att_only': _fam(_mc(ctc_weight=0.0), 'no head; side_ctc must stay off', joint=False),
    'sampled': _fam(_mc(), 'att_decoder_forward_sampled and _ss_counter', tf_rate=0.5),
    'emb': _fam(_mc(), "step_emb_optimizer reading the model's norm", emb=True),
}
CASES = [(f, p) for f, fam in FAMILIES.items() for p in fam['precs']]


def family_cfg(fid):
    fam = FAMILIES[fid]
    return fam, O.ModelCfg(fam['mc'], D, V)


def shapes(fam):
    return [(fam['T'], fam['L']), (fam['T2'], fam['L'] - 2), (fam['T'], fam['L'])]


def batches(fid):
    """The K batches of a family as CPU tensors (feat, lens, txt): seeded per family and step."""
    fam = FAMILIES[fid]
    seed = 100 * (1 + sorted(FAMILIES).index(fid))
    return [tuple(torch.from_numpy(x) for x in make_batch(seed + k, fam['B'], T, D, L, V)) for k, (T, L) in enumerate(shapes(fam))]


def first_frames(cfg, T):
    """Frames that reach the first recurrent layer (a quarter of the input behind vgg 1)."""
    return T // 4 if cfg.vgg == 1 else T


def mask_shapes(cfg, B, T):
    """(B, T_l, width) of every layer's dropout mask: the mask covers the LSTM output, in front of the time down-sampling."""
    out, Tl = [], first_frames(cfg, T)
    for l, h in enumerate(cfg.enc_dim):
        out.append((B, Tl, (2 if cfg.bidirection else 1) * h))
        r = cfg.enc_sample_rate[l]
        if r > 1:
            Tl = (Tl + r - 1) // r if cfg.enc_sample_style == 'drop' else Tl // r
    return out


def host_masks(cfg, B, T, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return [torch.from_numpy((g.random(s) >= p).astype(np.float64)) for s, p in zip(mask_shapes(cfg, B, T), cfg.enc_dropout)]


def fed_tokens(txt, decisions, seed):
    """What scheduled sampling feeds: column t + 1 is the label of step t where decisions[t], else another token."""
    g = torch.Generator().manual_seed(seed)
    fed = txt.clone()
    for t, keep in enumerate(decisions):
        if not keep:
            fed[:, t] = torch.randint(1, V, (txt.shape[0],), generator=g)
    return fed


def decisions_for(L, step):
    """Teacher (True) or sample (False) behind each of the first L - 1 decoder steps: both kinds in every step of the schedule."""
    return [(t + step) % 2 == 0 for t in range(L - 1)]


def oracle_step(cfg, P, batch, masks, fed=None):
    """One forward + backward of the oracle at P's dtype: (outputs as numpy / floats, gradients as numpy, CTC-feasible).
    fed: the tokens fed to the decoder where they are not the labels (scheduled sampling); the losses read the labels."""
    feat, lens, txt = batch
    dt = next(iter(P.values())).dtype
    P = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    masks = None if masks is None else [m.to(dt) for m in masks]
    if fed is None:
        ref = O.asr_losses(feat.to(dt), lens, txt, P, cfg, label_smoothing=False, drop_masks=masks, lstm_impl=O.bilstm_aten)
    else:
        txt_len = (txt != 0).sum(-1)
        L = int(txt_len.max())
        ctc_out, enc_len, att_out, att_seq = O.asr_forward(feat.to(dt), lens, P, cfg, L, teacher=fed, drop_masks=masks, lstm_impl=O.bilstm_aten)
        ref = {'enc_len': enc_len, 'ctc_output': ctc_out, 'att_output': att_out, 'att_seq': att_seq,
               'ctc_loss': O.ctc_loss_aten(ctc_out, txt, enc_len, txt_len), 'att_loss': O.seq_loss(att_out, txt[:, :L], False)}
        ref['total_loss'] = ref['ctc_loss'] * cfg.ctc_weight + ref['att_loss'] * (1 - cfg.ctc_weight)
    ref['total_loss'].backward()
    out = {k: (ref[k].detach().numpy() if ref.get(k) is not None else None) for k in ('ctc_output', 'att_output', 'att_seq')}
    for k in ('ctc_loss', 'att_loss', 'total_loss'):
        out[k] = float(ref[k].detach()) if ref.get(k) is not None else None
    out['enc_len'] = ref['enc_len'].numpy()
    grads = {k: (P[k].grad.numpy() if P[k].grad is not None else np.zeros(tuple(P[k].shape), P[k].detach().numpy().dtype)) for k in P}
    feasible = bool(torch.isfinite(ref['total_loss'].detach()))
    return out, grads, feasible


def flat(d, keys):
    return np.concatenate([np.asarray(d[k], dtype=np.float64).reshape(-1) for k in keys])


def adadelta_update(keys, p, g, sq, ad, clip):
    """_adadelta_ref over the concatenation of the parameters in `keys` order, with the global norm of g for the clip."""
    normsq = math.fsum((g * g).tolist())
    return _adadelta_ref(p, g, sq, ad, 0.0, clip, normsq, 1.0)


def float64_schedule(fid, prec_seed=0):
    """The family's K steps in float64 from the seeded weights: list of (outputs, gradients, feasible, parameters after)."""
    fam, cfg = family_cfg(fid)
    sd = O.seeded_state_dict(O.param_shapes(cfg), 3)
    keys = list(sd)
    p = flat({k: v.numpy() for k, v in sd.items()}, keys)
    sq, ad = np.zeros_like(p), np.zeros_like(p)
    out = []
    for k, batch in enumerate(batches(fid)):
        P = unflat(p, sd, keys, torch.float64)
        masks = host_masks(cfg, fam['B'], batch[0].shape[1], 7 + k)
        fed = fed_tokens(batch[2], decisions_for(batch[2].shape[1], k), k) if fam['tf_rate'] != 1 else None
        o, g, ok = oracle_step(cfg, P, batch, masks, fed)
        p, sq, ad = adadelta_update(keys, p, flat(g, keys), sq, ad, fam['clip'])
        out.append((o, g, ok, p.copy()))
    return out


def unflat(p, sd, keys, dtype):
    P, o = {}, 0
    for k in keys:
        n = sd[k].numel()
        P[k] = torch.from_numpy(p[o:o + n].reshape(tuple(sd[k].shape))).to(dtype)
        o += n
    return P


@pytest.mark.parametrize('fid', sorted(FAMILIES))
def test_float64_schedule_is_finite_and_ctc_feasible(fid):
    fam, cfg = family_cfg(fid)
    p_prev = None
    for k, (o, g, ok, p) in enumerate(float64_schedule(fid)):
        assert ok and math.isfinite(o['total_loss']), (fid, k, o['total_loss'])
        assert all(np.isfinite(v).all() for v in g.values()) and np.isfinite(p).all()
        gn = math.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in g.values()))
        assert gn > 0 and (gn > fam['clip']) == (fid == 'base'), (fid, k, gn)      # the clip is active on base alone
        assert p_prev is None or not np.array_equal(p, p_prev)
        p_prev = p


@pytest.mark.parametrize('fid', sorted(FAMILIES))
def test_float32_host_run_agrees_with_float64(fid):
    """The float32 CPU run in the device's place: before each step the float64 oracle starts from the float32 run's parameters."""
    fam, cfg = family_cfg(fid)
    sd = O.seeded_state_dict(O.param_shapes(cfg), 3)
    keys = list(sd)
    P32 = {k: v.clone().float() for k, v in sd.items()}
    n = sum(v.numel() for v in sd.values())
    sq32, ad32 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for k, batch in enumerate(batches(fid)):
        masks = host_masks(cfg, fam['B'], batch[0].shape[1], 7 + k)
        fed = fed_tokens(batch[2], decisions_for(batch[2].shape[1], k), k) if fam['tf_rate'] != 1 else None
        o64, g64, ok = oracle_step(cfg, {kk: v.double() for kk, v in P32.items()}, batch, masks, fed)
        o32, g32, _ = oracle_step(cfg, P32, batch, masks, fed)
        assert ok and np.array_equal(o32['enc_len'], o64['enc_len'])
        shim = types.SimpleNamespace(named_parameters=lambda: [(kk, types.SimpleNamespace(grad=torch.from_numpy(g32[kk]))) for kk in keys])
        res = {kk: torch.as_tensor(v) for kk, v in o32.items() if v is not None}
        report = []
        compare(shim, res, o64, g64, 'fp32', report)
        finish(report)
        # the update in float32 torch arithmetic from the float32 gradient, against _adadelta_ref fed the same gradient
        gf = flat(g32, keys)
        p0 = flat({kk: v.numpy() for kk, v in P32.items()}, keys)
        want = adadelta_update(keys, p0, gf, sq32.astype(np.float64), ad32.astype(np.float64), fam['clip'])
        normsq = math.fsum((gf * gf).tolist())
        coef = np.float32(min(1.0, fam['clip'] / (math.sqrt(normsq) + 1e-6)))
        gi = gf.astype(np.float32) * coef
        sq32 = np.float32(0.9) * sq32 + np.float32(0.1) * gi * gi
        delta = np.sqrt(ad32 + np.float32(1e-8)) / np.sqrt(sq32 + np.float32(1e-8)) * gi
        ad32 = np.float32(0.9) * ad32 + np.float32(0.1) * delta * delta
        p1 = p0.astype(np.float32) - delta
        for name, got, ref in (('param', p1, want[0]), ('square_avg', sq32, want[1]), ('acc_delta', ad32, want[2])):
            err = np.abs(got.astype(np.float64) - ref)
            assert (err <= _adadelta_tol(ref)).all(), (fid, k, name, float(err.max()))
        P32 = unflat(p1.astype(np.float64), sd, keys, torch.float32)


def _hipabi():
    from test_decoder_dims_vs_oracle import _hipabi as h
    return h()


def plans_of(H, model, B, Tp, L):
    """(forward plan, backward plan) of the shipped decoder at a shape, from the host queries; None without that decoder."""
    from src import functions as F
    if not (model.enable_att and model.decoder.fast and model.attention.fast):
        return None
    d = F._dec_dims(model, B, Tp, L)
    return (int(H.lib().asr_att_decoder_fwd_plan(ctypes.byref(d))), int(H.lib().asr_att_decoder_bwd_plan(ctypes.byref(d))))


def storage_of(H, model, B, prec):
    """'bf16' / 'f32' per encoder LSTM layer: what rnn_fast_ok picks for a batch of B rows in contraction mode `prec`."""
    from src import functions as F
    from src.module import RNNLayer
    out = []
    for m in model.encoder.layers:
        if isinstance(m, RNNLayer):
            x = types.SimpleNamespace(shape=(B, 1, m.w_ih_cat.shape[1]))
            out.append('bf16' if F.rnn_fast_ok(m, x, H.BF16 if prec == 'bf16' else H.F32) else 'f32')
    return out


def encoder_frames(cfg, T):
    Tl = first_frames(cfg, T)
    for l, r in enumerate(cfg.enc_sample_rate):
        if r > 1:
            Tl = (Tl + r - 1) // r if cfg.enc_sample_style == 'drop' else Tl // r
    return Tl


def build_model(fid, prec, seed=9):
    """The family's model on the host with the seeded weights (the caller moves it to the device)."""
    from src.asr import ASR
    fam, cfg = family_cfg(fid)
    sd = O.seeded_state_dict(O.param_shapes(cfg), 3)
    model = ASR(D, V, fam['B'], prec=prec, seed=seed, **copy.deepcopy(fam['mc']))
    assert list(model.state_dict().keys()) == list(sd.keys())
    model.load_state_dict(sd)
    return fam, cfg, sd, model


@pytest.mark.parametrize('fid,prec', CASES)
def test_table_entry_builds_and_takes_its_row(fid, prec, monkeypatch):
    H = _hipabi()
    monkeypatch.delenv('ASR_FAST16', raising=False)
    fam, cfg, sd, model = build_model(fid, prec)
    assert storage_of(H, model, fam['B'], prec) == (fam['storage'] if prec == 'bf16' else ['f32'] * len(fam['storage']))
    assert model.enable_ctc == (cfg.ctc_weight > 0) and model.enable_att == (cfg.ctc_weight < 1)
    assert (model.enable_ctc and model.enable_att) == fam['joint']
    if model.enable_att:
        assert (model.decoder.fast and model.attention.fast) == fam['dec_fast']
    for T, L in shapes(fam):           # every down-sampling layer sees a multiple of its rate: ceil and floor agree
        assert cfg.vgg != 1 or T % 4 == 0
        for (_, Tl, _), r in zip(mask_shapes(cfg, fam['B'], T), cfg.enc_sample_rate):
            assert Tl % r == 0, (fid, T, Tl, r)
    assert plans_of(H, model, fam['B'], encoder_frames(cfg, fam['T']), fam['L']) == fam['plans']
    assert model.encoder.out_dim == cfg.enc_out_dim()


def test_dec_plan_shape_is_pinned_by_the_host_plan_query():
    H = _hipabi()
    fam, cfg, sd, model = build_model('dec_plan', 'bf16')
    ok = [t for t in range(1, 65) if min(plans_of(H, model, fam['B'], t, fam['L'])) > 0]
    assert ok and ok[0] == PLAN_MIN_TP
    for T, L in shapes(fam):
        assert T >= PLAN_MIN_TP and plans_of(H, model, fam['B'], T, L) == (1, 1), (T, L)
