"""The seam for an outside gradient on the decoder states (asr_att_decoder_bwd_hs, AttDecoderFn.backward), alone.

The backward pass forms dh_top = dlogits W_c with one contraction before any recurrence kernel; an outside gradient on the top
layer's h_t is added at that spot.  So, for a fixed C (B,L,V), the two runs
    A: dlogits = C,  no outside gradient                    B: dlogits = 0,  outside gradient = C W_c
hand the recurrence the same dh_top and must return the same denc and the same gradient of every parameter except W_c and b_c,
which only the first sees.  The allowed difference is the rounding of that one contraction of depth V against the product
formed in float64 on the host and rounded to float32.  It is derived here by making it zero: C holds multiples of 1/8 in [-2, 2]
and W_c is replaced by multiples of 1/64 in [-1, 1] - both exact in bf16 as well - so every product is a multiple of 2^-9 below
2 in size, any partial sum of V = 31 of them is a multiple of 2^-9 below 64 and fits float32's 24 bits: the device's sum is exact
in whichever order and at either precision, equal to the rounded float64 product, and everything behind it runs on equal bits.
The comparison is therefore for equality.

dhs_ext = NULL must be asr_att_decoder_bwd_ex bit for bit (the entry points called directly on one saved state).

Shapes: the debug decoder (two layers: the per-step loop) at B = 2, T' = 6, L = 4 in fp32 and bf16; the one-layer decoder of
librispeech_asr.yaml in bf16 on the streamed plan (B = 3, T' = 40, preferred by flag as tests/test_hip_decoder_stream.py does)
and, with the persistent backward switched off, on the per-step loop in bf16 and fp32 (fp32 has no persistent plan).  The
per-step shapes keep T' within one tile of the energy backward (8 frames): with more tiles that kernel adds its partial query
gradients with float atomics in arrival order, and two runs of the SAME call may differ in the last bit - equality of bits is
a statement about shapes without such sums only (the weight-gradient contractions cut their reduction from 512 rows on and
asr_colsum adds row blocks atomically above 128 rows - B T' = 120 here; at B T' = 510 the key bias gradient of two runs of the
same call differed in its last bit)."""
import ctypes
import os

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'e2e-asr-pytorch_amd')
V = 31

# (config, precision, B, T', L, persistent flags or None for the default, backward plan expected)
CASES = [('debug.yaml', 'fp32', 2, 6, 4, None, 0), ('debug.yaml', 'bf16', 2, 6, 4, None, 0),
         ('librispeech_asr.yaml', 'bf16', 3, 40, 4, 15, 2), ('librispeech_asr.yaml', 'bf16', 3, 8, 4, 1, 0),
         ('librispeech_asr.yaml', 'fp32', 3, 8, 4, 1, 0)]
IDS = ['%s-%s-B%d-T%d-L%d-%s' % (c[0].split('.')[0], c[1], c[2], c[3], c[4], 'default' if c[5] is None else 'flags%d' % c[5]) for c in CASES]


def _setup(cfg_name, prec, B, Tp, L):
    from src.asr import ASR
    config = yaml.safe_load(open(os.path.join(PKG, 'config', cfg_name)))
    D = config['data']['audio']['feat_dim'] * (config['data']['audio']['delta_order'] + 1)
    torch.manual_seed(3)
    model = ASR(D, V, 16, prec=prec, seed=5, **config['model']).cuda().train()
    assert model.decoder.fast and model.attention.fast
    g = torch.Generator().manual_seed(B + Tp)
    with torch.no_grad():
        wc = model.decoder.char_trans.weight
        wc.copy_((torch.round(torch.randn(wc.shape, generator=g).clamp(-1, 1) * 64) / 64).cuda())
    E = model.encoder.out_dim
    enc = torch.tanh(torch.randn(B, Tp, E, generator=g)).cuda()
    enc_len = torch.randint(max(Tp // 3, 1), Tp + 1, (B,), generator=g)
    enc_len[0] = Tp
    teacher = torch.randint(2, V, (B, L), generator=g).cuda()
    C = torch.randint(-16, 17, (B, L, V), generator=g).float() / 8
    G = (C.double() @ wc.detach().cpu().double()).float()                 # exact: see the module docstring
    assert torch.equal(G.double(), C.double() @ wc.detach().cpu().double())
    return model, enc, enc_len.cuda(), teacher, C.cuda(), G.cuda()


def _grads(model, enc):
    out = {n: p.grad.detach().clone() for n, p in model.named_parameters() if n.startswith(('decoder', 'attention', 'pre_embed'))}
    out['enc'] = enc.grad.detach().clone()
    return out


@pytest.mark.parametrize('cfg_name,prec,B,Tp,L,flags,plan', CASES, ids=IDS)
def test_outside_state_gradient_equals_the_logit_gradient_it_stands_for(cfg_name, prec, B, Tp, L, flags, plan):
    from src import functions as F
    from src import hipabi as H
    model, enc0, enc_len, teacher, C, G = _setup(cfg_name, prec, B, Tp, L)
    d = F._dec_dims(model, B, Tp, L)
    old = H.lib().asr_att_decoder_set_persistent(3)
    H.lib().asr_att_decoder_set_persistent(old if flags is None else flags)
    try:
        if flags == 15:                                   # (the plan query reports the shape's plan whether or not bit 1 enables it)
            assert int(H.lib().asr_att_decoder_bwd_plan(ctypes.byref(d))) == plan
        runs = {}
        for which in ('logits', 'states'):
            model.zero_grad()
            enc = enc0.clone().requires_grad_(True)
            logits, _, hs = F.AttDecoderFn.apply(model._anchor, enc, enc_len, teacher, L, model, model.prec)
            loss = (logits * C).sum() if which == 'logits' else (hs[:, :, -1, :] * G).sum()
            loss.backward()
            H.join_side()
            torch.cuda.synchronize()
            runs[which] = _grads(model, enc)
    finally:
        H.lib().asr_att_decoder_set_persistent(old)
    a, b = runs['logits'], runs['states']
    assert float(a['enc'].abs().max()) > 0 and float(a['decoder.layers.weight_hh_l0'].abs().max()) > 0
    for n in a:
        assert torch.isfinite(a[n]).all() and torch.isfinite(b[n]).all(), n
        if n.startswith('decoder.char_trans'):
            assert float(b[n].abs().max()) == 0.0, n                    # nothing of run B passes the output layer
            continue
        diff = float((a[n].double() - b[n].double()).abs().max())
        print('DHS %-40s max |A| %.3e  max |A - B| %.3e' % (n, float(a[n].abs().max()), diff))
        assert torch.equal(a[n], b[n]), (n, diff)


@pytest.mark.parametrize('cfg_name,prec,B,Tp,L,flags,plan', CASES, ids=IDS)
def test_null_state_gradient_is_the_plain_backward_bit_for_bit(cfg_name, prec, B, Tp, L, flags, plan):
    from src import functions as F
    from src import hipabi as H
    model, enc, enc_len, teacher, C, G = _setup(cfg_name, prec, B, Tp, L)
    d = F._dec_dims(model, B, Tp, L)
    old = H.lib().asr_att_decoder_set_persistent(3)
    H.lib().asr_att_decoder_set_persistent(old if flags is None else flags)
    runs = {}
    try:
        for entry in ('asr_att_decoder_bwd_ex', 'asr_att_decoder_bwd_hs', 'asr_att_decoder_bwd_hs+G'):
            # the backward overwrites the saved gates: a fresh forward state per call
            _, st = F.att_decoder_forward(model, enc, enc_len, L, teacher, model.prec)
            model.zero_grad()
            denc = torch.zeros_like(enc)
            w = H.dec_weights_struct(F._dec_tensors(model, False), d.NL)
            g = H.dec_weights_struct(F._dec_tensors(model, True), d.NL)
            s = H.dec_state_struct(st)
            nbytes = H.lib().asr_att_decoder_bwd_workspace_bytes(ctypes.byref(d))
            ws = F._dec_workspace(model, 'bwd', (d.B, d.Tp, d.L), nbytes, enc.device)
            off = int(H.lib().asr_att_decoder_bwd_status_offset(ctypes.byref(d))) if plan else 0
            if plan:
                H.abort_guard(ws, off)
            looped = ctypes.c_int(0)
            head = (ctypes.byref(d), ctypes.byref(w), ctypes.byref(g), H.ptr(enc), H.ptr(enc_len), ctypes.byref(s), H.ptr(C))
            tail = (H.ptr(denc), H.ptr(ws), nbytes, model.prec, 0, ctypes.byref(looped), H.stream_ptr())
            if entry == 'asr_att_decoder_bwd_ex':
                H.call(entry, *head, *tail)
            else:
                H.call('asr_att_decoder_bwd_hs', *head, H.ptr(G) if entry.endswith('+G') else None, *tail)
            if plan:
                H.watch_abort(ws, off)
            torch.cuda.synchronize()
            assert bool(looped.value) == bool(plan)
            runs[entry] = {n: p.grad.detach().clone() for n, p in model.named_parameters() if n.startswith(('decoder', 'attention', 'pre_embed'))}
            runs[entry]['enc'] = denc
    finally:
        H.lib().asr_att_decoder_set_persistent(old)
    a, b, c = (runs[k] for k in ('asr_att_decoder_bwd_ex', 'asr_att_decoder_bwd_hs', 'asr_att_decoder_bwd_hs+G'))
    for n in a:
        assert torch.equal(a[n], b[n]), n
    # and a gradient that is handed over arrives: with G = C W_c on top of dlogits = C the recurrence sees twice dh_top
    assert not torch.equal(a['enc'], c['enc'])
    assert torch.equal(a['decoder.char_trans.weight'], c['decoder.char_trans.weight'])
