"""Beam search of the model variants on the HIP path (src/decode_variants.py, csrc/decode_variants.hip::asr_beam_attend):
the fused attention kernel against float64 torch, the search against the genuine reference's hypotheses
(tests/golden/g11_beam_*.npz) and against the CPU restatement of tests/test_beam_variants_golden.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import asr_oracle as O
from test_beam_variants_golden import CASES, beam_search_variants, case_weights, lm_weights, load_case

pytestmark = pytest.mark.gpu

VARIANT_CASES = [c for c in CASES if load_case(c)[0]['path'] == 'variant']


# ---------------------------------------------------------------------------------------------------------------------
# asr_beam_attend
# ---------------------------------------------------------------------------------------------------------------------
def _attend_ref(mode, key, value, q, loc, wg, bg, enc_len, rows, temperature):
    """float64: key (U,NH,T,A), value (U,NHv,T,Dv), q (R,NH,A), loc (R,T,A) -> attn (R,NH,T), ctx (R,NH*Dv)."""
    U, NH, T, A = key.shape
    R = q.shape[0]
    u_of = torch.arange(R) // rows
    k = key[u_of]                                                             # (R,NH,T,A)
    if mode == 'dot':
        e = torch.einsum('rnta,rna->rnt', k, q)
    else:
        e = torch.tanh(k + q[:, :, None, :] + loc[:, None]) @ wg + bg
    mask = torch.arange(T)[None, None, :] >= enc_len[u_of][:, None, None]
    attn = torch.softmax((e / temperature).masked_fill(mask, float('-inf')), dim=-1)
    v = value[u_of]
    if v.shape[1] == 1:
        v = v.expand(R, NH, T, v.shape[-1])
    ctx = torch.einsum('rnt,rntd->rnd', attn, v).reshape(R, -1)
    return attn, ctx


def _run_attend(mode, key, value, q, loc, wg, bg, enc_len, rows, temperature, bf16, ctx_pad=(3, 5)):
    """Device run; key/value stored with 16-byte-multiple row strides, ctx written into a wider buffer at column ctx_pad[0]."""
    from src import hipabi as H
    dev = torch.device('cuda')
    U, NH, T, A = key.shape
    NHv, Dv = value.shape[1], value.shape[-1]
    R = q.shape[0]
    vw = 8 if bf16 else 4
    ldk, ldv = (A + vw - 1) // vw * vw, (Dv + vw - 1) // vw * vw
    dt = torch.bfloat16 if bf16 else torch.float32
    kd = torch.zeros(U, NH, T, ldk, dtype=dt, device=dev)
    kd[..., :A] = key.to(dev, dt)
    vd = torch.zeros(U, NHv, T, ldv, dtype=dt, device=dev)
    vd[..., :Dv] = value.to(dev, dt)
    qd = q.float().contiguous().to(dev)
    ld = (A + 3) // 4 * 4
    locd = None
    if mode == 'loc':
        locd = torch.zeros(R, T, ld, device=dev)
        locd[..., :A] = loc.float().to(dev)
    wgd = wg.float().to(dev) if mode == 'loc' else None
    bgd = bg.float().view(1).to(dev) if mode == 'loc' else None
    lend = enc_len.to(dev, torch.int64)
    attn = torch.full((R, NH * T), 7.0, device=dev)
    ctx_ld = ctx_pad[0] + NH * Dv + ctx_pad[1]
    ctxbuf = torch.full((R, ctx_ld), -3.0, device=dev)
    a = H.BeamAttend()
    a.key, a.value, a.q, a.enc_len = kd.data_ptr(), vd.data_ptr(), qd.data_ptr(), lend.data_ptr()
    a.loc = locd.data_ptr() if locd is not None else None
    a.wg = wgd.data_ptr() if wgd is not None else None
    a.bg = bgd.data_ptr() if bgd is not None else None
    a.attn, a.attn_ld = attn.data_ptr(), NH * T
    a.ctx, a.ctx_ld = ctxbuf[:, ctx_pad[0]:].data_ptr(), ctx_ld
    a.ld_k, a.ld_v, a.ld_l = ldk, ldv, ld
    a.U, a.rows_per_utt, a.NH, a.NHv, a.Tp, a.A, a.Dv = U, rows, NH, NHv, T, A, Dv
    a.mode = H.ATT_LOC if mode == 'loc' else H.ATT_DOT
    a.kv_bf16 = 1 if bf16 else 0
    a.temperature = temperature
    rc = H.lib().asr_beam_attend(ctypes.byref(a), H.stream_ptr())
    torch.cuda.synchronize()
    return rc, attn.view(R, NH, T).cpu().double(), ctxbuf.cpu().double(), (kd, vd)


def _resident_max(rows):
    from src import hipabi as H
    return int(H.lib().asr_beam_attend_resident_max_t(rows))


# mode, NH, v_proj, rows_per_utt, U, T' (int or 'resident' / 'resident+1' / 'max'), A, Dv, bf16
ATTEND_SHAPES = [
    ('dot', 1, False, 4, 3, 37, 12, 20, False),
    ('loc', 1, False, 8, 3, 37, 12, 20, False),
    ('loc', 1, False, 1, 1, 5, 7, 9, False),
    ('dot', 2, True, 4, 3, 100, 300, 640, False),
    ('loc', 4, False, 8, 1, 'resident', 300, 640, False),
    ('loc', 2, True, 8, 3, 'resident+1', 13, 37, False),
    ('dot', 4, False, 1, 3, 'max', 12, 20, False),
    ('dot', 4, True, 8, 3, 4096, 33, 65, False),
    ('loc', 2, False, 4, 3, 'max', 40, 72, False),
    ('dot', 2, False, 8, 3, 1500, 300, 640, True),
    ('loc', 4, True, 4, 2, 'max', 40, 72, True),
    ('loc', 1, False, 1, 1, 5, 7, 9, True),
    ('dot', 1, True, 8, 3, 'resident', 19, 23, True),
]


@pytest.mark.parametrize('idx', range(len(ATTEND_SHAPES)))
def test_beam_attend_matches_float64(idx):
    mode, NH, vproj, rows, U, T, A, Dv, bf16 = ATTEND_SHAPES[idx]
    from src import hipabi as H
    if T == 'resident':
        T = _resident_max(rows)
    elif T == 'resident+1':
        T = _resident_max(rows) + 1
    elif T == 'max':
        T = H.BEAM_ATTEND_MAX_T
    g = torch.Generator().manual_seed(1000 + idx)
    R = U * rows
    key = torch.tanh(torch.randn(U, NH, T, A, generator=g, dtype=torch.float64))
    value = torch.randn(U, NH if vproj else 1, T, Dv, generator=g, dtype=torch.float64)
    if bf16:        # the kernel reads the bf16-rounded key / value: the float64 reference takes the same rounded numbers
        key, value = key.to(torch.bfloat16).double(), value.to(torch.bfloat16).double()
    q = (torch.rand(R, NH, A, generator=g, dtype=torch.float64) - 0.5) * (2.0 / A ** 0.5)
    q = q.float().double()
    loc = torch.tanh(torch.randn(R, T, A, generator=g, dtype=torch.float64)).float().double() if mode == 'loc' else None
    wg = (torch.randn(A, generator=g, dtype=torch.float64) / A ** 0.5).float().double() if mode == 'loc' else None
    bg = torch.tensor(0.1, dtype=torch.float64) if mode == 'loc' else None
    if U == 1:
        enc_len = torch.tensor([T])
    else:
        enc_len = torch.tensor([1, T, max(1, (T * 2) // 3)])[:U]
    temperature = 0.5
    rc, attn, ctxbuf, _ = _run_attend(mode, key, value, q, loc, wg, bg, enc_len, rows, temperature, bf16)
    assert rc == 0, H.lib().asr_last_error().decode()
    ra, rcx = _attend_ref(mode, key, value, q, loc, wg, bg, enc_len, rows, temperature)
    # the kernel's only error is fp32 arithmetic (inputs are the reference's own, bf16-rounded in bf16 mode): energies,
    # exp and a T'-term sum, so 1e-5 relative for both storage types
    np.testing.assert_allclose(attn.numpy(), ra.numpy(), rtol=1e-5, atol=1e-7)
    p0, w = 3, NH * Dv
    ctx = ctxbuf[:, p0:p0 + w]
    scale = float(rcx.abs().max())
    np.testing.assert_allclose(ctx.numpy(), rcx.numpy(), rtol=1e-5, atol=1e-5 * scale)
    # rows sum to one, exact zeros past the length, neighbouring columns untouched
    u_of = torch.arange(R) // rows
    L = enc_len[u_of]
    np.testing.assert_allclose(attn.sum(-1).numpy(), np.ones((R, NH)), rtol=0, atol=1e-5)
    tail = torch.arange(T)[None, None, :] >= L[:, None, None]
    assert bool((attn[tail.expand_as(attn)] == 0).all())
    assert bool((ctxbuf[:, :p0] == -3.0).all()) and bool((ctxbuf[:, p0 + w:] == -3.0).all())


def test_beam_attend_refuses_beyond_limits():
    from src import hipabi as H
    g = torch.Generator().manual_seed(5)
    for rows, T in ((1, H.BEAM_ATTEND_MAX_T + 1), (H.BEAM_ATTEND_MAX_ROWS + 1, 8)):
        key = torch.randn(1, 1, T, 8, generator=g, dtype=torch.float64)
        value = torch.randn(1, 1, T, 8, generator=g, dtype=torch.float64)
        q = torch.randn(rows, 1, 8, generator=g, dtype=torch.float64)
        rc, attn, _, _ = _run_attend('dot', key, value, q, None, None, None, torch.tensor([T]), rows, 1.0, False)
        assert rc == -3, rc                                                   # ASR_E_UNSUPPORTED, nothing launched
        assert bool((attn == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------------------------
def _decoder(meta, ctc_w, lm_w, beam=None, prec='fp32', sd=None, model_cfg=None):
    from src.asr import ASR
    from src.decode import BeamDecoder
    from src.lm import RNNLM
    mc = model_cfg or meta['model']
    if sd is None:
        _, sd = case_weights(meta)
    model = ASR(meta['D'], meta['V'], 4, prec=prec, **mc)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    dec = BeamDecoder(model, None, beam_size=beam or meta['beam'], min_len_ratio=meta['min_len_ratio'], max_len_ratio=meta['max_len_ratio'],
                      ctc_weight=ctc_w)
    if lm_w > 0:
        lm = RNNLM(meta['V'], **meta['lm'])
        lm.load_state_dict(lm_weights(meta))
        dec.set_lm(lm.cuda().eval(), lm_w)
    return dec


@pytest.mark.parametrize('name', CASES)
def test_beam_hypotheses_match_reference(name):
    meta, z = load_case(name)
    for tag, ctc_w, lm_w in meta['modes']:
        dec = _decoder(meta, ctc_w, lm_w)
        assert dec.fast == (meta['path'] == 'fast'), (name, dec.fast)
        hyps = dec(torch.from_numpy(z['feat']).cuda(), torch.from_numpy(z['feat_len']).cuda())
        assert len(hyps) == int(z['n_' + tag]), (name, tag, len(hyps))
        for i, h in enumerate(hyps):
            assert h.outIndex == z['%s_seq%d' % (tag, i)].tolist(), (name, tag, i, h.outIndex, z['%s_seq%d' % (tag, i)].tolist())
            np.testing.assert_allclose(np.array(h.output_scores, dtype=np.float32), z['%s_score%d' % (tag, i)], rtol=1e-4, atol=2e-3)
            assert abs(h.avgScore() - float(z['%s_avg%d' % (tag, i)])) < 2e-3


def _ragged_batch(meta, z, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    T = int(z['feat_len'][0])
    lens = [T, T - 21, T - 8]
    feats = torch.zeros(3, T, meta['D'])
    feats[0] = torch.from_numpy(z['feat'][0])
    for u in (1, 2):
        feats[u, :lens[u]] = torch.from_numpy(g.random((lens[u], meta['D']), dtype=np.float32))
    return feats, lens


@pytest.mark.parametrize('name', VARIANT_CASES)
def test_batched_equals_single(name):
    meta, z = load_case(name)
    feats, lens = _ragged_batch(meta, z, 11)
    flen = torch.tensor(lens)
    for ctc_w, lm_w in ((0.0, 0.0), (0.3, 0.5)):
        dec = _decoder(meta, ctc_w, lm_w)
        batched = dec(feats.cuda(), flen.cuda())
        assert len(batched) == 3
        for u in range(3):
            single = dec(feats[u:u + 1, :lens[u]].cuda(), flen[u:u + 1].cuda())
            assert len(single) == len(batched[u]) > 0, (name, u, len(single), len(batched[u]))
            for a, b in zip(single, batched[u]):
                assert a.outIndex == b.outIndex, (name, u, a.outIndex, b.outIndex)
                np.testing.assert_allclose(np.array(a.output_scores), np.array(b.output_scores), rtol=0, atol=1e-5)


def _compare_to_cpu(got, want, what):
    """Same hypotheses in the same order where the CPU list has no near-ties; by content where it does."""
    avg = lambda sc: sum(sc) / len(sc)
    gaps = [abs(avg(a[1]) - avg(b[1])) for a, b in zip(want, want[1:])]
    assert len(got) == len(want), what
    if not want:                # beam 1 whose single hypothesis ended before min_len: nothing to return, as in the reference
        return
    assert abs(got[0].avgScore() - avg(want[0][1])) < 1e-4, what
    if not gaps or min(gaps) > 1e-4:
        for h, (seq, sc) in zip(got, want):
            assert h.outIndex == seq, (what, h.outIndex, seq)
            np.testing.assert_allclose(np.array(h.output_scores), np.array(sc), rtol=0, atol=1e-4)
    else:
        ref = {tuple(s): sc for s, sc in want}
        common = [h for h in got if tuple(h.outIndex) in ref]
        assert len(common) >= len(want) // 2, what
        for h in common:
            np.testing.assert_allclose(np.array(h.output_scores), np.array(ref[tuple(h.outIndex)]), rtol=0, atol=1e-4)


@pytest.mark.parametrize('name', ['dot_mh3', 'loc_mh2_vproj', 'gru2', 'gru1_dot', 'lstm5'])
@pytest.mark.parametrize('beam', [1, 4, 8])
def test_random_inputs_match_cpu_restatement(name, beam):
    meta, _ = load_case(name)
    cfg, P = case_weights(meta)
    lm = (lm_weights(meta), meta['lm'])
    g = np.random.Generator(np.random.PCG64(300 + beam))
    for T in (44, 67):
        feat = g.random((1, T, meta['D']), dtype=np.float32)
        flen = np.array([T], dtype=np.int64)
        modes = [(0.0, 0.0)] if beam == 1 else [(0.0, 0.0), (0.3, 0.5)]
        for ctc_w, lm_w in modes:
            want = beam_search_variants(torch.from_numpy(feat), torch.from_numpy(flen), P, cfg, beam, meta['min_len_ratio'],
                                        meta['max_len_ratio'], ctc_weight=ctc_w, lm=lm if lm_w > 0 else None, lm_weight=lm_w)
            got = _decoder(meta, ctc_w, lm_w, beam=beam)(torch.from_numpy(feat).cuda(), torch.from_numpy(flen).cuda())
            _compare_to_cpu(got, want, (name, beam, T, ctc_w, lm_w))


# bf16 contraction mode: every linear layer rounds its operands to bf16 (relative 2^-9 each) and the keys / values are stored
# as bf16; through the encoder and at most a dozen decoder steps of these small models the token log-probs move by a few 1e-3.
# 5e-2 bounds that with a wide margin while still catching a wrong head, row or state (those move log-probs by O(1)).
BF16_SCORE_BOUND = 5e-2


@pytest.mark.parametrize('name', VARIANT_CASES)
def test_bf16_scores_are_teacher_forced_log_probs(name):
    meta, z = load_case(name)
    cfg, P = case_weights(meta)
    P64 = {k: v.double() for k, v in P.items()}
    feat, flen = torch.from_numpy(z['feat']), torch.from_numpy(z['feat_len'])
    hyps = _decoder(meta, 0.0, 0.0, prec='bf16')(feat.cuda(), flen.cuda())
    best32 = _decoder(meta, 0.0, 0.0, prec='fp32')(feat.cuda(), flen.cuda())[0].avgScore()
    assert len(hyps) > 0
    with torch.no_grad():
        enc, enc_len = O.encoder(feat.double(), flen, P64, cfg)
        for h in hyps:
            seq = torch.tensor([h.outIndex])
            logits, _ = O.att_decoder_variants(enc, enc_len, P64, cfg, seq.shape[1], teacher=seq)
            lp = torch.log_softmax(logits[0], -1)
            want = lp[torch.arange(seq.shape[1]), seq[0]].numpy()
            np.testing.assert_allclose(np.array(h.output_scores), want, rtol=0, atol=BF16_SCORE_BOUND)
    assert abs(hyps[0].avgScore() - best32) < BF16_SCORE_BOUND


def test_decdrop2_runs_the_fast_path_like_its_dropout_free_twin():
    import copy
    meta, z = load_case('decdrop2')
    assert meta['model']['decoder']['dropout'] > 0 and meta['model']['emb_drop'] > 0
    twin = copy.deepcopy(meta['model'])
    twin['decoder']['dropout'] = 0
    twin['emb_drop'] = 0.0
    feat, flen = torch.from_numpy(z['feat']).cuda(), torch.from_numpy(z['feat_len']).cuda()
    for ctc_w, lm_w in ((0.0, 0.0), (0.3, 0.5)):
        a = _decoder(meta, ctc_w, lm_w)
        b = _decoder(meta, ctc_w, lm_w, model_cfg=twin)
        assert a.fast and b.fast
        ha, hb = a(feat, flen), b(feat, flen)
        assert [h.outIndex for h in ha] == [h.outIndex for h in hb]
        assert [h.output_scores for h in ha] == [h.output_scores for h in hb]


def test_forward_host_refuses_variant_models():
    meta, z = load_case('gru2')
    dec = _decoder(meta, 0.0, 0.0)
    assert not dec.fast
    with pytest.raises(NotImplementedError, match='forward'):
        dec.forward_host(torch.from_numpy(z['feat']).cuda(), torch.from_numpy(z['feat_len']).cuda())
