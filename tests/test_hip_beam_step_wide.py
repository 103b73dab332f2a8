"""The joint beam search above V = 2048 on the device: asr_beam_candidates_wide and asr_beam_step_wide (csrc/beam_step.hip) on
canary-bordered buffers against the float64 restatement of tests/test_beam_step_reference.py over the cases of
tests/test_beam_step_wide_reference.py; the narrow kernels' cases through the wide entries; the refusals; BeamDecoder end to
end at V = 2100 and V = 5000 against oracle/decode_oracle.py; and the vocabulary projection of asr_att_decoder_step.

Integers must be exact.  Scores are held to the restatement within TOL_FACTOR x the deviation of the restatement's OWN float32
transcription on the same case (W.step_fp32_dev, computed here on the CPU): the wide kernel evaluates the fused score in the
transcription's operation order without contraction, so it should sit on the transcription itself.  The buffers, the guards
and the comparison of one step are those of tests/test_hip_beam_step.py."""
import ctypes

import numpy as np
import pytest
import torch

import test_beam_step_reference as R
import test_beam_step_wide_reference as W
import test_gemm_reference as G
import test_hip_beam_step as N
from test_hip_beam_step import CAN_F, CAN_I, E_ARG, E_UNSUPPORTED, TOL_FACTOR, Guarded

pytestmark = pytest.mark.gpu


# ---- one drive of a case through either entry ------------------------------------------------------------------------------
def new_aux(c, dims, s0):
    U, R_, Lmax, tok_ld = dims
    i32, f32, i64, beam = torch.int32, torch.float32, torch.int64, c['beam']
    aux = {'tokens': Guarded((R_, tok_ld), i64), 'done': Guarded((U,), i32, s0['done']),
           'fin_n': Guarded((U,), i32, [len(f) for f in s0['finals']]), 'fin_len': Guarded((U, beam), i32),
           'fin_avg': Guarded((U, beam), f32), 'fin_seq': Guarded((U, beam, Lmax + 1), i32), 'fin_sc': Guarded((U, beam, Lmax + 1), f32),
           'min_len': torch.tensor(c['min_len'], dtype=i32, device='cuda'), 'max_len': torch.tensor(c['max_len'], dtype=i32, device='cuda')}
    for u, fin in enumerate(s0['finals']):
        for i, (avg, seq, score) in enumerate(fin):
            aux['fin_len'].t[u, i], aux['fin_avg'].t[u, i] = len(seq), float(avg)
            aux['fin_seq'].t[u, i, :len(seq)] = torch.tensor(seq, dtype=i32)
            aux['fin_sc'].t[u, i, :len(seq)] = torch.tensor([float(s) for s in score], dtype=f32)
    return aux


def workspace(U, beam):
    from src import hipabi as H
    nbytes = H.lib().asr_beam_step_wide_workspace_bytes(U, beam)
    assert nbytes > 0 and nbytes % (4 * U * beam) == 0
    return Guarded((U * beam, nbytes // (4 * U * beam)), torch.int32), nbytes


def launch(wide, tab, st_in, st_out, aux, c, dims, p, t, ws=None, ws_bytes=None, **override):
    from src import hipabi as H
    U, R_, Lmax, tok_ld = dims
    a = H.BeamStep()
    dev = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to('cuda', torch.int32 if k == 'cand' else torch.float32))
           for k, v in tab.items()}
    ptrs = {'att_logp': dev['att'], 'lm_logp': dev['lm'], 'psi': dev['psi'], 'candidates': dev['cand'],
            'alive_in': st_in['alive'].t, 'sum_in': st_in['sum'].t, 'ctcp_in': st_in['ctcp'].t, 'len_in': st_in['len'].t,
            'seq_in': st_in['seq'].t, 'score_in': st_in['sc'].t, 'alive_out': st_out['alive'].t, 'sum_out': st_out['sum'].t,
            'ctcp_out': st_out['ctcp'].t, 'len_out': st_out['len'].t, 'seq_out': st_out['seq'].t, 'score_out': st_out['sc'].t,
            'last_token': aux['last_tok'].t, 'parent': aux['parent'].t, 'ctc_index': aux['ctcidx'].t, 'tokens': aux['tokens'].t,
            'min_len': aux['min_len'], 'max_len': aux['max_len'], 'done': aux['done'].t, 'fin_n': aux['fin_n'].t,
            'fin_len': aux['fin_len'].t, 'fin_avg': aux['fin_avg'].t, 'fin_seq': aux['fin_seq'].t, 'fin_score': aux['fin_sc'].t}
    for k, v in ptrs.items():
        setattr(a, k, None if v is None else v.data_ptr())
    a.tokens_ld = tok_ld
    a.U, a.beam, a.V, a.C, a.Lmax, a.t = U, c['beam'], c['V'], c['C'], Lmax, t
    a.ctc_weight, a.lm_weight, a.eos_threshold = float(p['ctc_w']), float(p['lm_w']), float(p['eos_thr'])
    for k, v in override.items():
        setattr(a, k, v)
    if wide:
        rc = H.lib().asr_beam_step_wide(ctypes.byref(a), None if ws is None else ws.ptr(), ws_bytes, H.stream_ptr())
    else:
        rc = H.lib().asr_beam_step(ctypes.byref(a), H.stream_ptr())
    torch.cuda.synchronize()
    return rc


def drive(wide, c, dims, s0, tables, params, ref):
    """Multi-step drive with the kernel's own state fed back; every step is compared with the restatement.  -> ([the buffers
    after step t], largest float deviation)."""
    U, R_, Lmax, tok_ld = dims
    st_in = N.state_bufs(R_, Lmax)
    for k in ('alive', 'sum', 'ctcp', 'len'):
        st_in[k].t.copy_(torch.as_tensor(s0[k]).to(st_in[k].t.dtype))
    aux = new_aux(c, dims, s0)
    ws, ws_bytes = workspace(U, c['beam']) if wide else (None, None)
    tok_model = np.full((R_, tok_ld), CAN_I, dtype=np.int64)
    fin_hi = [max([0] + [len(f[1]) for f in fin]) for fin in s0['finals']]
    dev, gots = 0.0, []
    for t in range(len(ref)):
        st_out = N.state_bufs(R_, Lmax)
        N.fresh_step_outputs(aux, R_)
        assert launch(wide, tables(t), st_in, st_out, aux, c, dims, params(t), t, ws, ws_bytes) == 0
        for b in st_in.values():
            b.host()                                    # inputs: guards intact
        if wide:
            ws.host()                                   # the workspace's border
        got = N.read_step(st_out, aux)
        dev = max(dev, N.compare_step(got, ref[t], tok_model, fin_hi, c['beam']))
        gots.append(got)
        st_in = st_out
    assert all(ref[-1]['done'])
    return gots, dev


@pytest.mark.parametrize('name', sorted(W.WIDE_CASES))
def test_wide_step_drive_equals_float64_restatement(name):
    c = W.WIDE_CASES[name]
    ref = W.reference(name)[0]
    allowed = TOL_FACTOR * W.step_fp32_dev(name)
    _, dev = drive(True, c, W.case_dims(name), W.case_state0(name), lambda t: W.case_tables(name, t), lambda t: W.case_params(name, t), ref)
    print('%s: largest float deviation %.3g (allowed %.3g = %d x its fp32 transcription)' % (name, dev, allowed, TOL_FACTOR))
    assert dev <= allowed


def _narrow_fp32_dev(name):
    dev = 0.0
    for a, b in zip(R.run_case(name)[0], R.run_case(name, np.float32)[0]):
        dev = max(dev, N.rel_dev(b['sum'], a['sum']), N.rel_dev(b['ctcp'], a['ctcp']))
        for x, y in zip(a['score'], b['score']):
            dev = max(dev, N.rel_dev(y, x))
        for fa, fb in zip(a['finals'], b['finals']):
            for (avg, _, sc), (avg2, _, sc2) in zip(fa, fb):
                dev = max(dev, N.rel_dev(avg2, avg), N.rel_dev(sc2, sc))
    return dev


@pytest.mark.parametrize('name', ['v2047_b8_ctc', 'v2048_b16_lm', 'tie_v2048_b16'])
def test_narrow_cases_through_the_wide_entries(name):
    """Where both kernels apply they must decide alike, and they evaluate the fused score in one function (BeamFuse,
    csrc/beam_step.hip): integers identical to asr_beam_step's, the float outputs of the live rows and of the filled finals bit
    for bit identical, and the scores within the bound."""
    c = R.CASES[name]
    ref = N.reference(name)
    args = (c, R.case_dims(name), R.case_state0(name), lambda t: R.case_tables(name, t), lambda t: R.case_params(name, t), ref)
    narrow, _ = drive(False, *args)
    wide, dev = drive(True, *args)
    for t, (a, b) in enumerate(zip(narrow, wide)):
        for k in ('alive', 'len', 'seq', 'last_tok', 'parent', 'ctcidx', 'tokens', 'done', 'fin_n', 'fin_len', 'fin_seq'):
            assert (a[k] == b[k]).all(), k
        live = a['alive'] == 1
        for k in ('sum', 'ctcp'):
            assert (a[k][live] == b[k][live]).all(), (t, k)
        for r in np.nonzero(live)[0]:
            n = int(a['len'][r])
            assert (a['sc'][r, :n] == b['sc'][r, :n]).all(), (t, 'sc', r)
        for u in range(len(a['fin_n'])):
            for i in range(int(a['fin_n'][u])):
                n = int(a['fin_len'][u, i])
                assert a['fin_avg'][u, i] == b['fin_avg'][u, i], (t, 'fin_avg', u, i)
                assert (a['fin_sc'][u, i, :n] == b['fin_sc'][u, i, :n]).all(), (t, 'fin_sc', u, i)
    allowed = TOL_FACTOR * _narrow_fp32_dev(name)
    print('%s through the wide entry: deviation %.3g (allowed %.3g)' % (name, dev, allowed))
    assert dev <= allowed


# ---- refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('what', ['null_att', 'null_fin_seq', 'null_ctcp_out', 'null_workspace', 'beam17', 'v65537', 'c33', 'small_workspace',
                                  'psi_without_candidates'])
def test_wide_step_refuses_before_any_launch(what):
    name = 'v2049_b5_ctc'
    c, dims = W.WIDE_CASES[name], W.case_dims(name)
    U, R_, Lmax, tok_ld = dims
    st_in, st_out, aux = N.state_bufs(R_, Lmax), N.state_bufs(R_, Lmax), new_aux(c, dims, W.case_state0(name))
    N.fresh_step_outputs(aux, R_)
    ws, ws_bytes = workspace(U, c['beam'])
    over = {'null_att': {'att_logp': None}, 'null_fin_seq': {'fin_seq': None}, 'null_ctcp_out': {'ctcp_out': None}, 'null_workspace': {},
            'beam17': {'beam': 17}, 'v65537': {'V': W.WIDE_VMAX + 1}, 'c33': {'C': W.WIDE_CMAX + 1}, 'small_workspace': {},
            'psi_without_candidates': {'candidates': None}}[what]
    rc = launch(True, W.case_tables(name, 0), st_in, st_out, aux, c, dims, W.case_params(name, 0), 0,
                None if what == 'null_workspace' else ws, ws_bytes - 1 if what == 'small_workspace' else ws_bytes, **over)
    assert rc == (E_UNSUPPORTED if what == 'v65537' else E_ARG)
    if what == 'v65537':
        from src import hipabi as H
        assert str(W.WIDE_VMAX) in H.lib().asr_last_error().decode()
    for b in list(st_out.values()) + [aux[k] for k in ('last_tok', 'parent', 'ctcidx', 'tokens', 'fin_len', 'fin_avg', 'fin_seq', 'fin_sc')] + [ws]:
        assert (b.host() == b.fill).all()                # nothing was launched


def test_wide_candidates_refusals():
    from src import hipabi as H
    x = torch.zeros(2, 4096, device='cuda')
    out = Guarded((2, W.WIDE_CMAX + 1), torch.int32)
    f = H.lib().asr_beam_candidates_wide
    assert f(H.ptr(x), out.ptr(), 2, W.WIDE_VMAX + 1, 8, H.stream_ptr()) == E_UNSUPPORTED
    assert str(W.WIDE_VMAX) in H.lib().asr_last_error().decode()
    assert f(H.ptr(x), out.ptr(), 2, 4096, W.WIDE_CMAX + 1, H.stream_ptr()) == E_ARG
    assert f(H.ptr(x), out.ptr(), 2, 5, 6, H.stream_ptr()) == E_ARG
    assert f(H.ptr(x), out.ptr(), 2, 1, 1, H.stream_ptr()) == E_ARG
    assert f(None, out.ptr(), 2, 4096, 8, H.stream_ptr()) == E_ARG
    assert f(H.ptr(x), None, 2, 4096, 8, H.stream_ptr()) == E_ARG
    torch.cuda.synchronize()
    assert (out.host() == CAN_I).all()
    assert H.lib().asr_beam_step_wide_workspace_bytes(1, 17) == 0 and H.lib().asr_beam_step_wide_workspace_bytes(0, 4) == 0


# ---- asr_beam_candidates_wide ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', sorted(set(c['V'] for c in W.WIDE_CASES.values())))
def test_wide_candidates_equal_the_restatement(V):
    from src import hipabi as H
    rows = 6
    x = N.candidate_rows(rows, V, V + rows)
    xd = torch.from_numpy(x).cuda()
    want = R.beam_candidates(x, W.WIDE_CMAX)               # the top-32 once: the top-C is its head, token 0 where the row ran out
    for C in (1, 12, W.WIDE_CMAX):
        out = Guarded((rows, C), torch.int32)
        H.call('asr_beam_candidates_wide', H.ptr(xd), out.ptr(), rows, V, C, H.stream_ptr())
        torch.cuda.synchronize()
        got = out.host()
        assert (got == want[:, :C]).all(), (C, np.argwhere(got != want[:, :C])[:4].tolist())


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [2100, 5000])
@pytest.mark.parametrize('tag', sorted(W.E2E_SETTINGS))
def test_beam_decoder_matches_the_decode_oracle_at_a_wide_vocabulary(V, tag):
    """BeamDecoder in fp32 on the single utterance and on the ragged batch of 3 against oracle/decode_oracle.py::beam_search:
    token sequences identical, scores within fp32 accumulation noise.  The seeds hold every decision of the oracle's search
    apart by more than R.GAP (tests/test_beam_step_wide_reference.py); char_trans.weight is scaled in both models (there)."""
    from src.asr import ASR
    from src.decode import BeamDecoder
    from src.lm import RNNLM
    wseed, fseed = W.E2E_SEEDS[(V, tag)]
    ctc_w, lm_w = W.E2E_SETTINGS[tag]
    _, P, P_lm = W.e2e_weights(V, wseed)
    model = ASR(W.E2E_D, V, 4, prec='fp32', **W.E2E_MODEL)
    model.load_state_dict(P)
    dec = BeamDecoder(model.cuda().eval(), None, beam_size=W.E2E_BEAM, min_len_ratio=W.E2E_MIN_RATIO, max_len_ratio=W.E2E_MAX_RATIO,
                      ctc_weight=ctc_w)
    if lm_w > 0:
        lm = RNNLM(V, **W.E2E_LM)
        lm.load_state_dict(P_lm)
        dec.set_lm(lm.cuda().eval(), lm_w)
    feats = W.e2e_features(fseed)
    lens = [f.shape[1] for f in feats]
    batch = torch.zeros(len(feats), max(lens), W.E2E_D)
    for u, f in enumerate(feats):
        batch[u, :lens[u]] = f[0]
    refs = [ref for ref, _ in W.e2e_oracle(V, tag)]

    def check(hyps, ref, what):
        assert len(hyps) == len(ref), what
        for i, (h, (seq, scores)) in enumerate(zip(hyps, ref)):
            assert h.outIndex == seq, (what, i, h.outIndex, seq)
            np.testing.assert_allclose(np.array(h.output_scores, dtype=np.float32), np.array(scores, np.float32), rtol=1e-4, atol=2e-3)

    check(dec(feats[0].cuda(), torch.tensor(lens[:1]).cuda()), refs[0], 'single')
    batched = dec(batch.cuda(), torch.tensor(lens).cuda())
    for u in range(len(feats)):
        check(batched[u], refs[u], 'batched, utterance %d' % u)


def test_joint_search_names_its_vocabulary_limit():
    from src.decode import BeamDecoder

    class Stub(object):
        enable_att, ctc_weight, vocab_size = True, 0.5, W.WIDE_VMAX + 1

    with pytest.raises(ValueError, match=str(W.WIDE_VMAX)):
        BeamDecoder(Stub(), None, beam_size=4, min_len_ratio=0.0, max_len_ratio=0.1)


# ---- the vocabulary projection of the decode step ----------------------------------------------------------------------------------
def _decode_step_logits(V, prec, dec_dim):
    """Two steps of asr_att_decoder_step on 5 rows with their own encoder outputs -> (hs of the top layer at t = 1, Wc, bc, the
    logits buffer after the steps), the buffer filled with the canary before."""
    from oracle import asr_oracle as O
    from src.asr import ASR
    from src.decode import _FastStep
    mc = dict(W.E2E_MODEL, decoder={'module': 'LSTM', 'dim': dec_dim, 'layer': 2, 'dropout': 0})
    model = ASR(W.E2E_D, V, 4, prec=prec, **mc)
    model.load_state_dict(O.seeded_state_dict(O.param_shapes(O.ModelCfg(mc, W.E2E_D, V)), 11))
    model = model.cuda().eval()
    rows, Tp = 5, 9
    g = torch.Generator().manual_seed(V)
    enc = torch.randn(rows, Tp, model.encoder.out_dim, generator=g).cuda()
    enc_len = torch.tensor([9, 7, 5, 9, 3], dtype=torch.int64).cuda()
    with torch.no_grad():
        fs = _FastStep(model, enc, enc_len, 1, 2)
        fs.sd['logits'].fill_(CAN_F)
        fs.tokens[:, 1] = torch.tensor([3, V - 1, 7, 1, V // 2])
        fs.step(0)
        fs.step(1)
        torch.cuda.synchronize()
    dec = model.decoder
    return (fs.sd['hs'][:, 1, dec.layer - 1].cpu().numpy(), dec.char_trans.weight.detach().cpu().numpy(),
            dec.char_trans.bias.detach().cpu().numpy(), fs.sd['logits'].cpu().numpy())


def _float64_product(hs, Wc, bc, bf16):
    """-> (ref, S = sum |terms| + |bias|) of the operands the contraction multiplies (bf16 mode rounds them on the way in)."""
    a, b = (G.bf16_round(hs), G.bf16_round(Wc)) if bf16 else (hs.astype(np.float64), Wc.astype(np.float64))
    return a @ b.T + bc.astype(np.float64), np.abs(a) @ np.abs(b).T + np.abs(bc.astype(np.float64))


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('V', [2049, 16385])
def test_decode_step_projection_above_2048_equals_float64(V, prec):
    """logits[:, t] of one decode step against the float64 product of the same hs, Wc and bc, within the per-element bound
    tests/test_gemm_reference.py holds asr_gemm to (G.bound: 2 (K + 2) 2^-24 S, in bf16 mode on the rounded operands); the
    other positions of the logits buffer stay untouched."""
    hs, Wc, bc, logits = _decode_step_logits(V, prec, 12)
    ref, S = _float64_product(hs, Wc, bc, prec == 'bf16')
    tol = G.bound(ref, S, hs.shape[1], False, False)
    err = np.abs(logits[:, 1].astype(np.float64) - ref)
    print('V %d %s: largest error / bound %.3g' % (V, prec, float((err / tol).max())))
    assert (err <= tol).all(), np.argwhere(err > tol)[:4].tolist()
    assert (logits[:, 2] == CAN_F).all()


def _row_kernel_logits(hs, Wc, bc):
    """dec_logits_kernel in numpy float32, operation by operation: lane k holds the rounded product h[k] Wc[v, k] (decoder dim
    <= 64: one term per lane, so a contracted multiply-add rounds the same), the wave's butterfly sum over strides 32..1,
    then the bias."""
    rows, K = hs.shape
    assert K <= 64
    p = np.zeros((rows, Wc.shape[0], 64), dtype=np.float32)
    p[:, :, :K] = hs[:, None, :].astype(np.float32) * Wc[None, :, :].astype(np.float32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[:, :, lanes ^ o]
    return p[:, :, 0] + bc[None, :].astype(np.float32)


def test_decode_step_projection_at_2048_is_the_row_kernel_bit_for_bit():
    """At V <= 2048 the per-row kernel still runs.  Its result is pinned to a float32 recomputation in the kernel's operation
    order, itself checked against float64 - not to a recorded device dump."""
    hs, Wc, bc, logits = _decode_step_logits(2048, 'fp32', 40)
    want = _row_kernel_logits(hs, Wc, bc)
    ref, S = _float64_product(hs, Wc, bc, False)
    assert (np.abs(want.astype(np.float64) - ref) <= G.bound(ref, S, hs.shape[1], False, False)).all()
    assert want.dtype == np.float32 and (logits[:, 1] == want).all(), np.argwhere(logits[:, 1] != want)[:4].tolist()
    assert (logits[:, 2] == CAN_F).all()
