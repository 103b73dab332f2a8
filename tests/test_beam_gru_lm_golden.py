"""BeamDecoder with a GRU language model (shallow fusion) against the genuine reference's hypotheses
(tests/golden/g12_beam_gru_lm_*.npz, tests/golden/gen_lm_gru.py): the LM is loaded as the reference loads it, from an
lm_config yaml and a {'model': state_dict} checkpoint.  Covered: the shipped-decoder fast path (case 'small'), the variant path
(case 'gru1_dot'), forward_host, a batch of three utterances, fp32 and bf16.

Hypotheses must match exactly and in order.  fp32 scores: 1e-4.  bf16 scores: BF16_SCORE_BOUND = 5e-2, the bound of
tests/test_hip_beam_variants.py (bf16 decoder and LM contractions move a log-prob by O(1e-2); a wrong row or state moves it by
O(1)).  The fixtures were generated with every adjacent pair of hypotheses at least 1e-3 apart in average score."""
import glob
import os

import numpy as np
import pytest
import torch
import yaml

from test_beam_variants_golden import case_weights, lm_weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(p)[len('g12_beam_gru_lm_'):-4] for p in glob.glob(os.path.join(GOLDEN, 'g12_beam_gru_lm_*.npz')))
FP32_SCORE_TOL = 1e-4
BF16_SCORE_BOUND = 5e-2


def load_case(name):
    z = np.load(os.path.join(GOLDEN, 'g12_beam_gru_lm_%s.npz' % name))
    return yaml.safe_load(str(z['meta'])), z


def _decoder(meta, ctc_w, lm_w, tmp_path, prec='fp32'):
    from src.asr import ASR
    from src.decode import BeamDecoder
    lm_config, lm_path = str(tmp_path / 'lm.yaml'), str(tmp_path / 'lm.pth')
    yaml.safe_dump({'model': meta['lm']}, open(lm_config, 'w'))
    torch.save({'model': lm_weights(meta)}, lm_path)
    _, sd = case_weights(meta)
    model = ASR(meta['D'], meta['V'], 4, prec=prec, **meta['model'])
    model.load_state_dict(sd)
    model = model.cuda().eval()
    dec = BeamDecoder(model, None, beam_size=meta['beam'], min_len_ratio=meta['min_len_ratio'], max_len_ratio=meta['max_len_ratio'],
                      lm_path=lm_path, lm_config=lm_config, lm_weight=lm_w, ctc_weight=ctc_w)
    assert dec.lm.module == 'GRU'
    dec.lm = dec.lm.cuda().eval()
    return dec


def _check(hyps, z, tag, tol, what):
    assert len(hyps) == int(z['n_' + tag]), (what, len(hyps))
    for i, h in enumerate(hyps):
        assert h.outIndex == z['%s_seq%d' % (tag, i)].tolist(), (what, i, h.outIndex, z['%s_seq%d' % (tag, i)].tolist())
        np.testing.assert_allclose(np.array(h.output_scores, dtype=np.float64), z['%s_score%d' % (tag, i)], rtol=0, atol=tol)
        assert abs(h.avgScore() - float(z['%s_avg%d' % (tag, i)])) < tol, what


def test_fixture_set():
    assert set(CASES) == {'small', 'gru1_dot'}
    for c in CASES:
        meta, _ = load_case(c)
        assert meta['lm']['module'] == 'GRU' and meta['lm']['n_layers'] == 2 and meta['min_gap'] >= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_hypotheses_match_reference(name, prec, tmp_path):
    meta, z = load_case(name)
    feat, flen = torch.from_numpy(z['feat']).cuda(), torch.from_numpy(z['feat_len']).cuda()
    tol = FP32_SCORE_TOL if prec == 'fp32' else BF16_SCORE_BOUND
    for tag, ctc_w, lm_w in meta['modes']:
        dec = _decoder(meta, ctc_w, lm_w, tmp_path, prec)
        assert dec.fast == (meta['path'] == 'fast')
        _check(dec(feat, flen), z, tag, tol, (name, prec, tag))
        if dec.fast:
            _check(dec.forward_host(feat, flen), z, tag, tol, (name, prec, tag, 'host'))


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_batched_search_matches_reference(name, tmp_path):
    """U = 3: the fixture's utterance among two others; its hypotheses are the reference's, the others equal their single runs."""
    meta, z = load_case(name)
    T = int(z['feat_len'][0])
    lens = [T - 9, T, T - 20]
    g = np.random.Generator(np.random.PCG64(31))
    feats = torch.zeros(3, T, meta['D'])
    feats[1] = torch.from_numpy(z['feat'][0])
    for u in (0, 2):
        feats[u, :lens[u]] = torch.from_numpy(g.random((lens[u], meta['D']), dtype=np.float32))
    flen = torch.tensor(lens)
    for tag, ctc_w, lm_w in meta['modes']:
        dec = _decoder(meta, ctc_w, lm_w, tmp_path)
        batched = dec(feats.cuda(), flen.cuda())
        assert len(batched) == 3
        _check(batched[1], z, tag, FP32_SCORE_TOL, (name, tag, 'batched'))
        for u in (0, 2):
            single = dec(feats[u:u + 1, :lens[u]].cuda(), flen[u:u + 1].cuda())
            assert [h.outIndex for h in single] == [h.outIndex for h in batched[u]], (name, tag, u)
            for a, b in zip(single, batched[u]):
                np.testing.assert_allclose(np.array(a.output_scores), np.array(b.output_scores), rtol=0, atol=1e-5)
