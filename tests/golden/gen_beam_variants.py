#!/usr/bin/env python
"""Generates tests/golden/g11_beam_<case>.npz: the GENUINE reference's BeamDecoder (src/decode.py:65-183) on the model variants
the config surface accepts, run on the CPU in the build container only:

    python tests/golden/gen_beam_variants.py

Each case is a small seeded model (gen_golden.small_model_cfg with the variant's attention / decoder settings), decoded with
beam 4 three times: attention only, + CTC 0.3, + CTC 0.3 + RNN-LM 0.5 (the LM of g7_decode).  Weights are not stored: they are
rebuilt from `wseed` with oracle.asr_oracle.seeded_state_dict, then char_trans (weight and bias) is multiplied by `ct_scale`
and `eos_shift` is added to char_trans.bias[1] - the tests apply the same two changes.  Random weights give near-ties between
returned hypotheses, so the generator searches weight seeds and scales until every adjacent pair of returned hypotheses, in
every mode, differs by at least MIN_GAP in average score; the smallest gap is recorded in the meta.

One stand-in is patched into the reference, for the dot-attention cases ONLY: its ScaleDotAttention inherits
BaseAttention.set_mem(self) while BeamDecoder calls asr.set_state(..., prev_attn) -> att_layer.set_mem(prev_attn) and crashes
(TypeError, src/module.py:1098 vs src/decode.py).  Dot attention keeps no memory, so the stand-in is a set_mem(prev_att) that
does nothing - the intended semantics.  It is patched on the instance, like gen_golden.MaskDrop.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import O, REF, save, small_model_cfg  # noqa: E402,F401

MIN_GAP = 1e-3
V, D, T = 31, 20, 61
BEAM, MIN_RATIO, MAX_RATIO = 4, 0.01, 0.12
LM_CFG = {'emb_tying': True, 'emb_dim': 16, 'module': 'LSTM', 'dim': 16, 'n_layers': 2, 'dropout': 0.0}
LM_WSEED = 43
MODES = (('att', 0.0, 0.0), ('ctc', 0.3, 0.0), ('ctc_lm', 0.3, 0.5))


def case_cfg(att=None, dec=None, emb_drop=0.0):
    mc = small_model_cfg()
    mc['attention'].update(att or {})
    mc['decoder'].update(dec or {})
    if emb_drop:
        mc['emb_drop'] = emb_drop
    return mc


# name, model cfg, first weight seed, path of our build
CASES = [
    ('dot', case_cfg(att={'mode': 'dot'}), 1100, 'variant'),
    ('dot_mh3', case_cfg(att={'mode': 'dot', 'num_head': 3}), 1200, 'variant'),
    ('loc_mh2', case_cfg(att={'num_head': 2}), 1300, 'variant'),
    ('loc_mh2_vproj', case_cfg(att={'num_head': 2, 'v_proj': True}), 1400, 'variant'),
    ('gru2', case_cfg(dec={'module': 'GRU', 'layer': 2}), 1500, 'variant'),
    ('gru1_dot', case_cfg(att={'mode': 'dot'}, dec={'module': 'GRU'}), 1600, 'variant'),
    ('lstm5', case_cfg(dec={'layer': 5}), 1700, 'variant'),
    ('decdrop2', case_cfg(dec={'layer': 2, 'dropout': 0.25}, emb_drop=0.2), 1800, 'fast'),
]
SCALES = (2.0, 3.0, 4.0)
EOS_SHIFTS = (0.0, 2.0)


def tweak(sd, scale, shift):
    """char_trans x scale, + shift on the <eos> logit bias (applied identically by the tests)."""
    sd = dict(sd)
    sd['decoder.char_trans.weight'] = sd['decoder.char_trans.weight'] * scale
    b = sd['decoder.char_trans.bias'] * scale
    b[1] += shift
    sd['decoder.char_trans.bias'] = b
    return sd


def build(mc, wseed, scale, shift):
    from src.asr import ASR
    cfg = O.ModelCfg(mc, D, V)
    model = ASR(D, V, 4, **mc)
    model.load_state_dict(tweak(O.seeded_state_dict(O.param_shapes(cfg), wseed), scale, shift))
    model.eval()
    if mc['attention']['mode'] == 'dot':
        model.attention.att_layer.set_mem = types.MethodType(lambda self, prev_att=None: None, model.attention.att_layer)
    return model


def the_lm():
    from src.lm import RNNLM
    lm = RNNLM(V, **LM_CFG)
    lm.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in lm.state_dict().items()}, LM_WSEED))
    return lm.eval()


def decode(model, lm, feat, flen, beam, ctc_w, lm_w):
    from src.decode import BeamDecoder
    dec = BeamDecoder(model, None, beam_size=beam, min_len_ratio=MIN_RATIO, max_len_ratio=MAX_RATIO, ctc_weight=ctc_w)
    if lm_w > 0:
        dec.apply_lm, dec.lm_w, dec.lm = True, lm_w, lm
    with torch.no_grad():
        hyps = dec(torch.from_numpy(feat), torch.from_numpy(flen))
    return [(list(h.outIndex), [float(s) for s in h.output_scores], float(h.avgScore())) for h in hyps]


def min_gap(results):
    gaps = [abs(a[2] - b[2]) for r in results.values() for a, b in zip(r, r[1:])]
    return min(gaps) if gaps else float('inf')


def search(name, mc, seed0, beam, feat, flen, lm, need_early=False, modes=MODES):
    max_len = int(np.ceil(int(flen[0]) * MAX_RATIO))
    for seed in range(seed0, seed0 + 60):
        for scale in SCALES:
            for shift in EOS_SHIFTS:
                model = build(mc, seed, scale, shift)
                res = {tag: decode(model, lm, feat, flen, beam, cw, lw) for tag, cw, lw in modes}
                g = min_gap(res)
                early = any(len(h[0]) < max_len for r in res.values() for h in r)
                if g >= MIN_GAP and (early or not need_early) and all(len(r) > 0 for r in res.values()):
                    print('%s: seed %d scale %.1f shift %.1f min gap %.2e early-<eos> %s' % (name, seed, scale, shift, g, early))
                    return seed, scale, shift, g, res, early
    raise RuntimeError('%s: no seed without near-ties' % name)


def write(name, mc, path, beam, feat, flen, seed, scale, shift, g, res, modes=MODES):
    arrays = dict(feat=feat, feat_len=flen)
    for tag, r in res.items():
        arrays['n_' + tag] = np.array(len(r))
        for i, (seq, sc, avg) in enumerate(r):
            arrays['%s_seq%d' % (tag, i)] = np.array(seq, dtype=np.int64)
            arrays['%s_score%d' % (tag, i)] = np.array(sc, dtype=np.float32)
            arrays['%s_avg%d' % (tag, i)] = np.array(avg, dtype=np.float32)
    meta = {'model': mc, 'D': D, 'V': V, 'wseed': seed, 'ct_scale': scale, 'eos_shift': shift, 'min_gap': float(g),
            'lm': LM_CFG, 'lm_wseed': LM_WSEED, 'beam': beam, 'min_len_ratio': MIN_RATIO, 'max_len_ratio': MAX_RATIO,
            'modes': [[t, c, l] for t, c, l in modes], 'path': path, 'set_mem_standin': mc['attention']['mode'] == 'dot'}
    save('g11_beam_' + name, meta, arrays)


def main():
    torch.manual_seed(0)
    lm = the_lm()
    any_early = False
    for i, (name, mc, seed0, path) in enumerate(CASES):
        g = np.random.Generator(np.random.PCG64(1100 + i))
        feat = g.random((1, T, D), dtype=np.float32)
        flen = np.array([T], dtype=np.int64)
        seed, scale, shift, gap, res, early = search(name, mc, seed0, BEAM, feat, flen, lm)
        any_early |= early
        write(name, mc, path, BEAM, feat, flen, seed, scale, shift, gap, res)
    assert any_early, 'no case ends a hypothesis with <eos> before max_len'
    # beam 1: the reference returns as soon as the single hypothesis ends (src/decode.py:170-171).  Attention only: with CTC
    # its single candidate (int(1.5 * 1) = 1) can miss the fused top-1 and the reference fails (list.index, src/decode.py:252)
    name, mc = 'beam1', case_cfg(att={'num_head': 2})
    g = np.random.Generator(np.random.PCG64(1190))
    feat = g.random((1, T, D), dtype=np.float32)
    flen = np.array([T], dtype=np.int64)
    seed, scale, shift, gap, res, early = search(name, mc, 1900, 1, feat, flen, lm, need_early=True, modes=MODES[:1])
    write(name, mc, 'variant', 1, feat, flen, seed, scale, shift, gap, res, modes=MODES[:1])


if __name__ == '__main__':
    main()
