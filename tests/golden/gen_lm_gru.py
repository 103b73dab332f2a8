#!/usr/bin/env python
"""Generates the GRU language-model fixtures from the GENUINE reference (src/lm.py, src/decode.py), run on the CPU in the build
container only:

    python tests/golden/gen_lm_gru.py

g12_lm_gru_train_<tied|untied>_l<1|2>.npz: the reference RNNLM(V=31, ..., 'GRU', ..., dropout=0) in training mode on a padded
token batch (packed by `lens`, as the reference does).  Stored: tokens, lengths, targets (0 = padding), every weight, the logits
at the valid positions, the cross-entropy loss (ignore_index 0) and every parameter gradient.

g12_beam_gru_lm_<case>.npz: the reference BeamDecoder with a 2-layer GRU LM loaded through lm_config / lm_path (a reference
checkpoint {'model': state_dict} written to a temporary directory), beam 4, in the modes att + LM (0, 0.5) and CTC + LM
(0.3, 0.5).  The ASR weights are rebuilt by the tests from `wseed` exactly as for g11_beam_* (gen_beam_variants.tweak); the LM
weights from `lm_wseed` with oracle.asr_oracle.seeded_state_dict.  Weight seeds are searched until every adjacent pair of
returned hypotheses differs by at least MIN_GAP in average score (recorded as min_gap), so no test has to accept a reordering.
"""
import os
import sys
import tempfile

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import O, save  # noqa: E402
from gen_beam_variants import BEAM, MAX_RATIO, MIN_GAP, MIN_RATIO, D, T, V, build, case_cfg, min_gap, SCALES, EOS_SHIFTS  # noqa: E402

LM_CFG = {'emb_tying': True, 'emb_dim': 16, 'module': 'GRU', 'dim': 16, 'n_layers': 2, 'dropout': 0.0}
LM_WSEED = 47
MODES = (('att_lm', 0.0, 0.5), ('ctc_lm', 0.3, 0.5))
BEAM_CASES = [
    ('small', case_cfg(), 2100, 'fast'),
    ('gru1_dot', case_cfg(att={'mode': 'dot'}, dec={'module': 'GRU'}), 2200, 'variant'),
]
TRAIN_CASES = [('tied_l1', True, 1), ('tied_l2', True, 2), ('untied_l1', False, 1), ('untied_l2', False, 2)]
TRAIN_DIM, TRAIN_B, TRAIN_T = 24, 4, 13


def gen_train():
    from src.lm import RNNLM
    for i, (name, tying, nl) in enumerate(TRAIN_CASES):
        torch.manual_seed(1200 + i)
        lm = RNNLM(V, tying, TRAIN_DIM, 'GRU', TRAIN_DIM, nl, 0.0)
        lm.train()
        g = np.random.Generator(np.random.PCG64(1210 + i))
        lens = np.array([TRAIN_T, 9, TRAIN_T - 1, 4], dtype=np.int64)
        x = g.integers(1, V, (TRAIN_B, TRAIN_T)).astype(np.int64)
        y = g.integers(1, V, (TRAIN_B, TRAIN_T)).astype(np.int64)
        for b, n in enumerate(lens):
            x[b, n:] = 0
            y[b, n:] = 0
        out, _ = lm(torch.from_numpy(x), torch.from_numpy(lens))
        loss = torch.nn.functional.cross_entropy(out.reshape(-1, V), torch.from_numpy(y).view(-1), ignore_index=0)
        loss.backward()
        arrays = dict(tokens=x, lens=lens, targets=y, logits=out.detach().numpy(), loss=np.array(loss.item(), dtype=np.float32))
        for k, v in lm.state_dict().items():
            arrays['w:' + k] = v.numpy()
        for k, p in lm.named_parameters():
            arrays['g:' + k] = p.grad.numpy()
        meta = {'V': V, 'emb_tying': tying, 'emb_dim': TRAIN_DIM, 'module': 'GRU', 'dim': TRAIN_DIM, 'n_layers': nl, 'dropout': 0.0,
                'torch_seed': 1200 + i}
        save('g12_lm_gru_train_' + name, meta, arrays)


def lm_state_dict():
    from src.lm import RNNLM
    lm = RNNLM(V, **LM_CFG)
    return O.seeded_state_dict({k: tuple(v.shape) for k, v in lm.state_dict().items()}, LM_WSEED)


def decode(model, feat, flen, ctc_w, lm_w, lm_config, lm_path):
    from src.decode import BeamDecoder
    dec = BeamDecoder(model, None, beam_size=BEAM, min_len_ratio=MIN_RATIO, max_len_ratio=MAX_RATIO, lm_path=lm_path,
                      lm_config=lm_config, lm_weight=lm_w, ctc_weight=ctc_w)
    with torch.no_grad():
        hyps = dec(torch.from_numpy(feat), torch.from_numpy(flen))
    return [(list(h.outIndex), [float(s) for s in h.output_scores], float(h.avgScore())) for h in hyps]


def gen_beam():
    with tempfile.TemporaryDirectory() as tmp:
        lm_config, lm_path = os.path.join(tmp, 'lm.yaml'), os.path.join(tmp, 'lm.pth')
        yaml.safe_dump({'model': LM_CFG}, open(lm_config, 'w'))
        torch.save({'model': lm_state_dict()}, lm_path)
        for i, (name, mc, seed0, path) in enumerate(BEAM_CASES):
            g = np.random.Generator(np.random.PCG64(2100 + i))
            feat = g.random((1, T, D), dtype=np.float32)
            flen = np.array([T], dtype=np.int64)
            found = None
            for seed in range(seed0, seed0 + 60):
                for scale in SCALES:
                    for shift in EOS_SHIFTS:
                        model = build(mc, seed, scale, shift)
                        res = {tag: decode(model, feat, flen, cw, lw, lm_config, lm_path) for tag, cw, lw in MODES}
                        gap = min_gap(res)
                        if gap >= MIN_GAP and all(len(r) > 1 for r in res.values()):
                            found = (seed, scale, shift, gap, res)
                            break
                    if found:
                        break
                if found:
                    break
            if found is None:
                raise RuntimeError('%s: no seed without near-ties' % name)
            seed, scale, shift, gap, res = found
            print('%s: seed %d scale %.1f shift %.1f min gap %.2e' % (name, seed, scale, shift, gap))
            arrays = dict(feat=feat, feat_len=flen)
            for tag, r in res.items():
                arrays['n_' + tag] = np.array(len(r))
                for j, (seq, sc, avg) in enumerate(r):
                    arrays['%s_seq%d' % (tag, j)] = np.array(seq, dtype=np.int64)
                    arrays['%s_score%d' % (tag, j)] = np.array(sc, dtype=np.float32)
                    arrays['%s_avg%d' % (tag, j)] = np.array(avg, dtype=np.float32)
            meta = {'model': mc, 'D': D, 'V': V, 'wseed': seed, 'ct_scale': scale, 'eos_shift': shift, 'min_gap': float(gap),
                    'lm': LM_CFG, 'lm_wseed': LM_WSEED, 'beam': BEAM, 'min_len_ratio': MIN_RATIO, 'max_len_ratio': MAX_RATIO,
                    'modes': [[t, c, l] for t, c, l in MODES], 'path': path, 'set_mem_standin': mc['attention']['mode'] == 'dot'}
            save('g12_beam_gru_lm_' + name, meta, arrays)


def main():
    torch.manual_seed(0)
    gen_train()
    gen_beam()


if __name__ == '__main__':
    main()
