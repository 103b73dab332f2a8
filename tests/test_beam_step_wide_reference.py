"""Cases of the wide bookkeeping kernels (csrc/beam_step.hip: asr_beam_candidates_wide, asr_beam_step_wide; 2048 < V <= 65536),
held to the SAME yardstick as the narrow ones: R.beam_step, R.beam_candidates, R.init_state, R.log_softmax32 and
R.candidate_gap of tests/test_beam_step_reference.py.  Nothing is added to R.CASES - the existing files parametrize over
that dict at collection - so this file keeps its own table, its own table generator and its own drive (copies of the few
lines of R.case_tables / R.run_case / R.case_ok keyed on WIDE_CASES), and tests/test_hip_beam_step_wide.py imports them.

The sizes come from the constants the wide kernels loop with (test_constants_are_the_kernels reads them back from the source):
  WIDE_NT   = 512   the workgroup of a row, and the stride of a thread over V         -> V = 2559, 2560, 2561 (5 strides +- 1)
  WIDE_BITS = 32    tokens per word of the candidate bit map (CTC modes only)         -> V = 2079, 2080, 2081 (65 words +- 1)
  WAVE      = 64    the wave-level reduction inside the workgroup                     -> V = 2111, 2112, 2113 (33 waves' width +- 1)
  4 * WAVE  = 256   tokens per wave up to WIDE_NT threads: the workgroup grows with V only below 1793 tokens, so every wide
                    vocabulary runs at 512 threads; the narrow cross-check of the GPU file (V = 2047, 2048) does too
plus the sizes the feature is for: 2049 (the first the narrow kernels refuse), 4097, 10 000, 16 385 and 65 536 (the limit).

The second half pins the end-to-end cases of the GPU file: a tiny seeded model at V = 2100 and V = 5000, whose oracle search
(oracle/decode_oracle.py::beam_search) is replayed through R.beam_step; a committed seed holds every decision of that replay
apart by more than R.GAP, so that an fp32 device search must find the same tokens."""
import os
import re

import numpy as np
import pytest

import test_beam_step_reference as R

WIDE_NT, WIDE_BITS, WAVE, WIDE_VMAX, WIDE_CMAX, NARROW_VMAX = 512, 32, 64, 65536, 32, 2048

_c = R._c
# options as in R.CASES; `hi` here pushes tokens 2..2048 down, so that every winner sits where the narrow kernels cannot reach;
# `tie`: every other row holds its best value on the tokens of ONE thread's stride (v, v + 512, ...)
WIDE_CASES = {
    'v2049_b5_ctc': _c(2049, 5, 'ctc', 8, [1], [5], 0, p_eos=0.3),
    'v2079_b5_ctc_lm': _c(2079, 5, 'ctc_lm', 7, [0], [4], 0, p_eos=0.3),
    'v2080_b1_ctc': _c(2080, 1, 'ctc', 3, [1], [6], 0, p_eos=0.4),
    'v2081_b16_ctc': _c(2081, 16, 'ctc', 24, [0], [3], 0, p_eos=0.3),
    'v2111_b5_att': _c(2111, 5, 'att', 0, [0], [4], 0, p_eos=0.3),
    'v2112_b16_lm': _c(2112, 16, 'lm', 0, [0], [3], 0, p_eos=0.3),
    'v2113_b1_lm': _c(2113, 1, 'lm', 0, [0], [4], 0, want=['b1_flush']),
    'v2559_b16_att': _c(2559, 16, 'att', 0, [0], [3], 0, p_eos=0.4, want=['multi_term']),
    'v2560_b5_ctc_lm': _c(2560, 5, 'ctc_lm', 8, [2], [5], 0, p_eos=0.3),
    'v2561_b1_att': _c(2561, 1, 'att', 0, [0], [8], 0, p_eos=0.4, want=['b1_stop']),
    'v4097_b16_ctc_lm': _c(4097, 16, 'ctc_lm', 24, [1], [3], 0, p_eos=0.3),
    'hi_v4097_b8_att': _c(4097, 8, 'att', 0, [0], [4], 0, hi=True, want=['all_hi']),
    'hi_v10000_b5_ctc_lm': _c(10000, 5, 'ctc_lm', 32, [0], [4], 0, hi=True, want=['all_hi']),
    'v10000_b5_lm': _c(10000, 5, 'lm', 0, [0], [4], 0, p_eos=0.3),
    'v16385_b16_att': _c(16385, 16, 'att', 0, [0], [3], 0, p_eos=0.3),
    'v16385_b1_ctc': _c(16385, 1, 'ctc', 3, [0], [4], 0),
    'v65536_b5_ctc_lm': _c(65536, 5, 'ctc_lm', 7, [0], [3], 0, p_eos=0.3),
    'v65536_b16_att': _c(65536, 16, 'att', 0, [0], [2], 0),
    'ragged_u3_b4_ctc_lm_v3000': _c(3000, 4, 'ctc_lm', 6, [0, 2, 1], [4, 7, 3], 0, p_eos=0.3, done0=True, want=['early_term']),
    'tie_v2561_b4': _c(2561, 4, 'att', 0, [0], [4], 0, tie=True),
    'tie_v10000_b16': _c(10000, 16, 'att', 0, [1], [3], 0, tie=True),
}
# the committed seeds, chosen on the CPU by the conditions of case_ok alone (first seed from 0 that holds them)
SEEDS = {'hi_v4097_b8_att': 2, 'ragged_u3_b4_ctc_lm_v3000': 1, 'v16385_b16_att': 4, 'v2049_b5_ctc': 1, 'v2081_b16_ctc': 3, 'v2112_b16_lm': 3,
         'v2559_b16_att': 10, 'v4097_b16_ctc_lm': 7}          # every other case: seed 0
for _n, _s in SEEDS.items():
    WIDE_CASES[_n]['seed'] = _s


def case_dims(name):
    c = WIDE_CASES[name]
    U, Lmax = len(c['max_len']), max(c['max_len'])
    return U, U * c['beam'], Lmax, Lmax + 1          # U, R, Lmax, tok_ld


def case_tables(name, t, seed=None):
    """The tables of step t: they depend on (seed, t) alone, not on the hypotheses."""
    c = WIDE_CASES[name]
    U, R_, _, _ = case_dims(name)
    V, opt = c['V'], c['opt']
    rng = np.random.RandomState(100003 * (c['seed'] if seed is None else seed) + 17 * t + V)
    if opt.get('tie'):
        att = -rng.randint(2, 7, size=(R_, V)) / 4.0
        for r in range(0, R_, 2):
            att[r, rng.randint(2, WIDE_NT)::WIDE_NT] = -0.25
        return {'att': att.astype(np.float32), 'lm': None, 'psi': None, 'cand': None}
    x = R.SCALE * rng.randn(R_, V)
    if opt.get('hi'):
        x[:, 2:NARROW_VMAX + 1] -= 4 * R.SCALE
    x[rng.rand(R_) < opt.get('p_eos', 0.0), 1] += 4 * R.SCALE
    tab = {'att': R.log_softmax32(x), 'lm': None, 'psi': None, 'cand': None}
    if 'lm' in c['mode']:
        tab['lm'] = R.log_softmax32(R.SCALE * rng.randn(R_, V))
    if 'ctc' in c['mode']:
        tab['cand'] = R.beam_candidates(tab['att'], c['C'])
        tab['psi'] = (-2.0 * (t + 1) + 2.0 * rng.randn(R_, c['C'])).astype(np.float32)
    return tab


def case_params(name, t):
    c = WIDE_CASES[name]
    return {'beam': c['beam'], 't': t, 'min_len': c['min_len'], 'max_len': c['max_len'], 'ctc_w': R.CTC_W if 'ctc' in c['mode'] else 0.0,
            'lm_w': R.LM_W if 'lm' in c['mode'] else 0.0, 'eos_thr': R.EOS_THR, 'tok_ld': case_dims(name)[3]}


def case_state0(name, dtype=np.float64):
    c = WIDE_CASES[name]
    st = R.init_state(len(c['max_len']), c['beam'], dtype)
    if c['opt'].get('done0'):
        st['done'][0] = 1
        st['finals'][0] = [(dtype(R.DONE0_FINAL[0]), list(R.DONE0_FINAL[1]), [dtype(s) for s in R.DONE0_FINAL[2]])]
    return st


def run_case(name, dtype=np.float64, seed=None):
    """The whole drive on the restatement alone -> ([state after step t], info); one call more than the longest utterance needs."""
    info = R.new_info()
    info['cand'] = R.INF
    st, outs = case_state0(name, dtype), []
    for t in range(max(WIDE_CASES[name]['max_len']) + 1):
        tab = case_tables(name, t, seed)
        info['events'].append(('step', t))
        if tab['cand'] is not None:
            info['cand'] = min(info['cand'], R.candidate_gap(tab['att'], WIDE_CASES[name]['C']))
        st = R.beam_step(st, tab, case_params(name, t), dtype, info=info)
        outs.append(st)
    return outs, info


_RUNS = {}


def reference(name, dtype=np.float64):
    """run_case of the committed seed, computed once and shared (the GPU file reads it too; nobody changes it)."""
    if (name, dtype) not in _RUNS:
        _RUNS[(name, dtype)] = run_case(name, dtype)
    return _RUNS[(name, dtype)]


def case_ok(name, seed=None):
    """The conditions a seed must meet, on the float64 restatement alone (R.case_ok's, with `all_hi` for R's `k1`)."""
    c = WIDE_CASES[name]
    outs, info = run_case(name, np.float64, seed) if seed is not None else reference(name)
    ev = info['events']
    fin = outs[-1]['finals'][0]
    has = {'all_hi': len(info['picked']) > 0 and all(v > NARROW_VMAX for v in info['picked']),
           'multi_term': R._multi_term(ev),
           'early_term': any(e[0] == 'term' and not e[2] for e in ev),
           'b1_stop': len(fin) == 1 and len(fin[0][1]) < c['max_len'][0] and fin[0][1][-1] == 1,
           'b1_flush': len(fin) == 1 and len(fin[0][1]) == c['max_len'][0]}
    if not all(has[w] for w in c['opt'].get('want', [])):
        return False
    if not all(outs[-1]['done']):
        return False
    if c['opt'].get('tie'):
        return info['topk'] == 0 and info['pool'] == 0 and info['final'] == 0
    if 'ctc' in c['mode'] and info['noncand']:
        return False
    return min(info['topk'], info['pool'], info['final'], info['eos'], info['cand']) > R.GAP


@pytest.mark.parametrize('name', sorted(WIDE_CASES))
def test_committed_seeds_hold_the_conditions(name):
    assert case_ok(name)


def test_the_table_covers_what_it_must():
    Vs = set(c['V'] for c in WIDE_CASES.values())
    assert {2049, 2112, 4097, 10000, 16385, 65536} <= Vs
    for width, k in ((WIDE_NT, 5), (WIDE_BITS, 65), (WAVE, 33)):
        assert {k * width - 1, k * width, k * width + 1} <= Vs
    assert all(NARROW_VMAX < v <= WIDE_VMAX for v in Vs)
    assert set(c['mode'] for c in WIDE_CASES.values()) == {'att', 'ctc', 'lm', 'ctc_lm'}
    assert {1, 5, 16} <= set(c['beam'] for c in WIDE_CASES.values())
    assert all(c['C'] <= WIDE_CMAX for c in WIDE_CASES.values()) and any(c['C'] == WIDE_CMAX for c in WIDE_CASES.values())
    assert any(len(c['max_len']) == 3 and c['opt'].get('done0') for c in WIDE_CASES.values())
    assert sum(1 for c in WIDE_CASES.values() if c['opt'].get('tie')) == 2


def test_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'e2e-asr-pytorch_amd', 'csrc', 'beam_step.hip')).read()
    const = lambda n: int(re.search(r'\b%s = (\d+)\b' % n, src).group(1))
    assert (const('WIDE_NT'), const('WIDE_BITS'), const('WIDE_VMAX'), const('WIDE_CMAX')) == (WIDE_NT, WIDE_BITS, WIDE_VMAX, WIDE_CMAX)
    assert const('VPL') * WAVE == NARROW_VMAX


def test_tie_cases_hold_ties_in_one_stride_and_across_threads():
    ties = []
    for name in WIDE_CASES:
        if WIDE_CASES[name]['opt'].get('tie'):
            ties += reference(name)[1]['ties']
    assert any((b - a) % WIDE_NT == 0 for a, b in ties)          # v and v + 512k: one thread's stride
    assert any((b - a) % WIDE_NT != 0 for a, b in ties)          # different threads
    assert all(a < b for a, b in ties)                           # the lower token was the one taken


def test_fp32_transcription_decides_alike():
    for name in WIDE_CASES:
        o64, o32 = reference(name)[0], reference(name, np.float32)[0]
        for a, b in zip(o64, o32):
            assert a['seq'] == b['seq'] and [[f[1] for f in u] for u in a['finals']] == [[f[1] for f in u] for u in b['finals']], name
            for k in ('alive', 'len', 'parent', 'ctc_index', 'last_token', 'tok_val', 'done'):
                assert (a[k] == b[k]).all(), (name, k)


def step_fp32_dev(name):
    """deviation of the fp32 transcription of the drive from float64 on one case: what sizes the GPU file's tolerance."""
    rel = lambda got, want: 0.0 if np.size(got) == 0 else float((np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
                                                                  / np.maximum(1.0, np.abs(np.asarray(want, np.float64)))).max())
    dev = 0.0
    for a, b in zip(reference(name)[0], reference(name, np.float32)[0]):
        dev = max(dev, rel(b['sum'], a['sum']), rel(b['ctcp'], a['ctcp']))
        for x, y in zip(a['score'], b['score']):
            dev = max(dev, rel(y, x))
        for fa, fb in zip(a['finals'], b['finals']):
            for (avg, _, sc), (avg2, _, sc2) in zip(fa, fb):
                dev = max(dev, rel(avg2, avg), rel(sc2, sc))
    return dev


# ---- end to end: a tiny seeded model at a wide vocabulary --------------------------------------------------------------------
E2E_MODEL = {'ctc_weight': 0.5,
             'encoder': {'vgg': 0, 'vgg_freq': -1, 'vgg_low_filt': -1, 'module': 'LSTM', 'bidirection': True, 'dim': [16, 16],
                         'dropout': [0.0, 0.0], 'layer_norm': [False, False], 'proj': [True, True], 'sample_rate': [1, 2],
                         'sample_style': 'drop'},
             'attention': {'mode': 'loc', 'dim': 12, 'num_head': 1, 'v_proj': False, 'temperature': 0.5, 'loc_kernel_size': 3,
                           'loc_kernel_num': 4},
             'decoder': {'module': 'LSTM', 'dim': 12, 'layer': 1, 'dropout': 0}}
E2E_LM = {'dim': 16, 'dropout': 0.0, 'emb_dim': 16, 'emb_tying': True, 'module': 'LSTM', 'n_layers': 2}
E2E_D, E2E_BEAM, E2E_MIN_RATIO, E2E_MAX_RATIO = 20, 4, 0.01, 0.12
E2E_LENS = (41, 29, 50)                  # the ragged batch of 3; the single utterance is the first
# Seeded weights are N(0, 1/fan_in): over thousands of tokens the 12-wide decoder state gives log-probs that differ in the
# fourth digit only.  char_trans.weight is scaled by this factor in BOTH models (the oracle's and the device's), which
# spreads them as a trained output layer does.
E2E_CHAR_SCALE = 20.0
E2E_SETTINGS = {'att': (0.0, 0.0), 'ctc': (0.3, 0.0), 'lm': (0.0, 0.5), 'ctc_lm': (0.3, 0.5)}
# (V, setting) -> (weight seed, feature seed); chosen on the CPU by e2e_gaps alone
E2E_SEEDS = {(2100, 'att'): (501, 701), (2100, 'ctc'): (507, 707), (2100, 'ctc_lm'): (507, 707), (2100, 'lm'): (500, 700),
             (5000, 'att'): (502, 702), (5000, 'ctc'): (502, 702), (5000, 'ctc_lm'): (511, 711), (5000, 'lm'): (500, 700)}
_E2E = {}


def e2e_weights(V, wseed):
    """-> (cfg, P, lm parameters): what the oracle decodes with and what the GPU file loads into ASR / RNNLM."""
    import torch
    from oracle import asr_oracle as O
    cfg = O.ModelCfg(E2E_MODEL, E2E_D, V)
    P = O.seeded_state_dict(O.param_shapes(cfg), wseed)
    P['decoder.char_trans.weight'] = P['decoder.char_trans.weight'] * E2E_CHAR_SCALE
    g = np.random.Generator(np.random.PCG64(wseed + 1))
    lm_shapes = {'emb.weight': (V, E2E_LM['emb_dim'])}
    for l in range(E2E_LM['n_layers']):
        k = E2E_LM['emb_dim'] if l == 0 else E2E_LM['dim']
        lm_shapes.update({'rnn.weight_ih_l%d' % l: (4 * E2E_LM['dim'], k), 'rnn.weight_hh_l%d' % l: (4 * E2E_LM['dim'], E2E_LM['dim']),
                          'rnn.bias_ih_l%d' % l: (4 * E2E_LM['dim'],), 'rnn.bias_hh_l%d' % l: (4 * E2E_LM['dim'],)})
    P_lm = {k: torch.from_numpy((g.standard_normal(s) * (0.5 if len(s) > 1 else 0.1)).astype(np.float32)) for k, s in lm_shapes.items()}
    return cfg, P, P_lm


def e2e_features(fseed):
    import torch
    g = np.random.Generator(np.random.PCG64(fseed))
    return [torch.from_numpy(g.random((1, T, E2E_D), dtype=np.float32)) for T in E2E_LENS]


def e2e_oracle(V, tag):
    """-> [(hypotheses of utterance u as the oracle returns them, info of their replay through R.beam_step)], cached."""
    import torch
    from oracle import decode_oracle as DO
    if (V, tag) not in _E2E:
        wseed, fseed = E2E_SEEDS[(V, tag)]
        ctc_w, lm_w = E2E_SETTINGS[tag]
        cfg, P, P_lm = e2e_weights(V, wseed)
        out = []
        for feat in e2e_features(fseed):
            flen = torch.tensor([feat.shape[1]], dtype=torch.int64)
            trace = []
            ref = DO.beam_search(feat, flen, P, cfg, E2E_BEAM, E2E_MIN_RATIO, E2E_MAX_RATIO, ctc_weight=ctc_w,
                                 lm=(P_lm, E2E_LM) if lm_w > 0 else None, lm_weight=lm_w, trace=trace)
            out.append((ref, e2e_replay(trace, V, feat.shape[1], ctc_w, lm_w, ref)))
        _E2E[(V, tag)] = out
    return _E2E[(V, tag)]


def e2e_replay(trace, V, T, ctc_w, lm_w, want):
    """The oracle's tables through R.beam_step (scores in float32, sums in float64: the oracle's arithmetic, as R._replay has
    it) -> info with the smallest margin of every kind of decision; asserts that the replay ends in the oracle's hypotheses."""
    beam = E2E_BEAM
    max_len, min_len = int(np.ceil(T * E2E_MAX_RATIO)), int(np.ceil(T * E2E_MIN_RATIO))
    tab = {(t, seq): (att, cand, ctcp, lm) for t, seq, att, cand, ctcp, lm in trace}
    C = len(trace[0][3]) if trace[0][3] is not None else 0
    info = R.new_info()
    info['cand'] = R.INF
    st = R.init_state(1, beam, np.float32)
    st['sum'] = st['sum'].astype(np.float64)
    for t in range(max_len):
        tables = {'att': np.zeros((beam, V), np.float32), 'lm': np.zeros((beam, V), np.float32) if lm_w > 0 else None,
                  'psi': np.zeros((beam, C), np.float32) if C else None, 'cand': np.zeros((beam, C), np.int64) if C else None}
        for i in range(beam):
            if st['alive'][i]:
                assert (t, tuple(st['seq'][i])) in tab, 'the replay expands a hypothesis the oracle did not'
                att, cand, ctcp, lm = tab[(t, tuple(st['seq'][i]))]
                tables['att'][i] = att.numpy()
                if C:
                    tables['cand'][i], tables['psi'][i] = cand, ctcp
                    info['cand'] = min(info['cand'], R.candidate_gap(tables['att'][i:i + 1], C))
                if lm_w > 0:
                    tables['lm'][i] = lm.numpy()[0]
        st = R.beam_step(st, tables, {'beam': beam, 't': t, 'min_len': [min_len], 'max_len': [max_len], 'ctc_w': np.float32(ctc_w),
                                      'lm_w': np.float32(lm_w), 'eos_thr': 1.5, 'tok_ld': max_len + 1}, np.float32, np.float64, info=info)
        if st['done'][0]:
            break
    assert st['done'][0]
    assert [f[1] for f in st['finals'][0]] == [seq for seq, _ in want]
    return info


def e2e_gaps(V, tag):
    gaps = []
    for _, info in e2e_oracle(V, tag):
        if tag.startswith('ctc') and info['noncand']:
            return 0.0
        gaps.append(min(info['topk'], info['pool'], info['final'], info['eos'], info['cand']))
    return min(gaps)


@pytest.mark.parametrize('V', [2100, 5000])
@pytest.mark.parametrize('tag', sorted(E2E_SETTINGS))
def test_end_to_end_seeds_hold_every_decision_apart(V, tag):
    assert e2e_gaps(V, tag) > R.GAP
    assert all(len(ref) >= 1 and max(max(seq) for seq, _ in ref) > 1 for ref, _ in e2e_oracle(V, tag))
