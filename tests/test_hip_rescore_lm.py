"""asr_rescore_lm_input / asr_rescore_token_logp / asr_rescore_rank_lm (csrc/rescore.hip) and
BeamDecoder(rescore=True, lm_rescore=True) against the float64 restatements of tests/test_rescore_lm_reference.py.

Kernel cases: the table of that file (its seeds hold GAP between adjacent totals, so `order` must match EXACTLY).  The device
reads the logits from a block whose row and position strides exceed V, with NaN in all padding and at every position >= len;
`out` has a leading dimension above L with NaN canary columns behind L, lm_in a canary tail; all must survive.  Scores are held to
SCORE_TOL = 4 x the recorded deviation of the fp32 transcription, relative to max(1, |score| / 20).

End to end: the seeded joint model of tests/test_hip_rescore.py and the seeded LSTM / GRU LMs of tests/test_hip_ctc_beam_lm.py.
The first pass must equal the float64 prefix beam search WITHOUT an LM on the model's own CTC log-probs; att_score holds as in
tests/test_hip_rescore.py; lm_score must equal the restatement on the float64 torch.nn.LSTM / GRU with the same weights within
2 x logit bound x n (SURVEY 8d bounds the logits by 1e-4 in fp32 and 5e-2 in bf16, and log_softmax at most doubles a uniform logit
error); the total's bound is the sum of the two, and in fp32 the order must be the oracle's, whose adjacent totals are asserted to
be further apart than twice that."""
import numpy as np
import pytest
import torch

from test_hip_ctc_beam import SCORE_TOL as CTC_SCORE_TOL
from test_hip_ctc_beam_lm import _restated_lm, _seeded_lm
from test_hip_rescore import (BF16_LOGIT_TOL, E2E_BEAM, E2E_LENS, E2E_W, FP32_LOGIT_TOL, SCORE_TOL as NBEST_SCORE_TOL, _first_pass,
                              _joint_model, case_inputs as nbest_case_inputs, oracle_second_pass, run_nbest)
from test_rescore_lm_reference import (CASES, FP32_DEV, NEG_INF, SCORE_TOL, SOS, case_inputs, rank_lm, reference, rel)
from test_rescore_reference import pack, targets_of

E_ARG = -1
CANARY = 3                              # NaN columns of `out` behind L, -7 elements behind lm_in


# ---- the kernels -----------------------------------------------------------------------------------------------------------
def _device_case(name):
    """A case on the device: the logits in a NaN-filled block with the case's padding, numbers only at [r, t < min(len, L), :V];
    teacher with a leading dimension above L; every output pre-filled with a sentinel."""
    dev = torch.device('cuda')
    K, V, L, (w, lw, bonus), pad, utts = case_inputs(name)
    U, R = len(utts), len(utts) * K
    ps, Lr = V + pad, L + 2
    rs = L * ps + 2 * pad
    host = np.full((R, rs), np.nan, dtype=np.float32)
    teacher, lens = np.zeros((R, Lr), dtype=np.int64), np.zeros(R, dtype=np.int32)
    att, ctc, n = np.zeros((U, K), dtype=np.float32), np.zeros((U, K), dtype=np.float32), np.zeros(U, dtype=np.int32)
    for u, c in enumerate(utts):
        teacher[u * K:(u + 1) * K] = pack(c['hyps'], Lr)[0]
        lens[u * K:(u + 1) * K], att[u], ctc[u], n[u] = c['lens'], c['att'], c['ctc'], c['n']
        for i in range(K):
            for t in range(max(0, min(int(c['lens'][i]), L))):
                host[u * K + i, t * ps:t * ps + V] = c['logits'][i, t]
    t_ = lambda a: torch.from_numpy(a).to(dev)
    b = {'logits': t_(host), 'teacher': t_(teacher), 'len': t_(lens), 'att': t_(att), 'ctc': t_(ctc), 'n': t_(n),
         'lm_in': torch.full((R * L + CANARY,), -7, dtype=torch.int64, device=dev),
         'out': torch.full((R, L + CANARY), float('nan'), dtype=torch.float32, device=dev),
         'lm_score': torch.full((U, K), 7.0, dtype=torch.float32, device=dev), 'total': torch.full((U, K), 7.0, dtype=torch.float32, device=dev),
         'order': torch.full((U, K), -7, dtype=torch.int32, device=dev)}
    return b, dict(U=U, R=R, K=K, V=V, L=L, Lr=Lr, ps=ps, rs=rs, out_ld=L + CANARY, w=w, lw=lw, bonus=bonus)


def _ptrs(b, null=None):
    from src import hipabi as H
    return {k: (None if k == null else H.ptr(v)) for k, v in b.items()}


def _lm_input(b, d, null=None, **over):
    from src import hipabi as H
    a, p = dict(d, **over), _ptrs(b, null)
    return H.lib().asr_rescore_lm_input(p['teacher'], a['Lr'], a['R'], a['L'], a.get('sos', SOS), p['lm_in'], H.stream_ptr())


def _token_logp(b, d, null=None, r0=0, r1=None, **over):
    """One launch over the rows r0..r1 (all by default)."""
    from src import hipabi as H
    a, p = dict(d, **over), _ptrs(b, null)
    r1 = d['R'] if r1 is None else r1
    sub = lambda k, t: None if p[k] is None else H.ptr(t[r0:r1])
    return H.lib().asr_rescore_token_logp(sub('logits', b['logits']), a['rs'], a['ps'], sub('teacher', b['teacher']), a['Lr'], sub('len', b['len']),
                                          a.get('rows', r1 - r0), a['L'], a['V'], sub('out', b['out']), a['out_ld'], H.stream_ptr())


def _rank_lm(b, d, null=None, **over):
    from src import hipabi as H
    a, p = dict(d, **over), _ptrs(b, null)
    return H.lib().asr_rescore_rank_lm(p['att'], p['ctc'], p['out'], a['out_ld'], p['len'], p['n'], a['U'], a['K'], a['L'], a['w'], a['lw'],
                                       a['bonus'], p['lm_score'], p['total'], p['order'], H.stream_ptr())


def _close(what, got, want, where):
    if want == NEG_INF:
        assert got == NEG_INF, (where, what, got)
        return 0.0
    err = rel(float(got), float(want))
    assert err <= SCORE_TOL, (where, what, float(got), float(want), err)
    return err


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_kernels_equal_the_float64_restatement(name):
    b, d = _device_case(name)
    U, R, K, L = d['U'], d['R'], d['K'], d['L']
    assert _lm_input(b, d) == 0 and _token_logp(b, d) == 0 and _rank_lm(b, d) == 0
    torch.cuda.synchronize()
    lm_in, out = b['lm_in'].cpu().numpy(), b['out'].cpu().numpy()
    lm_score, total, order = b['lm_score'].cpu().numpy(), b['total'].cpu().numpy(), b['order'].cpu().numpy()
    assert (lm_in[R * L:] == -7).all() and np.isnan(out[:, L:]).all()                 # the canaries survive
    assert not np.isnan(out[:, :L]).any() and not np.isnan(lm_score).any() and not np.isnan(total).any()
    worst = 0.0
    for u, (teacher64, lm_in64, tl64, lm64, total64, order64) in enumerate(reference(name)):
        rows = slice(u * K, (u + 1) * K)
        assert np.array_equal(lm_in[:R * L].reshape(R, L)[rows], lm_in64), u            # bit for bit
        assert order[u].tolist() == order64, (u, order[u].tolist(), order64)
        for i in range(K):
            for t in range(L):
                worst = max(worst, _close('tok_logp', out[u * K + i, t], tl64[i, t], (u, i, t)))
            worst = max(worst, _close('lm_score', lm_score[u, i], lm64[i], (u, i)), _close('total', total[u, i], total64[i], (u, i)))
            print('utt %d slot %d: lm_score %.6f (float64 %.6f) total %.6f (float64 %.6f)' % (u, i, lm_score[u, i], lm64[i], total[u, i], total64[i]))
    print('%s: largest relative deviation %.3g (allowed %.3g = 4 x the fp32 transcription\'s recorded %.3g)' % (name, worst, SCORE_TOL, FP32_DEV))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['v31_l2_k4', 'v65_l37_k16', 'v300_l37_k4_ragged_u3', 'v1025_l2_k4_second_block', 'holes'])
def test_token_logp_in_two_chunks_is_one_launch_bit_for_bit(name):
    b, d = _device_case(name)
    assert _token_logp(b, d) == 0
    torch.cuda.synchronize()
    whole = b['out'].cpu().numpy().copy()
    b['out'].fill_(float('nan'))
    cut = d['R'] // 2 + 1                                                               # inside an utterance, not at a workgroup's edge
    assert _token_logp(b, d, r0=0, r1=cut) == 0 and _token_logp(b, d, r0=cut) == 0
    torch.cuda.synchronize()
    assert np.array_equal(whole.view(np.uint32), b['out'].cpu().numpy().view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['v31_l2_k4', 'v65_l37_k16', 'v300_l37_k4_ragged_u3', 'holes', 'target_hole'])
def test_without_lm_weight_and_bonus_rank_lm_is_rescore_nbest(name):
    """Cases of tests/test_hip_rescore.py whose first_score == ctc_score: asr_rescore_nbest's att_score goes into
    asr_rescore_rank_lm with lm_weight = 0 and len_bonus = 0; total and order must be asr_rescore_nbest's own."""
    from src import hipabi as H
    dev = torch.device('cuda')
    K, V, L, w, pad, utts = nbest_case_inputs(name)
    rc, att, total_n, order_n = run_nbest(name)
    assert rc == 0
    U = len(utts)
    ctc = np.stack([c for _, _, c, f in utts]).astype(np.float32)
    assert all((c == f).all() for _, _, c, f in utts)
    n = np.array([sum(x is not None for x in h) for h, _, _, _ in utts], dtype=np.int32)
    lens = np.array([[len(x) if x is not None else 0 for x in h] for h, _, _, _ in utts], dtype=np.int32)
    t_ = lambda a: torch.from_numpy(a).to(dev)
    tok = torch.full((U * K, L), -1.0, dtype=torch.float32, device=dev)              # summed into lm_score, which lm_weight = 0 leaves out
    lm_score, total = torch.empty((U, K), dtype=torch.float32, device=dev), torch.empty((U, K), dtype=torch.float32, device=dev)
    order = torch.empty((U, K), dtype=torch.int32, device=dev)
    att_d, ctc_d, lens_d, n_d = t_(att), t_(ctc), t_(lens), t_(n)
    H.call('asr_rescore_rank_lm', H.ptr(att_d), H.ptr(ctc_d), H.ptr(tok), L, H.ptr(lens_d), H.ptr(n_d), U, K, L, w, 0.0, 0.0,
           H.ptr(lm_score), H.ptr(total), H.ptr(order), H.stream_ptr())
    torch.cuda.synchronize()
    total, order = total.cpu().numpy(), order.cpu().numpy()
    assert np.array_equal(order, order_n)
    for got, want in zip(total.ravel(), total_n.ravel()):
        if want == NEG_INF:
            assert got == NEG_INF
        else:
            assert rel(float(got), float(want)) <= NBEST_SCORE_TOL, (got, want)
    print('%s: total bit for bit asr_rescore_nbest\'s: %s' % (name, np.array_equal(total.view(np.uint32), total_n.view(np.uint32))))


def _untouched(b):
    torch.cuda.synchronize()
    assert (b['lm_in'] == -7).all() and torch.isnan(b['out']).all()
    assert (b['lm_score'] == 7.0).all() and (b['total'] == 7.0).all() and (b['order'] == -7).all()


@pytest.mark.gpu
@pytest.mark.parametrize('bad', ['R', 'L', 'teacher_ld', 'sos', 'null_teacher', 'null_lm_in'])
def test_lm_input_refuses_bad_arguments_and_launches_nothing(bad):
    from src import hipabi as H
    b, d = _device_case('v31_l2_k4')
    kw = {'R': {'R': 0}, 'L': {'L': 0}, 'teacher_ld': {'Lr': d['L'] - 1}, 'sos': {'sos': -1}, 'null_teacher': {'null': 'teacher'},
          'null_lm_in': {'null': 'lm_in'}}[bad]
    assert _lm_input(b, d, **kw) == E_ARG
    assert b'asr_rescore_lm_input' in H.lib().asr_last_error()
    _untouched(b)


@pytest.mark.gpu
@pytest.mark.parametrize('bad', ['R', 'L', 'V', 'pos_stride', 'row_stride', 'target_ld', 'out_ld', 'null_logits', 'null_teacher', 'null_len',
                                 'null_out'])
def test_token_logp_refuses_bad_arguments_and_launches_nothing(bad):
    from src import hipabi as H
    b, d = _device_case('v31_l2_k4')
    kw = {'R': {'rows': 0}, 'L': {'L': 0}, 'V': {'V': 1}, 'pos_stride': {'ps': d['V'] - 1}, 'row_stride': {'rs': d['V'] - 1},
          'target_ld': {'Lr': d['L'] - 1}, 'out_ld': {'out_ld': d['L'] - 1}, 'null_logits': {'null': 'logits'}, 'null_teacher': {'null': 'teacher'},
          'null_len': {'null': 'len'}, 'null_out': {'null': 'out'}}[bad]
    assert _token_logp(b, d, **kw) == E_ARG
    assert b'asr_rescore_token_logp' in H.lib().asr_last_error()
    _untouched(b)


@pytest.mark.gpu
@pytest.mark.parametrize('bad', ['U', 'K0', 'K', 'L', 'tok_ld', 'lm_weight', 'null_att', 'null_ctc', 'null_out', 'null_len', 'null_n',
                                 'null_lm_score', 'null_total', 'null_order'])
def test_rank_lm_refuses_bad_arguments_and_launches_nothing(bad):
    from src import hipabi as H
    b, d = _device_case('v31_l2_k4')
    kw = {'U': {'U': 0}, 'K0': {'K': 0}, 'K': {'K': H.CTC_BEAM_MAX + 1}, 'L': {'L': 0}, 'tok_ld': {'out_ld': d['L'] - 1}, 'lm_weight': {'lw': -0.5}}
    kw = kw[bad] if bad in kw else {'null': bad[len('null_'):]}
    assert _rank_lm(b, d, **kw) == E_ARG
    assert b'asr_rescore_rank_lm' in H.lib().asr_last_error()
    _untouched(b)


# ---- end to end: BeamDecoder(rescore=True, lm_rescore=True) on the seeded joint model and LMs -------------------------------------
# The models' and LMs' seeds are those of the imported tests; LM weight and length bonus were chosen on the oracle's float64 scores
# alone so that, for both LMs, every adjacent pair of totals is more than 3 x its bound apart and the LM term changes an order
# (at 0.5 / 0.25 one pair of the LSTM LM is 0.75 x its bound apart)
E2E_LM_WEIGHT, E2E_LEN_BONUS = 0.3, 0.5
_E2E = {}


def _decoder(model, lm, **kw):
    from src.decode import BeamDecoder
    kw.setdefault('lm_rescore', True)
    bd = BeamDecoder(model, None, E2E_BEAM, 0.0, 1.0, ctc_weight=E2E_W, rescore=True, len_bonus=E2E_LEN_BONUS, **kw)
    bd.set_lm(lm, E2E_LM_WEIGHT)
    return bd


def _e2e(module, prec):
    """Model, LM, the decoder's result and the oracle's, computed once per (LM module, precision) and left unchanged."""
    if (module, prec) in _E2E:
        return _E2E[(module, prec)]
    model, cfg, sd, feat, lens = _joint_model('shipped', prec)
    lm, lm_sd = _seeded_lm(module)
    lm = lm.cuda().eval()
    bd = _decoder(model, lm)
    enc, enc_len, first = _first_pass(bd, feat, lens)                                  # the float64 search, no LM
    hyps = [[h for h, _ in f] for f in first]
    ctc = [[np.float32(s) for _, s in f] for f in first]
    att_ref = oracle_second_pass(cfg, sd, enc, enc_len, hyps, ctc, ctc, E2E_W)
    lm64 = _restated_lm(module, lm_sd, torch.float64)
    ref = []
    for u in range(len(hyps)):
        att64, _, _, tgt_len = att_ref[u]
        K, L = len(hyps[u]), max(1, max(len(h) for h in hyps[u]))
        tl = np.zeros((K, L))
        for i, h in enumerate(hyps[u]):
            tl[i, :len(h)] = [lm64(h[:j])[h[j]] for j in range(len(h))]
        n_tok = np.array([len(h) for h in hyps[u]])
        lm_s, total, order = rank_lm(att64, np.array(ctc[u], dtype=np.float64), tl, n_tok, K, L, E2E_W, E2E_LM_WEIGHT, E2E_LEN_BONUS)
        ref.append({'att': att64, 'lm': lm_s, 'total': total, 'order': order, 'tgt_len': tgt_len, 'n_tok': n_tok})
    phases = []
    bd.phase_hook = phases.append
    got = bd(feat, lens)
    bd.phase_hook = None
    _E2E[(module, prec)] = dict(model=model, lm=lm, lm_sd=lm_sd, feat=feat, lens=lens, bd=bd, first=first, ref=ref, got=got, phases=phases)
    return _E2E[(module, prec)]


def _check(got, first, ref, logit_tol, strict_order):
    """One utterance's result against its first pass [(tokens, score)] and the oracle."""
    K = len(first)
    assert sorted(h.outIndex for h in got) == sorted(h for h, _ in first) and len(got) == K         # the n-best set is the first pass's
    slot = {tuple(h): i for i, (h, _) in enumerate(first)}
    got_order = [slot[tuple(h.outIndex)] for h in got]
    b_att = {i: 2 * logit_tol * int(ref['tgt_len'][i]) for i in range(K)}
    b_lm = {i: 2 * logit_tol * int(ref['n_tok'][i]) for i in range(K)}
    bound = {i: b_att[i] + b_lm[i] for i in range(K)}
    for h, i in zip(got, got_order):
        assert h.output_seq == first[i][0]
        print('slot %d: att %.5f (oracle %.5f, bound %.2g) lm %.5f (oracle %.5f, bound %.2g) total %.5f (oracle %.5f) ctc %.5f'
              % (i, h.att_score, ref['att'][i], b_att[i], h.lm_score, ref['lm'][i], b_lm[i], h.score, ref['total'][i], h.ctc_score))
        assert abs(h.att_score - ref['att'][i]) <= b_att[i], (i, h.att_score, ref['att'][i])
        assert abs(h.lm_score - ref['lm'][i]) <= b_lm[i], (i, h.lm_score, ref['lm'][i])
        assert abs(h.score - ref['total'][i]) <= bound[i] + CTC_SCORE_TOL * max(1.0, abs(first[i][1]) / 20), (i, h.score, ref['total'][i])
        assert abs(h.ctc_score - first[i][1]) <= CTC_SCORE_TOL * max(1.0, abs(first[i][1]) / 20)
        assert h.avgScore() == h.score
    assert [h.score for h in got] == sorted((h.score for h in got), reverse=True)
    ranked = [i for i in ref['order'] if i < K]
    gaps = [float(ref['total'][a] - ref['total'][b]) for a, b in zip(ranked, ranked[1:])]
    need = [2 * max(bound[a], bound[b]) for a, b in zip(ranked, ranked[1:])]
    if strict_order:
        assert all(g > n for g, n in zip(gaps, need)), 'the seeded model and LM do not hold the second pass\'s gaps %s (needed %s): choose ' \
                                                       'another seed, LM weight or length bonus' % (gaps, need)
        assert got_order == ranked
    else:                                                       # only across the pairs the oracle separates clearly
        pos = {i: r for r, i in enumerate(got_order)}
        for r, a in enumerate(ranked):
            for c in ranked[r + 1:]:
                if float(ref['total'][a] - ref['total'][c]) > 2 * max(bound[a], bound[c]):
                    assert pos[a] < pos[c], (a, c)
    return got_order


def _same(a, b, tol_of):
    assert [h.outIndex for h in a] == [h.outIndex for h in b]
    same_bits = True
    for x, y in zip(a, b):
        for f in ('att_score', 'lm_score', 'score'):
            assert abs(getattr(x, f) - getattr(y, f)) <= tol_of(x), (f, getattr(x, f), getattr(y, f))
            same_bits = same_bits and getattr(x, f) == getattr(y, f)
        assert x.ctc_score == y.ctc_score
    return same_bits


@pytest.mark.gpu
@pytest.mark.parametrize('module', ['LSTM', 'GRU'])
def test_lm_rescore_on_a_joint_model_fp32(module):
    e = _e2e(module, 'fp32')
    assert len(e['got']) == len(E2E_LENS)
    changed = False
    for u in range(len(E2E_LENS)):
        order = _check(e['got'][u], e['first'][u], e['ref'][u], FP32_LOGIT_TOL, True)
        no_lm = rank_lm(e['ref'][u]['att'], np.array([s for _, s in e['first'][u]]), np.zeros((len(order), 1)), np.zeros(len(order), dtype=int),
                        len(order), 1, E2E_W, 0.0, 0.0)[2]
        changed = changed or order != no_lm
    assert changed, 'the LM term changes no order: the ranking check proves nothing about it; choose another LM weight'
    assert e['phases'] == ['encoder', 'first_pass', 'decoder_pass', 'lm_pass', 'rescore_launch', 'read_back']
    msg = e['bd'].create_msg()
    assert any('LM scores the n-best list in the second pass' in l and 'weight = %.2f' % E2E_LM_WEIGHT in l and 'length bonus = %.2f' % E2E_LEN_BONUS in l
               for l in msg)


@pytest.mark.gpu
@pytest.mark.parametrize('module', ['LSTM', 'GRU'])
def test_lm_rescore_on_a_joint_model_bf16(module):
    e = _e2e(module, 'bf16')
    for u in range(len(E2E_LENS)):
        _check(e['got'][u], e['first'][u], e['ref'][u], BF16_LOGIT_TOL, False)


@pytest.mark.gpu
@pytest.mark.parametrize('module', ['LSTM', 'GRU'])
def test_both_placements_of_the_lm_score_a_shared_hypothesis_alike(module):
    """The same input decoded with the LM in the first pass: for every hypothesis in both lists lm_weight * lm_score + len_bonus * n
    is that pass's score - ctc_score, within the tolerance of the carry-over test of tests/test_hip_rescore.py."""
    e = _e2e(module, 'fp32')
    first_bd = _decoder(e['model'], e['lm'], lm_rescore=False)
    with torch.no_grad():
        _, _, tlen, ctc_lp = first_bd._encode(e['feat'], e['lens'])
        fused = first_bd._read_ctc(first_bd._search_ctc_lm(ctc_lp, tlen))
    shared = 0
    for u in range(len(E2E_LENS)):
        want = {tuple(h.outIndex): h for h in fused[u]}
        for h in e['got'][u]:
            f = want.get(tuple(h.outIndex))
            if f is None:
                continue
            shared += 1
            mine, theirs = E2E_LM_WEIGHT * h.lm_score + E2E_LEN_BONUS * len(h.outIndex), f.score - f.ctc_score
            tol = NBEST_SCORE_TOL * max(1.0, abs(h.score) / 20, abs(h.att_score) / 20)
            print('utt %d %s: LM part in the second pass %.6f, in the first %.6f (tolerance %.3g)' % (u, h.outIndex, mine, theirs, tol))
            assert abs(mine - theirs) <= tol
    assert shared >= 1


@pytest.mark.gpu
def test_lm_rescore_batches_chunks_and_encoder_passes_agree():
    e = _e2e('LSTM', 'fp32')
    bd, model, lm, feat, lens, got = e['bd'], e['model'], e['lm'], e['feat'], e['lens'], e['got']
    tol = lambda h: 2 * 2 * FP32_LOGIT_TOL * (2 * len(h.outIndex) + 1)
    # U = 3 in one call equals three U = 1 calls
    for u, l in enumerate(E2E_LENS):
        one = bd(feat[u:u + 1, :l], lens[u:u + 1])
        assert isinstance(one[0], type(got[0][0]))
        print('utt %d alone: bit for bit %s' % (u, _same(one, got[u], tol)))
        _check(one, e['first'][u], e['ref'][u], FP32_LOGIT_TOL, True)
    # chunks of 3 rows cut the 12 hypothesis rows inside the utterances, in the LM pass and in the decoder pass
    for kw in ({'lm_rescore_rows': 3}, {'rescore_rows': 3}, {'lm_rescore_rows': 3, 'rescore_rows': 3}):
        got3 = _decoder(model, lm, **kw)(feat, lens)
        for u in range(3):
            print('%s utt %d: bit for bit %s' % (kw, u, _same(got3[u], got[u], tol)))
            _check(got3[u], e['first'][u], e['ref'][u], FP32_LOGIT_TOL, True)
    # the batched encoder pass agrees to rounding: the same n-best set
    got_b = _decoder(model, lm, batch_encode=True)(feat, lens)
    for u in range(3):
        assert sorted(h.outIndex for h in got_b[u]) == sorted(h.outIndex for h in got[u])
        assert all(h.lm_score is not None for h in got_b[u])


@pytest.mark.gpu
@pytest.mark.parametrize('module', ['LSTM', 'GRU'])
def test_the_lm_steps_alike_before_and_after_a_rescoring_call(module):
    """lm.forward flattens the LM's parameters on first use; step() must not notice."""
    model, cfg, sd, feat, lens = _joint_model('shipped', 'fp32')
    lm = _seeded_lm(module)[0].cuda().eval()
    lm.prec = model.prec
    assert '_layers' not in lm.__dict__                                               # not flattened yet

    def steps():
        state, out = lm.init_state(5, feat.device), []
        for toks in ([0, 0, 0, 0, 0], [2, 7, 30, 1, 4], [9, 9, 3, 2, 30]):
            lp, state = lm.step(torch.tensor(toks, dtype=torch.int64, device=feat.device), state)
            out.append(lp.clone())
        return torch.stack(out).cpu()
    before = steps()
    got = _decoder(model, lm)(feat, lens)
    assert '_layers' in lm.__dict__ and not lm.training
    after = steps()
    assert torch.equal(before, after)
    # a training-mode LM is put back into training mode
    lm.train()
    _decoder(model, lm)(feat[:1, :E2E_LENS[0]], lens[:1])
    assert lm.training


@pytest.mark.gpu
def test_lm_rescore_refusals():
    import yaml
    from src.decode import BeamDecoder
    e = _e2e('LSTM', 'fp32')
    model, lm, feat, lens = e['model'], e['lm'], e['feat'], e['lens']
    args = (model, None, E2E_BEAM, 0.0, 1.0)
    with pytest.raises(ValueError, match='rescore=True'):
        BeamDecoder(*args, ctc_weight=E2E_W, lm_rescore=True)
    with pytest.raises(ValueError, match='lm_rescore_rows'):
        BeamDecoder(*args, ctc_weight=E2E_W, rescore=True, lm_rescore=True, lm_rescore_rows=0)
    launched = []
    bd = BeamDecoder(*args, ctc_weight=E2E_W, rescore=True, lm_rescore=True)
    bd.phase_hook = launched.append
    with pytest.raises(ValueError, match='needs an LM'):                              # no LM by the time forward is called
        bd(feat, lens)
    bd.set_lm(lm, 0.0)
    with pytest.raises(ValueError, match='lm_weight'):
        bd(feat, lens)
    assert launched == []                                                             # refused before the encoder ran

    class StepOnly(object):                                                           # the first-pass interface alone
        def init_state(self, n, device): return None
        def step(self, tokens, state): return None, None
        def gather_state(self, state, index): return None
    with pytest.raises(ValueError, match='full-sequence forward'):
        bd.set_lm(StepOnly(), 0.5)
    with pytest.raises(ValueError, match='full-sequence forward'):
        bd.set_lm(torch.nn.Module(), 0.5)
    bd = BeamDecoder(*args, ctc_weight=E2E_W, rescore=True, lm_rescore=True)
    bd.phase_hook = launched.append
    bd.apply_lm, bd.lm_w, bd.lm = True, 0.5, StepOnly()                               # slipped past set_lm: forward refuses it too
    with pytest.raises(ValueError, match='full-sequence forward'):
        bd(feat, lens)
    assert launched == []
    # the decode block of a config reaches the constructor as keywords
    block = yaml.safe_load('beam_size: 4\nmin_len_ratio: 0.0\nmax_len_ratio: 1.0\nctc_weight: 0.5\nrescore: true\nlm_rescore: true\nlm_rescore_rows: 8\n')
    bd = BeamDecoder(model, None, **block)
    assert bd.rescore and bd.lm_rescore and bd.lm_rescore_rows == 8


@pytest.mark.gpu
def test_without_lm_rescore_the_lm_stays_in_the_first_pass():
    e = _e2e('LSTM', 'fp32')
    bd = _decoder(e['model'], e['lm'], lm_rescore=False)
    phases = []
    bd.phase_hook = phases.append
    got = bd(e['feat'], e['lens'])
    assert bd.launches > 1                                                            # the resumable search with the LM ran
    assert 'lm_pass' not in phases and all(h.lm_score is None for hs in got for h in hs)
    assert any('shallow fusion in the first pass' in l for l in bd.create_msg())
    # and with lm_rescore the first pass is the one-launch search, whatever the LM weight: nothing counts launches
    e['bd'].launches = -1
    e['bd'](e['feat'][:1, :E2E_LENS[0]], e['lens'][:1])
    assert e['bd'].launches == -1
