"""asr_ctc_beam_search (csrc/ctc_decode.hip) and BeamDecoder on a CTC-only model against the float64 restatement of
tests/test_ctc_beam_reference.py.

Inputs are log_softmax(scale * randn) from committed seeds.  The seeds were searched on the CPU with the restatement alone
(`_case_ok`): at every frame of every case the K-th kept entry is more than 1e-3 ahead of the best rejected one, the
`cand`-th token more than 1e-3 ahead of the next, and adjacent final hypotheses more than 1e-3 apart, so fp32 rounding
cannot change a decision and the sequences must match EXACTLY, in rank order, with equal counts.
test_committed_seeds_hold_the_gaps re-checks that without a GPU.

Score tolerance: the restatement transcribed to fp32 numpy (prefix_beam_search(dtype=np.float32)) deviates from float64 by
at most FP32_DEV = 3.63e-6 over all cases below; the kernel is allowed SCORE_TOL = 4 x FP32_DEV = 1.45e-5 (the factor
covers the different order of the sums across lanes and the device's exp/log)."""
import numpy as np
import pytest
import torch

from test_ctc_beam_reference import NEG_INF, peaked_logp, prefix_beam_search

GAP = 1e-3
FP32_DEV = 3.632158041000366e-06          # largest |fp32 transcription - float64| over every hypothesis of every case (ragged_u3, T' = 37)
SCORE_TOL = 4 * FP32_DEV
E_ARG = -1

# name -> K, cand, V, scale, [(seed, T) per utterance]
CASES = {
    'one_frame': (4, 0, 31, 3.0, [(0, 1)]),
    'repeat_two_frames': (4, 0, 5, 2.0, [(2, 2)]),
    'v3_k8': (8, 0, 3, 2.0, [(0, 6)]),
    'v31_k1_one_hot': (1, 0, 31, 60.0, [(24, 20)]),
    'v31_k4': (4, 0, 31, 3.0, [(0, 24)]),
    'v31_k16': (16, 0, 31, 3.0, [(0, 24)]),
    'v31_k8_cand12': (8, 12, 31, 3.0, [(0, 24)]),
    'v300_k8_cand12': (8, 12, 300, 3.0, [(2, 16)]),
    'v300_k8_all': (8, 0, 300, 3.0, [(0, 12)]),
    'ragged_u3': (8, 12, 31, 3.0, [(0, 1), (0, 37), (3, 64)]),
    'no_frames': (4, 0, 31, 3.0, [(0, 0)]),
    'minus_inf': (8, 0, 31, 3.0, [(0, 16)]),
}


def case_inputs(name, seeds=None):
    K, cand, V, scale, utts = CASES[name]
    lps = []
    for n, (seed, T) in enumerate(utts):
        seed = seed if seeds is None else seeds[n]
        lp = peaked_logp(1000 * seed + T, T, V, scale)
        if name == 'minus_inf' and T:
            # a fifth of the entries impossible, the blank of every fourth frame among them; the frame's best token stays
            hole = np.random.RandomState(seed + 77).rand(T, V) < 0.2
            hole[::4, 0] = True
            hole[np.arange(T), lp.argmax(axis=1)] = False
            lp = np.where(hole, np.float32(NEG_INF), lp)
        lps.append(lp)
    return K, cand, V, lps


_REF = {}


def reference(name):
    """float64 restatement of a case, computed once: per utterance (hyps, gaps)."""
    if name not in _REF:
        K, cand, V, lps = case_inputs(name)
        _REF[name] = [prefix_beam_search(lp.astype(np.float64), K, cand) for lp in lps]
    return _REF[name]


def best_path(lp):
    path = lp.argmax(axis=1).tolist()
    return [c for c, prev in zip(path, [None] + path[:-1]) if c != 0 and c != prev]


def _case_ok(name, seeds=None):
    """The conditions the seed search asked of a case, on the reference alone."""
    K, cand, V, lps = case_inputs(name, seeds)
    for lp in lps:
        hyps, gaps = prefix_beam_search(lp.astype(np.float64), K, cand)
        if min(gaps.values()) <= GAP:
            return False
        if name == 'repeat_two_frames' and not (lp[0].argmax() == lp[1].argmax() != 0 and hyps[0][0] == [int(lp[0].argmax())]):
            return False
        if name == 'v31_k1_one_hot' and not (hyps[0][0] == best_path(lp) and np.exp(lp.max(axis=1)).min() > 0.99):
            return False
        if name == 'v3_k8' and len(hyps) != 8:
            return False
    return True


@pytest.mark.parametrize('name', sorted(CASES))
def test_committed_seeds_hold_the_gaps(name):
    assert _case_ok(name)
    K, cand, V, lps = case_inputs(name)
    for lp, (hyps, _) in zip(lps, reference(name)):
        h32, _ = prefix_beam_search(lp, K, cand, dtype=np.float32)
        assert [h for h, _ in h32] == [h for h, _ in hyps]
        dev = max(abs(a[1] - b[1]) for a, b in zip(h32, hyps))
        print('%s: fp32 transcription deviates by %.3g' % (name, dev))
        assert dev <= FP32_DEV


def run_kernel(lps, K, cand, V):
    """One launch for the utterances in `lps`; frames past each length and the outputs are pre-filled with garbage."""
    from src import hipabi as H
    dev = torch.device('cuda')
    U, Tmax = len(lps), max(1, max(lp.shape[0] for lp in lps))
    if max(lp.shape[0] for lp in lps) == 0:
        Tmax = 4
    host = np.full((U, Tmax, V), np.nan, dtype=np.float32)
    for u, lp in enumerate(lps):
        host[u, :lp.shape[0]] = lp
    logp = torch.from_numpy(host).to(dev)
    tlen = torch.tensor([lp.shape[0] for lp in lps], dtype=torch.int32, device=dev)
    toks = torch.full((U, K, Tmax), -7, dtype=torch.int32, device=dev)
    lens = torch.full((U, K), -7, dtype=torch.int32, device=dev)
    score = torch.full((U, K), 7.0, dtype=torch.float32, device=dev)
    n = torch.full((U,), -7, dtype=torch.int32, device=dev)
    nbytes = int(H.lib().asr_ctc_beam_search_workspace_bytes(U, Tmax, min(K, H.CTC_BEAM_MAX)))
    ws = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device=dev)
    rc = H.lib().asr_ctc_beam_search(H.ptr(logp), H.ptr(tlen), U, Tmax, V, K, cand, Tmax, H.ptr(toks), H.ptr(lens), H.ptr(score), H.ptr(n),
                                     H.ptr(ws), nbytes, H.stream_ptr())
    torch.cuda.synchronize()
    return rc, toks.cpu().numpy(), lens.cpu().numpy(), score.cpu().numpy(), n.cpu().numpy()


def check_against(ref_hyps, toks, lens, score, n, u, K):
    assert int(n[u]) == len(ref_hyps)
    assert not np.isnan(score[u]).any()
    for i, (want, want_score) in enumerate(ref_hyps):
        got = toks[u, i, :lens[u, i]].tolist()
        assert got == want, (u, i, got, want)
        err = abs(float(score[u, i]) - want_score)
        print('utt %d rank %d: score %.6f (float64 %.6f) |diff| %.3g' % (u, i, score[u, i], want_score, err))
        assert err <= SCORE_TOL, (u, i, float(score[u, i]), want_score)
        assert (toks[u, i, lens[u, i]:] == 0).all()
    for i in range(len(ref_hyps), K):                 # unused rows: empty, never a hypothesis
        assert lens[u, i] == 0 and score[u, i] == NEG_INF


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_kernel_equals_float64_restatement(name):
    K, cand, V, lps = case_inputs(name)
    rc, toks, lens, score, n = run_kernel(lps, K, cand, V)
    assert rc == 0
    for u, (hyps, _) in enumerate(reference(name)):
        check_against(hyps, toks, lens, score, n, u, K)
    if name == 'v31_k1_one_hot':
        assert toks[0, 0, :lens[0, 0]].tolist() == best_path(lps[0])
    if name == 'no_frames':
        assert int(n[0]) == 1 and lens[0, 0] == 0 and score[0, 0] == 0.0


@pytest.mark.gpu
def test_beam_above_the_compiled_maximum_is_refused():
    from src import hipabi as H
    K, cand, V, lps = case_inputs('v31_k4')
    rc, toks, lens, score, n = run_kernel(lps, H.CTC_BEAM_MAX + 1, cand, V)
    assert rc == E_ARG
    assert b'beam' in H.lib().asr_last_error()
    assert (toks == -7).all() and (lens == -7).all() and (n == -7).all() and (score == 7.0).all()      # nothing was launched


# ---- end to end: BeamDecoder on a CTC-only model ----------------------------------------------------------------------
E2E_SEED, E2E_HEAD_SCALE, E2E_BEAM = 0, 40.0, 4
E2E_LENS = (50, 37, 44)


def _ctc_only_model():
    from src.asr import ASR
    D, V = 40, 31
    enc = {'vgg': 0, 'vgg_freq': -1, 'vgg_low_filt': -1, 'module': 'LSTM', 'bidirection': True, 'dim': [32, 32], 'dropout': [0.0, 0.0],
           'layer_norm': [False, False], 'proj': [True, True], 'sample_rate': [1, 2], 'sample_style': 'drop'}
    torch.manual_seed(E2E_SEED)
    model = ASR(D, V, 1, ctc_weight=1, encoder=enc, prec='fp32')
    sd = model.state_dict()
    g = torch.Generator().manual_seed(E2E_SEED)
    sd = {k: torch.randn(v.shape, generator=g) * (0.3 if v.dim() > 1 else 0.1) for k, v in sd.items()}
    sd['ctc_layer.0.weight'] = sd['ctc_layer.0.weight'] * E2E_HEAD_SCALE            # peaked frames: the gaps of the search must hold
    model.load_state_dict(sd)
    feat = torch.randn((len(E2E_LENS), max(E2E_LENS), D), generator=g)
    for u, l in enumerate(E2E_LENS):
        feat[u, l:] = 0
    return model.cuda().eval(), feat.cuda(), torch.tensor(E2E_LENS, dtype=torch.int64).cuda()


@pytest.mark.gpu
def test_beam_decoder_on_a_ctc_only_model():
    from src.decode import BeamDecoder
    model, feat, lens = _ctc_only_model()
    assert not model.enable_att
    bd = BeamDecoder(model, None, E2E_BEAM, 0.0, 1.0, ctc_weight=0.3)
    assert any('ignored' in line for line in bd.create_msg())
    with torch.no_grad():
        _, _, tlen, ctc_lp = bd._encode(feat, lens)            # the model's own ctc_output, read back once
    lp_host, tl = ctc_lp.cpu().numpy(), tlen.cpu().tolist()
    want = []
    for u in range(len(E2E_LENS)):
        hyps, gaps = prefix_beam_search(lp_host[u, :tl[u]].astype(np.float64), E2E_BEAM, bd.ctc_cand)
        print('utt %d: T\' = %d gaps %s best %s' % (u, tl[u], gaps, hyps[0]))
        assert min(gaps.values()) > GAP, 'the seeded model does not hold the gaps: choose another E2E_SEED / E2E_HEAD_SCALE'
        want.append(hyps)
    got3 = bd(feat, lens)
    assert len(got3) == 3
    for u in range(3):
        assert [h.outIndex for h in got3[u]] == [h for h, _ in want[u]]
        assert got3[u][0].output_seq == want[u][0][0]
        for h, (_, s) in zip(got3[u], want[u]):
            assert abs(h.avgScore() - s) <= SCORE_TOL * max(1.0, abs(s) / 20)
    got1 = bd(feat[:1, :E2E_LENS[0]], lens[:1])
    assert [h.outIndex for h in got1] == [h for h, _ in want[0]]
    with pytest.raises(NotImplementedError, match='RNN-LM fusion for CTC-only decoding is not built'):
        BeamDecoder(model, None, E2E_BEAM, 0.0, 1.0, lm_weight=0.5)
