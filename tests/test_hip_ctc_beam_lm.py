"""The resumable CTC prefix beam search with RNN-LM shallow fusion (asr_ctc_beam_lm_init / _advance / _readout,
csrc/ctc_decode.hip), asr_masked_copy_rows and BeamDecoder with an LM on a CTC-only model, against the float64 restatement
of tests/test_ctc_beam_lm_reference.py.

Kernel cases: CTC inputs are log_softmax(scale * randn) from committed seeds, the LM is a seeded table (`TableLM`: the state is
the last two tokens; a (V,V,V) log_softmax table for V <= 31, a bigram table at V = 300), rounded to the fp32 the device reads.
The seeds were searched on the CPU with the restatement alone (`_case_ok`): every `keep`, `cand` and `final` gap of every
utterance is above GAP = 1e-3, so fp32 rounding cannot change a decision and sequences, order and counts must match EXACTLY.
test_committed_seeds_hold_the_gaps re-checks that without a GPU, and that the table has a merge, a returning prefix, a case
where the LM changes the winner and one with a length bonus.

Score tolerance: the restatement transcribed to fp32 numpy deviates from float64 by at most FP32_DEV_LM over all cases (fused
and CTC scores); the kernel is allowed SCORE_TOL_LM = 4 x FP32_DEV_LM (the factor covers the different order of the sums across
lanes, the fused multiply-add of the LM term and the device's exp/log: the convention of tests/test_hip_ctc_beam.py).

End to end: the seeded CTC-only model of tests/test_hip_ctc_beam.py and a seeded RNNLM; the reference LM is a float64
torch.nn.LSTM / GRU with the same weights.  E2E_FP32_DEV is measured the same way (fp32 CPU LM and fp32 search against float64
on the model's read-back ctc_output; the largest value over the two LMs and three utterances), the decoder is allowed 4 x it."""
import numpy as np
import pytest
import torch

from test_ctc_beam_reference import NEG_INF, peaked_logp, prefix_beam_search
from test_ctc_beam_lm_reference import prefix_beam_search_lm

GAP = 1e-3
FP32_DEV_LM = 1.5165540702355429e-05      # largest |fp32 transcription - float64| over every hypothesis of every case (ragged_u3, T' = 37)
SCORE_TOL_LM = 4 * FP32_DEV_LM
E_ARG = -1

# name -> K, cand, V, scale, lm_weight, len_bonus, lm seed, [(seed, T) per utterance]
CASES = {
    'one_frame': (4, 0, 31, 3.0, 0.5, 0.0, 0, [(0, 1)]),
    'repeat_two_frames': (4, 0, 5, 2.0, 0.5, 0.0, 0, [(2, 2)]),
    'v3_k8': (8, 0, 3, 2.0, 0.5, 0.0, 0, [(0, 6)]),
    'v31_k1': (1, 0, 31, 3.0, 0.5, 0.0, 0, [(0, 20)]),
    'v31_k4': (4, 0, 31, 3.0, 0.5, 0.0, 0, [(0, 24)]),
    'v31_k4_runs': (4, 0, 31, 12.0, 0.5, 0.0, 0, [(0, 24)]),          # every frame three times: frames of stays only, launches run ahead
    'v31_k16': (16, 0, 31, 3.0, 0.5, 0.0, 0, [(0, 24)]),
    'v31_k8_cand12': (8, 12, 31, 3.0, 0.5, 0.3, 0, [(0, 24)]),
    'v300_k8_cand12': (8, 12, 300, 3.0, 0.5, 0.0, 0, [(0, 16)]),
    'ragged_u3': (8, 12, 31, 3.0, 0.5, 0.0, 0, [(0, 1), (0, 37), (0, 64)]),
    'no_frames': (4, 0, 31, 3.0, 0.5, 0.0, 0, [(0, 0)]),
    'minus_inf': (8, 0, 31, 3.0, 0.5, -0.2, 0, [(0, 16)]),
}


def lm_table(seed, V):
    """Seeded log_softmax table rounded to fp32: (V,V,V) - row [a, b] = distribution after the tokens a, b - for V <= 31, a
    bigram table (V,V) above."""
    shape = (V, V, V) if V <= 31 else (V, V)
    x = 2.0 * np.random.RandomState(4000 + seed).randn(*shape)
    x = x - x.max(axis=-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)


def table_fn(table, dtype=np.float64):
    """The table as the restatement's `lm`: prefix -> (V,) log-probs, <sos> = 0 in front."""
    tab = table.astype(dtype)
    if tab.ndim == 2:
        return lambda pre: tab[pre[-1] if pre else 0]
    return lambda pre: tab[((0, 0) + tuple(pre))[-2], ((0, 0) + tuple(pre))[-1]]


class TableLM(object):
    """The table behind RNNLM's decoding interface (init_state, step, gather_state); the state is the last two tokens, one
    fp32 (1, n, 2) tensor as a GRU's."""

    def __init__(self, table, device):
        self.table = torch.from_numpy(table).to(device)
        self.vocab_size = table.shape[-1]

    def init_state(self, n, device):
        return torch.zeros((1, n, 2), dtype=torch.float32, device=device)

    def gather_state(self, state, index):
        return state[:, index].contiguous()

    def step(self, tokens, state):
        prev = state[0, :, 1].long()
        tok = tokens.long()
        lp = self.table[tok] if self.table.dim() == 2 else self.table[prev, tok]
        new = torch.stack([prev.float(), tok.float()], dim=1).unsqueeze(0).contiguous()
        return lp.contiguous(), new


def case_inputs(name, seeds=None, lm_seed=None):
    K, cand, V, scale, w, bonus, lseed, utts = CASES[name]
    lps = []
    for n, (seed, T) in enumerate(utts):
        seed = seed if seeds is None else seeds[n]
        lp = peaked_logp(1000 * seed + T, T, V, scale)
        if name == 'v31_k4_runs':
            lp = np.repeat(lp[:T // 3], 3, axis=0)
        if name == 'minus_inf' and T:
            # a fifth of the entries impossible, the blank of every fourth frame among them; the frame's best token stays
            hole = np.random.RandomState(seed + 77).rand(T, V) < 0.2
            hole[::4, 0] = True
            hole[np.arange(T), lp.argmax(axis=1)] = False
            lp = np.where(hole, np.float32(NEG_INF), lp)
        lps.append(lp)
    return K, cand, V, w, bonus, lm_table(lseed if lm_seed is None else lm_seed, V), lps


_REF = {}


def reference(name):
    """float64 restatement of a case, computed once: per utterance (hyps, gaps, info)."""
    if name not in _REF:
        K, cand, V, w, bonus, table, lps = case_inputs(name)
        _REF[name] = [prefix_beam_search_lm(lp.astype(np.float64), K, cand, table_fn(table), w, bonus) for lp in lps]
    return _REF[name]


def _case_ok(name, seeds=None, lm_seed=None):
    """The conditions the seed search asked of a case, on the reference alone."""
    K, cand, V, w, bonus, table, lps = case_inputs(name, seeds, lm_seed)
    for lp in lps:
        hyps, gaps, _ = prefix_beam_search_lm(lp.astype(np.float64), K, cand, table_fn(table), w, bonus)
        if min(gaps.values()) <= GAP:
            return False
        if name == 'repeat_two_frames' and not lp[0].argmax() == lp[1].argmax() != 0:
            return False
        if name == 'v3_k8' and len(hyps) != 8:
            return False
    return True


def _lm_changes_the_winner(name):
    K, cand, V, w, bonus, table, lps = case_inputs(name)
    return any(prefix_beam_search(lp.astype(np.float64), K, cand)[0][0][0] != ref[0][0][0] for lp, ref in zip(lps, reference(name)))


def test_committed_seeds_hold_the_gaps():
    worst, merges, returns = 0.0, 0, 0
    for name in sorted(CASES):
        assert _case_ok(name), name
        K, cand, V, w, bonus, table, lps = case_inputs(name)
        for lp, (hyps, _, info) in zip(lps, reference(name)):
            h32, _, i32 = prefix_beam_search_lm(lp, K, cand, table_fn(table, np.float32), w, bonus, dtype=np.float32)
            assert [h[0] for h in h32] == [h[0] for h in hyps], name
            assert i32['stops'] == info['stops'], name
            dev = max([max(abs(a[1] - b[1]), abs(a[2] - b[2])) for a, b in zip(h32, hyps)] + [0.0])
            print('%s: fp32 transcription deviates by %.4g; stops %s merges %d returns %d' % (name, dev, info['stops'], info['merges'],
                                                                                              info['returns']))
            worst = max(worst, dev)
            merges += info['merges']
            returns += info['returns']
    print('FP32_DEV_LM measured: %r' % worst)
    assert worst <= FP32_DEV_LM
    assert merges > 0 and returns > 0
    assert any(_lm_changes_the_winner(name) for name in CASES)
    assert any(CASES[name][5] != 0 for name in CASES)


# ---- the kernels -----------------------------------------------------------------------------------------------------------
def run_search(lps, K, cand, V, table, w, bonus, max_frames=0, lm_null=False, short_ws=False):
    """init, advance until every utterance is done (the glue in torch), readout.  Frames past each length are NaN; outputs
    and workspace are pre-filled with garbage.  Returns (rc, outputs dict, frames per launch, done per launch)."""
    from src import hipabi as H
    dev = torch.device('cuda')
    L, st = H.lib(), H.stream_ptr()
    U, Tmax = len(lps), max(1, max(lp.shape[0] for lp in lps))
    if max(lp.shape[0] for lp in lps) == 0:
        Tmax = 4
    host = np.full((U, Tmax, V), np.nan, dtype=np.float32)
    for u, lp in enumerate(lps):
        host[u, :lp.shape[0]] = lp
    logp = torch.from_numpy(host).to(dev)
    tlen = torch.tensor([lp.shape[0] for lp in lps], dtype=torch.int32, device=dev)
    R = U * K
    g32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)
    toks, lens, n = g32(U, K, Tmax), g32(U, K), g32(U)
    score, ctc = torch.full((U, K), 7.0, device=dev), torch.full((U, K), 7.0, device=dev)
    src_row, step_tok = torch.full((R,), -7, dtype=torch.int64, device=dev), torch.full((R,), -7, dtype=torch.int64, device=dev)
    need, frame, done = g32(R), g32(U), g32(U)
    nbytes = int(L.asr_ctc_beam_lm_workspace_bytes(U, Tmax, min(K, H.CTC_BEAM_MAX)))
    ws = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device=dev)
    if short_ws:
        nbytes -= 4
    lm = TableLM(table, dev)
    lm_lp, state = lm.step(torch.zeros(R, dtype=torch.int64, device=dev), lm.init_state(R, dev))
    out = lambda: {'toks': toks.cpu().numpy(), 'lens': lens.cpu().numpy(), 'score': score.cpu().numpy(), 'ctc': ctc.cpu().numpy(),
                   'n': n.cpu().numpy(), 'need': need.cpu().numpy(), 'frame': frame.cpu().numpy(), 'done': done.cpu().numpy(),
                   'src_row': src_row.cpu().numpy(), 'ws': ws.cpu().numpy()}
    rc = L.asr_ctc_beam_lm_init(U, Tmax, K, H.ptr(ws), nbytes, st)
    if rc != 0:
        torch.cuda.synchronize()
        return rc, out(), [], []
    frames, dones = [], []
    for it in range(Tmax):
        rc = L.asr_ctc_beam_lm_advance(H.ptr(logp), H.ptr(tlen), None if lm_null else H.ptr(lm_lp), U, Tmax, V, K, cand, w, bonus, max_frames,
                                       H.ptr(src_row), H.ptr(step_tok), H.ptr(need), H.ptr(frame), H.ptr(done), H.ptr(ws), nbytes, st)
        if rc != 0:
            torch.cuda.synchronize()
            return rc, out(), frames, dones
        frames.append(frame.cpu().tolist())
        dones.append(done.cpu().tolist())
        assert ((src_row >= 0) & (src_row < R)).all() and ((step_tok >= 0) & (step_tok < V)).all()
        state_g, lp_g = lm.gather_state(state, src_row), lm_lp[src_row]
        lp_n, state_n = lm.step(step_tok, state_g)
        m = need.bool()
        lm_lp = torch.where(m[:, None], lp_n, lp_g).contiguous()
        state = torch.where(m[None, :, None], state_n, state_g).contiguous()
        if all(dones[-1]):
            break
    rc = L.asr_ctc_beam_lm_readout(U, Tmax, K, Tmax, H.ptr(toks), H.ptr(lens), H.ptr(score), H.ptr(ctc), H.ptr(n), H.ptr(ws), nbytes, st)
    torch.cuda.synchronize()
    return rc, out(), frames, dones


def check_against(ref_hyps, o, u, K):
    toks, lens, score, ctc, n = o['toks'], o['lens'], o['score'], o['ctc'], o['n']
    assert int(n[u]) == len(ref_hyps)
    assert not np.isnan(score[u]).any() and not np.isnan(ctc[u]).any()
    for i, (want, want_score, want_ctc) in enumerate(ref_hyps):
        got = toks[u, i, :lens[u, i]].tolist()
        assert got == want, (u, i, got, want)
        err, err_c = abs(float(score[u, i]) - want_score), abs(float(ctc[u, i]) - want_ctc)
        print('utt %d rank %d: fused %.6f (float64 %.6f) |diff| %.3g, ctc |diff| %.3g' % (u, i, score[u, i], want_score, err, err_c))
        assert err <= SCORE_TOL_LM and err_c <= SCORE_TOL_LM, (u, i, float(score[u, i]), want_score, float(ctc[u, i]), want_ctc)
        assert (toks[u, i, lens[u, i]:] == 0).all()
    for i in range(len(ref_hyps), K):                 # unused rows: empty, never a hypothesis
        assert lens[u, i] == 0 and score[u, i] == NEG_INF and ctc[u, i] == NEG_INF


def expected_launches(refs, tl):
    """Per launch the frame counter and done flag of every utterance: launch j stops utterance u at its j-th stop frame."""
    stops = [info['stops'] for _, _, info in refs]
    nl = max(1, max(len(s) for s in stops))
    frames = [[(s[j] if j < len(s) else t) for s, t in zip(stops, tl)] for j in range(nl)]
    dones = [[int(f == t) for f, t in zip(fr, tl)] for fr in frames]
    return frames, dones


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_search_equals_float64_restatement_and_stops_where_it_must(name):
    K, cand, V, w, bonus, table, lps = case_inputs(name)
    rc, o, frames, dones = run_search(lps, K, cand, V, table, w, bonus)
    assert rc == 0
    refs = reference(name)
    for u, (hyps, _, _) in enumerate(refs):
        check_against(hyps, o, u, K)
    # the stop rule, launch by launch
    want_frames, want_dones = expected_launches(refs, [lp.shape[0] for lp in lps])
    print('frames per launch', frames)
    assert frames == want_frames
    assert dones == want_dones
    if name == 'no_frames':
        assert int(o['n'][0]) == 1 and o['lens'][0, 0] == 0 and o['score'][0, 0] == 0.0 and o['ctc'][0, 0] == 0.0
    # one frame per launch: the same result bit for bit
    rc1, o1, frames1, _ = run_search(lps, K, cand, V, table, w, bonus, max_frames=1)
    assert rc1 == 0
    assert all(f == [min(j + 1, lp.shape[0]) for lp in lps] for j, f in enumerate(frames1))
    for key in ('toks', 'lens', 'n'):
        assert np.array_equal(o[key], o1[key]), key
    for key in ('score', 'ctc'):
        assert np.array_equal(o[key].view(np.int32), o1[key].view(np.int32)), key


@pytest.mark.gpu
def test_without_lm_weight_it_is_asr_ctc_beam_search_bit_for_bit():
    import test_hip_ctc_beam as P
    for name in sorted(P.CASES):
        K, cand, V, lps = P.case_inputs(name)
        rc0, toks, lens, score, n = P.run_kernel(lps, K, cand, V)
        rc, o, _, _ = run_search(lps, K, cand, V, lm_table(1, V), 0.0, 0.0)
        assert rc0 == 0 and rc == 0
        assert np.array_equal(o['toks'], toks) and np.array_equal(o['lens'], lens) and np.array_equal(o['n'], n), name
        assert np.array_equal(o['score'].view(np.int32), score.view(np.int32)), name
        assert np.array_equal(o['ctc'].view(np.int32), score.view(np.int32)), name


@pytest.mark.gpu
@pytest.mark.parametrize('rows,width,src_ld,dst_ld', [(5, 7, 7, 7), (64, 31, 31, 40), (130, 300, 320, 300), (3, 1024, 1024, 1024)])
def test_masked_copy_rows(rows, width, src_ld, dst_ld):
    from src import hipabi as H
    rs = np.random.RandomState(rows)
    src, dst0 = rs.randn(rows, src_ld).astype(np.float32), rs.randn(rows, dst_ld).astype(np.float32)
    for mask in (np.zeros(rows, np.int32), np.ones(rows, np.int32), (rs.rand(rows) < 0.5).astype(np.int32) * 3):
        d = torch.from_numpy(dst0).cuda()
        s, m = torch.from_numpy(src).cuda(), torch.from_numpy(mask).cuda()
        assert H.lib().asr_masked_copy_rows(H.ptr(s), H.ptr(m), H.ptr(d), rows, width, src_ld, dst_ld, H.stream_ptr()) == 0
        torch.cuda.synchronize()
        want = dst0.copy()
        want[mask != 0, :width] = src[mask != 0, :width]
        assert np.array_equal(d.cpu().numpy().view(np.int32), want.view(np.int32))
    d = torch.from_numpy(dst0).cuda()
    assert H.lib().asr_masked_copy_rows(H.ptr(s), None, H.ptr(d), rows, width, src_ld, dst_ld, H.stream_ptr()) == E_ARG
    assert H.lib().asr_masked_copy_rows(H.ptr(s), H.ptr(m), H.ptr(d), rows, width, width - 1, dst_ld, H.stream_ptr()) == E_ARG
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.int32), dst0.view(np.int32))


@pytest.mark.gpu
def test_bad_arguments_are_refused_and_nothing_is_launched():
    from src import hipabi as H
    K, cand, V, w, bonus, table, lps = case_inputs('v31_k4')

    def untouched(o):
        assert (o['toks'] == -7).all() and (o['lens'] == -7).all() and (o['n'] == -7).all()
        assert (o['score'] == 7.0).all() and (o['ctc'] == 7.0).all()
        assert (o['need'] == -7).all() and (o['frame'] == -7).all() and (o['done'] == -7).all() and (o['src_row'] == -7).all()

    rc, o, _, _ = run_search(lps, H.CTC_BEAM_MAX + 1, cand, V, table, w, bonus)
    assert rc == E_ARG and b'beam' in H.lib().asr_last_error()
    untouched(o)
    assert (o['ws'] == 0x5a).all()
    rc, o, _, _ = run_search(lps, K, cand, V, table, w, bonus, short_ws=True)
    assert rc == E_ARG and b'workspace' in H.lib().asr_last_error()
    untouched(o)
    assert (o['ws'] == 0x5a).all()
    rc, o, frames, _ = run_search(lps, K, cand, V, table, w, bonus, lm_null=True)          # init ran, advance refused
    assert rc == E_ARG and b'null' in H.lib().asr_last_error() and frames == []
    untouched(o)
    U, Tmax = 1, lps[0].shape[0]
    nb = int(H.lib().asr_ctc_beam_lm_workspace_bytes(U, Tmax, K))
    assert nb > int(H.lib().asr_ctc_beam_search_workspace_bytes(U, Tmax, K))
    assert H.lib().asr_ctc_beam_lm_readout(U, Tmax, K, Tmax - 1, None, None, None, None, None, None, nb, H.stream_ptr()) == E_ARG


# ---- end to end: BeamDecoder with an LM on a CTC-only model -----------------------------------------------------------------
E2E_LM_WEIGHT, E2E_LEN_BONUS = 0.5, 0.0
E2E_LMS = {'LSTM': (2, 0), 'GRU': (1, 0)}            # module -> (layers, seed)
E2E_FP32_DEV = 1.2969887421832027e-05     # largest |fp32 transcription - float64|, fused and CTC scores (GRU, utterance 0; LSTM: 4.08e-06)
E2E_TOL = 4 * E2E_FP32_DEV


def _seeded_lm(module):
    from src.lm import RNNLM
    layers, seed = E2E_LMS[module]
    torch.manual_seed(100 + seed)
    lm = RNNLM(31, False, 32, module, 32, layers, 0.0)
    g = torch.Generator().manual_seed(100 + seed)
    sd = {k: torch.randn(v.shape, generator=g) * (0.6 if v.dim() > 1 else 0.1) for k, v in lm.state_dict().items()}
    lm.load_state_dict(sd)
    return lm, sd


def _restated_lm(module, sd, dtype):
    """prefix -> log-probs of the next token from torch.nn.LSTM / GRU with the RNNLM's weights, <sos> = 0 in front."""
    layers, _ = E2E_LMS[module]
    rnn = getattr(torch.nn, module)(32, 32, num_layers=layers, batch_first=True).to(dtype)
    rnn.load_state_dict({k[len('rnn.'):]: v.to(dtype) for k, v in sd.items() if k.startswith('rnn.')})
    emb, tw, tb = sd['emb.weight'].to(dtype), sd['trans.weight'].to(dtype), sd['trans.bias'].to(dtype)
    cache = {}

    def lm(pre):
        pre = tuple(pre)
        if pre not in cache:
            with torch.no_grad():
                y, _ = rnn(emb[torch.tensor((0,) + pre)].unsqueeze(0))
                cache[pre] = torch.log_softmax(y[0, -1] @ tw.t() + tb, dim=-1).numpy()
        return cache[pre]
    return lm


@pytest.mark.gpu
@pytest.mark.parametrize('module', sorted(E2E_LMS))
def test_beam_decoder_with_an_lm_on_a_ctc_only_model(module, tmp_path):
    import yaml
    from src.decode import BeamDecoder
    from test_hip_ctc_beam import E2E_BEAM, E2E_LENS, _ctc_only_model
    model, feat, lens = _ctc_only_model()
    lm, sd = _seeded_lm(module)
    bd = BeamDecoder(model, None, E2E_BEAM, 0.0, 1.0, len_bonus=E2E_LEN_BONUS)
    bd.set_lm(lm.cuda().eval(), E2E_LM_WEIGHT)
    assert any('weight = %.2f' % E2E_LM_WEIGHT in line for line in bd.create_msg())
    with torch.no_grad():
        _, _, tlen, ctc_lp = bd._encode(feat, lens)            # the model's own ctc_output, read back once
    lp_host, tl = ctc_lp.cpu().numpy(), tlen.cpu().tolist()
    lm64, lm32 = _restated_lm(module, sd, torch.float64), _restated_lm(module, sd, torch.float32)
    want, worst = [], 0.0
    for u in range(len(E2E_LENS)):
        lp = lp_host[u, :tl[u]]
        hyps, gaps, info = prefix_beam_search_lm(lp.astype(np.float64), E2E_BEAM, bd.ctc_cand, lm64, E2E_LM_WEIGHT, E2E_LEN_BONUS)
        h32, _, _ = prefix_beam_search_lm(lp, E2E_BEAM, bd.ctc_cand, lm32, E2E_LM_WEIGHT, E2E_LEN_BONUS, dtype=np.float32)
        dev = max(max(abs(a[1] - b[1]), abs(a[2] - b[2])) for a, b in zip(h32, hyps))
        print('utt %d: T\' = %d gaps %s stops %d best %s fp32 transcription deviates by %.4g' % (u, tl[u], gaps, len(info['stops']), hyps[0], dev))
        assert min(gaps.values()) > GAP, 'the seeded model and LM do not hold the gaps: choose another LM seed in E2E_LMS'
        assert [h[0] for h in h32] == [h[0] for h in hyps]
        worst = max(worst, dev)
        want.append(hyps)
    # printed, not asserted: torch's fp32 LSTM / GRU on the CPU differs in the last bits between hosts; the tolerance is the recorded one
    print('E2E_FP32_DEV measured (%s): %r (recorded %r)' % (module, worst, E2E_FP32_DEV))

    def check(got, u):
        assert [h.outIndex for h in got] == [h[0] for h in want[u]]
        for h, (_, fused, ctc) in zip(got, want[u]):
            print('utt %d: fused %.6f (float64 %.6f) ctc %.6f (float64 %.6f)' % (u, h.avgScore(), fused, h.ctc_score, ctc))
            assert abs(h.avgScore() - fused) <= E2E_TOL and abs(h.ctc_score - ctc) <= E2E_TOL
            assert h.score == h.avgScore()

    got3 = bd(feat, lens)
    assert len(got3) == 3
    for u in range(3):
        check(got3[u], u)
    assert 1 <= bd.launches <= max(tl)
    check(bd(feat[:1, :E2E_LENS[0]], lens[:1]), 0)
    # the batched encoder pass agrees with the per-utterance one to rounding only: sequences and order
    bd_b = BeamDecoder(model, None, E2E_BEAM, 0.0, 1.0, batch_encode=True, len_bonus=E2E_LEN_BONUS)
    bd_b.set_lm(lm, E2E_LM_WEIGHT)
    got_b = bd_b(feat, lens)
    for u in range(3):
        assert [h.outIndex for h in got_b[u]] == [h[0] for h in want[u]]
    if module == 'LSTM':
        # the same LM named by an lm_config / lm_path pair
        cfg, ckpt = tmp_path / 'lm.yaml', tmp_path / 'lm.pth'
        cfg.write_text(yaml.safe_dump({'model': {'emb_tying': False, 'emb_dim': 32, 'module': 'LSTM', 'dim': 32, 'n_layers': 2, 'dropout': 0.0}}))
        torch.save({'model': sd}, str(ckpt))
        bd_c = BeamDecoder(model, None, E2E_BEAM, 0.0, 1.0, lm_path=str(ckpt), lm_config=str(cfg), lm_weight=E2E_LM_WEIGHT,
                           len_bonus=E2E_LEN_BONUS).cuda()
        assert bd_c.apply_lm and any('weight = %.2f' % E2E_LM_WEIGHT in line for line in bd_c.create_msg())
        got_c = bd_c(feat, lens)
        for u in range(3):
            check(got_c[u], u)
        with pytest.raises(NotImplementedError, match='RNN-LM fusion for CTC-only decoding is not built'):
            BeamDecoder(model, None, E2E_BEAM, 0.0, 1.0, lm_weight=0.5)
