"""asr_ctc_align (csrc/ctc_align.hip), src.ctc.ctc_forced_align and src.align.CTCAligner against the float64 restatement
of tests/test_ctc_align_reference.py.

Inputs are log_softmax(scale * randn + bump along a random valid alignment of the target) from committed seeds
(`bumped_logp`).  The seeds were searched on the CPU with the restatement alone (`_case_ok`): on every utterance of every
case the best alignment is ahead of the second-best one by `gap` > 8 x the score tolerance of that utterance, so fp32 rounding
cannot change the path (8 x = twice the kernel's allowance on either of two paths) and frame_token / frame_pos / tok_start / tok_end must match EXACTLY.
test_committed_seeds_hold_the_gaps re-checks that without a GPU, for every case.

Score tolerance: the restatement transcribed to fp32 numpy (viterbi_align(dtype=np.float32)) finds the same path as float64
on every case and deviates from it, in `score` and in every per-token score, by at most FP32_DEV over all cases.  The
kernel is allowed 4 x FP32_DEV, scaled by max(1, |value| / 20) (the factor covers the device's order of the
sums; the convention of tests/test_hip_ctc_beam.py).

Long inputs (T = 3000): fp32 sums are coarse there, so that case is not held to the tolerance: the kernel's path must be a
valid alignment of length T, and its float64 rescoring on the CPU must be strictly above the reference's second-best score -
which makes it the optimum."""
import numpy as np
import pytest
import torch

from test_ctc_align_reference import NEG_INF, bumped_logp, collapse, frames_of, spans_of, viterbi_align
from test_ctc_beam_reference import prefix_beam_search

FP32_DEV = 9.270518967241514e-05          # largest |fp32 transcription - float64| over every score of every case (l511_t600, score -585.6)
E_ARG, E_UNSUPPORTED = -1, -3

# name -> V, scale, bump, [(seed, T, L, kind of target) per utterance]
CASES = {
    't1_l1': (31, 3.0, 8.0, [(0, 1, 1, 'any')]),
    'empty_target': (31, 3.0, 8.0, [(0, 12, 0, 'any')]),
    't_equals_l_distinct': (31, 3.0, 8.0, [(0, 6, 6, 'distinct')]),
    'yy_one_forced_blank': (31, 3.0, 8.0, [(1, 5, 4, 'yy')]),
    'yy_infeasible': (31, 3.0, 8.0, [(1, 4, 4, 'yy')]),
    'v31': (31, 3.0, 8.0, [(0, 40, 12, 'any')]),
    'v300': (300, 3.0, 8.0, [(0, 40, 12, 'any')]),
    'ragged': (31, 3.0, 8.0, [(0, 1, 1, 'any'), (0, 37, 9, 'any'), (0, 64, 20, 'any')]),
    'minus_inf_holes': (31, 3.0, 8.0, [(0, 40, 12, 'any')]),
    'blocked_row': (31, 3.0, 8.0, [(0, 40, 12, 'any'), (1, 40, 12, 'any'), (2, 33, 12, 'any')]),
    'l511_t600': (31, 3.0, 8.0, [(0, 600, 511, 'any')]),
    'long': (31, 1.0, 10.0, [(0, 3000, 400, 'any'), (1, 2900, 390, 'any')]),
}
NOT_OK = {('yy_infeasible', 0), ('blocked_row', 1)}          # (case, utterance) without an alignment


def make_target(seed, L, V, kind):
    rng = np.random.RandomState(50000 + seed)
    if kind == 'distinct':
        return [int(y) for y in 1 + rng.permutation(V - 1)[:L]]
    tgt = [int(y) for y in rng.randint(1, V, size=L)]
    if kind == 'yy':
        tgt[2] = tgt[1]                                          # ... y y ...: needs a blank between
        assert sum(a == b for a, b in zip(tgt, tgt[1:])) == 1
    return tgt


def case_inputs(name, seeds=None):
    """[(lp (T,V) fp32, target)] of a case."""
    V, scale, bump, utts = CASES[name]
    out = []
    for n, (seed, T, L, kind) in enumerate(utts):
        seed = seed if seeds is None else seeds[n]
        tgt = make_target(seed, L, V, kind)
        # an infeasible target has no alignment to bump along: the bump of the empty target
        lp, path = bumped_logp(1000 * seed + T, T, V, [] if (name, n) == ('yy_infeasible', 0) else tgt, scale, bump, with_path=True)
        if name == 'minus_inf_holes':
            # a fifth of the entries impossible, off the bump: its own path stays open
            hole = np.random.RandomState(seed + 77).rand(T, V) < 0.2
            hole[np.arange(T), path] = False
            lp = np.where(hole, np.float32(NEG_INF), lp)
        if (name, n) == ('blocked_row', 1):
            lp[T // 2, :] = np.float32(NEG_INF)                                # a frame no path gets through
        out.append((lp, tgt))
    return V, out


_REF = {}


def reference(name):
    """float64 restatement of a case, computed once: one Viterbi tuple per utterance."""
    if name not in _REF:
        _REF[name] = [viterbi_align(lp.astype(np.float64), tgt) for lp, tgt in case_inputs(name)[1]]
    return _REF[name]


def tol(value):
    return 4 * FP32_DEV * max(1.0, abs(value) / 20)


def token_scores(lp, states, target, dtype=np.float64):
    """per-token sum of log-probs over the token's frames, added in frame order in `dtype`."""
    out = [dtype(0)] * len(target)
    for t, s in enumerate(states):
        if s & 1:
            out[s >> 1] = dtype(out[s >> 1] + dtype(lp[t, target[s >> 1]]))
    return [float(x) for x in out]


def fp32_deviation(lp, tgt, ref):
    """The fp32 transcription must find the float64 path; -> largest deviation of its score and per-token scores."""
    h32 = viterbi_align(lp, tgt, dtype=np.float32)
    assert h32.ok and h32.states == ref.states
    dev = abs(h32.score - ref.score)
    a, b = token_scores(lp, ref.states, tgt, np.float32), token_scores(lp.astype(np.float64), ref.states, tgt)
    return max([dev] + [abs(x - y) for x, y in zip(a, b)])


def _case_ok(name, seeds=None):
    """The conditions the seed search asked of a case, on the reference alone."""
    for n, (lp, tgt) in enumerate(case_inputs(name, seeds)[1]):
        ref = viterbi_align(lp.astype(np.float64), tgt)
        if (name, n) in NOT_OK:
            if ref.ok:
                return False
            continue
        if not ref.ok:
            return False
        if not ref.gap > 8 * tol(ref.score):
            return False
        if name == 'minus_inf_holes' and not np.isinf(lp[:, tgt]).any():
            return False
    return True


@pytest.mark.parametrize('name', sorted(CASES))
def test_committed_seeds_hold_the_gaps(name):
    assert _case_ok(name)
    for n, ((lp, tgt), ref) in enumerate(zip(case_inputs(name)[1], reference(name))):
        if (name, n) in NOT_OK:
            assert not viterbi_align(lp, tgt, dtype=np.float32).ok
            continue
        dev = fp32_deviation(lp, tgt, ref)
        print('%s utt %d: score %.6f gap %.4g, fp32 transcription deviates by %.3g' % (name, n, ref.score, ref.gap, dev))
        assert dev <= FP32_DEV
        assert collapse(frames_of(ref.states, tgt)[0]) == tgt and len(ref.states) == lp.shape[0]
    if name == 'l511_t600':
        assert len(case_inputs(name)[1][0][1]) == 511          # all 1023 states live
    if name == 'yy_one_forced_blank':
        assert frames_of(reference(name)[0].states, case_inputs(name)[1][0][1])[0].count(0) == 1


def run_kernel(V, utts, L=None, ws_bytes=None, null=None):
    """One launch for the utterances in `utts` = [(lp, target)].  Frames past each length are NaN, targets past each length
    and every output are pre-filled with garbage.  -> (rc, dict of host arrays)."""
    from src import hipabi as H
    dev = torch.device('cuda')
    B, T = len(utts), max(lp.shape[0] for lp, _ in utts)
    L = max(len(tgt) for _, tgt in utts) if L is None else L
    host = np.full((B, T, V), np.nan, dtype=np.float32)
    tg = np.full((B, max(L, 1)), 10 ** 9, dtype=np.int64)[:, :L]
    for b, (lp, tgt) in enumerate(utts):
        host[b, :lp.shape[0]] = lp
        tg[b, :len(tgt)] = tgt
    logp = torch.from_numpy(host).to(dev)
    targets = torch.from_numpy(np.ascontiguousarray(tg)).to(dev)
    in_len = torch.tensor([lp.shape[0] for lp, _ in utts], dtype=torch.int64, device=dev)
    tg_len = torch.tensor([len(tgt) for _, tgt in utts], dtype=torch.int64, device=dev)
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=dev)
    f32 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=dev)
    o = {'frame_token': i32(B, T), 'frame_pos': i32(B, T), 'tok_start': i32(B, L), 'tok_end': i32(B, L), 'tok_score': f32(B, L),
         'score': f32(B), 'ok': i32(B)}
    need = int(H.lib().asr_ctc_align_workspace_bytes(B, T, min(L, 511)))
    nbytes = need if ws_bytes is None else ws_bytes
    ws = torch.full((max(need, 4),), 0x5a, dtype=torch.uint8, device=dev)
    ptrs = {k: H.ptr(v) for k, v in o.items()}
    if null is not None:
        ptrs[null] = None
    rc = H.lib().asr_ctc_align(H.ptr(logp), H.ptr(targets), H.ptr(in_len), H.ptr(tg_len), B, T, V, L, ptrs['frame_token'], ptrs['frame_pos'],
                               ptrs['tok_start'], ptrs['tok_end'], ptrs['tok_score'], ptrs['score'], ptrs['ok'], H.ptr(ws), nbytes,
                               H.stream_ptr())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def check_row(o, b, lp, tgt, ref, T, L, long_rule=False):
    Tb, n = lp.shape[0], len(tgt)
    ftok, fpos = o['frame_token'][b], o['frame_pos'][b]
    assert (o['tok_start'][b, n:] == -1).all() and (o['tok_end'][b, n:] == -1).all() and (o['tok_score'][b, n:] == 0).all()
    assert (ftok[Tb:] == -1).all() and (fpos[Tb:] == -1).all()
    if not ref.ok:
        assert o['ok'][b] == 0 and o['score'][b] == NEG_INF
        assert (ftok == -1).all() and (fpos == -1).all()
        assert (o['tok_start'][b] == -1).all() and (o['tok_end'][b] == -1).all() and (o['tok_score'][b] == 0).all()
        return
    assert o['ok'][b] == 1
    if long_rule:
        # a valid alignment of length Tb whose float64 score beats the second-best path: the optimum
        got_tok, got_pos = ftok[:Tb].tolist(), fpos[:Tb].tolist()
        assert collapse(got_tok) == tgt
        assert all((c == 0) == (p < 0) and (p < 0 or tgt[p] == c) for c, p in zip(got_tok, got_pos))
        assert [p for p, q in zip(got_pos, [None] + got_pos[:-1]) if p >= 0 and p != q] == list(range(n))
        rescored = float(sum(np.float64(lp[t, c]) for t, c in enumerate(got_tok)))
        print('row %d: float64 rescoring %.6f, reference best %.6f, second best %.6f, kernel score %.6f'
              % (b, rescored, ref.score, ref.score - ref.gap, o['score'][b]))
        assert rescored > ref.score - ref.gap
        want_tok, _ = frames_of(ref.states, tgt)
        assert got_tok == want_tok                                   # follows from the two asserts above; kept as a plain statement
    want_tok, want_pos = frames_of(ref.states, tgt)
    assert ftok[:Tb].tolist() == want_tok
    assert fpos[:Tb].tolist() == want_pos
    start, end = spans_of(ref.states, n)
    assert o['tok_start'][b, :n].tolist() == start and o['tok_end'][b, :n].tolist() == end
    if long_rule:
        assert np.isfinite(o['score'][b]) and np.isfinite(o['tok_score'][b, :n]).all()
        return
    err = abs(float(o['score'][b]) - ref.score)
    print('row %d: score %.6f (float64 %.6f) |diff| %.3g, allowed %.3g' % (b, o['score'][b], ref.score, err, tol(ref.score)))
    assert err <= tol(ref.score)
    for j, want in enumerate(token_scores(lp.astype(np.float64), ref.states, tgt)):
        assert abs(float(o['tok_score'][b, j]) - want) <= tol(want), (b, j, float(o['tok_score'][b, j]), want)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_kernel_equals_float64_restatement(name):
    V, utts = case_inputs(name)
    rc, o = run_kernel(V, utts)
    assert rc == 0
    T, L = o['frame_token'].shape[1], o['tok_start'].shape[1]
    for b, ((lp, tgt), ref) in enumerate(zip(utts, reference(name))):
        assert ref.ok == ((name, b) not in NOT_OK)
        check_row(o, b, lp, tgt, ref, T, L, long_rule=name == 'long')
    if name == 'empty_target':
        assert (o['frame_token'][0] == 0).all() and (o['frame_pos'][0] == -1).all()
        assert abs(float(o['score'][0]) - float(utts[0][0][:, 0].astype(np.float64).sum())) <= tol(float(o['score'][0]))


@pytest.mark.gpu
def test_ties_go_by_the_stated_rules():
    """All entries -2 (sums exact in fp32): every path scores the same, the rules alone pick it - see test_tie_rules."""
    lp = np.full((5, 4), -2.0, dtype=np.float32)
    rc, o = run_kernel(4, [(lp, [1, 2]), (lp, [3, 3]), (lp[:2], [1, 2])])
    assert rc == 0
    assert o['frame_token'].tolist() == [[1, 2, 0, 0, 0], [3, 0, 3, 0, 0], [1, 2, -1, -1, -1]]
    assert o['frame_pos'].tolist() == [[0, 1, -1, -1, -1], [0, -1, 1, -1, -1], [0, 1, -1, -1, -1]]
    assert o['score'].tolist() == [-10.0, -10.0, -4.0] and o['ok'].tolist() == [1, 1, 1]
    assert o['tok_start'].tolist() == [[0, 1], [0, 2], [0, 1]] and o['tok_end'].tolist() == [[0, 1], [0, 2], [0, 1]]
    assert o['tok_score'].tolist() == [[-2.0, -2.0]] * 3


@pytest.mark.gpu
@pytest.mark.parametrize('what', ['too_many_states', 'small_workspace', 'null_pointer', 'token_out_of_range'])
def test_refusals(what):
    from src import hipabi as H
    V, utts = case_inputs('v31')
    if what == 'too_many_states':
        rc, o = run_kernel(V, utts, L=512)
        assert rc == E_UNSUPPORTED and b'states' in H.lib().asr_last_error()
    elif what == 'small_workspace':
        need = int(H.lib().asr_ctc_align_workspace_bytes(1, 40, 12))
        assert need > 0
        rc, o = run_kernel(V, utts, ws_bytes=need - 1)
        assert rc == E_ARG and b'workspace' in H.lib().asr_last_error()
    elif what == 'null_pointer':
        rc, o = run_kernel(V, utts, null='tok_score')
        assert rc == E_ARG and b'null' in H.lib().asr_last_error()
    else:
        # not an argument error (the host cannot see the tokens): the row is reported as not aligned, its neighbour is
        lp, tgt = utts[0]
        rc, o = run_kernel(V, [(lp, tgt[:5] + [V] + tgt[6:]), (lp, tgt)])
        assert rc == 0 and o['ok'].tolist() == [0, 1] and o['score'][0] == NEG_INF and (o['frame_token'][0] == -1).all()
        check_row(o, 1, lp, tgt, reference('v31')[0], 40, 12)
        return
    for k, v in o.items():                                           # nothing was launched
        assert (v == (7.0 if v.dtype == np.float32 else -7)).all(), k


@pytest.mark.gpu
def test_ctc_forced_align_wrapper():
    from src.ctc import ctc_forced_align
    V, utts = case_inputs('ragged')
    dev = torch.device('cuda')
    T, L = max(lp.shape[0] for lp, _ in utts), max(len(t) for _, t in utts)
    logp = torch.zeros((3, T, V))
    targets = torch.zeros((3, L), dtype=torch.int64)
    for b, (lp, tgt) in enumerate(utts):
        logp[b, :lp.shape[0]] = torch.from_numpy(lp)
        targets[b, :len(tgt)] = torch.tensor(tgt)
    res = ctc_forced_align(logp.to(dev), targets.to(dev), torch.tensor([lp.shape[0] for lp, _ in utts]).to(dev),
                           torch.tensor([len(t) for _, t in utts]).to(dev))
    assert all(t.is_cuda for t in res)
    o = {k: getattr(res, k).cpu().numpy() for k in res._fields}
    for b, ((lp, tgt), ref) in enumerate(zip(utts, reference('ragged'))):
        check_row(o, b, lp, tgt, ref, T, L)


# ---- end to end: CTCAligner on the seeded CTC-only model of tests/test_hip_ctc_beam.py (the recipe restated) ----------------
E2E_SEED, E2E_HEAD_SCALE, E2E_BEAM = 0, 40.0, 4
E2E_LENS = (50, 37, 44)
ENC = {'vgg': 0, 'vgg_freq': -1, 'vgg_low_filt': -1, 'module': 'LSTM', 'bidirection': True, 'dim': [32, 32], 'dropout': [0.0, 0.0],
       'layer_norm': [False, False], 'proj': [True, True], 'sample_rate': [1, 2], 'sample_style': 'drop'}


def _seeded_model(ctc_weight, **kw):
    from src.asr import ASR
    D, V = 40, 31
    torch.manual_seed(E2E_SEED)
    model = ASR(D, V, 1, ctc_weight=ctc_weight, encoder=ENC, prec='fp32', **kw)
    sd = model.state_dict()
    g = torch.Generator().manual_seed(E2E_SEED)
    sd = {k: torch.randn(v.shape, generator=g) * (0.3 if v.dim() > 1 else 0.1) for k, v in sd.items()}
    if 'ctc_layer.0.weight' in sd:
        sd['ctc_layer.0.weight'] = sd['ctc_layer.0.weight'] * E2E_HEAD_SCALE            # peaked frames
    model.load_state_dict(sd)
    feat = torch.randn((len(E2E_LENS), max(E2E_LENS), D), generator=g)
    for u, l in enumerate(E2E_LENS):
        feat[u, l:] = 0
    return model.cuda().eval(), feat.cuda(), torch.tensor(E2E_LENS, dtype=torch.int64).cuda()


ATT = {'attention': {'mode': 'loc', 'dim': 24, 'num_head': 1, 'v_proj': False, 'temperature': 0.5, 'loc_kernel_size': 5, 'loc_kernel_num': 4},
       'decoder': {'module': 'LSTM', 'dim': 24, 'layer': 1, 'dropout': 0}}


def _check_aligner(model, feat, lens):
    from src.align import CTCAligner
    from src.decode import encode_unpadded
    aligner = CTCAligner(model)
    assert aligner.frames_per_output == 2
    with torch.no_grad():
        _, enc_len, tlen, ctc_lp = encode_unpadded(model, feat, lens, True)     # the model's own ctc_output, read back once
    lp_host, tl = ctc_lp.cpu().numpy(), tlen.cpu().tolist()
    texts, refs = [], []
    for u in range(len(E2E_LENS)):
        lp = lp_host[u, :tl[u]]
        hyps, _ = prefix_beam_search(lp.astype(np.float64), E2E_BEAM, 6)
        tgt = hyps[0][0]
        ref = viterbi_align(lp.astype(np.float64), tgt)
        print('utt %d: T\' = %d target %s score %.6f gap %.4g' % (u, tl[u], tgt, ref.score, ref.gap))
        assert ref.ok and len(tgt) >= 1
        assert ref.gap > 8 * tol(ref.score), 'the seeded model does not hold the gap: choose another E2E_SEED / E2E_HEAD_SCALE'
        texts.append(tgt)
        refs.append(ref)
    L = max(len(t) for t in texts)
    text = torch.zeros((len(texts), L), dtype=torch.int64)
    for u, t in enumerate(texts):
        text[u, :len(t)] = torch.tensor(t)
    text_len = torch.tensor([len(t) for t in texts])

    def check(al, u):
        start, end = spans_of(refs[u].states, len(texts[u]))
        assert al.ok and al.tokens == texts[u] and al.start_frame == start and al.end_frame == end
        assert abs(al.score - refs[u].score) <= tol(refs[u].score)
        want = token_scores(lp_host[u, :tl[u]].astype(np.float64), refs[u].states, texts[u])
        assert all(abs(a - b) <= tol(b) for a, b in zip(al.token_score, want))

    got3, rate = aligner(feat, lens, text.cuda(), text_len.cuda())
    assert rate == 2 and len(got3) == 3
    for u in range(3):
        check(got3[u], u)
    got1, _ = aligner(feat[:1, :E2E_LENS[0]], lens[:1], text[:1, :len(texts[0])].cuda(), text_len[:1].cuda())
    assert len(got1) == 1
    check(got1[0], 0)
    # a transcript with more tokens than frames cannot be aligned
    too_long = torch.ones((1, tl[0] + 1), dtype=torch.int64) * 5
    bad, _ = aligner(feat[:1, :E2E_LENS[0]], lens[:1], too_long.cuda(), torch.tensor([tl[0] + 1]).cuda())
    assert not bad[0].ok and bad[0].score == NEG_INF and bad[0].start_frame == [-1] * (tl[0] + 1)


@pytest.mark.gpu
def test_aligner_on_a_ctc_only_model():
    _check_aligner(*_seeded_model(1))


@pytest.mark.gpu
def test_aligner_on_a_joint_model_and_refusal_without_ctc():
    from src.align import CTCAligner
    _check_aligner(*_seeded_model(0.3, **ATT))
    model, _, _ = _seeded_model(0, **ATT)
    with pytest.raises(ValueError, match='ctc_weight = 0'):
        CTCAligner(model)


# ---- host side, no GPU ------------------------------------------------------------------------------------------------
def test_tsv_formatter():
    from bin.align_asr import HEADER, format_alignment
    from src.align import Alignment
    assert HEADER.split('\t') == ['idx', 'token', 'start_s', 'end_s', 'score']
    al = Alignment([5, 9], [0, 3], [1, 3], [-0.25, -1.5], -2.0, True)
    assert format_alignment('utt1', ['a', 'b'], al, 0.04) == ['utt1\ta\t0.000\t0.080\t-0.2500', 'utt1\tb\t0.120\t0.160\t-1.5000']
    bad = Alignment([5, 9], [-1, -1], [-1, -1], [0.0, 0.0], NEG_INF, False)
    assert format_alignment('utt2', ['a', 'b'], bad, 0.04) == ['utt2\t\t\t\t-inf']


def test_main_routes_align_to_the_new_solver():
    import main
    import bin.align_asr
    import bin.test_asr
    assert main.select_solver(main.parser.parse_args(['--config', 'x', '--align'])) == (bin.align_asr.Solver, 'test')
    assert main.select_solver(main.parser.parse_args(['--config', 'x', '--test'])) == (bin.test_asr.Solver, 'test')
    assert issubclass(bin.align_asr.Solver, bin.test_asr.Solver)
