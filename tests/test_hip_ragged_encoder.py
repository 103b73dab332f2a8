"""The length-aware batched encoder pass on the GPU: the movement kernels of csrc/ragged.hip bit for bit against numpy
indexing, encode_batched against encode_unpadded (both measured with the float64 restatement of
tests/test_ragged_encoder_reference.py), and BeamDecoder / CTCAligner with batch_encode=True end to end.

Error bound of encode_batched: with e_batched and e_unpadded the largest absolute errors of the two passes against float64,
e_batched <= 2 * e_unpadded + 1e-6.  Both passes run the same kernels on the same valid data and can differ only in GEMM
tiling and in the recurrence plan chosen for another B and T; the factor 2 covers a different summation order, the floor keeps
an exact fp32 case from dividing by nothing.  Each case prints a RATIO line."""
import os

import numpy as np
import pytest
import torch

from test_ctc_beam_reference import prefix_beam_search
from test_ragged_encoder_reference import encoder_f64

GAP = 1e-3
LENS = (7, 4, 1)
GARBAGE, GARBAGE_DST = 7.0, -7.0


# ---- movement kernels -------------------------------------------------------------------------------------------------------
def _payload(shape, dtype, seed):
    """Values that are never 0, 7 or -7, as raw bits: fp32 in [1,2), bf16 bit patterns in [1, 0x3f00) (positive, below 1)."""
    rs = np.random.RandomState(seed)
    if dtype == 'fp32':
        return (1.0 + rs.rand(*shape)).astype(np.float32).view(np.int32)
    return rs.randint(1, 0x3f00, size=shape).astype(np.int16)


def _bits(value, dtype):
    if dtype == 'fp32':
        return np.array([value], dtype=np.float32).view(np.int32)[0]
    return torch.tensor([value], dtype=torch.bfloat16).view(torch.int16).numpy()[0]


def _to_dev(bits, dtype):
    t = torch.from_numpy(np.ascontiguousarray(bits)).cuda()
    return t.view(torch.float32 if dtype == 'fp32' else torch.bfloat16)


def _from_dev(t, dtype):
    return t.view(torch.int32 if dtype == 'fp32' else torch.int16).cpu().numpy()


def _check_clean(got, want, dtype):
    assert np.array_equal(got, want)                                     # bit for bit
    for g in (GARBAGE, GARBAGE_DST):
        assert not (got == _bits(g, dtype)).any()                        # no garbage anywhere in the output


# dtype, ND, W (elements per (b,t,direction)): fp32 inner extent 8; the bf16 layout (H,4) with H = 16; ND = 1; and extents
# that are no multiple of the 16-byte vector (the ABI accepts them: element-wise path)
ALIGN_CASES = [('fp32', 2, 8), ('fp32', 1, 8), ('fp32', 2, 6), ('bf16', 2, 64), ('bf16', 1, 64), ('bf16', 2, 12)]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,ND,W', ALIGN_CASES)
def test_align_kernel_is_exact(dtype, ND, W):
    from src import hipabi as H
    B, T = len(LENS), max(LENS)
    data = _payload((B, T, ND, W), dtype, 1)
    src = np.full_like(data, _bits(GARBAGE, dtype))
    want = np.zeros_like(data)
    for b, n in enumerate(LENS):
        src[b, :n] = data[b, :n]
        want[b, :n, 0] = data[b, :n, 0]
        if ND == 2:
            want[b, T - n:, 1] = data[b, :n, 1]
    dst = _to_dev(np.full_like(data, _bits(GARBAGE_DST, dtype)), dtype)
    lens = torch.tensor(LENS, dtype=torch.int64).cuda()
    H.call('asr_ragged_align', H.ptr(_to_dev(src, dtype)), H.ptr(dst), H.ptr(lens), B, T, ND, W, 4 if dtype == 'fp32' else 2, H.stream_ptr())
    torch.cuda.synchronize()
    _check_clean(_from_dev(dst, dtype), want, dtype)


# dtype, ND, H: fp32 (ND*H = inner extent 8), bf16 H = 16, ND = 1, and H no multiple of the vector
UNALIGN_CASES = [('fp32', 2, 4), ('fp32', 1, 8), ('fp32', 2, 3), ('bf16', 2, 16), ('bf16', 1, 16), ('bf16', 2, 12)]


@pytest.mark.gpu
@pytest.mark.parametrize('rate,style', [(1, 0), (2, 0), (2, 1)])
@pytest.mark.parametrize('dtype,ND,Hd', UNALIGN_CASES)
def test_unalign_kernel_is_exact(dtype, ND, Hd, rate, style):
    """y as the recurrence leaves it (direction 1 right-aligned, garbage where it ran over padding; the bf16 form time-padded
    with its h(-1) / h(T) rows) -> z left-aligned, down-sampled, exact zeros past every row's output length."""
    from src import hipabi as H
    B, T = len(LENS), max(LENS)
    pad = 1 if dtype == 'bf16' else 0
    data = _payload((B, T, ND, Hd), dtype, 2)                            # the unpadded pass's y of every row, left-aligned
    y = np.full((B, T + 2 * pad, ND, Hd), _bits(GARBAGE, dtype), dtype=data.dtype)
    segs = rate if style == 1 else 1
    T2 = -(-T // rate) if style == 0 else T // rate
    want = np.zeros((B, T2, segs, ND, Hd), dtype=data.dtype)
    for b, n in enumerate(LENS):
        y[b, pad:pad + n, 0] = data[b, :n, 0]
        if ND == 2:
            y[b, pad + T - n:pad + T, 1] = data[b, :n, 1]
        nout = -(-n // rate) if style == 0 else n // rate
        for t2 in range(nout):
            for i in range(segs):
                want[b, t2, i] = data[b, t2 * rate + i]
    dst = _to_dev(np.full_like(want, _bits(GARBAGE_DST, dtype)), dtype)
    lens = torch.tensor(LENS, dtype=torch.int64).cuda()
    D = ND * Hd
    H.call('asr_ragged_unalign', H.ptr(_to_dev(y, dtype)), (T + 2 * pad) * D, pad * D, H.ptr(dst), H.ptr(lens), B, T, ND, Hd, T2, rate, style,
           4 if dtype == 'fp32' else 2, H.stream_ptr())
    torch.cuda.synchronize()
    _check_clean(_from_dev(dst, dtype), want, dtype)


@pytest.mark.gpu
def test_refusals_launch_nothing():
    from src import hipabi as H
    x = torch.full((3, 7, 2, 8), GARBAGE, device='cuda')
    dst = torch.full((3, 7, 2, 8), GARBAGE_DST, device='cuda')
    lens = torch.tensor(LENS, dtype=torch.int64).cuda()
    lib, st = H.lib(), H.stream_ptr()
    assert lib.asr_ragged_align(H.ptr(x), H.ptr(x), H.ptr(lens), 3, 7, 2, 8, 4, st) == -1           # in place
    assert lib.asr_ragged_align(H.ptr(x), H.ptr(dst), H.ptr(lens), 3, 7, 3, 8, 4, st) == -1         # three directions
    assert lib.asr_ragged_align(H.ptr(x), H.ptr(dst), H.ptr(lens), 3, 7, 2, 8, 8, st) == -1         # element size
    assert lib.asr_ragged_align(H.ptr(x), H.ptr(dst), None, 3, 7, 2, 8, 4, st) == -1
    assert lib.asr_ragged_unalign(H.ptr(x), 7 * 16 - 1, 0, H.ptr(dst), H.ptr(lens), 3, 7, 2, 8, 7, 1, 0, 4, st) == -1      # stride too short
    assert lib.asr_ragged_unalign(H.ptr(x), 7 * 16, 0, H.ptr(dst), H.ptr(lens), 3, 7, 2, 8, 4, 2, 2, 4, st) == -1          # style
    assert lib.asr_ragged_unalign(H.ptr(x), 7 * 16, 0, H.ptr(dst), H.ptr(lens), 3, 7, 2, 8, 4, 0, 0, 4, st) == -1          # rate
    torch.cuda.synchronize()
    assert (dst == GARBAGE_DST).all()


# ---- encode_batched against encode_unpadded ---------------------------------------------------------------------------------
SEED, HEAD_SCALE, BEAM = 0, 40.0, 4          # the seeded CTC-only model of tests/test_hip_ctc_beam.py (the recipe restated)
E2E_LENS = (50, 37, 44)
ENC = {'vgg': 0, 'vgg_freq': -1, 'vgg_low_filt': -1, 'module': 'LSTM', 'bidirection': True, 'dim': [32, 32], 'dropout': [0.0, 0.0],
       'layer_norm': [False, False], 'proj': [True, True], 'sample_rate': [1, 2], 'sample_style': 'drop'}
ATT = {'attention': {'mode': 'loc', 'dim': 24, 'num_head': 1, 'v_proj': False, 'temperature': 0.5, 'loc_kernel_size': 5, 'loc_kernel_num': 4},
       'decoder': {'module': 'LSTM', 'dim': 24, 'layer': 1, 'dropout': 0}}


def _model(lens=E2E_LENS, prec='fp32', ctc_weight=1, seed=SEED, enc=None, **kw):
    """-> (model, state dict on the host, feat (U,T,D) with the padding filled with 7.0, lens)."""
    from src.asr import ASR
    D, V = 40, 31
    enc = dict(ENC, **(enc or {}))
    torch.manual_seed(seed)
    model = ASR(D, V, 1, ctc_weight=ctc_weight, encoder=enc, prec=prec, **kw)
    sd = model.state_dict()
    g = torch.Generator().manual_seed(seed)
    sd = {k: torch.randn(v.shape, generator=g) * (0.3 if v.dim() > 1 else 0.1) for k, v in sd.items()}
    if 'ctc_layer.0.weight' in sd:
        sd['ctc_layer.0.weight'] = sd['ctc_layer.0.weight'] * HEAD_SCALE            # peaked frames: the gaps of the search must hold
    model.load_state_dict(sd)
    feat = torch.randn((len(lens), max(lens), D), generator=g)
    for u, l in enumerate(lens):
        feat[u, l:] = GARBAGE
    return model.cuda().eval(), sd, feat.cuda(), torch.tensor(lens, dtype=torch.int64).cuda()


_F64 = {}


def _reference(key, sd, enc_cfg, feat, lens):
    """float64 restatement per utterance, unpadded; computed once per case and shared."""
    if key not in _F64:
        host = feat.cpu()
        _F64[key] = [encoder_f64(sd, enc_cfg, host[u, :n]) for u, n in enumerate(lens)]
    return _F64[key]


def _errors(ref, enc, ctc, tlen):
    e = 0.0
    for u, (r_enc, r_ctc) in enumerate(ref):
        n = int(tlen[u])
        assert r_enc.shape[0] == n
        e = max(e, float((enc[u, :n].double().cpu() - r_enc).abs().max()), float((ctc[u, :n].double().cpu() - r_ctc).abs().max()))
    return e


def _compare(key, model, sd, enc_cfg, feat, lens):
    from src.decode import encode_batched, encode_unpadded
    lens_l = lens.cpu().tolist()
    ref = _reference(key, sd, enc_cfg, feat, lens_l)
    clean = feat.clone()
    for u, n in enumerate(lens_l):
        clean[u, n:] = 0
    with torch.no_grad():
        a_enc, a_len, a_tlen, a_ctc = encode_unpadded(model, clean, lens, True)
        b_enc, b_len, b_tlen, b_ctc = encode_batched(model, feat, lens, True)          # sees 7.0 in the feature padding
    assert b_enc.shape == a_enc.shape and b_ctc.shape == a_ctc.shape
    assert b_enc.dtype == a_enc.dtype == torch.float32 and b_len.dtype == a_len.dtype and b_tlen.dtype == a_tlen.dtype
    assert torch.equal(a_len, b_len) and torch.equal(a_tlen, b_tlen)
    for u in range(len(lens_l)):
        n = int(b_tlen[u])
        assert (b_enc[u, n:] == 0).all() and (b_ctc[u, n:] == 0).all()                 # padding exactly 0
    e_unp, e_bat = _errors(ref, a_enc, a_ctc, a_tlen), _errors(ref, b_enc, b_ctc, b_tlen)
    print('RATIO %s: e_batched %.3e e_unpadded %.3e ratio %.3f' % (key, e_bat, e_unp, e_bat / max(e_unp, 1e-30)))
    assert e_bat <= 2 * e_unp + 1e-6
    return b_enc, b_ctc, b_tlen


@pytest.mark.gpu
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('lens', [E2E_LENS, (9, 1, 6)])
def test_encode_batched_equals_encode_unpadded(lens, prec):
    model, sd, feat, lens_t = _model(lens, prec)
    _compare('%s %s' % (prec, lens), model, sd, ENC, feat, lens_t)


@pytest.mark.gpu
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_one_utterance(prec):
    model, sd, feat, lens_t = _model(E2E_LENS[:1], prec)
    _compare('%s one utterance' % prec, model, sd, ENC, feat, lens_t)


@pytest.mark.gpu
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_layer_norm_and_concat(prec):
    """LayerNorm and 'concat' down-sampling take the fp32-storage kernels in either precision (src/functions.rnn_fast_ok).
    The first layer stacks pairs of frames (37 -> 18, the tail dropped) in front of the second one's alignment; `pj` is sized
    for the un-concatenated width, so the concatenating layer has no projection."""
    over = {'layer_norm': [True, True], 'sample_rate': [2, 1], 'sample_style': 'concat', 'proj': [False, True]}
    model, sd, feat, lens_t = _model(E2E_LENS, prec, enc=over)
    _compare('%s LayerNorm concat' % prec, model, sd, dict(ENC, **over), feat, lens_t)


@pytest.mark.gpu
def test_chunks_of_the_recurrence_batch(monkeypatch):
    """More utterances than one pass takes: the chunks are merged into one zero-padded result."""
    from src import ragged
    from src.decode import encode_batched
    model, sd, feat, lens_t = _model(E2E_LENS, 'fp32')
    with torch.no_grad():
        whole = encode_batched(model, feat, lens_t, True)
        monkeypatch.setattr(ragged, 'max_batch', lambda asr: 2)
        parts = encode_batched(model, feat, lens_t, True)
    assert parts[0].shape == whole[0].shape and torch.equal(parts[1], whole[1]) and torch.equal(parts[2], whole[2])
    ref = _reference('fp32 %s' % (E2E_LENS,), sd, ENC, feat, list(E2E_LENS))
    e_whole, e_parts = _errors(ref, whole[0], whole[3], whole[2]), _errors(ref, parts[0], parts[3], parts[2])
    print('RATIO chunks of 2: e_chunked %.3e e_whole %.3e' % (e_parts, e_whole))
    assert e_parts <= 2 * e_whole + 1e-6
    for u in range(3):
        n = int(parts[2][u])
        assert (parts[0][u, n:] == 0).all() and (parts[3][u, n:] == 0).all()


@pytest.mark.gpu
def test_gru_encoder_falls_back():
    from src.decode import BeamDecoder, encode_batched, encode_unpadded
    model, sd, feat, lens_t = _model(E2E_LENS, 'fp32', enc={'module': 'GRU'})
    clean = feat.clone()
    for u, n in enumerate(E2E_LENS):
        clean[u, n:] = 0
    with torch.no_grad():
        a, b = encode_unpadded(model, clean, lens_t, True), encode_batched(model, clean, lens_t, True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    msg = BeamDecoder(model, None, BEAM, 0.0, 1.0, batch_encode=True).create_msg()
    assert any('fell back' in line and 'GRU' in line for line in msg)
    lstm = _model(E2E_LENS, 'fp32')[0]
    assert any('batched' in line for line in BeamDecoder(lstm, None, BEAM, 0.0, 1.0, batch_encode=True).create_msg())
    assert any('one utterance at a time' in line for line in BeamDecoder(lstm, None, BEAM, 0.0, 1.0).create_msg())


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_beam_decoder_batch_encode_on_a_ctc_only_model():
    from src.decode import BeamDecoder
    from test_hip_ctc_beam import SCORE_TOL
    model, sd, feat, lens = _model()
    bd = BeamDecoder(model, None, BEAM, 0.0, 1.0, ctc_weight=0.3, batch_encode=True)
    with torch.no_grad():
        _, _, tlen, ctc_lp = bd._encode(feat, lens)            # the batched pass's own ctc_output, read back once
    lp_host, tl = ctc_lp.cpu().numpy(), tlen.cpu().tolist()
    want = []
    for u in range(len(E2E_LENS)):
        hyps, gaps = prefix_beam_search(lp_host[u, :tl[u]].astype(np.float64), BEAM, bd.ctc_cand)
        print('utt %d: T\' = %d gaps %s best %s' % (u, tl[u], gaps, hyps[0]))
        assert min(gaps.values()) > GAP, 'the seeded model does not hold the gaps: choose another SEED / HEAD_SCALE'
        want.append(hyps)
    got = bd(feat, lens)
    clean = feat.clone()
    for u, n in enumerate(E2E_LENS):
        clean[u, n:] = 0
    default = BeamDecoder(model, None, BEAM, 0.0, 1.0, ctc_weight=0.3)(clean, lens)
    for u in range(3):
        assert [h.outIndex for h in got[u]] == [h for h, _ in want[u]]
        for h, (_, s) in zip(got[u], want[u]):
            assert abs(h.avgScore() - s) <= SCORE_TOL * max(1.0, abs(s) / 20)
        assert [h.outIndex for h in got[u]] == [h.outIndex for h in default[u]]


ATT_SEED = 6            # chosen so that adjacent hypotheses of the default mode are more than GAP apart (asserted below)


@pytest.mark.gpu
@pytest.mark.parametrize('ctc_weight', [0.0, 0.3])
def test_attention_model_decodes_the_same(ctc_weight):
    from src.decode import BeamDecoder
    model, sd, feat, lens = _model(ctc_weight=0.3, seed=ATT_SEED, **ATT)
    clean = feat.clone()
    for u, n in enumerate(E2E_LENS):
        clean[u, n:] = 0
    ref = BeamDecoder(model, None, BEAM, 0.0, 0.2, ctc_weight=ctc_weight)(clean, lens)
    for u, hyps in enumerate(ref):
        scores = [h.avgScore() for h in hyps]
        print('utt %d: default mode %s' % (u, [(h.outIndex, round(s, 5)) for h, s in zip(hyps, scores)]))
        assert len(hyps) >= 2
        assert all(a - b > GAP for a, b in zip(scores, scores[1:])), 'hypotheses closer than 1e-3: choose another ATT_SEED'
    got = BeamDecoder(model, None, BEAM, 0.0, 0.2, ctc_weight=ctc_weight, batch_encode=True)(feat, lens)
    for u in range(3):
        assert [h.outIndex for h in got[u]] == [h.outIndex for h in ref[u]]
        for a, b in zip(got[u], ref[u]):
            print('utt %d: avgScore %.7f (default mode %.7f)' % (u, a.avgScore(), b.avgScore()))
            assert abs(a.avgScore() - b.avgScore()) <= 1e-4            # the fp32 bound for log-probs


@pytest.mark.gpu
def test_aligner_batch_encode():
    from src.align import CTCAligner
    from src.decode import encode_unpadded
    from test_hip_ctc_align import tol
    model, sd, feat, lens = _model()
    clean = feat.clone()
    for u, n in enumerate(E2E_LENS):
        clean[u, n:] = 0
    with torch.no_grad():
        _, _, tlen, ctc_lp = encode_unpadded(model, clean, lens, True)
    lp_host, tl = ctc_lp.cpu().numpy(), tlen.cpu().tolist()
    texts = [prefix_beam_search(lp_host[u, :tl[u]].astype(np.float64), BEAM, 6)[0][0][0] for u in range(3)]
    L = max(len(t) for t in texts)
    text = torch.zeros((3, L), dtype=torch.int64)
    for u, t in enumerate(texts):
        text[u, :len(t)] = torch.tensor(t)
    text_len = torch.tensor([len(t) for t in texts])
    want, rate_w = CTCAligner(model)(clean, lens, text.cuda(), text_len.cuda())
    aligner = CTCAligner(model, batch_encode=True)
    assert any('batched' in line for line in aligner.create_msg())
    got, rate_g = aligner(feat, lens, text.cuda(), text_len.cuda())
    assert rate_g == rate_w == 2
    for u in range(3):
        a, b = got[u], want[u]
        print('utt %d: score %.6f (default mode %.6f)' % (u, a.score, b.score))
        assert a.ok and b.ok and a.tokens == b.tokens == texts[u]
        assert a.start_frame == b.start_frame and a.end_frame == b.end_frame          # token boundaries identical
        assert abs(a.score - b.score) <= tol(b.score)
        assert all(abs(x - y) <= tol(y) for x, y in zip(a.token_score, b.token_score))


# ---- main.py --test --decode-batch N: the batched Solver as a whole ---------------------------------------------------------
@pytest.mark.gpu
def test_batched_solver_writes_the_rows_in_order(tmp_path):
    """bin/batch_asr.Solver (--decode-batch 3) against bin/test_asr.Solver on the reference-written checkpoint of
    tests/test_checkpoint_interop.py (LSTM encoder, no front-end: eligible).  Names and transcripts are data and must be the
    same rows in the same order; the hypotheses come from two encoder passes that agree to rounding only, so the number of
    rows whose hypothesis differs is printed, not asserted (the decoder tests above hold the tokens under a margin)."""
    import bin.batch_asr
    import bin.test_asr
    from test_checkpoint_interop import CKPT, _meta, _paras, _train_config
    meta, _ = _meta()
    _, train_yaml = _train_config(tmp_path, meta, 'fp32')
    cfg = {'src': {'config': train_yaml, 'ckpt': CKPT},
           'decode': {'beam_size': meta['beam'], 'min_len_ratio': meta['min_len_ratio'], 'max_len_ratio': meta['max_len_ratio'],
                      'ctc_weight': meta['ctc_weight']},
           'data': {'corpus': {'name': 'LibriSpeech'}}}
    rows = {}
    for key, cls, extra in (('one', bin.test_asr.Solver, {}), ('batched', bin.batch_asr.Solver, {'decode_batch': 3})):
        out = tmp_path / key
        solver = cls(cfg, _paras(out, outdir=str(out / 'result'), **extra), 'test')
        solver.load_data()
        solver.set_model()
        assert solver.decoder.batch_encode == (key == 'batched')
        solver.exec()
        for split in ('dev', 'test'):
            with open(os.path.join(solver.paras.outdir, '{}_{}.tsv'.format(solver.exp_name, split))) as f:
                lines = f.read().split('\n')
            assert lines[0] == 'idx\thyp\ttruth' and lines[-1] == ''
            rows[key, split] = [line.split('\t') for line in lines[1:-1]]
    assert any('batched' in line for line in solver.decoder.create_msg())
    for split in ('dev', 'test'):
        one, got = rows['one', split], rows['batched', split]
        assert len(one) > 3 and len(one) % 3 != 0, 'the split must give more than one group and a short last one'
        assert [(r[0], r[2]) for r in got] == [(r[0], r[2]) for r in one]
        assert all(len(r) == 3 for r in got)
        print('%s: %d rows, %d hypotheses differ from --decode-batch 1' % (split, len(one), sum(a[1] != b[1] for a, b in zip(one, got))))
