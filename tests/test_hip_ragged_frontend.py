"""The batched encoder pass for models with a front-end on the GPU: asr_ragged_zero_tail bit for bit against numpy,
encode_batched against encode_unpadded for vgg 1..7 (both measured with the float64 restatement of
tests/test_ragged_frontend_reference.py), chunking by the front-end byte budget, and BeamDecoder(batch_encode=True) end to end
on a vgg 1 model.

Error bound of encode_batched (the rule of tests/test_hip_ragged_encoder.py, unchanged): with e_batched and e_unpadded the
largest absolute errors of the two passes against float64, e_batched <= 2 * e_unpadded + 1e-6.  Both passes run the same
kernels on the same valid data and differ only in tiling and plans chosen for another B and T.  Each case prints a RATIO line."""
import ctypes

import numpy as np
import pytest
import torch

from test_ctc_beam_reference import prefix_beam_search
from test_ragged_frontend_reference import D_, V_, enc_cfg, encoder_f64, seeded_state_dict

GAP = 1e-3
SENTINEL = -7.0


# ---- asr_ragged_zero_tail -----------------------------------------------------------------------------------------------------
def _sentinel_bits(dtype):
    if dtype == 'fp32':
        return np.array([SENTINEL], dtype=np.float32).view(np.int32)[0]
    return torch.tensor([SENTINEL], dtype=torch.bfloat16).view(torch.int16).numpy()[0]


def _np_dtype(dtype):
    return np.int32 if dtype == 'fp32' else np.int16


def _run_zero_tail(dtype, t_off, W, lens, B=3, T=7, skew=0):
    """Sentinel-filled (B, T + 2 t_off, W) buffer with one guard element on each side, `skew` further elements in front (a
    pointer that is element-aligned only); returns (raw bits after the launch with the guards, expected bits)."""
    from src import hipabi as H
    Ttot, eb = T + 2 * t_off, 4 if dtype == 'fp32' else 2
    n_el = B * Ttot * W
    s = _sentinel_bits(dtype)
    host = np.full(1 + skew + n_el + 1, s, dtype=_np_dtype(dtype))
    want = host.copy()
    body = want[1 + skew:1 + skew + n_el].reshape(B, Ttot, W)
    for b, n in enumerate(lens):
        body[b, t_off + min(max(n, 0), T):t_off + T] = 0
    dev = torch.from_numpy(host).cuda()
    lens_d = torch.tensor(lens, dtype=torch.int64).cuda()
    p = ctypes.c_void_p(dev.data_ptr() + (1 + skew) * eb)
    H.call('asr_ragged_zero_tail', p, H.ptr(lens_d), B, T, Ttot, t_off, W, eb, H.stream_ptr())
    torch.cuda.synchronize()
    return dev.cpu().numpy(), want


@pytest.mark.gpu
@pytest.mark.parametrize('lens', [(7, 0, 3), (9, -2, 3)])
@pytest.mark.parametrize('W', [24, 5])
@pytest.mark.parametrize('t_off', [0, 1])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_zero_tail_kernel_is_exact(dtype, t_off, W, lens):
    """The tail is zero; every other element - valid frames, the border rows of the bordered layout, the guard elements in
    front of and behind the buffer - still holds the sentinel.  The guard element puts the buffer 4 resp. 2 bytes behind a
    16-byte boundary, so these cases take the element-wise stores; `skew` 3 (fp32) / 7 (bf16) puts it ON the boundary and
    W = 24 then takes the 16-byte stores, W = 5 never does."""
    for skew in (0, 3 if dtype == 'fp32' else 7):
        got, want = _run_zero_tail(dtype, t_off, W, lens, skew=skew)
        assert np.array_equal(got, want), (dtype, t_off, W, lens, skew)
        assert (want == 0).sum() == sum(7 - min(max(n, 0), 7) for n in lens) * W


@pytest.mark.gpu
def test_zero_tail_two_byte_offset_pointer():
    """bf16 buffer 2 bytes behind a 16-byte boundary with a row width that would allow 16-byte stores: element-wise, exact."""
    got, want = _run_zero_tail('bf16', 1, 24, (7, 0, 3), skew=0)
    assert np.array_equal(got, want)
    got, want = _run_zero_tail('bf16', 1, 24, (7, 0, 3), skew=8)            # 18 bytes behind: still 2 off
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_zero_tail_refusals_launch_nothing():
    from src import hipabi as H
    buf = torch.full((3, 9, 24), SENTINEL, device='cuda')
    lens = torch.tensor((7, 0, 3), dtype=torch.int64).cuda()
    fn, st, p, lp = H.lib().asr_ragged_zero_tail, H.stream_ptr(), H.ptr(buf), H.ptr(lens)
    assert fn(None, lp, 3, 7, 9, 1, 24, 4, st) == -1                         # null buffer
    assert fn(p, None, 3, 7, 9, 1, 24, 4, st) == -1                          # null lengths
    assert fn(p, lp, 0, 7, 9, 1, 24, 4, st) == -1                            # no rows
    assert fn(p, lp, 3, 0, 9, 1, 24, 4, st) == -1                            # no frames
    assert fn(p, lp, 3, 7, 9, 1, 0, 4, st) == -1                             # no width
    assert fn(p, lp, 3, 7, 9, -1, 24, 4, st) == -1                           # negative offset
    assert fn(p, lp, 3, 7, 8, 2, 24, 4, st) == -1                            # t_off + T > Ttot
    assert fn(p, lp, 3, 7, 9, 1, 24, 8, st) == -1                            # element size
    assert fn(ctypes.c_void_p(buf.data_ptr() + 2), lp, 3, 7, 9, 1, 24, 4, st) == -1          # fp32 on a 2-byte offset
    assert fn(p, lp, 1 << 12, 1, 1 << 11, 0, 24, 4, st) == -3                # 2^23 time rows: unsupported, not launched
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()


# ---- encode_batched against encode_unpadded -----------------------------------------------------------------------------------
SEED, HEAD_SCALE, BEAM = 0, 40.0, 4
E2E_LENS = (50, 37, 44)           # three different n % 4: truncation and masking are both exercised
SHORT_LENS = (9, 4, 6)
GARBAGE = 7.0


def _model(vgg, lens=E2E_LENS, prec='fp32', seed=SEED):
    """-> (model, state dict on the host, feat (U,T,D) with the padding filled with 7.0, lens)."""
    from src.asr import ASR
    torch.manual_seed(seed)
    model = ASR(D_, V_, 1, ctc_weight=1, encoder=enc_cfg(vgg), prec=prec)
    sd = seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed, HEAD_SCALE)
    model.load_state_dict(sd)
    g = torch.Generator().manual_seed(seed + 1)
    feat = torch.randn((len(lens), max(lens), D_), generator=g)
    for u, l in enumerate(lens):
        feat[u, l:] = GARBAGE
    return model.cuda().eval(), sd, feat.cuda(), torch.tensor(lens, dtype=torch.int64).cuda()


_F64 = {}


def _reference(vgg, sd, feat, lens):
    """float64 restatement per utterance, unpadded; computed once per (front-end, lengths) and shared (the weights and the
    features depend on the seed and the shapes only, not on the precision)."""
    key = (vgg, tuple(lens))
    if key not in _F64:
        host = feat.cpu()
        _F64[key] = [encoder_f64(sd, enc_cfg(vgg), host[u, :n]) for u, n in enumerate(lens)]
    return _F64[key]


def _errors(ref, enc, ctc, tlen):
    e = 0.0
    for u, (r_enc, r_ctc, _) in enumerate(ref):
        n = int(tlen[u])
        assert r_enc.shape[0] == n
        e = max(e, float((enc[u, :n].double().cpu() - r_enc).abs().max()), float((ctc[u, :n].double().cpu() - r_ctc).abs().max()))
    return e


def _compare(key, vgg, model, sd, feat, lens):
    from src.decode import encode_batched, encode_unpadded
    from src.ragged import ineligible_reason
    assert ineligible_reason(model) is None
    lens_l = lens.cpu().tolist()
    ref = _reference(vgg, sd, feat, lens_l)
    clean = feat.clone()
    for u, n in enumerate(lens_l):
        clean[u, n:] = 0
    with torch.no_grad():
        a_enc, a_len, a_tlen, a_ctc = encode_unpadded(model, clean, lens, True)
        b_enc, b_len, b_tlen, b_ctc = encode_batched(model, feat, lens, True)          # sees 7.0 in the feature padding
    assert b_enc.shape == a_enc.shape and b_ctc.shape == a_ctc.shape
    assert b_enc.dtype == a_enc.dtype == torch.float32 and b_len.dtype == a_len.dtype and b_tlen.dtype == a_tlen.dtype
    assert torch.equal(a_len, b_len) and torch.equal(a_tlen, b_tlen)
    assert b_len.cpu().tolist() == [r[2] for r in ref]
    for u in range(len(lens_l)):
        n = int(b_tlen[u])
        assert (b_enc[u, n:] == 0).all() and (b_ctc[u, n:] == 0).all()                 # padding exactly 0
    e_unp, e_bat = _errors(ref, a_enc, a_ctc, a_tlen), _errors(ref, b_enc, b_ctc, b_tlen)
    print('RATIO %s: e_batched %.3e e_unpadded %.3e ratio %.3f' % (key, e_bat, e_unp, e_bat / max(e_unp, 1e-30)))
    assert e_bat <= 2 * e_unp + 1e-6
    return b_enc, b_ctc, b_tlen


# vgg 1 and 5 in both precisions (bf16: the bordered bf16 images of _VGG16Fn; fp32: the plain fp32 images of _VGGFn); vgg 3
# (time_div 2, frequency-only second pooling), vgg 2 (frequency split at bin 12, 4 low filters), vgg 6 and vgg 7 in fp32
CASES = [(1, 'fp32'), (1, 'bf16'), (5, 'fp32'), (5, 'bf16'), (3, 'fp32'), (2, 'fp32'), (6, 'fp32'), (7, 'fp32')]


@pytest.mark.gpu
@pytest.mark.parametrize('lens', [E2E_LENS, SHORT_LENS])
@pytest.mark.parametrize('vgg,prec', CASES)
def test_encode_batched_equals_encode_unpadded(vgg, prec, lens):
    model, sd, feat, lens_t = _model(vgg, lens, prec)
    _compare('vgg %d %s %s' % (vgg, prec, lens), vgg, model, sd, feat, lens_t)


@pytest.mark.gpu
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('lens', [(48,), (44, 44, 44)])
def test_equal_lengths(lens, prec):
    """One utterance, and a batch of equal lengths that are multiples of 4: no row has a tail, nothing is masked."""
    model, sd, feat, lens_t = _model(1, lens, prec)
    _compare('vgg 1 %s equal lengths %s' % (prec, lens), 1, model, sd, feat, lens_t)


@pytest.mark.gpu
def test_chunks_of_the_front_end_budget(monkeypatch):
    """The byte budget low enough for two rows of T = 50 per chunk: the chunks are merged into one zero-padded result."""
    from src import ragged
    from src.decode import encode_batched
    from src.vgg import largest_activation_bytes
    model, sd, feat, lens_t = _model(1, E2E_LENS, 'fp32')
    with torch.no_grad():
        whole = encode_batched(model, feat, lens_t, True)
        monkeypatch.setattr(ragged, 'FRONTEND_ACT_BYTES', 2 * largest_activation_bytes(model.encoder.layers[0], max(E2E_LENS), model.prec))
        assert ragged.frontend_max_batch(model, max(E2E_LENS)) == 2
        parts = encode_batched(model, feat, lens_t, True)
    assert parts[0].shape == whole[0].shape and torch.equal(parts[1], whole[1]) and torch.equal(parts[2], whole[2])
    ref = _reference(1, sd, feat, list(E2E_LENS))
    e_whole, e_parts = _errors(ref, whole[0], whole[3], whole[2]), _errors(ref, parts[0], parts[3], parts[2])
    print('RATIO chunks of 2: e_chunked %.3e e_whole %.3e' % (e_parts, e_whole))
    assert e_parts <= 2 * e_whole + 1e-6
    for u in range(3):
        n = int(parts[2][u])
        assert (parts[0][u, n:] == 0).all() and (parts[3][u, n:] == 0).all()


@pytest.mark.gpu
def test_rows_without_frames():
    """A row shorter than time_div has no frame behind the front-end: allowed beside others (all zeros, lengths 0); a batch
    in which no row has one is refused."""
    from src.decode import encode_batched
    model, sd, feat, _ = _model(1, (9, 3, 6), 'fp32')
    with torch.no_grad():
        enc, enc_len, tlen, ctc = encode_batched(model, feat, torch.tensor((9, 3, 6)).cuda(), True)
        assert enc_len.tolist() == [1, 0, 0] and tlen.tolist() == [1, 0, 1]
        assert (enc[1] == 0).all() and (ctc[1] == 0).all()
        for u, n in ((0, 9), (2, 6)):                  # the rows beside it are what they are without it (|enc| <= 1, fp32)
            ref = encoder_f64(sd, enc_cfg(1), feat[u, :n].cpu())
            assert float((enc[u, :1].double().cpu() - ref[0]).abs().max()) <= 1e-4
        with pytest.raises(ValueError):
            encode_batched(model, feat[:, :3], torch.tensor((3, 2, 1)).cuda(), True)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_beam_decoder_batch_encode_on_a_vgg_model():
    from src.decode import BeamDecoder
    from test_hip_ctc_beam import SCORE_TOL
    model, sd, feat, lens = _model(1)
    bd = BeamDecoder(model, None, BEAM, 0.0, 1.0, ctc_weight=0.3, batch_encode=True)
    msg = bd.create_msg()
    assert any('batched' in line for line in msg) and not any('fell back' in line for line in msg)
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
    for u in range(3):
        assert [h.outIndex for h in got[u]] == [h for h, _ in want[u]]
        for h, (_, s) in zip(got[u], want[u]):
            assert abs(h.avgScore() - s) <= SCORE_TOL * max(1.0, abs(s) / 20)
