"""asr_cmvn (csrc/frontend.hip) against the float64 restatement, the case table and the bound of tests/test_cmvn_reference.py, through
the C entry point (src.hipabi), and the CMVN module / create_transform(apply_cmvn=True) against the explicit chain of entry points.

Conditions on every case, as in tests/test_hip_frontend_vs_float64.py: one guard utterance of NaN behind the B that are passed
(x, and stats_out) which must come back untouched; a sentinel in the padding rows t >= len which must come back bit-identical;
a RATIO line (largest error / bound) printed before the assertion.

Per recipe: `integer` bit for bit against cmvn64 rounded to float32; `normal`, `clamped`, `jitter` inside
      |y - y64| <= 2^-24 |y64| + 70 n 2^-53 (max_t|x_t| / (eps + std64)) (1 + |y64|)
(derived in test_cmvn_reference.py from the Welford / Chan scheme, not measured); constant columns exactly 0; a single-frame
utterance NaN in its one valid row, as the fixture shows for the reference; len <= 0 untouched.  stats_out within one float32 ulp of
the float64 mean and std (0 for len <= 0, NaN std for len == 1), and accepted as NULL with the same output; two calls on the same
input bit-identical.  A correctly rounded result can reach a ratio of 1: the first term of the bound is the rounding itself.

Measured on the MI355X, worst error / bound per recipe: integer 0.75 (n == 2 and 3, where y is no multiple of 1/2; 0.0008 from
n == 4 on), normal 0.997, clamped 0.998 (the final rounding), jitter 0.70; stats_out 0.50 ulp at worst."""
import ctypes

import numpy as np
import pytest
import torch

import test_cmvn_reference as R
import test_frontend_reference as FR

gpu = pytest.mark.gpu
ASR_E_ARG = -1
NAN = float('nan')
ULP32 = 2.0 ** -23


def _H():
    from src import hipabi as H
    return H


def _cmvn_call(x, lens, B, T, D, eps=R.EPS, stats=True, ws_bytes=None, ws_offset=0, null=(), dims=None):
    """x (B + 1, T, D) float32 host array (copied), lens (B) -> (rc, x after (host), stats (B + 1, 2, D) host or None)."""
    H = _H()
    xd = torch.from_numpy(np.array(x)).cuda()
    ld = torch.tensor(list(lens) + [T], dtype=torch.int64).cuda()
    sd = torch.full((B + 1, 2, D), NAN).cuda() if stats else None
    need = H.lib().asr_cmvn_workspace_bytes(B, D)
    ws = torch.full((need // 8 + 8,), NAN, dtype=torch.float64, device='cuda')       # the work area's contents do not matter
    wp = ctypes.c_void_p(ws.data_ptr() + ws_offset)
    cB, cT, cD = dims if dims is not None else (B, T, D)
    rc = H.lib().asr_cmvn(None if 'x' in null else H.ptr(xd), None if 'lens' in null else H.ptr(ld), H.ptr(sd), cB, cT, cD, eps,
                          None if 'ws' in null else wp, need if ws_bytes is None else ws_bytes, H.stream_ptr())
    torch.cuda.synchronize()
    return rc, xd.cpu().numpy(), None if sd is None else sd.cpu().numpy()


def _ulps(a, b):
    b = np.asarray(b, dtype=np.float64)
    return np.abs(np.asarray(a, dtype=np.float64) - b) / (ULP32 * np.maximum(np.abs(b), 2.0 ** -126))


@gpu
@pytest.mark.parametrize('si,name', R.CMVN_CASES)
def test_cmvn_vs_float64(si, name):
    c = R.cmvn_case(si, name)
    B, T, D, lens = len(c['lens']), c['T'], c['D'], c['lens']
    assert _H().lib().asr_cmvn_workspace_bytes(B, D) == B * R.CM_SPLIT * 2 * D * 8
    rc, got, st = _cmvn_call(c['x'], lens, B, T, D)
    assert rc == 0
    assert np.isnan(got[B]).all() and np.isnan(st[B]).all(), 'the guard utterance was written'
    # stats_out first (it does not depend on the output being right), then the output
    worst_st = 0.0
    for b, n in enumerate(lens):
        nn = min(n, T)
        if nn == 0:
            assert (st[b] == 0.0).all(), (b, 'stats_out of an empty utterance')
            continue
        u = _ulps(st[b, 0], c['mean'][b])
        u[c['mean'][b] == 0.0] = np.abs(st[b, 0][c['mean'][b] == 0.0])
        assert (u <= 1.0).all(), (c['name'], b, 'mean', float(u.max()))
        if nn == 1:
            assert np.isnan(st[b, 1]).all(), (b, 'std of a single frame')
            continue
        zero = c['std'][b] == 0.0
        assert (st[b, 1][zero] == 0.0).all()
        us = _ulps(st[b, 1][~zero], c['std'][b][~zero])
        worst_st = max(worst_st, float(u.max()), float(us.max(initial=0.0)))
        assert (us <= 1.0).all(), (c['name'], b, 'std', float(us.max()))
    worst = R.judge(c, got[:B], 'asr_cmvn')
    print('RATIO cmvn %-24s worst err / bound %.4f   stats_out %.2f ulp (bound 1)' % (c['name'], worst, worst_st))
    # a second call on the same input, and one without stats_out: the same bits
    rc2, got2, st2 = _cmvn_call(c['x'], lens, B, T, D)
    assert rc2 == 0 and np.array_equal(got2, got, equal_nan=True) and np.array_equal(st2, st, equal_nan=True)
    assert torch.equal(torch.from_numpy(got2[:B]).nan_to_num(1e30), torch.from_numpy(got[:B]).nan_to_num(1e30))
    rc3, got3, _ = _cmvn_call(c['x'], lens, B, T, D, stats=False)
    assert rc3 == 0 and np.array_equal(got3, got, equal_nan=True)


@gpu
def test_cmvn_single_frame_is_nan_as_the_fixture_shows(golden_dir):
    """The reference's Delta -> CMVN -> Postprocess on one frame is NaN (g12_cmvn.npz); the kernel gives the same on that very row
    and leaves the padding behind it alone; the three longer fixture utterances, one padded batch, land inside the float32 bound."""
    import os
    g12 = np.load(os.path.join(golden_dir, 'g12_cmvn.npz'))
    k = int(g12['n'])
    lens = [int(g12['len%d' % i]) for i in range(k)]
    assert lens[-1] == 1 and np.isnan(g12['out%d' % (k - 1)]).all()
    T, D = max(lens) + 2, g12['out0'].shape[1]
    x = np.full((k + 1, T, D), R.SENTINEL, dtype=np.float32)
    for i, n in enumerate(lens):
        x[i, :n] = g12['delta%d' % i].transpose(2, 0, 1).reshape(n, D)
    x[k] = NAN
    rc, got, _ = _cmvn_call(x, lens, k, T, D, eps=float(g12['eps']))
    assert rc == 0 and np.isnan(got[k]).all()
    y, mean, std = R.cmvn64(x[:k], lens, eps=float(np.float32(g12['eps'])))
    for i, n in enumerate(lens):
        assert np.array_equal(got[i, n:], x[i, n:])
        if n == 1:
            assert np.isnan(got[i, 0]).all()
            continue
        out = g12['out%d' % i].astype(np.float64)
        assert (np.abs(got[i, :n] - out) <= 2 * R.bound(x[i, :n], y[i, :n], std[i], u=R.U24)).all()     # kernel and reference, each inside it
        assert (np.abs(got[i, :n] - y[i, :n]) <= R.bound(x[i, :n], y[i, :n], std[i])).all()


@gpu
def test_cmvn_refusals_leave_x_alone():
    c = R.cmvn_case(2, 'normal')
    B, T, D, lens = len(c['lens']), c['T'], c['D'], c['lens']
    need = _H().lib().asr_cmvn_workspace_bytes(B, D)
    bad = [{'null': ('x',)}, {'null': ('lens',)}, {'null': ('ws',)},
           {'dims': (0, T, D)}, {'dims': (-1, T, D)}, {'dims': (B, 0, D)}, {'dims': (B, -4, D)}, {'dims': (B, T, 0)}, {'dims': (B, T, -1)},
           {'ws_bytes': need - 1}, {'ws_bytes': 0}, {'ws_offset': 4}, {'ws_offset': 1}]
    for kw in bad:
        rc, got, st = _cmvn_call(c['x'], lens, B, T, D, **kw)
        assert rc == ASR_E_ARG, kw
        assert np.array_equal(got, c['x'], equal_nan=True) and np.isnan(st).all(), kw
    rc, got, st = _cmvn_call(c['x'], lens, B, T, D, ws_offset=8)
    assert rc == 0 and not np.array_equal(got, c['x'], equal_nan=True)
    assert _H().lib().asr_cmvn_workspace_bytes(0, D) == 0 and _H().lib().asr_cmvn_workspace_bytes(B, -3) == 0


@gpu
def test_cmvn_module_gives_what_the_entry_point_gives():
    from src.audio import CMVN
    with pytest.raises(NotImplementedError, match='Only support global mean variance normalization.'):
        CMVN(mode='utterance')
    m = CMVN().cuda()
    assert (m.mode, m.dim, m.eps) == ('global', 2, 1e-10)
    c = R.cmvn_case(5, 'clamped')
    B, T, D, lens = len(c['lens']), c['T'], c['D'], c['lens']
    xd = torch.from_numpy(np.array(c['x'][:B])).cuda()
    out, olens = m(xd, torch.tensor(lens).cuda())
    assert out.data_ptr() == xd.data_ptr() and olens.cpu().tolist() == lens
    rc, direct, _ = _cmvn_call(c['x'], lens, B, T, D)
    assert rc == 0 and np.array_equal(out.cpu().numpy(), direct[:B], equal_nan=True)


def _waves():
    wlens = [4 * 160 + 1, 30 * 160, 201, 45 * 160 + 7, 1]                    # the last one: a single frame
    N = max(wlens)
    waves = [FR.fbank_signal('tone+noise', b, n, 9) for b, n in enumerate(wlens)]
    wav = torch.zeros(len(wlens), N)
    for b, w in enumerate(waves):
        wav[b, :len(w)] = torch.from_numpy(w)
    return wlens, N, wav


@gpu
@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_create_transform_with_cmvn_is_the_chain_of_entry_points(mode):
    """ExtractAudioFeature, Delta, CMVN, Postprocess[, Augment] - the reference's order - and bit for bit what asr_fbank ->
    asr_delta_stack -> asr_cmvn [-> asr_specaug_ws with the first call's seed] give."""
    from src.audio import Augment, CMVN, Delta, ExtractAudioFeature, Postprocess, create_transform, delta_filters
    H = _H()
    fe, dim = create_transform({'feat_type': 'fbank', 'feat_dim': 40, 'delta_order': 2, 'apply_cmvn': True, 'augment': True}, mode)
    want = [ExtractAudioFeature, Delta, CMVN, Postprocess] + ([Augment] if mode == 'train' else [])
    assert [type(s) for s in fe.stages] == want and dim == 120
    fe = fe.cuda()
    wlens, N, wav = _waves()
    nb = len(wlens)
    feat, flen = fe(wav.cuda(), torch.tensor(wlens).cuda())
    T = FR.n_frames(N, 160)
    frames = [FR.n_frames(n, 160) for n in wlens]
    assert flen.cpu().tolist() == frames and feat.shape == (nb, T, 120)
    # the same chain through the entry points
    table, fb, window = FR.tables(1025, 400, 40)
    wd, wl = wav.cuda(), torch.tensor(wlens, dtype=torch.int64).cuda()
    mel = torch.full((nb, T, 40), NAN).cuda()
    nbytes = H.lib().asr_fbank_workspace_bytes(nb, T, 400, 1025)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    tb, fbd, wnd = torch.from_numpy(table).cuda(), torch.from_numpy(fb).cuda(), torch.from_numpy(window).cuda()
    H.call('asr_fbank', H.ptr(wd), H.ptr(wl), H.ptr(mel), H.ptr(tb), H.ptr(fbd), H.ptr(wnd), nb, N, T, 400, 160, 1025, 40,
           0.97, 20.0, -100.0, H.ptr(ws), nbytes, H.stream_ptr())
    filt = torch.from_numpy(delta_filters(2, 2)).cuda()
    fl = torch.tensor(frames, dtype=torch.int64).cuda()
    st = torch.full((nb, T, 120), NAN).cuda()
    H.call('asr_delta_stack', H.ptr(mel), H.ptr(fl), H.ptr(st), H.ptr(filt), nb, T, 40, 3, filt.shape[1], H.stream_ptr())
    cws = torch.empty(H.lib().asr_cmvn_workspace_bytes(nb, 120) // 8, dtype=torch.float64, device='cuda')
    H.call('asr_cmvn', H.ptr(st), H.ptr(fl), None, nb, T, 120, 1e-10, H.ptr(cws), cws.numel() * 8, H.stream_ptr())
    if mode == 'train':
        aws = torch.zeros(H.lib().asr_specaug_workspace_bytes(nb), dtype=torch.uint8, device='cuda')
        H.call('asr_specaug_ws', H.ptr(st), H.ptr(fl), None, None, nb, T, 120, 40, 27, 1, H.ptr(aws), aws.numel(), H.stream_ptr())
    torch.cuda.synchronize()
    got, ref = feat.cpu().numpy(), st.cpu().numpy()
    assert np.array_equal(got, ref, equal_nan=True)
    # what the stage did: the columns of every utterance with two frames or more have mean 0 and, unless constant, std 1
    if mode == 'eval':
        for b, n in enumerate(frames):
            if n == 1:
                assert np.isnan(got[b, 0]).all() and (got[b, 1:] == 0.0).all()
                continue
            v = got[b, :n].astype(np.float64)
            assert np.abs(v.mean(0)).max() < 1e-5 and (got[b, n:] == 0.0).all()
            sd = v.std(0, ddof=1)
            assert ((np.abs(sd - 1.0) < 1e-3) | (sd == 0.0)).all()


@gpu
def test_create_transform_without_cmvn_builds_no_such_stage():
    from src.audio import CMVN, create_transform
    for cfg in ({'apply_cmvn': False}, {}):
        fe, dim = create_transform(dict({'feat_type': 'fbank', 'feat_dim': 40, 'delta_order': 2, 'augment': True}, **cfg), 'train')
        assert [type(s).__name__ for s in fe.stages] == ['ExtractAudioFeature', 'Delta', 'Postprocess', 'Augment'] and dim == 120
        assert not any(isinstance(s, CMVN) for s in fe.modules())
