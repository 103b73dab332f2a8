"""The acoustic front-end kernels (csrc/frontend.hip: asr_fbank, asr_delta_stack, asr_specaug, asr_specaug_ws) against the float64
restatements of tests/test_frontend_reference.py, through the C entry points (src.hipabi), at the edges: frame counts at hop
multiples, utterances shorter than a window / a filter / a mask, lengths 0, 1 and beyond the padded extent, silent and
saturating input, the 40-bin configuration, every length class of the device-side SpecAugment draws.

Conditions on every case: outputs start as NaN (in-place buffers carry a sentinel in their padding); every input, output and
in-place buffer has one guard utterance behind the B that are passed in, NaN in the inputs and NaN / sentinel in the outputs, which
must come back untouched - a wrong index lands there and is caught by value.

Bounds (none is measured on a kernel)
  asr_fbank        |got - ref| <= 0.0869 * 4 E32 * ||frame||_2 sum_f fb[m,f] / mel64 + 2e-6 where mel64 >= 1e-4 and the reference is
                   not clamped (E32: the float32 transcription's error, test_frontend_reference.py); clamped elements agree to
                   1e-6; silence is exactly 0; the loud signal exactly 1 wherever mel64 >= 10.5; rows >= flen exactly 0;
                   utterances below win/2 + 1 samples: finite, in [0, 1], zero rows behind flen, no comparison.
  asr_delta_stack  taps * 2^-24 * sum_j |filt_j x| per element; rows >= len exactly 0.
  SpecAugment      draws_out == specaug_draws; untouched elements bit-identical; fills within 2 ulp (fp32) of the float64 means;
                   the two entries within 1 ulp of each other.
Every case prints a RATIO line (largest error / bound) before it asserts.

Measured on the MI355X, worst error / bound per family: asr_fbank 0.046 ((1025, 400, 160, 80), hop batch, step; the 2e-6 term
carries the bound there, the errors are one ulp of the output), no judged signal loses an element to the bound's conditions;
asr_delta_stack 0.42 (order 1, F 80, T 64); SpecAugment fills 0.56 ulp of the float64 mean at worst (bound 2), the two entries
within 1 ulp of each other on every case."""
import ctypes

import numpy as np
import pytest
import torch

import test_frontend_reference as R

gpu = pytest.mark.gpu
ULP32 = 2.0 ** -23
U24 = 2.0 ** -24
ASR_E_ARG = -1
NAN = float('nan')


def _H():
    from src import hipabi as H
    return H


def _rc(name, *args):
    """The entry point's return code (H.call raises on a non-zero one)."""
    H = _H()
    return getattr(H.lib(), name)(*args)


# =================================================================================================================================
# asr_fbank
# =================================================================================================================================
def _fbank_call(cfg, waves, call_lens, N, T, preemph=R.PREEMPH, n_fft=None):
    """-> (rc, out (B+1, T, nmel) on the host).  waves: B float32 arrays; padding and the guard utterance are NaN."""
    H = _H()
    cfg_n_fft, win, hop, nmel = cfg
    table, fb, window = R.tables(cfg_n_fft, win, nmel)
    n_fft = cfg_n_fft if n_fft is None else n_fft
    B = len(waves)
    wav = torch.full((B + 1, N), NAN)
    for b, w in enumerate(waves):
        wav[b, :len(w)] = torch.from_numpy(w)
    lens = torch.tensor(list(call_lens) + [N], dtype=torch.int64)
    out = torch.full((B + 1, T, nmel), NAN).cuda()
    nbytes = H.lib().asr_fbank_workspace_bytes(B, T, win, n_fft)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    wav_d, lens_d = wav.cuda(), lens.cuda()
    tb, fbd, wd = torch.from_numpy(table).cuda(), torch.from_numpy(fb).cuda(), torch.from_numpy(window).cuda()
    rc = _rc('asr_fbank', H.ptr(wav_d), H.ptr(lens_d), H.ptr(out), H.ptr(tb), H.ptr(fbd), H.ptr(wd), B, N, T, win, hop, n_fft, nmel,
             preemph, R.REF_DB, R.MIN_DB, H.ptr(ws), nbytes, H.stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu()


@gpu
@pytest.mark.parametrize('ci,bi', R.FBANK_CASES)
def test_fbank_vs_float64(ci, bi):
    cfg = R.FBANK_CONFIGS[ci]
    n_fft, win, hop, nmel = cfg
    for kind in R.FBANK_SIGNALS:
        c = R.fbank_case(ci, bi, kind)
        N, B = c['N'], len(c['lens'])
        T = R.n_frames(N, hop) + 1                          # one row that belongs to no utterance
        rc, out = _fbank_call(cfg, c['waves'], c['call_lens'], N, T)
        assert rc == 0
        assert torch.isnan(out[B]).all(), 'the guard utterance behind the output was written'
        got = out[:B].double().numpy()
        assert np.isfinite(got).all(), 'NaN left in (or read into) the output'
        worst, n_valid, n_out = 0.0, 0, 0
        for b, (n, (ref, mel, scale)) in enumerate(zip(c['lens'], c['refs'])):
            flen = R.n_frames(n, hop)
            assert (got[b, flen:] == 0.0).all(), (c['name'], b, 'rows behind the utterance')
            g = got[b, :flen]
            assert g.shape == ref.shape
            if n <= win // 2:                                # reflection is not single-valued here: no comparison
                assert ((g >= 0.0) & (g <= 1.0)).all()
                continue
            if kind == 'zeros':
                assert (g == 0.0).all(), (c['name'], b)
                continue
            if kind == 'loud':
                assert (g[mel >= R.LOUD_MEL] == 1.0).all(), (c['name'], b)
            jd = R.judged(ref, mel)
            err = np.abs(g - ref)
            assert (err[~jd] <= 1e-6).all(), (c['name'], b, 'clamped elements', float(err[~jd].max()))
            n_valid += g.size
            n_out += int((~jd).sum())
            if jd.any():
                bound = R.SLOPE * 4 * R.E32 * scale[jd] / mel[jd] + 2e-6
                ratio = err[jd] / bound
                worst = max(worst, float(ratio.max()))
                assert (ratio <= 1.0).all(), (c['name'], b, float(ratio.max()), float(err[jd].max()))
        share = n_out / max(n_valid, 1)
        print('RATIO fbank %-44s worst err / bound %.4f  excluded %d of %d (%.2f %%)' % (c['name'], worst, n_out, n_valid, 100 * share))
        if kind in R.JUDGED_SIGNALS:
            assert share <= 0.02
        if c['call_lens'] != c['lens']:
            # an utterance handed a length beyond the padded extent gives exactly the rows of the padded extent
            rc2, out2 = _fbank_call(cfg, c['waves'], c['lens'], N, T)
            assert rc2 == 0 and torch.equal(out2[:B], out[:B])


@gpu
def test_fbank_refuses_even_n_fft():
    cfg = (65, 24, 8, 7)
    w = [R.fbank_signal('noise', 0, 50, 1)]
    for n_fft in (64, 66):
        rc, out = _fbank_call(cfg, w, [50], 50, 8, n_fft=n_fft)
        assert rc == ASR_E_ARG
        assert torch.isnan(out).all(), 'a refused call wrote its output'
    rc, out = _fbank_call(cfg, w, [50], 50, 8)
    assert rc == 0 and not torch.isnan(out[0]).any()


@gpu
@pytest.mark.parametrize('nmel,frame_length', [(80, 25), (40, 25), (80, 20)])
def test_extract_audio_feature_frame_lengths(nmel, frame_length):
    """ExtractAudioFeature at the shipped configurations: flen = max(0, 1 + (n-1)//hop), and the module gives what the entry gives."""
    from src.audio import ExtractAudioFeature
    fe = ExtractAudioFeature(num_mel_bins=nmel, frame_length=frame_length).cuda()
    hop = fe.hop
    lens = [0, 1, 2, hop - 1, hop, hop + 1, 3 * hop - 1, 3 * hop, 3 * hop + 1, 4 * hop + 3]
    N = max(lens)
    waves = [R.fbank_signal('tone+noise', b, n, 5) for b, n in enumerate(lens)]
    wav = torch.zeros(len(lens), N)
    for b, w in enumerate(waves):
        wav[b, :len(w)] = torch.from_numpy(w)
    out, flen = fe(wav.cuda(), torch.tensor(lens).cuda())
    assert flen.cpu().tolist() == [R.n_frames(n, hop) for n in lens]
    T = R.n_frames(N, hop)
    assert out.shape == (len(lens), T, nmel)
    rc, direct = _fbank_call((fe.n_fft, fe.win, hop, nmel), waves, lens, N, T, preemph=0.97)
    assert rc == 0 and torch.equal(direct[:len(lens)], out.cpu())
    for b, n in enumerate(lens):
        assert float(out[b, R.n_frames(n, hop):].abs().sum()) == 0.0


# =================================================================================================================================
# asr_delta_stack
# =================================================================================================================================
def _delta_filters(order, window):
    from src.audio import delta_filters
    if order == 0:
        return np.ones((1, 1), dtype=np.float32)
    return delta_filters(order, window)


def _delta_lens(T, taps):
    pad = (taps - 1) // 2
    want = [0, 1, pad, pad + 1, taps, T]
    lens = [T + 7] + [n for n in want if n <= T]               # the over-long one is not the last utterance
    return lens


@gpu
@pytest.mark.parametrize('order,window', [(0, 0), (1, 2), (2, 2), (2, 3)])
@pytest.mark.parametrize('F', [1, 40, 80])
@pytest.mark.parametrize('T', [1, 9, 64])
def test_delta_stack_vs_float64(order, window, F, T):
    H = _H()
    filt = _delta_filters(order, window)
    C, taps = filt.shape
    lens = _delta_lens(T, taps)
    B = len(lens)
    g = np.random.Generator(np.random.PCG64([order, window, F, T]))
    x = g.standard_normal((B + 1, T, F)).astype(np.float32)
    x[0] = (np.arange(T)[:, None] * 1000.0 + np.arange(F)[None, :]).astype(np.float32)      # (t, f) in the value: the layout
    for b, n in enumerate(lens):
        x[b, min(n, T):] = 1e30 * (1 if b % 2 else -1)                                    # garbage in the padding
    x[B] = NAN
    out = torch.full((B + 1, T, C * F), NAN).cuda()
    xd = torch.from_numpy(x).cuda()
    ld = torch.tensor(lens + [T], dtype=torch.int64).cuda()
    fd = torch.from_numpy(filt).cuda()
    rc = _rc('asr_delta_stack', H.ptr(xd), H.ptr(ld), H.ptr(out), H.ptr(fd), B, T, F, C, taps, H.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    out = out.cpu()
    assert torch.isnan(out[B]).all(), 'the guard utterance behind the output was written'
    got = out[:B].double().numpy()
    assert np.isfinite(got).all()
    worst = 0.0
    for b, n in enumerate(lens):
        ref = R.delta64(x[b], n, filt)
        mag = R.delta64(np.abs(x[b].astype(np.float64)), n, np.abs(filt))
        nn = min(n, T)
        assert (got[b, nn:] == 0.0).all(), (b, n)
        err = np.abs(got[b, :nn] - ref[:nn])
        bound = taps * U24 * mag[:nn]
        assert (err <= bound).all(), (b, n, float(err.max()))
        if nn:
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    # layout: static channel of utterance 0 is the encoded map itself, channel-major behind it
    assert np.array_equal(got[0, :, :F], x[0].astype(np.float64))
    print('RATIO delta order %d window %d F %2d T %2d: worst err / bound %.4f' % (order, window, F, T, worst))


# =================================================================================================================================
# SpecAugment
# =================================================================================================================================
def _specaug_call(entry, x, lens, D, seed, draws_in=None, B=R.SA_B, ws_bytes=None, ws_offset=0):
    """x (B+1, T, D) float32 host array (copied), lens (B) -> (rc, x after (host), draws_out (B+1, 6) host)."""
    H = _H()
    xd = torch.from_numpy(x.copy()).cuda()
    ld = torch.tensor(list(lens) + [R.SA_T], dtype=torch.int64).cuda()
    dout = torch.full((B + 1, 6), -777, dtype=torch.int32).cuda()
    din = None if draws_in is None else torch.tensor(draws_in, dtype=torch.int32).cuda()
    if entry == 'asr_specaug':
        rc = _rc(entry, H.ptr(xd), H.ptr(ld), H.ptr(din), H.ptr(dout), B, R.SA_T, D, R.SA_TMASK, R.SA_FMASK, seed, H.stream_ptr())
    else:
        need = H.lib().asr_specaug_workspace_bytes(B)
        ws = torch.zeros(need + 64, dtype=torch.uint8, device='cuda')
        p = ctypes.c_void_p(ws.data_ptr() + ws_offset)
        rc = _rc(entry, H.ptr(xd), H.ptr(ld), H.ptr(din), H.ptr(dout), B, R.SA_T, D, R.SA_TMASK, R.SA_FMASK, seed, p,
                 need if ws_bytes is None else ws_bytes, H.stream_ptr())
    torch.cuda.synchronize()
    return rc, xd.cpu().numpy(), dout.cpu().numpy()


def _ulps(a, b):
    """distance in float32 ulps of b (both float32-representable or float64 references)."""
    return np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) / (ULP32 * np.maximum(np.abs(np.asarray(b, dtype=np.float64)), 2.0 ** -126))


def _specaug_input(D, seed, lens):
    x = R.specaug_input(D, seed)
    for b, n in enumerate(lens):
        x[b, min(n, R.SA_T):] = R.SA_SENTINEL
    return x


def _judge_specaug(name, x, lens, D, applied, got, dout, want_draws):
    """got / dout of one entry against specaug64 on the draws `applied` (inside the utterance); -> worst ulp distance."""
    B = len(lens)
    assert np.array_equal(got[B], x[B]), 'the guard utterance was written'
    assert (dout[B] == -777).all()
    assert np.array_equal(dout[:B], np.array(want_draws, dtype=np.int32)), (name, 'draws_out')
    worst = 0.0
    for b, n in enumerate(lens):
        nn = min(n, R.SA_T)
        assert np.array_equal(got[b, nn:], x[b, nn:]), (name, b, 'padding')
        if nn == 0:
            continue
        t, t0, tend, f, f0, fend = applied[b]
        ref, m1, m2 = R.specaug64(x[b], nn, applied[b])
        fmask = np.zeros((nn, D), dtype=bool)
        tmask = np.zeros((nn, D), dtype=bool)
        if f != 0:
            fmask[:, f0:fend] = True
        if t != 0:
            tmask[t0:tend] = True
        tmask &= ~fmask
        free = ~(fmask | tmask)
        assert np.array_equal(got[b, :nn][free], x[b, :nn][free]), (name, b, 'unmasked elements')
        for mask, mean, what in ((tmask, m1, 'mean1'), (fmask, m2, 'mean2')):
            if mask.any():
                vals = got[b, :nn][mask]
                assert (vals == vals[0]).all(), (name, b, what)
                u = float(_ulps(vals[0], mean))
                worst = max(worst, u)
                assert u <= 2.0, (name, b, n, what, float(vals[0]), mean, applied[b])
    return worst


@gpu
@pytest.mark.parametrize('D', R.SA_DIMS)
@pytest.mark.parametrize('seed', R.SA_SEEDS)
def test_specaug_device_draws_vs_float64(D, seed):
    lens = R.specaug_lens(shift=D + (seed & 7))
    assert set(lens) == set(R.SA_LEN_CYCLE)
    x = _specaug_input(D, seed, lens)
    want = [R.specaug_draws(b, min(n, R.SA_T), D, R.SA_TMASK, R.SA_FMASK, seed) for b, n in enumerate(lens)]
    res = {}
    for entry in ('asr_specaug', 'asr_specaug_ws'):
        rc, got, dout = _specaug_call(entry, x, lens, D, seed)
        assert rc == 0
        worst = _judge_specaug(entry, x, lens, D, want, got, dout, want)
        print('RATIO %-14s D %3d seed %d: worst fill %.2f ulp of the float64 mean (bound 2)' % (entry, D, seed, worst))
        res[entry] = (got, dout)
    assert np.array_equal(res['asr_specaug'][1], res['asr_specaug_ws'][1])
    assert float(_ulps(res['asr_specaug'][0][:R.SA_B], res['asr_specaug_ws'][0][:R.SA_B]).max()) <= 1.0


def _recorded_rows(g5, D):
    """Caller-supplied draws for 16 utterances: g5 rows, no time mask, no frequency mask, bands over the whole
    utterance, and one row each that reaches behind the utterance, behind D, and has t0 > tend."""
    rows = [tuple(int(v) for v in dr) for dr in g5['aug_draws']][:4]          # drawn for T = len(aug_in), D = 160: clamped below that
    rows += [(0, 3, 9, 5, 1, 4), (7, 2, 6, 0, 1, 5), (0, 0, 0, 0, 0, 0),
             (R.SA_T, 0, R.SA_T, 5, 2, 3),                    # every row of any utterance
             (5, 1, 3, D, 0, D),                              # every bin
             (R.SA_T, 0, R.SA_T, D, 0, D),
             (30, 5, 90, 3, 1, 2),                            # tend > len
             (4, 1, 2, 200, D - 1, D + 40),                   # fend > D
             (9, 12, 4, 6, 5, 2),                             # t0 > tend, f0 > fend
             (3, -5, 2, 4, -2, 1)]                            # negative starts
    while len(rows) < R.SA_B:
        rows.append(rows[len(rows) % 7 + 3])
    return rows[:R.SA_B]


@gpu
@pytest.mark.parametrize('D', [8, 40, 160])
def test_specaug_recorded_draws_vs_float64(golden_dir, D):
    import os
    g5 = np.load(os.path.join(golden_dir, 'g5_frontend.npz'))
    rows = _recorded_rows(g5, D)
    worst_all = 0.0
    for shift in (0, 4):
        lens = R.specaug_lens(shift)
        x = _specaug_input(D, 11 + shift, lens)
        applied = [R.clamp_draws(dr, min(n, R.SA_T), D) for dr, n in zip(rows, lens)]
        res = {}
        for entry in ('asr_specaug', 'asr_specaug_ws'):
            rc, got, dout = _specaug_call(entry, x, lens, D, 0, draws_in=rows)
            assert rc == 0
            worst_all = max(worst_all, _judge_specaug(entry, x, lens, D, applied, got, dout, applied))
            res[entry] = got
        assert float(_ulps(res['asr_specaug'][:R.SA_B], res['asr_specaug_ws'][:R.SA_B]).max()) <= 1.0
    print('RATIO specaug recorded draws D %3d: worst fill %.2f ulp of the float64 mean (bound 2)' % (D, worst_all))


@gpu
def test_specaug_g5_draws_at_full_length(golden_dir):
    """The recorded reference draws on the fixture utterance, both entries, against specaug64 (pinned to the fixture's outputs)."""
    import os
    H = _H()
    g5 = np.load(os.path.join(golden_dir, 'g5_frontend.npz'))
    x0 = g5['aug_in']
    T, D = x0.shape
    draws = g5['aug_draws'].astype(np.int32)
    nb = draws.shape[0]
    x = np.full((nb + 1, T + 3, D), R.SA_SENTINEL, dtype=np.float32)
    x[:nb, :T] = x0
    for entry in ('asr_specaug', 'asr_specaug_ws'):
        xd = torch.from_numpy(x.copy()).cuda()
        ld = torch.tensor([T] * (nb + 1), dtype=torch.int64).cuda()
        din = torch.from_numpy(draws).cuda()
        args = [H.ptr(xd), H.ptr(ld), H.ptr(din), None, nb, T + 3, D, 40, 27, 0]
        if entry == 'asr_specaug_ws':
            ws = torch.zeros(H.lib().asr_specaug_workspace_bytes(nb), dtype=torch.uint8, device='cuda')
            args += [H.ptr(ws), ws.numel()]
        assert _rc(entry, *args, H.stream_ptr()) == 0
        torch.cuda.synchronize()
        got = xd.cpu().numpy()
        assert np.array_equal(got[nb], x[nb]) and np.array_equal(got[:nb, T:], x[:nb, T:])
        for i in range(nb):
            ref, _, _ = R.specaug64(x0, T, draws[i])
            changed = ref != x0.astype(np.float64)
            assert np.array_equal(got[i, :T][~changed], x0[~changed])
            assert float(_ulps(got[i, :T][changed], ref[changed]).max()) <= 2.0
            np.testing.assert_allclose(got[i, :T], g5['aug_out%d' % i], atol=2e-6)


@gpu
def test_specaug_ws_refuses_a_bad_work_area():
    D, seed = 40, 7
    lens = R.specaug_lens()
    x = _specaug_input(D, seed, lens)
    need = _H().lib().asr_specaug_workspace_bytes(R.SA_B)
    assert need == R.SA_B * 16 * 2 * 8
    for kw in ({'ws_bytes': need - 1}, {'ws_bytes': 0}, {'ws_offset': 4}, {'ws_offset': 1}):
        rc, got, dout = _specaug_call('asr_specaug_ws', x, lens, D, seed, **kw)
        assert rc == ASR_E_ARG, kw
        assert np.array_equal(got, x) and (dout == -777).all(), kw
    rc, got, dout = _specaug_call('asr_specaug_ws', x, lens, D, seed, ws_offset=8)
    assert rc == 0 and not np.array_equal(got, x)


@gpu
def test_modules_give_what_the_entry_points_give():
    """Augment on utterances shorter than its time mask, and create_transform with feat_dim 40 (the VGG models' channel width)."""
    from src.audio import Augment, create_transform
    H = _H()
    D = 40
    lens = R.specaug_lens()
    x = _specaug_input(D, 3, lens)
    aug = Augment().cuda()
    xd = torch.from_numpy(x[:R.SA_B].copy()).cuda()
    out, _ = aug(xd, torch.tensor(lens).cuda())
    seed = (aug.seed * 1000003 + aug.calls) & 0xFFFFFFFFFFFF
    rc, direct, dout = _specaug_call('asr_specaug_ws', x, lens, D, seed)
    assert rc == 0 and np.array_equal(out.cpu().numpy(), direct[:R.SA_B])
    want = [R.specaug_draws(b, min(n, R.SA_T), D, 40, 27, seed) for b, n in enumerate(lens)]
    assert np.array_equal(dout[:R.SA_B], np.array(want, dtype=np.int32))
    assert any(0 < n < 40 and w[0] > 0 and w[2] > w[1] for n, w in zip(lens, want)), 'no short utterance drew a time mask'

    fe, dim = create_transform({'feat_type': 'fbank', 'feat_dim': 40, 'delta_order': 2, 'apply_cmvn': False, 'augment': True}, 'train')
    assert dim == 120
    fe = fe.cuda()
    wlens = [4 * 160 + 1, 30 * 160, 201, 45 * 160 + 7]
    N = max(wlens)
    waves = [R.fbank_signal('tone+noise', b, n, 9) for b, n in enumerate(wlens)]
    wav = torch.zeros(len(wlens), N)
    for b, w in enumerate(waves):
        wav[b, :len(w)] = torch.from_numpy(w)
    feat, flen = fe(wav.cuda(), torch.tensor(wlens).cuda())
    assert flen.cpu().tolist() == [R.n_frames(n, 160) for n in wlens] and feat.shape == (4, R.n_frames(N, 160), 120)
    # the same chain through the entry points
    T = R.n_frames(N, 160)
    rc, mel = _fbank_call((1025, 400, 160, 40), waves, wlens, N, T, preemph=0.97)
    assert rc == 0
    from src.audio import delta_filters
    filt = torch.from_numpy(delta_filters(2, 2)).cuda()
    mel_d = mel[:4].contiguous().cuda()
    fl = torch.tensor([R.n_frames(n, 160) for n in wlens], dtype=torch.int64).cuda()
    st = torch.full((4, T, 120), NAN).cuda()
    H.call('asr_delta_stack', H.ptr(mel_d), H.ptr(fl), H.ptr(st), H.ptr(filt), 4, T, 40, 3, filt.shape[1], H.stream_ptr())
    ws = torch.zeros(H.lib().asr_specaug_workspace_bytes(4), dtype=torch.uint8, device='cuda')
    aug_seed = 1                                       # the first call of a fresh Augment(seed=0)
    dout = torch.zeros(4, 6, dtype=torch.int32).cuda()
    H.call('asr_specaug_ws', H.ptr(st), H.ptr(fl), None, H.ptr(dout), 4, T, 120, 40, 27, aug_seed, H.ptr(ws), ws.numel(), H.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(st.cpu(), feat.cpu())
    want = [R.specaug_draws(b, R.n_frames(n, 160), 120, 40, 27, aug_seed) for b, n in enumerate(wlens)]
    assert dout.cpu().tolist() == [list(w) for w in want]
