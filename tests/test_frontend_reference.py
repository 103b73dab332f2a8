"""The yardstick of the acoustic front-end kernels (csrc/frontend.hip): float64 restatements of asr_fbank, asr_delta_stack and
asr_specaug[_ws], the rule of the device-side SpecAugment draws, the case tables, and their own pins.
tests/test_hip_frontend_vs_float64.py imports all of it; nothing here runs a kernel.

  fbank64        a brute-force float64 DFT from the definition (pre-emphasis; numpy `reflect` padding by n_fft//2; frames of n_fft
                 samples every hop; periodic Hann of `win` taps centred in the frame; |X_f|, f = 0..n_fft//2; mel table;
                 20 log10(max(., 1e-5)) - ref_db; clamp((x - min_db) / -min_db, 0, 1)).  Only samples within win/2 of the edges
                 meet a non-zero window tap, so the definition is single-valued for n > win/2.  n <= 1 gives zero rows.
                 Pins: oracle.frontend_oracle.fbank (torch.stft, float32) at the shipped configuration to 2e-5; torch.stft in
                 float64 at two small configurations.
  delta64        out[t, c F + f] = sum_j filt[c, j] x[t + j - pad, f], zero outside [0, len); rows >= len are zero.  Pin: g5.
  specaug64      mean over the valid len x D region -> time band; mean again -> frequency band.  Pin: g5.
  specaug_draws  the device draws of include/asr_hip.h on philox4x32_10 of tests/test_beam_step_reference.py;
  clamp_draws    what the kernels make of caller-supplied draws.
  parent_draws   the rule BEFORE this file existed (t = r0 % Tmask whatever the length; t0 = 0 and tend = r2 % t when
                 len <= t), kept as a restatement only to show what it did to short utterances: the rows of the time band
                 beyond `len` were counted in the second mean (test_parent_rule_misfills_short_utterances).

The fp32 yardstick.  fbank32 evaluates the same two contractions in numpy float32 on the module's own float32 tables (DFT
table, window, mel table), acc += a * b term after term - the plain loop, written with cumsum so that the figure does not
depend on the BLAS underneath numpy.  Over the whole case table below,
      E32 = max |mel32 - mel64| / (||frame||_2 * sum_f fb[m, f])  =  1.41e-6  (at (1025, 320, 160, 80), short batch, tone + noise)
in the pre-log mel domain - the error an honest fp32 implementation makes, table rounding included.  The GPU file bounds the
kernel by 4 * E32 (another accumulation order, MFMA's fp32 splitting), carried through the normalisation's derivative
20 / (100 ln 10) / mel.  The bound is never measured on the kernel.

Excluded share.  The bound applies where mel64 >= 1e-4 and the reference is not clamped; test_case_table_is_judgeable holds
the share of valid elements outside that to 2 % per case on fbank64 alone (measured: 0 for every judged signal)."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import frontend_oracle as FO
from test_beam_step_reference import philox4x32_10

E32 = 1.5e-6           # the measured figure (1.41e-6) rounded up, held by test_e32_is_the_measured_fp32_error
SLOPE = 20.0 / (100.0 * np.log(10.0))          # d out / d ln(mel) = 0.0869
MEL_MIN = 1e-4
LOUD_MEL = 10.5        # mel values from here on are 5 % above the upper clamp (mel = 10): the output is exactly 1
SR = 16000
PREEMPH, REF_DB, MIN_DB = float(np.float32(0.97)), 20.0, -100.0      # the C entry takes floats: the coefficient the kernel is handed


# ---- tables: the module's own construction (src/audio.py::ExtractAudioFeature.__init__) at any n_fft / win ---------------------
@functools.lru_cache(maxsize=None)
def tables(n_fft, win, nmel):
    """-> (dft_table (2 nb, win), mel_fb (nmel, nb), window (win)) float32, as ExtractAudioFeature builds them.  The mel table
    of a small n_fft is built for the sample rate that keeps the shipped bin width (16000 / 1025 Hz), so that its area-normalised
    weights - and with them the level of the mel values - are those of the shipped table."""
    from src.audio import create_mel_filterbank
    nb = n_fft // 2 + 1
    m = np.arange(win, dtype=np.float64) + (n_fft - win) // 2
    ang = 2.0 * np.pi * np.arange(nb, dtype=np.float64)[:, None] * m[None, :] / n_fft
    table = np.concatenate([np.cos(ang), -np.sin(ang)], 0).astype(np.float32)
    fb = create_mel_filterbank(SR * (n_fft - 1) // 1024, n_fft, nmel)
    window = torch.hann_window(win, periodic=True).numpy()
    return table, fb, window


# ---- asr_fbank ------------------------------------------------------------------------------------------------------------------
def n_frames(n, hop):
    return max(0, 1 + (n - 1) // hop)


def frames64(wav, n, n_fft, win, hop, preemph):
    """(T, n_fft) float64: the windowed frames of the pre-emphasised, reflect-padded wave (zero outside the centred window)."""
    T = n_frames(n, hop)
    if n <= 1:
        return np.zeros((T, n_fft))
    x = np.asarray(wav[:n], dtype=np.float64)
    y = np.concatenate([x[:1], x[1:] - preemph * x[:-1]])
    yp = np.pad(y, n_fft // 2, mode='reflect')
    w = np.zeros(n_fft)
    left = (n_fft - win) // 2
    w[left:left + win] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)
    return np.stack([yp[k * hop:k * hop + n_fft] * w for k in range(T)])


@functools.lru_cache(maxsize=None)
def _basis(n_fft):
    return np.exp(-2j * np.pi * np.outer(np.arange(n_fft), np.arange(n_fft // 2 + 1)) / n_fft)      # (n_fft, nb)


def normalise(mel, ref_db, min_db):
    db = 20.0 * np.log10(np.maximum(mel, 1e-5)) - ref_db
    return np.clip((db - min_db) / -min_db, 0.0, 1.0)


def fbank64(wav, n, n_fft, win, hop, fb, preemph=PREEMPH, ref_db=REF_DB, min_db=MIN_DB):
    """-> (out (T, nmel), mel (T, nmel)) float64, T = max(0, 1 + (n-1)//hop); fb (nmel, nb) float64."""
    fr = frames64(wav, n, n_fft, win, hop, preemph)
    mag = np.abs(fr @ _basis(n_fft))                                # (T, nb)
    mel = mag @ np.asarray(fb, dtype=np.float64).T
    return normalise(mel, ref_db, min_db), mel


def fbank32(wav, n, n_fft, win, hop, nmel, preemph=PREEMPH):
    """The pre-log mel values in numpy float32 on the module's float32 tables: frames, frames x table^T, magnitude, x fb^T."""
    table, fb, window = tables(n_fft, win, nmel)
    T = n_frames(n, hop)
    if n <= 1:
        return np.zeros((T, nmel), dtype=np.float32)
    x = np.asarray(wav[:n], dtype=np.float32)
    y = np.concatenate([x[:1], x[1:] - np.float32(preemph) * x[:-1]])
    yp = np.pad(y, n_fft // 2, mode='reflect')
    left = (n_fft - win) // 2
    fr = np.stack([yp[k * hop + left:k * hop + left + win] * window for k in range(T)]).astype(np.float32)
    # acc += a * b in float32, term after term (cumsum adds in order): the plain loop, and the same figures whatever BLAS numpy has
    spec = (fr[:, None, :] * table[None, :, :]).cumsum(-1, dtype=np.float32)[..., -1]
    nb = n_fft // 2 + 1
    mag = np.sqrt(spec[:, :nb] * spec[:, :nb] + spec[:, nb:] * spec[:, nb:])
    return (mag[:, None, :] * fb[None, :, :]).cumsum(-1, dtype=np.float32)[..., -1]


def fbank_scale(wav, n, n_fft, win, hop, fb, preemph=PREEMPH):
    """(T, nmel): ||frame||_2 * sum_f fb[m, f], the scale E32 is stated on."""
    fr = frames64(wav, n, n_fft, win, hop, preemph)
    return np.sqrt((fr * fr).sum(1))[:, None] * np.asarray(fb, dtype=np.float64).sum(1)[None, :]


# case table: configurations x batches of lengths x signals
FBANK_CONFIGS = [(65, 24, 8, 7), (129, 40, 16, 40), (1025, 400, 160, 40), (1025, 400, 160, 80), (1025, 320, 160, 80)]
FBANK_SIGNALS = ['tone+noise', 'noise', 'zeros', 'loud', 'step']
JUDGED_SIGNALS = ('tone+noise', 'noise', 'step')
OVERLONG = 1000


def fbank_batches(n_fft, win, hop):
    """Batches of 3-5 lengths, N = the longest of each; 'over' = utterance 0 is handed N + OVERLONG and must give the rows of N."""
    k = 5
    half = n_fft // 2
    long2 = max(7 * hop + 3, half + 1 + hop)
    return [
        {'name': 'hop', 'lens': [k * hop + 1, k * hop - 1, k * hop, k * hop + 1], 'over': True},
        {'name': 'edges', 'lens': [win // 2 + 1, win, half, half + 1, long2], 'over': False},
        {'name': 'short', 'lens': [0, 1, 2, win // 2, 3 * hop], 'over': False},
    ]


def fbank_signal(kind, b, n, seed):
    """float32 wave of n samples (n >= 0) for utterance b."""
    g = np.random.Generator(np.random.PCG64([seed, b, n]))
    t = np.arange(n) / float(SR)
    noise = g.standard_normal(n)
    if kind == 'tone+noise':
        x = 0.5 * np.sin(2 * np.pi * (200 + 900 * b) * t) + 0.25 * noise
    elif kind == 'noise':
        x = 0.3 * noise
    elif kind == 'zeros':
        x = np.zeros(n)
    elif kind == 'loud':
        x = 1e3 * noise
    elif kind == 'step':
        x = 0.5 + 0.1 * noise                   # the step is at sample 0: y[0] = x[0], y[p] = x[p] - 0.97 x[p-1] behind it
    else:
        raise KeyError(kind)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def fbank_case(ci, bi, kind):
    """One case, computed once: waves (list of float32 arrays at the padded length N), lens, and per utterance the float64
    reference (out, mel, scale) at min(len, N)."""
    n_fft, win, hop, nmel = FBANK_CONFIGS[ci]
    bt = fbank_batches(n_fft, win, hop)[bi]
    lens = list(bt['lens'])
    N = max(lens)
    fb = tables(n_fft, win, nmel)[1].astype(np.float64)
    waves, refs = [], []
    for b, n in enumerate(lens):
        w = fbank_signal(kind, b, n, 1000 * ci + 10 * bi)
        waves.append(w)
        out, mel = fbank64(w, n, n_fft, win, hop, fb)
        refs.append((out, mel, fbank_scale(w, n, n_fft, win, hop, fb)))
    call_lens = list(lens)
    if bt['over']:
        call_lens[0] = N + OVERLONG
    return {'cfg': FBANK_CONFIGS[ci], 'name': '%s %s %s' % (FBANK_CONFIGS[ci], bt['name'], kind), 'N': N, 'lens': lens,
            'call_lens': call_lens, 'waves': waves, 'refs': refs}


FBANK_CASES = [(ci, bi) for ci in range(len(FBANK_CONFIGS)) for bi in range(3)]


def judged(out, mel):
    """Elements the bound applies to: mel64 >= 1e-4 and an unclamped reference."""
    return (mel >= MEL_MIN) & (out > 0.0) & (out < 1.0)


# ---- asr_delta_stack -----------------------------------------------------------------------------------------------------------
def delta64(x, n, filters):
    """x (T, F), n = len, filters (C, taps) -> (T, C F) float64, channel-major; rows >= min(n, T) are zero."""
    x = np.asarray(x, dtype=np.float64)
    filters = np.asarray(filters, dtype=np.float64)
    T, F = x.shape
    C, taps = filters.shape
    pad = (taps - 1) // 2
    n = max(0, min(int(n), T))
    out = np.zeros((T, C * F))
    for t in range(n):
        for c in range(C):
            for j in range(taps):
                tt = t + j - pad
                if 0 <= tt < n:
                    out[t, c * F:(c + 1) * F] += filters[c, j] * x[tt]
    return out


# ---- SpecAugment ---------------------------------------------------------------------------------------------------------------
def specaug64(x, n, draws):
    """x (T, D), n = len, draws = (t, t0, tend, f, f0, fend) inside the utterance -> (out (T, D) float64, mean1, mean2).
    Rows >= min(n, T) are returned as they came."""
    out = np.array(x, dtype=np.float64)
    n = max(0, min(int(n), out.shape[0]))
    t, t0, tend, f, f0, fend = [int(v) for v in draws]
    if n == 0:
        return out, None, None
    v = out[:n]                                   # a view
    mean1 = v.mean()
    if t != 0:
        v[t0:tend] = mean1
    mean2 = v.mean()
    if f != 0:
        v[:, f0:fend] = mean2
    return out, mean1, mean2


def _words(b, seed):
    key = (seed & 0xffffffff, (seed >> 32) & 0xffffffff)
    return philox4x32_10((b, 0, 1, 0), key) + philox4x32_10((b, 0, 2, 0), key)[:2]


def specaug_draws(b, n, D, Tmask, Fmask, seed):
    """The device draws of utterance b with n = min(len, T) frames (include/asr_hip.h)."""
    r = _words(b, seed)
    n = max(int(n), 0)
    t = r[0] % min(Tmask, max(n, 1))
    t0 = r[1] % max(n - t, 1)
    tend = t0 + r[2] % t if t > 0 else t0
    f = r[3] % min(Fmask, D)
    f0 = r[4] % (D - f)
    fend = f0 + r[5] % f if f > 0 else f0
    return (t, t0, tend, f, f0, fend)


def parent_draws(b, n, D, Tmask, Fmask, seed):
    """The rule before: widths drawn below the mask widths whatever n and D are."""
    r = _words(b, seed)
    t = r[0] % Tmask
    t0 = r[1] % (n - t) if n - t > 0 else 0
    tend = t0 + r[2] % t if t > 0 else t0
    f = r[3] % Fmask
    f0 = r[4] % (D - f) if D - f > 0 else 0
    fend = f0 + r[5] % f if f > 0 else f0
    return (t, t0, tend, f, f0, fend)


def parent_means(x, n, draws):
    """mean1 / mean2 as the kernels formed them before: the row sum stops at n, the row count does not."""
    v = np.asarray(x, dtype=np.float64)[:n]
    D = v.shape[1]
    t, t0, tend = draws[:3]
    if t == 0:
        tend = t0
    tot = v.sum()
    mean1 = float(np.float32(tot / (n * D)))
    rowtot = v[t0:min(tend, n)].sum() if tend > t0 else 0.0
    nrow = max(tend - t0, 0) * D
    return mean1, (tot - rowtot + mean1 * nrow) / (n * D)


def clamp_draws(draws, n, D):
    """Caller-supplied draws as the kernels apply them: bands clamped into the utterance, t == 0 / f == 0 empty."""
    t, t0, tend, f, f0, fend = [int(v) for v in draws]
    n = max(int(n), 0)
    t0 = min(max(t0, 0), n)
    tend = min(max(tend, t0), n) if t > 0 else t0
    f0 = min(max(f0, 0), D)
    fend = min(max(fend, f0), D) if f > 0 else f0
    return (t, t0, tend, f, f0, fend)


SA_T, SA_B, SA_TMASK, SA_FMASK = 64, 16, 40, 27
SA_DIMS = [8, 26, 27, 40, 160]
SA_SEEDS = [0, 7, 2 ** 40 + 3]
SA_LEN_CYCLE = [0, 1, 2, 10, 39, 40, 41, 64, 70]
SA_SENTINEL = 9.0


def specaug_lens(shift=0):
    return [SA_LEN_CYCLE[(b + shift) % len(SA_LEN_CYCLE)] for b in range(SA_B)]


def specaug_input(D, seed, rows=SA_B + 1):
    """(rows, T, D) float32 in [0.25, 1.75): a different level per utterance, frame and bin, so that the two means differ
    from each other and from every element.  The last utterance is the guard."""
    g = np.random.Generator(np.random.PCG64([77, D, seed & 0xffff]))
    x = 0.5 + g.random((rows, SA_T, D)) + 0.25 * np.sin(np.arange(SA_T))[None, :, None] * np.cos(np.arange(D))[None, None, :]
    return x.astype(np.float32)


# =================================================================================================================================
# pins
# =================================================================================================================================
@pytest.fixture(scope='module')
def g5(golden_dir):
    return np.load(os.path.join(golden_dir, 'g5_frontend.npz'))


def test_tables_are_the_modules_tables():
    from src.audio import ExtractAudioFeature
    for nmel, fl in ((80, 25), (40, 25), (80, 20)):
        fe = ExtractAudioFeature(num_mel_bins=nmel, frame_length=fl)
        table, fb, window = tables(fe.n_fft, fe.win, nmel)
        assert (fe.n_fft, fe.win, fe.hop) == (1025, 16 * fl, 160)
        assert np.array_equal(fe.dft_table.numpy(), table)
        assert np.array_equal(fe.mel_fb.numpy(), fb)
        assert np.array_equal(fe.window.numpy(), window)


def test_fbank64_agrees_with_the_stft_oracle_at_the_shipped_configuration():
    g = np.random.Generator(np.random.PCG64(9))
    for n in (2000, 1601, 513):                                             # torch.stft refuses n <= n_fft // 2
        t = np.arange(n) / 16000.0
        wav = (0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 3000 * t + 1.0) + 0.05 * g.standard_normal(n)).astype(np.float32)
        fb = tables(1025, 400, 80)[1]
        want = FO.fbank(wav[None, :], fb)[0].numpy().astype(np.float64).T               # (T, 80)
        got, _ = fbank64(wav, n, 1025, 400, 160, fb.astype(np.float64))
        assert got.shape == want.shape == (n_frames(n, 160), 80)
        assert np.abs(got - want).max() < 2e-5, np.abs(got - want).max()


@pytest.mark.parametrize('n_fft,win,hop,nmel', [(65, 24, 8, 7), (129, 40, 16, 40)])
def test_fbank64_agrees_with_float64_stft_at_small_configurations(n_fft, win, hop, nmel):
    g = np.random.Generator(np.random.PCG64(11))
    fb = tables(n_fft, win, nmel)[1].astype(np.float64)
    for n in (n_fft // 2 + 1, 5 * hop, 5 * hop + 1, 211):                   # torch.stft refuses n <= n_fft // 2
        wav = (0.2 * g.standard_normal(n)).astype(np.float32)
        x = torch.from_numpy(wav.astype(np.float64))
        y = torch.cat([x[:1], x[1:] - PREEMPH * x[:-1]])
        spec = torch.stft(y[None], n_fft=n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, dtype=torch.float64),
                          center=True, pad_mode='reflect', onesided=True, return_complex=True)[0]
        mel = spec.abs().numpy().T @ fb.T
        got, gmel = fbank64(wav, n, n_fft, win, hop, fb)
        assert gmel.shape == mel.shape == (n_frames(n, hop), nmel)
        assert np.abs(gmel - mel).max() <= 1e-12 * max(1.0, np.abs(mel).max())
        assert np.abs(got - normalise(mel, REF_DB, MIN_DB)).max() < 1e-10


def test_frame_count():
    assert [n_frames(n, 160) for n in (-3, 0, 1, 2, 160, 161, 162, 320, 321)] == [0, 0, 1, 1, 1, 2, 2, 2, 3]
    for n in (513, 640, 641, 801, 12345, 16000):                              # torch.stft refuses n <= n_fft // 2
        assert FO.fbank(torch.zeros(1, n), tables(1025, 400, 80)[1]).shape[-1] == n_frames(n, 160)


def _e32_of_case(c):
    n_fft, win, hop, nmel = c['cfg']
    worst, worst_rel = 0.0, 0.0
    for w, n, (out, mel, scale) in zip(c['waves'], c['lens'], c['refs']):
        if n <= win // 2 or not scale.size or scale.max() == 0.0:
            continue
        mel32 = fbank32(w, n, n_fft, win, hop, nmel).astype(np.float64)
        worst = max(worst, float((np.abs(mel32 - mel) / scale).max()))
    return worst


def test_e32_is_the_measured_fp32_error():
    """E32 over the whole case table.  The constant is the measured figure rounded up: never below it, never twice it."""
    worst, where = 0.0, None
    for ci, bi in FBANK_CASES:
        for kind in FBANK_SIGNALS:
            e = _e32_of_case(fbank_case(ci, bi, kind))
            if e > worst:
                worst, where = e, fbank_case(ci, bi, kind)['name']
    print('E32 measured %.4e at %s (constant %.1e)' % (worst, where, E32))
    assert 0.5 * E32 < worst <= E32, (worst, where)


def test_case_table_is_judgeable():
    """Per case and on fbank64 alone: silence is exactly 0; the loud signal (white noise of rms 1e3) is exactly 1 wherever its mel
    value clears the clamp by 5 %, which is at least 90 % of every utterance - the area-normalised mel weights sum to 1/15.6
    per filter, so a narrow filter on a quiet bin of one frame stays below mel = 10 even at that level, and those elements are
    judged by the bound like any other; of the judged signals at most 2 % of the valid elements fall outside the bound's
    conditions (mel64 >= 1e-4, unclamped)."""
    for ci, bi in FBANK_CASES:
        n_fft, win, hop, nmel = FBANK_CONFIGS[ci]
        for kind in FBANK_SIGNALS:
            c = fbank_case(ci, bi, kind)
            tot = out_of = 0
            for n, (out, mel, scale) in zip(c['lens'], c['refs']):
                assert out.shape == (n_frames(n, hop), nmel)
                if n <= win // 2:
                    continue
                if kind == 'zeros':
                    assert (out == 0.0).all()
                elif kind == 'loud':
                    sat = mel >= LOUD_MEL                                   # 10 is the clamp; 4 E32 is 1e-5 of it
                    assert (out[sat] == 1.0).all() and sat.mean() >= 0.9, (c['name'], sat.mean())
                else:
                    tot += out.size
                    out_of += int((~judged(out, mel)).sum())
            if kind in JUDGED_SIGNALS:
                assert tot > 0 and out_of <= 0.02 * tot, (c['name'], out_of, tot)


def test_delta64_and_specaug64_match_the_reference_fixtures(g5):
    mel = g5['mel'][0].T                                                      # (T, F)
    for order in (1, 2):
        filt = g5['filters%d' % order].reshape(order + 1, -1)
        np.testing.assert_allclose(delta64(mel, mel.shape[0], filt), g5['post%d' % order], atol=1e-6)
        short = delta64(mel, mel.shape[0] - 9, filt)
        ref = FO.postprocess(FO.delta(g5['mel'][:, :, :mel.shape[0] - 9], filt)).numpy()
        np.testing.assert_allclose(short[:mel.shape[0] - 9], ref, atol=1e-6)
        assert (short[mel.shape[0] - 9:] == 0).all()
    x = g5['aug_in']
    for i, dr in enumerate(g5['aug_draws']):
        out, m1, m2 = specaug64(x, x.shape[0], dr)
        np.testing.assert_allclose(out, g5['aug_out%d' % i], atol=1e-6)
        assert clamp_draws(dr, x.shape[0], x.shape[1]) == tuple(int(v) for v in dr)      # the recorded draws are inside already


def test_delta64_layout_and_edges():
    x = np.arange(5)[:, None] * 100.0 + np.arange(3)[None, :]                # value encodes (t, f)
    out = delta64(x, 4, np.array([[0., 1., 0.], [-1., 0., 1.]]))
    assert out.shape == (5, 6) and (out[4] == 0).all()
    assert np.array_equal(out[:4, :3], x[:4])
    assert np.array_equal(out[:4, 3:], np.array([[100., 101., 102.], [200.] * 3, [200.] * 3, [-200., -201., -202.]]))
    assert (delta64(x, 0, np.ones((2, 3))) == 0).all()
    assert np.array_equal(delta64(x, 12, np.array([[1.0]])), x)              # a length beyond T is T


def test_specaug_draws_known_rows():
    """Seed 7: utterance 1 draws r0 % 40 = 39 and r2 % 39 = 15, utterance 8 draws r3 % 27 = 23 and r5 % 23 = 19 - the rows that,
    under the parent's rule, gave tend = 15 at len = 10 and fend = 19 at D = 16."""
    d1 = specaug_draws(1, 300, 160, 40, 27, 7)
    assert d1[0] == 39 and d1[2] - d1[1] == 15
    d8 = specaug_draws(8, 300, 160, 40, 27, 7)
    assert d8[3] == 23 and d8[5] - d8[4] == 19
    assert parent_draws(1, 10, 160, 40, 27, 7)[:3] == (39, 0, 15)
    assert parent_draws(8, 10, 16, 40, 27, 7)[3:] == (23, 0, 19)
    over = [b for b in range(16) if parent_draws(b, 10, 160, 40, 27, 7)[2] > 10]
    assert over == [1, 3, 9, 10, 11, 13, 14, 15]
    # wherever the reference has draws at all, the rule is the parent's
    for b in range(64):
        for n, D in ((40, 27), (41, 40), (300, 160), (3000, 160)):
            assert specaug_draws(b, n, D, 40, 27, 7) == parent_draws(b, n, D, 40, 27, 7)
    assert specaug_draws(3, 0, 40, 40, 27, 5)[:3] == (0, 0, 0)


def test_specaug_draws_stay_inside_the_utterance():
    for n in (1, 2, 39, 40, 41, 300):
        for D in (1, 8, 26, 27, 40, 160):
            for b in range(4096):
                t, t0, tend, f, f0, fend = specaug_draws(b, n, D, 40, 27, 7)
                assert 0 <= t0 <= tend <= n and 0 <= f0 <= fend <= D, (b, n, D)
                assert t < min(40, n) and f < min(27, D) and tend - t0 <= t and fend - f0 <= f


def test_clamp_draws():
    assert clamp_draws((5, 8, 15, 3, 2, 4), 10, 8) == (5, 8, 10, 3, 2, 4)          # tend > len
    assert clamp_draws((5, 1, 3, 30, 6, 19), 10, 8) == (5, 1, 3, 30, 6, 8)         # fend > D
    assert clamp_draws((5, 7, 3, 3, 2, 4), 10, 8) == (5, 7, 7, 3, 2, 4)            # t0 > tend: empty
    assert clamp_draws((0, 2, 9, 0, 1, 5), 10, 8) == (0, 2, 2, 0, 1, 1)            # t == 0, f == 0: off
    assert clamp_draws((5, -4, 99, 5, -1, 99), 10, 8) == (5, 0, 10, 5, 0, 8)
    assert clamp_draws((5, 3, 4, 5, 3, 4), 0, 8) == (5, 0, 0, 5, 3, 4)


def test_parent_rule_misfills_short_utterances():
    """What the GPU cases at len in {1, 2, 10} would have seen before: the parent's draws reach beyond the utterance and its
    second mean counts rows that are not there.  With the parent's own draws handed to specaug64 (clamped to the rows that
    exist - the fill it did make), mean2 is off by far more than the 2 ulp the GPU file allows; e.g. seed 7, len 10, utterance 1
    fills all ten rows with mean1 and then states their mean as 1.5 mean1.  At len 39 the parent's arithmetic holds (t <= 39 keeps
    tend <= len); those cases differ from it in the draws."""
    x = specaug_input(40, 7)
    m1, m2 = parent_means(x[1], 10, parent_draws(1, 10, 40, 40, 27, 7))
    assert abs(m2 / m1 - 1.5) < 1e-6
    for n in (1, 2, 10):
        bad = 0
        for seed in SA_SEEDS:
            for b in range(SA_B):
                dr = parent_draws(b, n, 40, SA_TMASK, SA_FMASK, seed)
                _, r1, r2 = specaug64(x[b], n, clamp_draws(dr, n, 40))
                p1, p2 = parent_means(x[b], n, dr)
                assert abs(p1 - r1) <= 2.0 ** -23 * abs(r1)
                if dr[2] > n:
                    assert abs(p2 - r2) > 1e-3 * abs(r2), (n, seed, b)
                    bad += 1
                else:
                    assert abs(p2 - r2) <= 2.0 ** -22 * abs(r2)
        assert bad > 0, n
    # len 39: t <= 39 keeps the parent's band inside the utterance; its width is r0 % 40 where the stated rule draws r0 % 39,
    # so the cases of that length differ from the parent in the draws themselves (and in every fill that follows from them)
    differ = sum(parent_draws(b, 39, 40, SA_TMASK, SA_FMASK, seed) != specaug_draws(b, 39, 40, SA_TMASK, SA_FMASK, seed)
                 for seed in SA_SEEDS for b in range(SA_B))
    assert differ > SA_B
