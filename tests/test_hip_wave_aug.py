"""csrc/wave_aug.hip against the float64 restatements, case tables and bounds of tests/test_wave_aug_reference.py, through the C entry
points (src.hipabi), and WaveAugment / create_transform(time_aug=True) against the explicit chain of entry points.

Conditions on every case, as in tests/test_hip_cmvn.py: one guard utterance of NaN behind the B that are passed, which must come back
untouched; a sentinel in the samples n >= len, which must come back bit-identical; whatever a kernel does not own (frames beyond an
utterance's count, the rows of a skipped utterance) stays NaN; a RATIO line (largest error / bound) printed before each assertion;
two calls bit-identical.  Every stage is step-forced: the float64 restatement is fed that kernel's own float32 inputs.

Measured on the MI355X, worst error / bound per stage over all cases: noise 0.95 and resample 0.9995 (both round a float64-accurate
value once: a correctly rounded result reaches 1), stft 0.026, pvoc 0.068, istft 0.026 (their bounds are worst-case norms); the
device draws equal the numpy rule bit for bit, switch rates 0.2986 / 0.3030 / 0.4978 over 4096 utterances."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import test_wave_aug_reference as R

gpu = pytest.mark.gpu
ASR_E_ARG = -1
NAN = float('nan')
F32 = np.float32
SEED = 0x51ED270B1


def _H():
    from src import hipabi as H
    return H


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _lens_dev(lens, N):
    return torch.tensor(list(lens) + [N], dtype=torch.int64).cuda()


def _rates_dev(rates, guard=1.0):
    """(B,) rates -> device (B + 1, 2) with the rate in column 1 (rate_stride 2, offset 1: a stride is exercised); the guard utterance
    carries a legal rate so that only B keeps it out."""
    r = np.zeros((len(rates) + 1, 2), dtype=F32)
    r[:-1, 1] = rates
    r[-1, 1] = guard
    return torch.from_numpy(r).cuda()


def _rp(rd):
    return ctypes.c_void_p(rd.data_ptr() + 4)


def _geom(N, n_fft):
    hop = n_fft // 4
    return hop, 1 + N // hop, n_fft // 2 + 1


def _active(n, N, n_fft, rate):
    return min(max(n, 0), N) > n_fft // 2 and bool(R.rate_ok(F32(rate)))


def _table_dev(n_fft):
    return torch.from_numpy(R.table(n_fft).copy()).cuda()


def _c64(t):
    """device float32 (..., 2) -> host complex128"""
    a = t.cpu().numpy().astype(np.float64)
    return a[..., 0] + 1j * a[..., 1]


def _stft_call(x, lens, rates, N, n_fft):
    H = _H()
    B = len(lens)
    hop, F, nb = _geom(N, n_fft)
    xd, ld, rd, tb = _dev(x), _lens_dev(lens, N), _rates_dev(rates), _table_dev(n_fft)
    spec = torch.full((B + 1, F, nb, 2), NAN, device='cuda')
    rc = H.lib().asr_wave_stft(H.ptr(xd), H.ptr(ld), _rp(rd), 2, H.ptr(tb), H.ptr(spec), B, N, n_fft, H.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu().nan_to_num(1e30), torch.from_numpy(np.array(x)).nan_to_num(1e30)), 'the wave was written'
    return rc, spec


def _pvoc_call(spec32, lens, rates, N, n_fft):
    """spec32 (B + 1, F, nb, 2) float32 host"""
    H = _H()
    B = len(lens)
    hop, F, nb = _geom(N, n_fft)
    sd, ld, rd = _dev(spec32), _lens_dev(lens, N), _rates_dev(rates)
    out = torch.full((B + 1, 2 * F, nb, 2), NAN, device='cuda')
    rc = H.lib().asr_wave_pvoc(H.ptr(sd), H.ptr(ld), _rp(rd), 2, H.ptr(out), B, N, n_fft, H.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


def _istft_call(ospec32, lens, rates, N, n_fft, keep_len, dst0):
    """dst0 (B + 1, stride) float32 host: what dst holds before the call"""
    H = _H()
    B = len(lens)
    od, ld, rd, tb, dd = _dev(ospec32), _lens_dev(lens, N), _rates_dev(rates), _table_dev(n_fft), _dev(dst0)
    rc = H.lib().asr_wave_istft(H.ptr(od), H.ptr(ld), _rp(rd), 2, H.ptr(tb), H.ptr(dd), dst0.shape[1], keep_len, B, N, n_fft, H.stream_ptr())
    torch.cuda.synchronize()
    return rc, dd.cpu().numpy()


def _resample_call(src, lens, rates, x0, N, n_fft):
    H = _H()
    B = len(lens)
    sd, ld, rd, xd = _dev(src), _lens_dev(lens, N), _rates_dev(rates), _dev(x0)
    rc = H.lib().asr_wave_resample(H.ptr(sd), src.shape[1], H.ptr(ld), _rp(rd), 2, H.ptr(xd), B, N, n_fft, H.stream_ptr())
    torch.cuda.synchronize()
    return rc, xd.cpu().numpy()


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


_CASE_RATES = [(n, r) for n in (64, 256, 2048) for r in R.CASE_RATES[n]]


def _spec_inputs(n_fft):
    """The float32 spectrogram batch the vocoder cases read: stft64 of the case's waves rounded to float32 (NaN elsewhere)."""
    c = R.wave_case(n_fft)
    N, B = c['N'], c['B']
    hop, F, nb = _geom(N, n_fft)
    s = np.full((B + 1, F, nb, 2), NAN, dtype=F32)
    for b, n in enumerate(c['lens']):
        m = min(n, N)
        if m > n_fft // 2:
            D = R.stft64(c['x'][b, :m], n_fft)
            s[b, :D.shape[0], :, 0], s[b, :D.shape[0], :, 1] = D.real, D.imag
    return s


# ---- draws and noise ------------------------------------------------------------------------------------------------------------------
@gpu
def test_device_draws_are_the_numpy_rule():
    H = _H()
    B, N, n_fft = 4096, 5000, 2048
    lens = (np.arange(B) % 7 == 3) * 1000 + 1100 * (np.arange(B) % 7 != 3)           # every seventh utterance too short to pad
    ld = torch.from_numpy(lens.astype(np.int64)).cuda()
    out = torch.full((B + 1, 6), NAN, device='cuda')
    rates = torch.full((B + 1, 2), NAN, device='cuda')
    H.call('asr_wave_draws', H.ptr(ld), None, H.ptr(out), H.ptr(rates), B, N, n_fft, SEED, H.stream_ptr())
    torch.cuda.synchronize()
    got, gr = out.cpu().numpy(), rates.cpu().numpy()
    assert np.isnan(got[B]).all() and np.isnan(gr[B]).all()
    raw = R.raw_draws(B, SEED)
    want, wr = R.finish_draws(raw, lens, N, n_fft)
    assert np.array_equal(got[:B], want) and np.array_equal(gr[:B], wr)
    assert (got[:B][lens <= 1024][:, [2, 4]] == 0).all()
    for col, p in ((0, 0.3), (2, 0.3), (4, 0.5)):
        rate = raw[:, col].mean()
        print('RATIO draws switch %d: rate %.4f, %.2f binomial standard deviations from %.1f (bound 4)'
              % (col, rate, abs(rate - p) / np.sqrt(p * (1 - p) / B), p))
        assert abs(rate - p) <= 4 * np.sqrt(p * (1 - p) / B)
    # draws_in: passed through, switches normalised and cleared where they cannot be taken; rates_out may be NULL
    din = np.array([[2, 0.005, 1, 0.8, 1, 4.0], [0, 0.005, 1, 0.4, 1, -13.0], [1, 0.005, 1, 2.0, 0, 1.0], [1, 0, 1, 1.0, 1, 0.0]], dtype=F32)
    l4 = [3000, 3000, 3000, 1024]
    o4 = torch.full((5, 6), NAN, device='cuda')
    l4d, dind = torch.tensor(l4).cuda(), _dev(din)
    H.call('asr_wave_draws', H.ptr(l4d), H.ptr(dind), H.ptr(o4), None, 4, N, n_fft, 0, H.stream_ptr())
    torch.cuda.synchronize()
    w4, _ = R.finish_draws(din, l4, N, n_fft)
    assert np.array_equal(o4.cpu().numpy()[:4], w4) and np.isnan(o4.cpu().numpy()[4]).all()
    assert w4[:, [0, 2, 4]].tolist() == [[1, 1, 1], [0, 0, 0], [1, 1, 0], [1, 0, 0]]


@gpu
@pytest.mark.parametrize('n_fft', [64, 256])
def test_noise_vs_float64(n_fft):
    H = _H()
    c = R.wave_case(n_fft)
    N, B, lens = c['N'], c['B'], c['lens']
    draws = np.zeros((B + 1, 6), dtype=F32)
    draws[:, 0] = (np.arange(B + 1) % 3 != 1)                   # mixed switches
    draws[:, 1] = 0.001 + 0.009 * (np.arange(B + 1) % 5) / 4
    draws[B, 0] = 1

    def run():
        xd, ld, dd = _dev(c['x']), _lens_dev(lens, N), _dev(draws)
        rc = H.lib().asr_wave_noise(H.ptr(xd), H.ptr(ld), H.ptr(dd), B, N, SEED, H.stream_ptr())
        torch.cuda.synchronize()
        return rc, xd.cpu().numpy()
    rc, got = run()
    assert rc == 0 and np.isnan(got[B]).all(), 'the guard utterance was written'
    y64, az = R.noise64(c['x'][:B], lens, draws, SEED)
    worst = 0.0
    for b, n in enumerate(lens):
        m = min(n, N)
        assert _same(got[b, m:], c['x'][b, m:]), (b, 'samples beyond len')
        if draws[b, 0] == 0:
            assert _same(got[b], c['x'][b]), (b, 'a switched-off utterance was touched')
            continue
        err, bnd = np.abs(got[b, :m] - y64[b, :m]), R.noise_bound(y64[b, :m], az[b, :m])
        if m:
            worst = max(worst, float((err / np.maximum(bnd, 1e-300)).max()))
            assert m < 8 or np.abs(got[b, :m] - c['x'][b, :m]).max() > 0
    print('RATIO noise n_fft-case %d: worst err / bound %.4f' % (n_fft, worst))
    assert worst <= 1.0
    rc2, got2 = run()
    assert rc2 == 0 and _same(got2, got)


# ---- the four kernels of a stage, step-forced -------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('n_fft', [64, 256, 2048])
def test_stft_vs_float64(n_fft):
    c = R.wave_case(n_fft)
    N, B, lens = c['N'], c['B'], c['lens']
    hop, F, nb = _geom(N, n_fft)
    rates = np.where(np.arange(B) % 4 == 1, 0.0, 1.0).astype(F32) if n_fft == 64 else np.ones(B, dtype=F32)    # a switched-off neighbour
    rc, spec = _stft_call(c['x'], lens, rates, N, n_fft)
    assert rc == 0
    raw = spec.cpu().numpy()
    assert np.isnan(raw[B]).all(), 'the guard utterance was written'
    got = _c64(spec)
    worst = 0.0
    for b, n in enumerate(lens):
        m = min(n, N)
        if not _active(n, N, n_fft, rates[b]):
            assert np.isnan(raw[b]).all(), (b, 'a skipped utterance was written')
            continue
        nfr = R.n_frames(m, n_fft)
        assert np.isnan(raw[b, nfr:]).all() and np.isfinite(raw[b, :nfr]).all(), (b, 'frames beyond the count')
        D = R.stft64(c['x'][b, :m], n_fft)
        err = np.sqrt((np.abs(got[b, :nfr] - D) ** 2).sum(1))
        bnd = R.stft_bound(c['x'][b, :m], n_fft)
        if R.CASES[n_fft][b][1] == 'zero':
            assert (raw[b, :nfr] == 0).all()
            continue
        ok = bnd > 0
        assert (err[~ok] == 0).all()
        worst = max(worst, float((err[ok] / bnd[ok]).max()))
    print('RATIO stft n_fft %d: worst ||err||_2 / bound %.4f' % (n_fft, worst))
    assert worst <= 1.0
    rc2, spec2 = _stft_call(c['x'], lens, rates, N, n_fft)
    assert rc2 == 0 and _same(spec2.cpu().numpy(), raw)


@gpu
@pytest.mark.parametrize('n_fft,rate', _CASE_RATES)
def test_pvoc_vs_float64(n_fft, rate):
    c = R.wave_case(n_fft)
    N, B, lens = c['N'], c['B'], c['lens']
    hop, F, nb = _geom(N, n_fft)
    s32 = _spec_inputs(n_fft)
    rates = np.full(B, rate, dtype=F32)
    if n_fft == 64:
        rates[4] = 0.0                       # mixed switches: utterance 4 off, its neighbours on
    rc, out = _pvoc_call(s32, lens, rates, N, n_fft)
    assert rc == 0
    raw = out.cpu().numpy()
    assert np.isnan(raw[B]).all(), 'the guard utterance was written'
    got = _c64(out)
    worst = 0.0
    for b, n in enumerate(lens):
        m = min(n, N)
        if not _active(n, N, n_fft, rates[b]):
            assert np.isnan(raw[b]).all(), (b, 'a skipped utterance was written')
            continue
        nfr = R.n_frames(m, n_fft)
        nout = R.out_frames(nfr, rates[b])
        assert np.isnan(raw[b, nout:]).all() and np.isfinite(raw[b, :nout]).all(), (b, nout, 'frames beyond the count')
        D = s32[b, :nfr].astype(np.float64)
        ref, mags, sums = R.pvoc64(D[..., 0] + 1j * D[..., 1], rates[b], with_parts=True)
        if R.CASES[n_fft][b][1] == 'zero':
            assert (raw[b, :nout] == 0).all()
            continue
        err, bnd = np.abs(got[b, :nout] - ref), R.pvoc_bound(mags, sums)
        ok = bnd > 0
        assert (err[~ok] == 0).all()
        worst = max(worst, float((err[ok] / bnd[ok]).max()))
    print('RATIO pvoc n_fft %d rate %.4f: worst err / bound %.4f' % (n_fft, rate, worst))
    assert worst <= 1.0
    rc2, out2 = _pvoc_call(s32, lens, rates, N, n_fft)
    assert rc2 == 0 and _same(out2.cpu().numpy(), raw)


def _ospec_inputs(n_fft, rate):
    """float32 stretched spectrograms (B + 1, 2F, nb, 2): pvoc64 of the float32 inputs of _spec_inputs, rounded."""
    c = R.wave_case(n_fft)
    N, B = c['N'], c['B']
    hop, F, nb = _geom(N, n_fft)
    s32 = _spec_inputs(n_fft)
    o = np.full((B + 1, 2 * F, nb, 2), NAN, dtype=F32)
    for b, n in enumerate(c['lens']):
        m = min(n, N)
        if m > n_fft // 2:
            D = s32[b, :R.n_frames(m, n_fft)].astype(np.float64)
            ref = R.pvoc64(D[..., 0] + 1j * D[..., 1], F32(rate))
            o[b, :ref.shape[0], :, 0], o[b, :ref.shape[0], :, 1] = ref.real, ref.imag
    return o


@gpu
@pytest.mark.parametrize('keep_len', [1, 0])
@pytest.mark.parametrize('n_fft,rate', _CASE_RATES)
def test_istft_vs_float64(n_fft, rate, keep_len):
    c = R.wave_case(n_fft)
    N, B, lens = c['N'], c['B'], c['lens']
    o32 = _ospec_inputs(n_fft, rate)
    rates = np.full(B, rate, dtype=F32)
    if n_fft == 64:
        rates[5] = 0.0
    stride = N if keep_len else 2 * N + 3
    dst0 = np.full((B + 1, stride), R.SENTINEL, dtype=F32)
    dst0[B] = NAN
    rc, got = _istft_call(o32, lens, rates, N, n_fft, keep_len, dst0)
    assert rc == 0 and np.isnan(got[B]).all(), 'the guard utterance was written'
    worst = 0.0
    for b, n in enumerate(lens):
        m = min(n, N)
        if not _active(n, N, n_fft, rates[b]):
            assert _same(got[b], dst0[b]), (b, 'a skipped utterance was written')
            continue
        M = R.out_len(m, rates[b])
        nout = R.out_frames(R.n_frames(m, n_fft), rates[b])
        O = o32[b, :nout].astype(np.float64)
        y, bnd = R.istft64(O[..., 0] + 1j * O[..., 1], M, n_fft, with_bound=True)
        lim = m if keep_len else M
        assert _same(got[b, lim:], dst0[b, lim:]), (b, 'samples beyond the utterance')
        k = min(M, lim)
        assert (got[b, k:lim] == 0).all(), (b, 'zeros from M on')
        assert np.isfinite(got[b, :lim]).all()
        if R.CASES[n_fft][b][1] == 'zero':
            assert (got[b, :lim] == 0).all()
            continue
        err = np.abs(got[b, :k] - y[:k])
        ok = bnd[:k] > 0
        assert (err[~ok] == 0).all()
        worst = max(worst, float((err[ok] / bnd[:k][ok]).max()))
    print('RATIO istft n_fft %d rate %.4f keep_len %d: worst err / bound %.4f' % (n_fft, rate, keep_len, worst))
    assert worst <= 1.0
    rc2, got2 = _istft_call(o32, lens, rates, N, n_fft, keep_len, dst0)
    assert rc2 == 0 and _same(got2, got)


@gpu
@pytest.mark.parametrize('n_fft,rate', _CASE_RATES)
def test_resample_vs_float64(n_fft, rate):
    c = R.wave_case(n_fft)
    N, B, lens = c['N'], c['B'], c['lens']
    rates = np.full(B, rate, dtype=F32)
    if n_fft == 64:
        rates[6] = 0.0
    stride = 2 * N + 5
    src = np.full((B + 1, stride), NAN, dtype=F32)               # NaN beyond M: a tap outside [0, M) would show
    for b, (n, name) in enumerate(R.CASES[n_fft]):
        m = min(n, N)
        M = R.out_len(m, rates[b]) if rates[b] else 0
        src[b, :M] = R.recipe(name, b + 100, M, n_fft)
    rc, got = _resample_call(src, lens, rates, c['x'], N, n_fft)
    assert rc == 0 and np.isnan(got[B]).all(), 'the guard utterance was written'
    worst = 0.0
    for b, n in enumerate(lens):
        m = min(n, N)
        if not _active(n, N, n_fft, rates[b]):
            assert _same(got[b], c['x'][b]), (b, 'a skipped utterance was written')
            continue
        assert _same(got[b, m:], c['x'][b, m:]), (b, 'samples beyond len')
        M = R.out_len(m, rates[b])
        y, bnd = R.resample64(src[b, :M], m, rates[b], with_bound=True)
        assert np.isfinite(got[b, :m]).all()
        if R.CASES[n_fft][b][1] == 'zero':
            assert (got[b, :m] == 0).all()
            continue
        err = np.abs(got[b, :m] - y)
        ok = bnd > 0
        assert (err[~ok] == 0).all()
        worst = max(worst, float((err[ok] / bnd[ok]).max()))
    print('RATIO resample n_fft %d rate %.4f: worst err / bound %.4f' % (n_fft, rate, worst))
    assert worst <= 1.0
    rc2, got2 = _resample_call(src, lens, rates, c['x'], N, n_fft)
    assert rc2 == 0 and _same(got2, got)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_write_nothing():
    H = _H()
    L = H.lib()
    n_fft = 64
    c = R.wave_case(n_fft)
    N, B, lens = c['N'], c['B'], c['lens']
    hop, F, nb = _geom(N, n_fft)
    xd, ld, rd, tb = _dev(c['x']), _lens_dev(lens, N), _rates_dev(np.ones(B, dtype=F32)), _table_dev(n_fft)
    spec = torch.full((B + 1, F, nb, 2), NAN, device='cuda')
    ospec = torch.full((B + 1, 2 * F, nb, 2), NAN, device='cuda')
    work = torch.full((B + 1, 2 * N), NAN, device='cuda')
    draws = torch.full((B + 1, 6), NAN, device='cuda')
    need = L.asr_wave_augment_workspace_bytes(B, N, n_fft)
    ws = torch.full((need // 4 + 8,), NAN, device='cuda')
    st = H.stream_ptr()
    p = H.ptr
    bad_fft = [0, 32, 63, 96, 4096, -64]
    calls = []
    for nf in bad_fft:
        calls += [lambda nf=nf: L.asr_wave_draws(p(ld), None, p(draws), None, B, N, nf, 1, st),
                  lambda nf=nf: L.asr_wave_stft(p(xd), p(ld), _rp(rd), 2, p(tb), p(spec), B, N, nf, st),
                  lambda nf=nf: L.asr_wave_pvoc(p(spec), p(ld), _rp(rd), 2, p(ospec), B, N, nf, st),
                  lambda nf=nf: L.asr_wave_istft(p(ospec), p(ld), _rp(rd), 2, p(tb), p(xd), N, 1, B, N, nf, st),
                  lambda nf=nf: L.asr_wave_resample(p(work), 2 * N, p(ld), _rp(rd), 2, p(xd), B, N, nf, st),
                  lambda nf=nf: L.asr_wave_augment(p(xd), p(ld), None, p(draws), p(tb), B, N, nf, 1, p(ws), ws.numel() * 4, st)]
    for bB, bN in ((0, N), (-1, N), (B, 0), (B, -5), (65536, N)):
        calls += [lambda bB=bB, bN=bN: L.asr_wave_draws(p(ld), None, p(draws), None, bB, bN, n_fft, 1, st),
                  lambda bB=bB, bN=bN: L.asr_wave_noise(p(xd), p(ld), p(draws), bB, bN, 1, st),
                  lambda bB=bB, bN=bN: L.asr_wave_stft(p(xd), p(ld), _rp(rd), 2, p(tb), p(spec), bB, bN, n_fft, st),
                  lambda bB=bB, bN=bN: L.asr_wave_pvoc(p(spec), p(ld), _rp(rd), 2, p(ospec), bB, bN, n_fft, st),
                  lambda bB=bB, bN=bN: L.asr_wave_istft(p(ospec), p(ld), _rp(rd), 2, p(tb), p(xd), N, 1, bB, bN, n_fft, st),
                  lambda bB=bB, bN=bN: L.asr_wave_resample(p(work), 2 * N, p(ld), _rp(rd), 2, p(xd), bB, bN, n_fft, st),
                  lambda bB=bB, bN=bN: L.asr_wave_augment(p(xd), p(ld), None, p(draws), p(tb), bB, bN, n_fft, 1, p(ws), ws.numel() * 4, st)]
    calls += [  # null pointers
        lambda: L.asr_wave_draws(None, None, p(draws), None, B, N, n_fft, 1, st),
        lambda: L.asr_wave_draws(p(ld), None, None, None, B, N, n_fft, 1, st),
        lambda: L.asr_wave_noise(None, p(ld), p(draws), B, N, 1, st),
        lambda: L.asr_wave_noise(p(xd), None, p(draws), B, N, 1, st),
        lambda: L.asr_wave_noise(p(xd), p(ld), None, B, N, 1, st),
        lambda: L.asr_wave_stft(None, p(ld), _rp(rd), 2, p(tb), p(spec), B, N, n_fft, st),
        lambda: L.asr_wave_stft(p(xd), None, _rp(rd), 2, p(tb), p(spec), B, N, n_fft, st),
        lambda: L.asr_wave_stft(p(xd), p(ld), None, 2, p(tb), p(spec), B, N, n_fft, st),
        lambda: L.asr_wave_stft(p(xd), p(ld), _rp(rd), 2, None, p(spec), B, N, n_fft, st),
        lambda: L.asr_wave_stft(p(xd), p(ld), _rp(rd), 2, p(tb), None, B, N, n_fft, st),
        lambda: L.asr_wave_stft(p(xd), p(ld), _rp(rd), 0, p(tb), p(spec), B, N, n_fft, st),
        lambda: L.asr_wave_pvoc(None, p(ld), _rp(rd), 2, p(ospec), B, N, n_fft, st),
        lambda: L.asr_wave_pvoc(p(spec), None, _rp(rd), 2, p(ospec), B, N, n_fft, st),
        lambda: L.asr_wave_pvoc(p(spec), p(ld), None, 2, p(ospec), B, N, n_fft, st),
        lambda: L.asr_wave_pvoc(p(spec), p(ld), _rp(rd), 2, None, B, N, n_fft, st),
        lambda: L.asr_wave_pvoc(p(spec), p(ld), _rp(rd), -1, p(ospec), B, N, n_fft, st),
        lambda: L.asr_wave_istft(None, p(ld), _rp(rd), 2, p(tb), p(xd), N, 1, B, N, n_fft, st),
        lambda: L.asr_wave_istft(p(ospec), None, _rp(rd), 2, p(tb), p(xd), N, 1, B, N, n_fft, st),
        lambda: L.asr_wave_istft(p(ospec), p(ld), None, 2, p(tb), p(xd), N, 1, B, N, n_fft, st),
        lambda: L.asr_wave_istft(p(ospec), p(ld), _rp(rd), 2, None, p(xd), N, 1, B, N, n_fft, st),
        lambda: L.asr_wave_istft(p(ospec), p(ld), _rp(rd), 2, p(tb), None, N, 1, B, N, n_fft, st),
        lambda: L.asr_wave_istft(p(ospec), p(ld), _rp(rd), 2, p(tb), p(xd), N - 1, 1, B, N, n_fft, st),
        lambda: L.asr_wave_istft(p(ospec), p(ld), _rp(rd), 2, p(tb), p(work), 2 * N - 1, 0, B, N, n_fft, st),
        lambda: L.asr_wave_istft(p(ospec), p(ld), _rp(rd), 2, p(tb), p(xd), N, 2, B, N, n_fft, st),
        lambda: L.asr_wave_resample(None, 2 * N, p(ld), _rp(rd), 2, p(xd), B, N, n_fft, st),
        lambda: L.asr_wave_resample(p(work), 2 * N, None, _rp(rd), 2, p(xd), B, N, n_fft, st),
        lambda: L.asr_wave_resample(p(work), 2 * N, p(ld), None, 2, p(xd), B, N, n_fft, st),
        lambda: L.asr_wave_resample(p(work), 2 * N, p(ld), _rp(rd), 2, None, B, N, n_fft, st),
        lambda: L.asr_wave_resample(p(work), 2 * N - 1, p(ld), _rp(rd), 2, p(xd), B, N, n_fft, st),
        lambda: L.asr_wave_augment(None, p(ld), None, p(draws), p(tb), B, N, n_fft, 1, p(ws), ws.numel() * 4, st),
        lambda: L.asr_wave_augment(p(xd), None, None, p(draws), p(tb), B, N, n_fft, 1, p(ws), ws.numel() * 4, st),
        lambda: L.asr_wave_augment(p(xd), p(ld), None, p(draws), None, B, N, n_fft, 1, p(ws), ws.numel() * 4, st),
        lambda: L.asr_wave_augment(p(xd), p(ld), None, p(draws), p(tb), B, N, n_fft, 1, None, ws.numel() * 4, st),
        lambda: L.asr_wave_augment(p(xd), p(ld), None, p(draws), p(tb), B, N, n_fft, 1, p(ws), need - 1, st),
        lambda: L.asr_wave_augment(p(xd), p(ld), None, p(draws), p(tb), B, N, n_fft, 1, p(ws), 0, st),
        lambda: L.asr_wave_augment(p(xd), p(ld), None, p(draws), p(tb), B, N, n_fft, 1, ctypes.c_void_p(ws.data_ptr() + 4), need, st),
    ]
    for i, f in enumerate(calls):
        assert f() == ASR_E_ARG, i
        assert L.asr_last_error()
    torch.cuda.synchronize()
    assert _same(xd.cpu().numpy(), c['x']) and np.isnan(spec.cpu().numpy()).all() and np.isnan(ospec.cpu().numpy()).all()
    assert np.isnan(work.cpu().numpy()).all() and np.isnan(draws.cpu().numpy()).all() and np.isnan(ws.cpu().numpy()).all()
    assert L.asr_wave_augment_workspace_bytes(0, N, n_fft) == 0 and L.asr_wave_augment_workspace_bytes(B, N, 100) == 0 and need > 0
    # a rate the device cannot take switches the utterance off: nothing is written for it
    for bad in (0.49, 2.01, NAN, 0.0, -1.0):
        rc, s = _stft_call(c['x'], lens, np.full(B, bad, dtype=F32), N, n_fft)
        assert rc == 0 and np.isnan(s.cpu().numpy()).all(), bad
    # the work area is sliced: 40 utterances of 24 s do not fit the cap, the query stays below cap + one utterance
    big = L.asr_wave_augment_workspace_bytes(40, 384000, 2048)
    one = L.asr_wave_augment_workspace_bytes(1, 384000, 2048)
    assert one < big <= (256 << 20) + 40 * 32 + 4 * 256 and big < 40 * (one - 512)


# ---- the chain ----------------------------------------------------------------------------------------------------------------------------
def _chain_by_entry_points(x, lens, draws_in, N, n_fft, seed):
    """The explicit chain over (B + 1)-row buffers -> (wave after (host), draws as applied (host))."""
    H = _H()
    L = H.lib()
    B = len(lens)
    hop, F, nb = _geom(N, n_fft)
    st = H.stream_ptr()
    xd, ld, tb = _dev(x), _lens_dev(lens, N), _table_dev(n_fft)
    dout = torch.full((B + 1, 6), NAN, device='cuda')
    rates = torch.zeros((B + 1, 2), device='cuda')
    din = None if draws_in is None else _dev(draws_in)
    assert L.asr_wave_draws(H.ptr(ld), H.ptr(din), H.ptr(dout), H.ptr(rates), B, N, n_fft, seed, st) == 0
    assert L.asr_wave_noise(H.ptr(xd), H.ptr(ld), H.ptr(dout), B, N, seed, st) == 0
    spec = torch.full((B, F, nb, 2), NAN, device='cuda')
    ospec = torch.full((B, 2 * F, nb, 2), NAN, device='cuda')
    work = torch.full((B, 2 * N), NAN, device='cuda')
    for stage in range(2):
        rp = ctypes.c_void_p(rates.data_ptr() + 4 * stage)
        assert L.asr_wave_stft(H.ptr(xd), H.ptr(ld), rp, 2, H.ptr(tb), H.ptr(spec), B, N, n_fft, st) == 0
        assert L.asr_wave_pvoc(H.ptr(spec), H.ptr(ld), rp, 2, H.ptr(ospec), B, N, n_fft, st) == 0
        if stage == 0:
            assert L.asr_wave_istft(H.ptr(ospec), H.ptr(ld), rp, 2, H.ptr(tb), H.ptr(xd), N, 1, B, N, n_fft, st) == 0
        else:
            assert L.asr_wave_istft(H.ptr(ospec), H.ptr(ld), rp, 2, H.ptr(tb), H.ptr(work), 2 * N, 0, B, N, n_fft, st) == 0
            assert L.asr_wave_resample(H.ptr(work), 2 * N, H.ptr(ld), rp, 2, H.ptr(xd), B, N, n_fft, st) == 0
    torch.cuda.synchronize()
    return xd.cpu().numpy(), dout.cpu().numpy()


def _augment_call(x, lens, draws_in, N, n_fft, seed, want_draws=True):
    H = _H()
    B = len(lens)
    xd, ld, tb = _dev(x), _lens_dev(lens, N), _table_dev(n_fft)
    dout = torch.full((B + 1, 6), NAN, device='cuda') if want_draws else None
    din = None if draws_in is None else _dev(draws_in)
    need = H.lib().asr_wave_augment_workspace_bytes(B, N, n_fft)
    ws = torch.full((need // 4 + 4,), NAN, device='cuda')
    rc = H.lib().asr_wave_augment(H.ptr(xd), H.ptr(ld), H.ptr(din), H.ptr(dout), H.ptr(tb), B, N, n_fft, seed, H.ptr(ws), need, H.stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(ws[need // 4:]).all(), 'written beyond the stated work area'
    return rc, xd.cpu().numpy(), None if dout is None else dout.cpu().numpy()


def _mixed_draws(B):
    """Every combination of the three switches over the batch, legal values."""
    d = np.zeros((B + 1, 6), dtype=F32)
    for b in range(B + 1):
        d[b] = [b & 1, 0.004 + 0.001 * (b % 3), (b >> 1) & 1, [0.8, 1.25, 1.0, 0.5, 2.0][b % 5], (b >> 2) & 1, [4.0, -4.0, 1.5][b % 3]]
    return d


@gpu
@pytest.mark.parametrize('n_fft', [64, 256])
def test_augment_is_the_chain_of_entry_points(n_fft):
    c = R.wave_case(n_fft)
    N, B, lens = c['N'], c['B'], c['lens']
    for draws_in in (_mixed_draws(B), None):
        rc, got, dgot = _augment_call(c['x'], lens, draws_in, N, n_fft, SEED)
        ref, dref = _chain_by_entry_points(c['x'], lens, draws_in, N, n_fft, SEED)
        assert rc == 0 and _same(got, ref) and _same(dgot, dref)
        assert np.isnan(got[B]).all() and np.isnan(dgot[B]).all(), 'the guard utterance was written'
        want, _ = R.finish_draws(draws_in[:B] if draws_in is not None else R.raw_draws(B, SEED), lens, N, n_fft)
        assert np.array_equal(dgot[:B], want)
        for b, n in enumerate(lens):
            m = min(n, N)
            assert _same(got[b, m:], c['x'][b, m:]), (b, 'samples beyond len')
            if not want[b, [0, 2, 4]].any():
                assert _same(got[b], c['x'][b]), (b, 'an utterance with every switch off was touched')
        rc2, got2, _ = _augment_call(c['x'], lens, draws_in, N, n_fft, SEED, want_draws=False)
        assert rc2 == 0 and _same(got2, got)
    # B = 3, mixed switches: the middle utterance off, and what its neighbours get does not depend on it
    i3 = [4, 5, 6] if n_fft == 64 else [1, 2, 3]
    x3 = np.array(c['x'][i3 + [B]])
    l3 = [lens[i] for i in i3]
    d3 = np.array([[1, 0.01, 1, 0.8, 1, 4.0], [0, 0.01, 0, 0.8, 0, 4.0], [0, 0.01, 1, 1.25, 1, -4.0], [1, 0.01, 1, 1.0, 1, 1.0]], dtype=F32)
    rc, g3, _ = _augment_call(x3, l3, d3, N, n_fft, SEED)
    assert rc == 0 and _same(g3[1], x3[1]) and np.isnan(g3[3]).all() and not _same(g3[0], x3[0]) and not _same(g3[2], x3[2])
    d3b = d3.copy()
    d3b[1] = [1, 0.01, 1, 2.0, 1, -2.0]
    rc, g3b, _ = _augment_call(x3, l3, d3b, N, n_fft, SEED)
    assert rc == 0 and _same(g3b[0], g3[0]) and _same(g3b[2], g3[2]) and not _same(g3b[1], g3[1])


@gpu
def test_augment_slices_the_batch():
    """A batch whose spectrograms exceed the cap goes through in slices of 2: the same bits as its utterances one by one (noise off:
    its stream is keyed by the utterance's index in the call)."""
    n_fft, N, B = 2048, 1 << 21, 5            # 118 MB of work area per utterance
    H = _H()
    one = H.lib().asr_wave_augment_workspace_bytes(1, N, n_fft)
    assert one < H.lib().asr_wave_augment_workspace_bytes(B, N, n_fft) < 2 * one + 4096
    lens = [4000 + 700 * b for b in range(B)]
    x = np.full((B + 1, N), R.SENTINEL, dtype=F32)
    for b, n in enumerate(lens):
        x[b, :n] = R.recipe('normal', b, n, n_fft)
    x[B] = NAN
    d = _mixed_draws(B)
    d[:, 0] = 0
    d[:, 2] = 1
    d[:, 4] = 1
    rc, got, _ = _augment_call(x, lens, d, N, n_fft, SEED)
    assert rc == 0 and np.isnan(got[B]).all()
    for b in (0, 1, 2, 4):                    # first, last and across a slice boundary
        rc1, g1, _ = _augment_call(np.stack([x[b], x[B]]), [lens[b]], np.stack([d[b], d[B]]), N, n_fft, SEED)
        assert rc1 == 0 and _same(g1[0], got[b]) and not _same(got[b], x[b]), b


@gpu
def test_module_and_create_transform():
    from src.audio import Augment, Delta, ExtractAudioFeature, Postprocess, WaveAugment, create_transform
    n_fft = 2048
    N = 512 * 12 + 5
    lens = [N, 1024, 3000, 0]
    B = len(lens)
    x = np.full((B + 1, N), 0, dtype=F32)
    for b, n in enumerate(lens):
        x[b, :n] = R.recipe('normal', b, n, n_fft)
    x[B] = NAN
    draws = _mixed_draws(B)
    draws[0, [0, 2, 4]] = 1
    m = WaveAugment(seed=5).cuda()
    assert (m.seed, m.n_fft, m.calls) == (5, 2048, 0) and _same(m.table.cpu().numpy(), R.table(n_fft))
    xd = _dev(x[:B])
    out, olen = m(xd, torch.tensor(lens).cuda(), draws=torch.from_numpy(draws[:B]))
    assert out.data_ptr() == xd.data_ptr() and olen.cpu().tolist() == lens and m.calls == 1
    ref, _ = _chain_by_entry_points(x, lens, draws, N, n_fft, 5 * 1000003 + 1)
    assert _same(out.cpu().numpy(), ref[:B]) and not _same(ref[0], x[0])
    assert _same(ref[3], x[3])                                          # an empty utterance
    # device draws: seed * 1000003 + calls, as Augment seeds its draws
    xd = _dev(x[:B])
    m(xd, torch.tensor(lens).cuda())
    ref, dref = _chain_by_entry_points(x, lens, None, N, n_fft, (5 * 1000003 + 2) & 0xFFFFFFFFFFFF)
    assert m.calls == 2 and _same(xd.cpu().numpy(), ref[:B])
    with pytest.raises(ValueError):
        m(_dev(x[:B]).double(), torch.tensor(lens).cuda())
    # create_transform: first in the chain in train mode, nowhere otherwise
    cfg = {'feat_type': 'fbank', 'feat_dim': 40, 'delta_order': 2, 'augment': True}
    fe, dim = create_transform(dict(cfg, time_aug=True), 'train')
    assert [type(s) for s in fe.stages] == [WaveAugment, ExtractAudioFeature, Delta, Postprocess, Augment] and dim == 120
    plain = [ExtractAudioFeature, Delta, Postprocess]
    for kw, mode in ((dict(time_aug=True), 'eval'), (dict(time_aug=False), 'train'), ({}, 'train'), (dict(time_aug=False), 'eval')):
        fe2, dim2 = create_transform(dict(cfg, **kw), mode)
        assert [type(s) for s in fe2.stages] == plain + ([Augment] if mode == 'train' else []) and dim2 == 120
    # the transform with time_aug is WaveAugment followed by the transform without: same seeds, same bits
    fe, fe0 = fe.cuda(), create_transform(dict(cfg, time_aug=False), 'train')[0].cuda()
    wl = torch.tensor(lens[:3]).cuda()
    feat, flen = fe(_dev(x[:3]), wl)
    xa = _dev(x[:3])
    WaveAugment().cuda()(xa, wl)
    feat0, flen0 = fe0(xa, wl)
    assert torch.equal(flen, flen0) and _same(feat.cpu().numpy(), feat0.cpu().numpy())
    # eval mode and time_aug False leave the wave bit-identical
    for kw, mode in ((dict(time_aug=True), 'eval'), (dict(time_aug=False), 'train')):
        xe = _dev(x[:3])
        create_transform(dict(cfg, **kw), mode)[0].cuda()(xe, wl)
        assert _same(xe.cpu().numpy(), x[:3])


@gpu
def test_end_to_end_against_the_float64_chain():
    """Unforced: normals at amplitude 0.1, n_fft 2048, 40 frames, stretch 0.8 and 1.25, the whole GPU chain against chain64.  The
    yardstick is what a float32 torch.stft in front of the float64 chain moves the same output by (recomputed here, not pinned).
    The yardstick commits float32 roundings in one of the chain's three transforms and none in the vocoder; the GPU chain commits
    them in all three (STFT, the stretched spectrogram it stores, inverse FFT with the overlap-add) and evaluates the vocoder's
    atan2 / hypot / sincospi in float32 besides.  Three independent stages of the yardstick's size and one more for the vocoder: a
    margin of 4 yardsticks.  Measured on the MI355X: rate 0.8 max error 9.2e-07 against a yardstick of 3.9e-07 (ratio 2.33), rate
    1.25 2.9e-07 against 2.1e-07 (ratio 1.36), at amplitude 0.39 / 0.36."""
    n_fft = 2048
    N = 512 * 39 + 7
    x = np.zeros((3, N), dtype=F32)
    g = np.random.Generator(np.random.PCG64(40))
    x[0] = x[1] = (0.1 * g.standard_normal(N)).astype(F32)
    x[2] = NAN
    lens = [N, N]
    d = np.array([[0, 0, 1, 0.8, 0, 0], [0, 0, 1, 1.25, 0, 0], [0, 0, 1, 1.0, 0, 0]], dtype=F32)
    rc, got, _ = _augment_call(x, lens, d, N, n_fft, 0)
    assert rc == 0 and np.isnan(got[2]).all()
    ref = R.chain64(x[:2], lens, d[:2], 0, n_fft)
    yard = R.chain64(x[:2], lens, d[:2], 0, n_fft, stft=R.stft32_torch)
    for b in range(2):
        e, y = np.abs(got[b] - ref[b]).max(), np.abs(yard[b] - ref[b]).max()
        print('RATIO end-to-end rate %.2f: max err %.3g, yardstick %.3g, ratio %.2f (margin 4), amplitude %.3g'
              % (d[b, 3], e, y, e / y, np.abs(ref[b]).max()))
    for b in range(2):
        assert np.abs(got[b] - ref[b]).max() <= 4 * np.abs(yard[b] - ref[b]).max()


# ---- one training step ---------------------------------------------------------------------------------------------------------------------
def _solver_step(tmp_path, time_aug, name):
    """One step of config/debug_timeaug.yaml (batch of 4) through bin/train_asr.Solver -> (loss, features of the step, solver)."""
    import yaml
    from test_checkpoint_interop import _paras
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, 'e2e-asr-pytorch_amd')
    sys.path.insert(0, pkg)
    from bin.train_asr import Solver
    cfg = yaml.safe_load(open(os.path.join(pkg, 'config', 'debug_timeaug.yaml')))
    assert cfg['data']['corpus']['path'] == 'synthetic-wav' and cfg['data']['audio']['time_aug'] is True
    if time_aug is None:
        del cfg['data']['audio']['time_aug']
    else:
        cfg['data']['audio']['time_aug'] = time_aug
    cfg['data']['corpus'].update(batch_size=4, subset=8)
    cfg['data']['text']['vocab_file'] = os.path.join(pkg, cfg['data']['text']['vocab_file'])
    cfg['hparas'].update(max_step=1, valid_step=1)
    torch.manual_seed(0)                                    # as main.py does before it builds a Solver
    solver = Solver(cfg, _paras(tmp_path, name=name), 'train')
    solver.load_data()
    solver.set_model()
    solver.validate = lambda *a, **k: None                  # the step is what is tested
    if time_aug:
        # a module seed whose first call switches something on for the first utterance (the default seed's first call draws three
        # zeros for both utterances of this batch: probability 0.245 each)
        wa = solver.tr_set.audio_transform.stages[0]
        wa.seed = next(k for k in range(1, 100) if R.raw_draws(1, k * 1000003 + 1)[0, [0, 2, 4]].any())
    seen = {}
    write, fetch = solver.write_log, solver.fetch_data

    def record(log, d):
        if log == 'loss' and 'tr_att' in (d or {}):
            seen['loss'] = float(d['tr_att'].detach())
        return write(log, d)

    def fetched(data, train=False):
        out = fetch(data, train=train)
        seen.setdefault('feat', out[0].clone())
        return out
    solver.write_log, solver.fetch_data = record, fetched
    solver.exec()
    torch.cuda.synchronize()
    return seen['loss'], seen['feat'], solver


@gpu
def test_one_training_step_with_time_aug(tmp_path):
    """config/debug_timeaug.yaml on synthetic-wav: one step through the training Solver gives a finite loss on an augmented batch;
    with time_aug False the chain, the batch and the loss are those of a config without the key."""
    from src.data import load_dataset
    loss_on, feat_on, s_on = _solver_step(tmp_path, True, 'ta_on')
    stages = [type(s).__name__ for s in s_on.tr_set.audio_transform.stages]
    assert stages[0] == 'WaveAugment' and 'WaveAugment' not in [type(s).__name__ for s in s_on.dv_set.audio_transform.stages]
    assert s_on.tr_set.audio_transform.stages[0].calls == 1 and np.isfinite(loss_on) and torch.isfinite(feat_on).all()
    loss_off, feat_off, s_off = _solver_step(tmp_path, False, 'ta_off')
    loss_none, feat_none, s_none = _solver_step(tmp_path, None, 'ta_none')
    print('RATIO one step: loss with time_aug %.6f, with time_aug False %.6f, without the key %.6f' % (loss_on, loss_off, loss_none))
    for s in (s_off, s_none):
        assert [type(m).__name__ for m in s.tr_set.audio_transform.stages] == stages[1:]
    assert torch.equal(feat_off, feat_none) and feat_on.shape == feat_off.shape and not torch.equal(feat_on, feat_off)
    assert np.isfinite(loss_off) and loss_off == loss_none
    # a feature corpus with time_aug True loads, says so once, and builds no transform
    import yaml
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'e2e-asr-pytorch_amd')
    cfg = yaml.safe_load(open(os.path.join(pkg, 'config', 'debug_timeaug.yaml')))
    text = dict(cfg['data']['text'], vocab_file=os.path.join(pkg, cfg['data']['text']['vocab_file']))
    for path, word in (('synthetic', 'ignored'), ('synthetic-wav', 'training batches only')):
        tr, dv, _, _, _, msg = load_dataset(0, True, False, False, dict(cfg['data']['corpus'], path=path), dict(cfg['data']['audio']), text)
        assert sum('time_aug' in m for m in msg) == 1 and sum(word in m for m in msg) == 1 and (tr.audio_transform is None) == (path == 'synthetic')
    tr, dv, _, _, _, msg = load_dataset(0, True, False, False, dict(cfg['data']['corpus']), dict(cfg['data']['audio'], time_aug=False), text)
    assert not any('time_aug' in m for m in msg)
