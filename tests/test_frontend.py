"""Front-end parity.  CPU: oracle + host tables vs the reference fixtures (g5).  GPU: HIP kernels vs the same
fixtures (delta/postprocess/SpecAugment with recorded draws: exact fp32) and vs the torch.stft oracle (fbank)."""
import os

import numpy as np
import pytest
import torch

from oracle import frontend_oracle as FO


@pytest.fixture(scope='module')
def g5(golden_dir):
    return np.load(os.path.join(golden_dir, 'g5_frontend.npz'))


def test_oracle_and_tables_match_reference(g5):
    from src.audio import create_mel_filterbank, delta_filters
    np.testing.assert_allclose(create_mel_filterbank(16000, 1025, 80), g5['melfb'], atol=1e-7)
    for order in (1, 2):
        filt = delta_filters(order, 2)
        np.testing.assert_allclose(filt, g5['filters%d' % order].reshape(order + 1, -1), atol=1e-7)
        d = FO.delta(g5['mel'], filt)
        np.testing.assert_allclose(d.numpy(), g5['delta%d' % order], atol=1e-6)
        np.testing.assert_allclose(FO.postprocess(d).numpy(), g5['post%d' % order], atol=1e-6)
    for i, dr in enumerate(g5['aug_draws']):
        np.testing.assert_allclose(FO.augment(g5['aug_in'], dr).numpy(), g5['aug_out%d' % i], atol=1e-6)


@pytest.mark.gpu
def test_hip_delta_stack_matches_reference(g5):
    from src.audio import Delta
    mel = torch.from_numpy(g5['mel'])[0].t().contiguous()            # (T,F)
    T, Fd = mel.shape
    for order in (1, 2):
        # batch of two: the fixture utterance and a shorter copy padded with garbage that must not leak in
        x = torch.zeros(2, T + 5, Fd)
        x[0, :T] = mel
        x[0, T:] = 7.0
        x[1, :T - 9] = mel[:T - 9]
        x[1, T - 9:] = -3.0
        out, _ = Delta(order, 2).cuda()(x.cuda(), torch.tensor([T, T - 9]).cuda())
        out = out.cpu()
        np.testing.assert_allclose(out[0, :T].numpy(), g5['post%d' % order], atol=1e-6)
        assert float(out[0, T:].abs().max()) == 0.0
        ref1 = FO.postprocess(FO.delta(g5['mel'][:, :, :T - 9], g5['filters%d' % order].reshape(order + 1, -1)))
        np.testing.assert_allclose(out[1, :T - 9].numpy(), ref1.numpy(), atol=1e-6)


@pytest.mark.gpu
def test_hip_specaugment_matches_reference(g5):
    from src.audio import Augment
    x0 = torch.from_numpy(g5['aug_in'])
    T, D = x0.shape
    draws = torch.from_numpy(g5['aug_draws']).int()
    nb = draws.shape[0]
    x = torch.zeros(nb, T + 11, D)
    x[:, :T] = x0
    x[:, T:] = 9.0          # padding must be ignored by the mean and left untouched
    aug = Augment().cuda()
    out, _ = aug(x.cuda(), torch.full((nb,), T).cuda(), draws=draws)
    out = out.cpu()
    for i in range(nb):
        np.testing.assert_allclose(out[i, :T].numpy(), g5['aug_out%d' % i], atol=2e-6)
        assert float((out[i, T:] - 9.0).abs().max()) == 0.0
    # device-side draws: masks must be legal (inside the utterance, widths below T / F) and mean-filled - and exactly the
    # bands of the stated rule (tests/test_frontend_reference.py::specaug_draws), also on utterances shorter than the time mask
    from test_frontend_reference import specaug_draws
    y = torch.rand(6, 300, 160)
    lens = torch.tensor([300, 250, 200, 41, 10, 1])
    yd = y.clone().cuda()
    aug(yd, lens.cuda())
    seed = (aug.seed * 1000003 + aug.calls) & 0xFFFFFFFFFFFF
    changed = (yd.cpu() != y)
    for b in range(6):
        assert not changed[b, lens[b]:].any()
        rows = changed[b].all(dim=1).nonzero().flatten()
        cols = changed[b, :lens[b]].all(dim=0).nonzero().flatten()
        assert len(rows) < 40 and len(cols) < 27
        t, t0, tend, f, f0, fend = specaug_draws(b, int(lens[b]), 160, 40, 27, seed)
        want = torch.zeros(300, 160, dtype=torch.bool)
        want[t0:tend] = True
        want[:lens[b], f0:fend] = True
        assert torch.equal(changed[b], want), (b, (t, t0, tend, f, f0, fend))


@pytest.mark.gpu
def test_hip_fbank_matches_stft_oracle():
    from src.audio import ExtractAudioFeature, create_mel_filterbank
    g = torch.Generator().manual_seed(0)
    lens = torch.tensor([16000, 12345, 801])
    wav = torch.zeros(3, 16000)
    for b in range(3):
        t = torch.arange(int(lens[b])) / 16000.0
        wav[b, :lens[b]] = 0.3 * torch.sin(2 * np.pi * (200 + 900 * b) * t) + 0.05 * torch.randn(int(lens[b]), generator=g)
    fe = ExtractAudioFeature().cuda()
    out, flen = fe(wav.cuda(), lens.cuda())
    out = out.cpu()
    fb = create_mel_filterbank(16000, 1025, 80)
    for b in range(3):
        ref = FO.fbank(wav[b:b + 1, :lens[b]], fb)[0].t()           # (T_b, 80)
        Tb = ref.shape[0]
        assert int(flen[b]) == Tb
        assert float((out[b, :Tb] - ref).abs().max()) < 2e-4         # fp32 DFT-as-contraction vs FFT
        if Tb < out.shape[1]:
            assert float(out[b, Tb:].abs().max()) == 0.0


def test_fbank_oracle_agrees_with_brute_force_dft():
    """The STFT leg of ExtractAudioFeature (reference src/audio.py:158-171) delegates to torchaudio, which is absent here,
    so the oracle's torch.stft restatement cannot be pinned to the reference ("STFT/mel parity unpinned").  This
    known-answer test derives the same quantity a second, independent way - a float64 brute-force DFT written from the
    documented definition (pre-emphasis 0.97; reflect padding by n_fft//2; frames of n_fft = 1025 samples every 160;
    periodic Hann window of 400 centred in the frame; |X_f| for f = 0..512; Slaney mel filterbank; 20 log10(max(.,1e-5))
    - 20; clamp((x + 100) / 100, 0, 1)) - and requires the two to agree to fp32 rounding."""
    import numpy as np
    from oracle import frontend_oracle as FO
    from src.audio import create_mel_filterbank
    g = np.random.Generator(np.random.PCG64(9))
    n = 2000
    t = np.arange(n) / 16000.0
    wav = (0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 3000 * t + 1.0) + 0.05 * g.standard_normal(n)).astype(np.float32)
    fb = create_mel_filterbank(16000, 1025, 80)
    got = FO.fbank(wav[None, :], fb)[0].numpy().astype(np.float64)                 # (80, T)
    # brute force, float64
    x = wav.astype(np.float64)
    x = np.concatenate([x[:1], x[1:] - 0.97 * x[:-1]])
    n_fft, win, hop = 1025, 400, 160
    pad = n_fft // 2
    xp = np.concatenate([x[1:pad + 1][::-1], x, x[-pad - 1:-1][::-1]])           # reflect
    T = 1 + n // hop
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)                        # periodic Hann
    wfull = np.zeros(n_fft)
    left = (n_fft - win) // 2
    wfull[left:left + win] = w
    k = np.arange(n_fft)
    f = np.arange(n_fft // 2 + 1)
    basis = np.exp(-2j * np.pi * np.outer(f, k) / n_fft)                            # (513, 1025)
    mag = np.stack([np.abs(basis @ (xp[i * hop:i * hop + n_fft] * wfull)) for i in range(T)], axis=1)   # (513, T)
    mel = fb.astype(np.float64) @ mag
    db = 20 * np.log10(np.maximum(mel, 1e-5)) - 20.0
    want = np.clip((db + 100.0) / 100.0, 0.0, 1.0)
    assert got.shape == want.shape
    assert np.abs(got - want).max() < 2e-5, np.abs(got - want).max()
