#!/usr/bin/env python
"""Times the waveform augmentation stage (asr_wave_augment, csrc/wave_aug.hip) at the training shape B = 16, N = 203 200 samples
(1 270 fbank frames) and the shipped n_fft = 2048, next to asr_fbank on the same batch: one JSON line with three figures,
  default_ms    the stage with the device draws (switch probabilities 0.3 / 0.3 / 0.5; the seed changes per call as in training),
  forced_ms     the stage with all three switches on for every utterance (rates spread over [0.8, 1.25], semitones over [-4, 4]),
  fbank_ms      asr_fbank alone,
each the median of 5 timed calls after a warm-up, in one process, between two device events with a synchronisation per call.  The
stage works in place, so every call starts from a fresh copy of the batch (the copy is outside the window).  forced_kernels_ms
gives the noise launch and the four launches of the forced call's pitch stage one by one (an event pair per kernel through the
single entry points, median of 5; the stretch stage runs the first three of them once more).  The line also
goes to profiles/wave_aug.json."""
import argparse
import ctypes
import datetime
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'e2e-asr-pytorch_amd')]

from src import hipabi as H  # noqa: E402
from src.audio import ExtractAudioFeature, wave_aug_table  # noqa: E402

B, N, N_FFT = 16, 203200, 2048


def timed(fn, reps, warmup, before=None):
    out = []
    for i in range(warmup + reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b))
    out.sort()
    return out


def main(reps, warmup):
    dev = torch.device('cuda')
    g = np.random.Generator(np.random.PCG64(7))
    t = np.arange(N) / 16000.0
    wav0 = torch.from_numpy(np.stack([(0.2 * np.sin(2 * np.pi * (120 + 40 * b) * t) + 0.02 * g.standard_normal(N)).astype(np.float32)
                                      for b in range(B)])).to(dev)
    lens = torch.full((B,), N, dtype=torch.int64, device=dev)
    wav = wav0.clone()
    table = torch.from_numpy(wave_aug_table(N_FFT)).to(dev)
    nbytes = int(H.lib().asr_wave_augment_workspace_bytes(B, N, N_FFT))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    forced = np.zeros((B, 6), dtype=np.float32)
    forced[:, [0, 2, 4]] = 1
    forced[:, 1] = 0.005
    forced[:, 3] = np.linspace(0.8, 1.25, B)
    forced[:, 5] = np.linspace(-4, 4, B)
    fd = torch.from_numpy(forced).to(dev)
    used = torch.zeros((B, 6), device=dev)
    calls = [0]

    def reset():
        wav.copy_(wav0)

    def stage(draws):
        calls[0] += 1
        H.call('asr_wave_augment', H.ptr(wav), H.ptr(lens), H.ptr(draws), H.ptr(used), H.ptr(table), B, N, N_FFT, calls[0], H.ptr(ws), nbytes,
               H.stream_ptr())

    on, d = [], []
    for i in range(warmup + reps):                    # the default figure with the switches each call drew
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        stage(None)
        b.record()
        b.synchronize()
        if i >= warmup:
            d.append(a.elapsed_time(b))
            on.append(used.cpu().numpy()[:, [0, 2, 4]].sum(0).astype(int).tolist())
    order = np.argsort(d)
    f = timed(lambda: stage(fd), reps, warmup, before=reset)
    fe = ExtractAudioFeature(num_mel_bins=40).to(dev)
    k = timed(lambda: fe(wav0, lens), reps, warmup)

    # the forced call launch by launch
    hop, F, nb = N_FFT // 4, 1 + N // (N_FFT // 4), N_FFT // 2 + 1
    spec = torch.empty((B, F, nb, 2), device=dev)
    ospec = torch.empty((B, 2 * F, nb, 2), device=dev)
    work = torch.empty((B, 2 * N), device=dev)
    rates = torch.zeros((B, 2), device=dev)
    dout = torch.zeros((B, 6), device=dev)
    L, st = H.lib(), H.stream_ptr()
    L.asr_wave_draws(H.ptr(lens), H.ptr(fd), H.ptr(dout), H.ptr(rates), B, N, N_FFT, 1, st)
    r1 = ctypes.c_void_p(rates.data_ptr() + 4)                   # the pitch rates: column 1, stride 2
    parts = {
        'noise': lambda: L.asr_wave_noise(H.ptr(wav), H.ptr(lens), H.ptr(dout), B, N, 1, st),
        'stft': lambda: L.asr_wave_stft(H.ptr(wav), H.ptr(lens), r1, 2, H.ptr(table), H.ptr(spec), B, N, N_FFT, st),
        'pvoc': lambda: L.asr_wave_pvoc(H.ptr(spec), H.ptr(lens), r1, 2, H.ptr(ospec), B, N, N_FFT, st),
        'istft': lambda: L.asr_wave_istft(H.ptr(ospec), H.ptr(lens), r1, 2, H.ptr(table), H.ptr(work), 2 * N, 0, B, N, N_FFT, st),
        'resample': lambda: L.asr_wave_resample(H.ptr(work), 2 * N, H.ptr(lens), r1, 2, H.ptr(wav), B, N, N_FFT, st),
    }
    reset()
    kern = {}
    for name, fn in parts.items():
        tt = timed(fn, reps, 1)
        kern[name] = round(tt[len(tt) // 2], 4)
    line = {'bench': 'wave_aug', 'date': datetime.date.today().isoformat(), 'B': B, 'N': N, 'n_fft': N_FFT, 'reps': reps, 'warmup': warmup,
            'default_ms': round(d[order[len(d) // 2]], 4), 'default_ms_all': [round(v, 4) for v in d], 'default_switches_on': on,
            'forced_ms': round(f[len(f) // 2], 4), 'forced_ms_min': round(f[0], 4), 'forced_ms_max': round(f[-1], 4),
            'fbank_ms': round(k[len(k) // 2], 4), 'forced_kernels_ms': kern, 'workspace_bytes': nbytes}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'wave_aug.json'), 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    main(a.reps, a.warmup)
