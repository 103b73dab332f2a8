#!/usr/bin/env python
"""Times the SpecAugment policy pass (asr_specaug_policy, csrc/specaug_policy.hip) at B = 16 x T = 1200 x D = 160 and B = 64 x
T = 3000 x D = 160, next to two kernels of the same front-end on the same batch, in one process, the kernels alternating call by
call: one JSON line per run, printed and appended to profiles/specaug_policy.json.  Per shape and kernel: the median time of
`reps` (>= 20) calls after a warm-up, each between two device events; the algorithmic bytes; and bytes / time as a share of 8 TB/s.

  delta_stack      asr_delta_stack, F = 80 -> 160 columns (order 1, window 2): reads 4 B T 80, writes 4 B T 160 bytes - the
                   read-once, write-once yardstick of this stage
  specaug_ws       today's Augment (asr_specaug_ws, widths 40 / 27), in place: reads 4 sum(n) D for its means, writes only the bands
  policy_ld_mean   the LD policy (warp 80, 2 x F 27, 2 x T 100), mean fill: 2 * 4 B T D + 4 sum(n) D
  policy_ld_zero   the same with zero fill (no reduction launch): 2 * 4 B T D
  policy_adaptive  LD with time_masks 20, time_count_ratio 0.04, time_ratio 0.04, mean fill

Lengths are spread evenly over [T / 2, T].  The tool needs the GPU and the built library; there is nothing else it could run on."""
import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'e2e-asr-pytorch_amd')]

from src import hipabi as H  # noqa: E402
from src.audio import delta_filters  # noqa: E402

SHAPES = [(16, 1200, 160), (64, 3000, 160)]
PEAK = 8e12                    # bytes / s
STEP_MS = 17.0                 # the training step of bench.py the share is stated against


def run_shape(B, T, D, reps, warmup):
    dev = torch.device('cuda')
    g = torch.Generator(device='cpu').manual_seed(5)
    x = torch.rand((B, T, D), generator=g).to(dev)
    lens_h = np.linspace(T // 2, T, B).astype(np.int64)
    lens = torch.from_numpy(lens_h).to(dev)
    out = torch.empty_like(x)
    inplace = x.clone()
    half = x[:, :, :D // 2].contiguous()
    filt = torch.from_numpy(delta_filters(1, 2)).to(dev)
    L, st = H.lib(), H.stream_ptr()
    sws = torch.empty(L.asr_specaug_workspace_bytes(B), dtype=torch.uint8, device=dev)
    pws = torch.empty(L.asr_specaug_policy_workspace_bytes(B) // 8, dtype=torch.float64, device=dev)
    calls = [0]

    def policy(tm, tr_pm, tc_pm, fill):
        def fn():
            calls[0] += 1
            H.call('asr_specaug_policy', H.ptr(x), H.ptr(lens), H.ptr(out), None, None, B, T, D, 80, 2, 27, tm, 100, tr_pm, tc_pm, fill,
                   calls[0], H.ptr(pws), pws.numel() * 8, st)
        return fn

    def specaug_ws():
        calls[0] += 1
        H.call('asr_specaug_ws', H.ptr(inplace), H.ptr(lens), None, None, B, T, D, 40, 27, calls[0], H.ptr(sws), sws.numel(), st)

    def delta_stack():
        H.call('asr_delta_stack', H.ptr(half), H.ptr(lens), H.ptr(out), H.ptr(filt), B, T, D // 2, 2, filt.shape[1], st)

    valid = int(lens_h.sum()) * D * 4
    full = B * T * D * 4
    kernels = [('delta_stack', delta_stack, full // 2 + full), ('specaug_ws', specaug_ws, valid),
               ('policy_ld_mean', policy(2, 1000, 0, 0), 2 * full + valid), ('policy_ld_zero', policy(2, 1000, 0, 1), 2 * full),
               ('policy_adaptive', policy(20, 40, 40, 0), 2 * full + valid)]
    times = {name: [] for name, _, _ in kernels}
    for i in range(warmup + reps):
        for name, fn, _ in kernels:                      # alternating: every kernel sees the same drift of clocks and caches
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                times[name].append(a.elapsed_time(b))
    res = {}
    for name, _, nbytes in kernels:
        t = sorted(times[name])
        med = t[len(t) // 2]
        res[name] = {'ms': round(med, 4), 'ms_min': round(t[0], 4), 'ms_max': round(t[-1], 4), 'bytes': nbytes,
                     'share_of_8TBs': round(nbytes / (med * 1e-3) / PEAK, 4), 'share_of_17ms_step': round(med / STEP_MS, 5)}
    return {'B': B, 'T': T, 'D': D, 'sum_len': int(lens_h.sum()), 'kernels': res}


def main(reps, warmup):
    if not torch.cuda.is_available():
        raise SystemExit('bench_specaug.py needs the GPU')
    if reps < 20:
        raise SystemExit('--reps must be at least 20')
    line = {'bench': 'specaug_policy', 'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0), 'reps': reps,
            'warmup': warmup, 'shapes': [run_shape(B, T, D, reps, warmup) for B, T, D in SHAPES]}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'specaug_policy.json'), 'a') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    main(a.reps, a.warmup)
