#!/usr/bin/env python
"""Times asr_cmvn (per-utterance CMVN, csrc/frontend.hip: two launches) alone at the training shape B = 16, T = 1200, D = 160:
one JSON line with every utterance at full length, one with SURVEY 8d's length model clip(N(1270, 480), 150, 2450) cut to T.
A window is --calls back-to-back calls between two device events, enqueued while the device is still busy with a large matrix
product issued just before (a call through ctypes takes the host longer than the device: without the product in front the window
would time the host); the figure is the median window over --iters, per call, after --warmup calls.  bytes = what the two
launches move (x read twice, written once, over the valid rows; the partial moments written and read); a device copy of the
same tensor is timed the same way as the yardstick for what this much traffic costs here - 12.3 MB stay in the caches between
calls, so neither figure is an HBM rate."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'e2e-asr-pytorch_amd')]

from src import hipabi as H  # noqa: E402

B, T, D = 16, 1200, 160


def window_us(fn, calls, iters, warmup):
    busy = torch.rand((4096, 4096), device='cuda')
    for _ in range(warmup):
        fn()
    torch.mm(busy, busy)
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.mm(busy, busy)                      # keeps the device busy while the host enqueues the window behind it
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / calls)
    times.sort()
    return times


def bench(kind, calls, iters, warmup):
    dev = torch.device('cuda')
    if kind == 'full':
        ln = np.full(B, T, dtype=np.int64)
    else:
        ln = np.minimum(np.clip(np.random.RandomState(1234).normal(1270, 480, B), 150, 2450).astype(np.int64), T)
    x = torch.rand((B, T, D), generator=torch.Generator().manual_seed(0)).to(dev)
    y = torch.empty_like(x)
    lens = torch.from_numpy(ln).to(dev)
    nbytes = int(H.lib().asr_cmvn_workspace_bytes(B, D))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)

    def launch():
        H.call('asr_cmvn', H.ptr(x), H.ptr(lens), None, B, T, D, 1e-10, H.ptr(ws), nbytes, H.stream_ptr())

    t = window_us(launch, calls, iters, warmup)
    c = window_us(lambda: y.copy_(x), calls, iters, warmup)
    valid = int(ln.sum()) * D * 4
    moved = 3 * valid + 2 * nbytes
    med = t[len(t) // 2]
    return {'bench': 'cmvn', 'lengths': kind, 'B': B, 'T': T, 'D': D, 'frames': int(ln.sum()), 'calls_per_window': calls, 'iters': iters,
            'us_median': round(med, 2), 'us_min': round(t[0], 2), 'us_p90': round(t[int(len(t) * 0.9)], 2),
            'bytes_moved': moved, 'GBps': round(moved / med / 1e3, 1), 'workspace_bytes': nbytes,
            'copy_us_median': round(c[len(c) // 2], 2), 'copy_bytes': 2 * B * T * D * 4}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=20)
    a = ap.parse_args()
    for kind in ('full', 'librispeech'):
        print(json.dumps(bench(kind, a.calls, a.iters, a.warmup)), flush=True)
