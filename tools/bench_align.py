#!/usr/bin/env python
"""Times asr_ctc_align (CTC forced alignment, csrc/ctc_align.hip) alone: one JSON line per shape.  The first shape is the
headline shape's encoder output (B = 16, T' = 300, L = 180, V = 31), the second a long-recording shape (B = 8, T' = 1500,
L = 400).  Inputs: log_softmax(randn), random targets without immediate repeats (every target is alignable)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'e2e-asr-pytorch_amd')]

from src import hipabi as H  # noqa: E402

SHAPES = [(16, 300, 180, 31), (8, 1500, 400, 31)]


def bench(B, T, L, V, iters, warmup):
    dev = torch.device('cuda')
    g = torch.Generator().manual_seed(0)
    lp = torch.log_softmax(torch.randn((B, T, V), generator=g), dim=-1).to(dev)
    tg = torch.randint(1, V, (B, L), generator=g)
    for j in range(1, L):
        same = tg[:, j] == tg[:, j - 1]
        tg[same, j] = tg[same, j] % (V - 1) + 1                             # the next token, wrapping inside 1..V-1
    tg = tg.to(dev)
    in_len = torch.full((B,), T, dtype=torch.int64, device=dev)
    tg_len = torch.full((B,), L, dtype=torch.int64, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    ftok, fpos, ts, te, ok = i32(B, T), i32(B, T), i32(B, L), i32(B, L), i32(B)
    tsc, score = torch.empty((B, L), device=dev), torch.empty(B, device=dev)
    nbytes = int(H.lib().asr_ctc_align_workspace_bytes(B, T, L))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def launch():
        H.call('asr_ctc_align', H.ptr(lp), H.ptr(tg), H.ptr(in_len), H.ptr(tg_len), B, T, V, L, H.ptr(ftok), H.ptr(fpos), H.ptr(ts),
               H.ptr(te), H.ptr(tsc), H.ptr(score), H.ptr(ok), H.ptr(ws), nbytes, H.stream_ptr())

    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    assert int(ok.sum()) == B
    med = times[len(times) // 2]
    return {'bench': 'ctc_align', 'B': B, 'T': T, 'L': L, 'V': V, 'iters': iters, 'us_median': round(med, 1), 'us_min': round(times[0], 1),
            'us_p90': round(times[int(len(times) * 0.9)], 1), 'us_per_frame': round(med / T, 3), 'workspace_bytes': nbytes}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    a = ap.parse_args()
    for shape in SHAPES:
        print(json.dumps(bench(*shape, a.iters, a.warmup)), flush=True)
