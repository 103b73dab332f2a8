"""asr_rescore_token_logp alone (csrc/rescore.hip): the launch that reduces the LM's logit block (R,L,V) fp32 to one log-probability
per (row, position), timed between two events over --reps launches after one warm-up.  Its bound is one read of the block, so the
figure printed is block bytes / kernel time, to be held against the HBM rate; only a block above the 256 MiB Infinity Cache is
sure to come from HBM at every launch.  Random logits, every row of full length.  Prints one JSON line per V.
usage: python tools/bench_rescore_lm.py [--rows 128] [--positions 392] [--vocab 31 1024 1025 10000 65536] [--reps 10]
Rows are cut so that a block stays under --max-bytes (default 1 GiB, the chunk budget of the host path)."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'e2e-asr-pytorch_amd'))
import torch
from src import hipabi as H
ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=128); ap.add_argument('--positions', type=int, default=392)
ap.add_argument('--vocab', type=int, nargs='+', default=[31, 1024, 1025, 10000, 65536]); ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--max-bytes', type=int, default=1 << 30)
a = ap.parse_args()
torch.manual_seed(0)
for V in a.vocab:
    L = a.positions
    R = max(1, min(a.rows, a.max_bytes // (4 * L * V)))
    logits = torch.randn((R, L, V), device='cuda')
    target = torch.randint(0, V, (R, L), dtype=torch.int64, device='cuda')
    lens = torch.full((R,), L, dtype=torch.int32, device='cuda')
    out = torch.empty((R, L), dtype=torch.float32, device='cuda')
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(1 + a.reps):
        if i == 1: ev[0].record()
        H.call('asr_rescore_token_logp', H.ptr(logits), L * V, V, H.ptr(target), L, H.ptr(lens), R, L, V, H.ptr(out), L, H.stream_ptr())
    ev[1].record(); torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / a.reps
    want = torch.log_softmax(logits[:2].double(), -1).gather(2, target[:2].unsqueeze(-1)).squeeze(-1)
    nbytes = 4 * R * L * V
    print(json.dumps({'metric': 'asr_rescore_token_logp, one launch', 'rows': R, 'positions': L, 'vocab': V, 'block_bytes': nbytes,
                      'blocks_per_row': (V + 1023) // 1024, 'kernel_ms': ms, 'block_GB_per_s': nbytes / ms * 1e-6,
                      'max_abs_err_vs_float64_first_rows': float((out[:2].double() - want).abs().max()), 'reps': a.reps}))
