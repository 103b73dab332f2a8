"""RNN-LM training step time at the dims of config/librispeech_lm.yaml (4 x 1024, tied embedding, dropout 0.5), random
tokens of a fixed batch: forward, cross entropy, backward, global-norm clip and the fused Adam step, as bin/train_lm.py runs
them.  Prints one JSON line.
usage: python tools/bench_lm.py [--module LSTM|GRU] [--batch 64] [--tokens 100] [--steps 10] [--warmup 3] [--prec bf16]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'e2e-asr-pytorch_amd')
sys.path.insert(0, ROOT); sys.path.insert(0, PKG)
import torch, yaml
from src import hipabi as H
from src.lm import RNNLM
from src.optim import Optimizer
from src.util import CrossEntropyLoss
ap = argparse.ArgumentParser()
ap.add_argument('--module', choices=('LSTM', 'GRU'), default='LSTM')
ap.add_argument('--batch', type=int, default=64); ap.add_argument('--tokens', type=int, default=100)
ap.add_argument('--steps', type=int, default=10); ap.add_argument('--warmup', type=int, default=3); ap.add_argument('--prec', default='bf16')
a = ap.parse_args()
torch.manual_seed(0)
cfg = yaml.safe_load(open(os.path.join(PKG, 'config', 'librispeech_lm.yaml')))
mc = dict(cfg['model'], module=a.module)
V = 31
lm = RNNLM(V, **mc).cuda().train()
lm.prec = H.BF16 if a.prec == 'bf16' else H.F32
lm.flatten()
opt = Optimizer(lm.parameters(), **cfg['hparas'])
xent = CrossEntropyLoss(ignore_index=0)
B, T = a.batch, a.tokens
txt = torch.randint(1, V, (B, T + 1), device='cuda')


def step(i):
    opt.pre_step(i)
    pred, _ = lm(txt[:, :-1], None)
    loss = xent(pred.reshape(-1, V), txt[:, 1:].reshape(-1))
    loss.backward()
    opt.opt.grad_norm()
    opt.opt.step(clip=5.0, use_norm=True)
    return loss


for i in range(a.warmup):
    step(i)
torch.cuda.synchronize()
t0 = time.perf_counter()
for i in range(a.steps):
    loss = step(a.warmup + i)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / a.steps
H.raise_if_aborted()
print(json.dumps({'metric': 'RNN-LM training step (fwd + bwd + clip + Adam)', 'module': a.module, 'ms_per_step': dt * 1e3,
                  'tokens_per_s': B * T / dt, 'batch': B, 'tokens_per_sentence': T, 'layers': mc['n_layers'], 'dim': mc['dim'],
                  'emb_tying': mc['emb_tying'], 'dropout': mc['dropout'], 'prec': a.prec, 'steps': a.steps, 'warmup': a.warmup,
                  'final_loss': float(loss)}))
