"""Generates g15_vgg_launch_trace.json: every entry point the VGG front-ends (src/vgg.py) launch, in order, with the scalar
arguments - for a training forward + backward through the extractor's `forward` and for one `forward_lens` over a padded
batch, vgg 1..5 in both precisions.  Needs the GPU and the built library.  The committed fixture was written by the code that
preceded the shared conv-stack loop of src/vgg.py (two autograd functions and a third, inference-only loop) and is the record
of the launch sequence that change had to preserve: regenerate it only when a launch is changed on purpose.

    python tests/golden/gen_vgg_launch_trace.py [out.json]     # default: tests/golden/g15_vgg_launch_trace.json

A call is recorded as [name, [the arguments whose declared type in hipabi.SIGNATURES[name] is not a pointer]]: ints, longs,
floats.  Buffers and the stream drop out by construction; the numeric tests hold the wiring."""
import ctypes
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'e2e-asr-pytorch_amd'))

B = 2
SPLIT_FREQ, LOW_DIM = 12, 4                 # vgg 2 / 4, as tests/test_ragged_frontend_reference.py
LENS_T, LENS = 8, (8, 4)                    # forward_lens: one row with a tail
# T = 11: both trims act (11 -> 8 for time_div 4, 11 -> 10 for time_div 2); D = 40: one input channel, D = 120: three (the
# first layer's patch width K1p pads 27 to 32).  T = 96 (bordered layout only): the smallest at which both weight-gradient
# `splits` expressions leave 1 (2 * 98 * 42 bordered pixels: 8232 // 4096 = 2 and 8232 // 2048 = 4).
CASES = ([(vgg, prec, D, 11) for vgg in (1, 5, 3, 2, 4) for prec in ('bf16', 'fp32') for D in (40, 120)]
         + [(vgg, 'bf16', 40, 96) for vgg in (1, 5)])


def case_key(case):
    return 'vgg%d %s D=%d T=%d' % case


def _is_scalar(argtype):
    return argtype is not ctypes.c_void_p and not issubclass(argtype, ctypes._Pointer)


def _extractor(vgg, D):
    from src import vgg as V
    if vgg in (2, 4):
        return (V.FreqVGGExtractor if vgg == 2 else V.FreqVGGExtractor2)(D, SPLIT_FREQ, LOW_DIM)
    return {1: V.VGGExtractor, 3: V.VGGExtractor2, 5: V.VGGExtractor_LN}[vgg](D)


def trace(case):
    """{'train': calls, 'forward_lens': calls} of one case; hipabi.call is put back afterwards."""
    import torch
    from src import hipabi as H
    from src.vgg import forward_lens
    vgg, prec, D, T = case
    prec = H.BF16 if prec == 'bf16' else H.F32
    torch.manual_seed(vgg * 1000 + D + T)
    mod = _extractor(vgg, D).cuda()
    for p in mod.parameters():
        p.grad = torch.zeros_like(p)
    calls, real = [], H.call

    def recording_call(name, *args):
        calls.append([name, [a for a, t in zip(args, H.SIGNATURES[name]) if _is_scalar(t)]])
        real(name, *args)
    out = {}
    H.call = recording_call
    try:
        ctx = types.SimpleNamespace(anchor=torch.zeros(1, device='cuda', requires_grad=True), prec=prec)
        y, _ = mod(torch.rand(B, T, D).cuda(), torch.full((B,), T, dtype=torch.int64), ctx)
        y.backward(torch.randn(y.shape).cuda().to(y.dtype))
        torch.cuda.synchronize()
        out['train'], calls = calls, []
        feat = torch.rand(B, LENS_T, D)
        for b, n in enumerate(LENS):
            feat[b, n:] = 0
        with torch.no_grad():
            forward_lens(mod, feat.cuda(), list(LENS), prec)
        torch.cuda.synchronize()
        out['forward_lens'] = calls
    finally:
        H.call = real
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'g15_vgg_launch_trace.json')
    table = {case_key(c): trace(c) for c in CASES}
    with open(path, 'w') as f:             # one call per line
        f.write('{\n' + ',\n'.join(
            '%s: {\n' % json.dumps(k) + ',\n'.join(
                ' %s: [\n' % json.dumps(part) + ',\n'.join('  ' + json.dumps(c) for c in calls) + '\n ]'
                for part, calls in t.items()) + '\n}' for k, t in table.items()) + '\n}\n')
    names = sorted({c[0] for t in table.values() for calls in t.values() for c in calls})
    print('%s: %d cases, %d calls, %d bytes; entry points: %s' % (
        path, len(table), sum(len(calls) for t in table.values() for calls in t.values()), os.path.getsize(path), ' '.join(names)))


if __name__ == '__main__':
    main()
