"""Generates g16_rnn_layer_launch_trace.json: every entry point one training step and one batched encoder pass launch, in order,
with the scalar arguments and the stream each launch was issued on - for LSTM encoder stacks on bf16 storage, on fp32 storage
and mixed, with and without the overlap of the backward pass, and for the LSTM language model.  Needs the GPU and the built
library.  The committed fixture was written by the code that preceded the shared layer loop of src/functions.py (two autograd
functions, RNNLayerFn and RNNLayerFastFn, and a third, inference-only copy of both in src/ragged.ragged_layer) and is the record
of the launch sequence that change had to preserve: regenerate it only when a launch is changed on purpose.

    python tests/golden/gen_rnn_layer_launch_trace.py [out.json]     # default: tests/golden/g16_rnn_layer_launch_trace.json

A call is recorded as [name, stream, [the arguments whose declared type in hipabi.SIGNATURES[name] is not a pointer]]: ints,
longs, floats.  stream is 'side' for the side stream (hipabi._side['stream']), 'rec' for another CU-masked stream, 'main'
otherwise: which launches were deferred, at which recurrence they were flushed and which ran in line at the join is part of the
record.  Buffers drop out by construction; the numeric tests hold the wiring.  asr_stream_create_cu_mask is left out by name: it
is no launch, and whether a masked stream already exists depends on what the process ran before.

Every case starts from the same host state (no abort word registered, no decoder work area cached), so that the bookkeeping
launches (asr_scrub_workspace, asr_status_collect) fall where they fall in a fresh process whatever ran before.  'train' is one
src.step.train_step on a fresh model, from its first launch to the return of its hipabi.join_side(); 'encode_chunk' is one
src.ragged.encode_chunk(with_ctc=True) of the same model over rows of 11, 6, 3 and 11 frames."""
import copy
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'e2e-asr-pytorch_amd'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

# hidden width 32 everywhere: the CU split between the recurrence stream and the side stream is the same for all cases
B, T, D, V, L = 4, 11, 40, 31, 3            # T odd: 'drop' keeps ceil(T / 2), 'concat' drops a tail
CHUNK_LENS = [11, 6, 3, 11]                 # 3 frames: shorter than rate^2, still yields a frame
LM_TOKENS = (4, 9)
NOT_A_LAUNCH = ('asr_stream_create_cu_mask',)

MC = {'ctc_weight': 0.5,                    # tests/test_dp_hooks.py: MC
      'encoder': {'vgg': 0, 'vgg_freq': -1, 'vgg_low_filt': -1, 'module': 'LSTM', 'bidirection': True, 'dim': [32, 32, 32],
                  'dropout': [0.1, 0.1, 0.1], 'layer_norm': [False, False, False], 'proj': [True, True, True],
                  'sample_rate': [1, 2, 1], 'sample_style': 'drop'},
      'attention': {'mode': 'loc', 'dim': 24, 'num_head': 1, 'v_proj': False, 'temperature': 0.5, 'loc_kernel_size': 5,
                    'loc_kernel_num': 4},
      'decoder': {'module': 'LSTM', 'dim': 24, 'layer': 1, 'dropout': 0}}

# (name, precision, what differs from MC: encoder keys, or 'ctc_weight', or 'lm'; environment)
CASES = [
    ('bf16 storage', 'bf16', {}, {}),
    ('bf16 storage in line', 'bf16', {}, {'ASR_OVERLAP': '0'}),
    ('fp32 storage', 'fp32', {}, {}),
    ('mixed storages', 'bf16', {'layer_norm': [False, True, False]}, {}),
    # fp32 storage: LayerNorm without down-sampling or dropout (z is the LayerNorm output: no down-sampling launch) with and
    # without projection, LayerNorm over 'concat' rows.  `pj` is sized for the un-concatenated width (as the reference's), so
    # the 'concat' layer of rate 2 runs with the projection off
    ('concat layer_norm no proj', 'bf16', {'sample_style': 'concat', 'layer_norm': [True, True, True], 'proj': [False, False, True],
                                           'dropout': [0, 0.1, 0]}, {}),
    ('one direction', 'bf16', {'bidirection': False}, {}),
    ('ctc only', 'bf16', {'ctc_weight': 1.0}, {}),
    ('lstm lm', 'bf16', {'lm': True}, {}),
]


def case_key(case):
    return case[0]


def _is_scalar(argtype):
    return argtype is not ctypes.c_void_p and not issubclass(argtype, ctypes._Pointer)


def _stream_label(H, torch):
    cur = torch.cuda.current_stream()
    if H._side['stream'] is not None and cur == H._side['stream']:
        return 'side'
    return 'rec' if any(cur == s for s, _h in H._masked.values()) else 'main'


def _asr(prec, diff):
    from oracle import asr_oracle as O
    from src.asr import ASR
    mc = copy.deepcopy(MC)
    for k, v in diff.items():
        if k == 'ctc_weight':
            mc[k] = v
        else:
            mc['encoder'][k] = v
    sd = O.seeded_state_dict(O.param_shapes(O.ModelCfg(mc, D, V)), 3)
    model = ASR(D, V, B, prec=prec, seed=9, **mc)
    model.load_state_dict(sd)
    return model.cuda().train()


def _train_asr(model, H, torch):
    from batchgen import make_batch
    from src.optim import Optimizer
    from src.step import train_step
    from src.util import CTCLoss, CrossEntropyLoss
    feat, lens, txt = [torch.from_numpy(x).cuda() for x in make_batch(5, B, T, D, L, V, min_frac=1.0)]
    opt = Optimizer(model.parameters(), 'Adadelta', 1.0, 1e-8)
    train_step(model, opt, CTCLoss(), CrossEntropyLoss(), feat, lens, txt, L, optimize=False)
    return feat


def _train_lm(H, torch):
    from src.lm import RNNLM
    from src.util import CrossEntropyLoss
    torch.manual_seed(3)
    lm = RNNLM(V, False, 32, 'LSTM', 32, 2, 0.1).cuda().train()
    g = torch.Generator().manual_seed(5)
    x, y = torch.randint(1, V, LM_TOKENS, generator=g).cuda(), torch.randint(1, V, LM_TOKENS, generator=g).cuda()
    out, _ = lm(x, None)
    CrossEntropyLoss(ignore_index=0)(out.view(-1, V), y.view(-1)).backward()
    H.join_side()


def trace(case):
    """{'train': calls[, 'encode_chunk': calls]} of one case; hipabi.call, hipabi.join_side and the environment are put back
    afterwards."""
    import torch
    from src import functions as F_hip
    from src import hipabi as H
    from src import ragged
    _name, prec, diff, env = case
    old_env = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    calls, joins, real_call, real_join = [], [], H.call, H.join_side

    def recording_call(name, *args):
        if name not in NOT_A_LAUNCH:
            calls.append([name, _stream_label(H, torch), [a for a, t in zip(args, H.SIGNATURES[name]) if _is_scalar(t)]])
        real_call(name, *args)

    def counting_join():
        real_join()
        joins.append(len(calls))
    out = {}
    try:
        # the same host state for every case, whatever the process ran before (see the module docstring)
        H.join_side()
        H.collect_status()
        while F_hip._DEC_WS:
            H.handoff_release(F_hip._DEC_WS.popitem()[1])
        torch.cuda.synchronize()
        H.call, H.join_side = recording_call, counting_join
        if diff.get('lm'):
            _train_lm(H, torch)
        else:
            model = _asr(prec, diff)
            feat = _train_asr(model, H, torch)
        torch.cuda.synchronize()
        out['train'] = calls[:joins[-1]]            # through the step's own join_side(): the gradient norm behind it is not the layers'
        if not diff.get('lm'):
            del calls[:]
            ragged.encode_chunk(model, feat, list(CHUNK_LENS), with_ctc=True)
            torch.cuda.synchronize()
            out['encode_chunk'] = list(calls)
    finally:
        H.call, H.join_side = real_call, real_join
        for k, v in old_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'g16_rnn_layer_launch_trace.json')
    table = {case_key(c): trace(c) for c in CASES}
    with open(path, 'w') as f:             # one call per line
        f.write('{\n' + ',\n'.join(
            '%s: {\n' % json.dumps(k) + ',\n'.join(
                ' %s: [\n' % json.dumps(part) + ',\n'.join('  ' + json.dumps(c, separators=(',', ':')) for c in calls) + '\n ]'
                for part, calls in t.items()) + '\n}' for k, t in table.items()) + '\n}\n')
    names = sorted({c[0] for t in table.values() for calls in t.values() for c in calls})
    print('%s: %d cases, %d calls, %d bytes; entry points: %s' % (
        path, len(table), sum(len(calls) for t in table.values() for calls in t.values()), os.path.getsize(path), ' '.join(names)))
    for k, t in table.items():
        print(k, {part: {s: sum(1 for c in calls if c[1] == s) for s in ('main', 'rec', 'side')} for part, calls in t.items()})


if __name__ == '__main__':
    main()
