"""Inference throughput at BASELINE config 4: config/librispeech_asr.yaml (random weights), beam 8, joint CTC weight 0.3,
RNN-LM of config/librispeech_lm.yaml (4 x LSTM-1024, tied, random weights) with weight 0.3, utterances of T frames decoded
U at a time by the device-side beam search (src/decode.BeamDecoder.forward).  Prints one JSON line.
usage: python tools/bench_decode.py [--utts 8] [--frames 400] [--max-len-ratio 0.05] [--reps 3] [--host]
       [--model-yaml PATH] [--attention-mode dot|loc] [--num-head N] [--decoder-module LSTM|GRU] [--lm-module LSTM|GRU]
       [--ctc-only] [--ctc-lm] [--batch-encode] [--lengths equal|librispeech] [--vgg N] [--rescore] [--vocab N] [--no-lm]
       [--profile-out PATH]
--vocab N builds the synthetic model and the LM with N tokens instead of the character table's 31 (above 2048 the joint search runs
asr_beam_candidates_wide / asr_beam_step_wide and the decode step's projection is one contraction); --no-lm leaves the LM out of
the joint search.
The model options decode a variant of the config's model (src/decode_variants.py) instead of the shipped one; --lm-module GRU
fuses a GRU language model of the same dims (csrc/gru_rec.hip) instead of the LSTM one.  --ctc-only decodes the config's
model built with ctc_weight = 1 (no attention decoder, no LM) by the CTC prefix beam search (csrc/ctc_decode.hip) and also
times the search launch alone on the encoded batch.  --ctc-only --ctc-lm fuses the RNN-LM into that search (shallow fusion, the
resumable search asr_ctc_beam_lm_advance) and measures, in one process and alternating, one warm-up each, then the median of
--reps runs: the whole decode without and with the LM, the search loop alone on the encoded batch (every launch of the LM and
of the search between init and read-out), and the advance launches per batch when a launch runs ahead until a slot needs a new
LM row against one frame per launch (max_frames = 1).  --batch-encode measures, in the same process, the encoder pass alone and
the whole decode with the per-utterance encoder pass (the default) and with the length-aware batched one
(BeamDecoder(batch_encode=True), src/ragged.py): one warm-up each, then the median of --reps runs.  --lengths librispeech
draws the U lengths from SURVEY 8d's length model clip(N(1270,480),150,2450) instead of --frames for every utterance.  --vgg N
overrides the yaml's encoder.vgg (0..7: the front-ends of src/vgg.py / src/module.py), so that --batch-encode measures the
batched pass of a front-end model.  --rescore measures, in one process, the joint CTC/attention/LM beam search and two-pass
decoding of the same model (BeamDecoder(rescore=True): CTC prefix beam search, then attention rescoring of its n-best list,
csrc/rescore.hip) without an LM, with the LM in the first pass and with the LM in the second pass (lm_rescore=True: the first pass
runs without it, the LM's full-sequence forward scores the n-best list): one warm-up each, then the median of --reps runs, and for
the two-pass modes one more run with a synchronisation after every phase, which splits the time into encoder, first pass, decoder
pass (teacher table, the 4-byte read of the step count, row expansion, the teacher-forced decoder forward), LM pass (second-pass LM
only: the LM's input table, its forward over chunks of rows, the per-token log-probabilities), rescoring launch and read-back.
With --batch-encode all four use the length-aware batched encoder pass.  The result line also replaces the line of the same
encoder pass in --profile-out (default profiles/rescore_lm_decode.json; '' writes nothing)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'e2e-asr-pytorch_amd')
sys.path.insert(0, ROOT); sys.path.insert(0, PKG)
import torch, yaml
from src.asr import ASR
from src.decode import BeamDecoder
from src.lm import RNNLM
from src import hipabi as H
ap = argparse.ArgumentParser()
ap.add_argument('--utts', type=int, default=8); ap.add_argument('--frames', type=int, default=400)
ap.add_argument('--max-len-ratio', type=float, default=0.05); ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--beam', type=int, default=8); ap.add_argument('--host', action='store_true'); ap.add_argument('--prec', default='bf16')
ap.add_argument('--model-yaml', default=os.path.join(PKG, 'config', 'librispeech_asr.yaml'))
ap.add_argument('--attention-mode'); ap.add_argument('--num-head', type=int); ap.add_argument('--decoder-module')
ap.add_argument('--lm-module', choices=('LSTM', 'GRU'), default='LSTM')
ap.add_argument('--ctc-only', action='store_true'); ap.add_argument('--ctc-lm', action='store_true')
ap.add_argument('--batch-encode', action='store_true'); ap.add_argument('--lengths', choices=('equal', 'librispeech'), default='equal')
ap.add_argument('--vgg', type=int, choices=range(8)); ap.add_argument('--rescore', action='store_true')
ap.add_argument('--vocab', type=int, default=31); ap.add_argument('--no-lm', action='store_true')
ap.add_argument('--profile-out', default=os.path.join(ROOT, 'profiles', 'rescore_lm_decode.json'))
a = ap.parse_args()
torch.manual_seed(0)
mc = yaml.safe_load(open(a.model_yaml))['model']
if a.attention_mode: mc['attention']['mode'] = a.attention_mode
if a.num_head: mc['attention']['num_head'] = a.num_head
if a.decoder_module: mc['decoder']['module'] = a.decoder_module
if a.ctc_only: mc['ctc_weight'] = 1
if a.vgg is not None: mc['encoder']['vgg'] = a.vgg
model = ASR(160, a.vocab, 1, prec=a.prec, **mc).cuda().eval()
lmc = yaml.safe_load(open(os.path.join(PKG, 'config', 'librispeech_lm.yaml')))['model']
lmc['module'] = a.lm_module
lm = RNNLM(a.vocab, **lmc).cuda().eval()
dec = BeamDecoder(model, None, beam_size=a.beam, min_len_ratio=0.01, max_len_ratio=a.max_len_ratio, ctc_weight=0.3)
with_lm = not a.ctc_only and not a.no_lm
if with_lm: dec.set_lm(lm, 0.3)
U, T = a.utts, a.frames
feat = torch.rand(U, T, 160, device='cuda')
flen = torch.full((U,), T, dtype=torch.int64, device='cuda')
if a.lengths == 'librispeech':
    import numpy as np
    ln = np.clip(np.random.RandomState(1234).normal(1270, 480, U), 150, 2450).astype(np.int64)
    T = int(ln.max())
    feat, flen = torch.rand(U, T, 160, device='cuda'), torch.from_numpy(ln).cuda()
    for u in range(U):
        feat[u, int(ln[u]):] = 0
steps = int(-(-T * a.max_len_ratio // 1))
if a.ctc_lm:
    import statistics
    assert a.ctc_only, '--ctc-lm measures the CTC-only search: give --ctc-only too'
    dec_lm = BeamDecoder(model, None, beam_size=a.beam, min_len_ratio=0.01, max_len_ratio=a.max_len_ratio)
    dec_lm.set_lm(lm, 0.3)
    _, _, tlen, lp = dec._encode(feat, flen)
    runs = {'no_lm': lambda: dec(feat, flen), 'lm': lambda: dec_lm(feat, flen), 'search_loop': lambda: dec_lm._forward_ctc_lm(lp, tlen),
            'search_loop_one_frame': lambda: dec_lm._forward_ctc_lm(lp, tlen, max_frames=1)}
    ts, launches = {k: [] for k in runs}, {}
    for rep in range(1 + a.reps):                      # rep 0 = warm-up: workspaces, packed weights, plans
        for name, fn in runs.items():
            torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
            if rep: ts[name].append((time.perf_counter() - t0) * 1e3)
            if name.startswith('search_loop'): launches[name] = dec_lm.launches
    H.raise_if_aborted()
    med = {k: statistics.median(v) for k, v in ts.items()}
    print(json.dumps({'metric': 'CTC prefix beam search with RNN-LM shallow fusion, CTC-only model of config 4', 'batch_utterances': U, 'frames': T,
                      'encoder_frames': int(lp.shape[1]), 'beam': a.beam, 'tokens_extended_per_frame': dec.ctc_cand, 'prec': a.prec,
                      'lm': '4x1024 tied, %s' % a.lm_module, 'lm_weight': 0.3, 'reps': a.reps, 'weights': 'random',
                      'decode_ms_no_lm': med['no_lm'], 'decode_ms_lm': med['lm'], 'utterances_per_s_no_lm': U * 1e3 / med['no_lm'],
                      'utterances_per_s_lm': U * 1e3 / med['lm'], 'search_loop_ms': med['search_loop'],
                      'search_loop_ms_one_frame_per_launch': med['search_loop_one_frame'], 'advance_launches': launches['search_loop'],
                      'advance_launches_one_frame_per_launch': launches['search_loop_one_frame'],
                      'search_loop_ms_per_advance': med['search_loop'] / launches['search_loop']}))
    sys.exit(0)
if a.rescore:
    import statistics
    assert not a.ctc_only, '--rescore decodes a joint model: drop --ctc-only'
    kw = dict(beam_size=a.beam, min_len_ratio=0.01, max_len_ratio=a.max_len_ratio, ctc_weight=0.3, batch_encode=a.batch_encode)
    dec_j = BeamDecoder(model, None, **kw); dec_j.set_lm(lm, 0.3)
    dec_r = BeamDecoder(model, None, rescore=True, **kw)
    dec_rl = BeamDecoder(model, None, rescore=True, **kw); dec_rl.set_lm(lm, 0.3)
    dec_r2 = BeamDecoder(model, None, rescore=True, lm_rescore=True, **kw); dec_r2.set_lm(lm, 0.3)
    runs = {'joint_lm': dec_j, 'rescore': dec_r, 'rescore_lm': dec_rl, 'rescore_lm_second_pass': dec_r2}
    ts = {k: [] for k in runs}
    for rep_ in range(1 + a.reps):                     # rep 0 = warm-up: workspaces, packed weights, plans
        for name, d in runs.items():
            torch.cuda.synchronize(); t0 = time.perf_counter(); out = d(feat, flen); torch.cuda.synchronize()
            if rep_: ts[name].append((time.perf_counter() - t0) * 1e3)
    res = {'metric': 'joint beam search vs two-pass decoding (CTC n-best, attention rescoring; LM in neither, the first or the second pass), config 4', 'batch_utterances': U,
           'lengths': a.lengths, 'frames': flen.tolist() if a.lengths != 'equal' else T, 'beam': a.beam, 'prec': a.prec, 'reps': a.reps,
           'ctc_weight': 0.3, 'lm': '4x1024 tied, %s' % a.lm_module, 'lm_weight': 0.3, 'weights': 'random',
           'encoder_pass': 'batched' if a.batch_encode else 'per utterance'}
    for name in runs:
        ms = statistics.median(ts[name])
        res[name] = {'decode_ms': ms, 'utterances_per_s': U * 1e3 / ms}
    for name in ('rescore', 'rescore_lm', 'rescore_lm_second_pass'):
        stamps = []
        def hook(phase):
            torch.cuda.synchronize(); stamps.append((phase, time.perf_counter()))
        runs[name].phase_hook = hook
        torch.cuda.synchronize(); t0 = time.perf_counter(); out = runs[name](feat, flen)
        runs[name].phase_hook = None
        res[name]['split_ms'] = {ph: (t - tp) * 1e3 for (ph, t), tp in zip(stamps, [t0] + [t for _, t in stamps[:-1]])}
        res[name]['hyps_first_utt'] = len(out[0]) if U > 1 else len(out)
        res[name]['longest_hypothesis'] = max(len(h.outIndex) for hs in (out if U > 1 else [out]) for h in hs)
    # the LM pass's shape: rows per chunk, positions, and the recurrence plan its LSTM layers get (include/asr_hip.h::asr_lstm_plan)
    L2 = res['rescore_lm_second_pass']['longest_hypothesis'] + 1
    rows = min(U * a.beam, dec_r2._rescore_lm_chunk_rows(L2))
    res['rescore_lm_second_pass']['lm_pass'] = {
        'rows': U * a.beam, 'rows_per_chunk': rows, 'positions': L2,
        'lstm_plan': int(H.lib().asr_lstm_plan(rows, L2, lm.dim, 1, model.prec)) if a.lm_module == 'LSTM' else None}
    H.raise_if_aborted()
    line = json.dumps(res)
    print(line)
    if a.profile_out:
        keep = []
        if os.path.exists(a.profile_out):
            keep = [l for l in open(a.profile_out).read().splitlines() if l.strip() and json.loads(l).get('encoder_pass') != res['encoder_pass']]
        os.makedirs(os.path.dirname(os.path.abspath(a.profile_out)), exist_ok=True)
        open(a.profile_out, 'w').write(''.join(l + '\n' for l in sorted(keep + [line], key=lambda l: json.loads(l)['encoder_pass'] == 'batched')))
    sys.exit(0)
if a.batch_encode:
    import statistics
    dec_b = BeamDecoder(model, None, beam_size=a.beam, min_len_ratio=0.01, max_len_ratio=a.max_len_ratio, ctc_weight=0.3, batch_encode=True)
    if with_lm: dec_b.set_lm(lm, 0.3)
    def median_ms(fn):
        fn(); torch.cuda.synchronize()                # warm-up: workspaces, packed weights, plans
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)
    res = {'metric': 'encoder pass per utterance vs batched, %s' % ('CTC-only model of config 4' if a.ctc_only else 'config 4'),
           'batch_utterances': U, 'lengths': a.lengths, 'frames': flen.tolist() if a.lengths != 'equal' else T, 'beam': a.beam,
           'prec': a.prec, 'reps': a.reps, 'vgg': mc['encoder']['vgg'], 'vocab': a.vocab, 'lm': with_lm}
    for name, d in (('per_utterance', dec), ('batched', dec_b)):
        enc_ms = median_ms(lambda: d._encode(feat, flen))
        dec_ms = median_ms(lambda: d(feat, flen))
        res[name] = {'encode_ms': enc_ms, 'decode_ms': dec_ms, 'utterances_per_s': U * 1e3 / dec_ms}
    H.raise_if_aborted()
    res['encode_speedup'] = res['per_utterance']['encode_ms'] / res['batched']['encode_ms']
    res['decode_speedup'] = res['per_utterance']['decode_ms'] / res['batched']['decode_ms']
    print(json.dumps(res))
    sys.exit(0)
def run():
    if a.host:
        return [dec.forward_host(feat[u:u + 1], flen[u:u + 1]) for u in range(U)]
    return dec(feat, flen)
run(); torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(a.reps):
    out = run()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / a.reps
H.raise_if_aborted()
n_hyp = len(out[0]) if (U > 1 or a.host) else len(out)
if a.ctc_only:
    # the search launch alone: the encoded batch is made once, the launch repeated between two events
    _, _, tlen, lp = dec._encode(feat, flen)
    Tp, K = lp.shape[1], a.beam
    i32 = lambda *s_: torch.empty(s_, dtype=torch.int32, device='cuda')
    toks, lens, n, score = i32(U, K, Tp), i32(U, K), i32(U), torch.empty(U, K, device='cuda')
    nb = int(H.lib().asr_ctc_beam_search_workspace_bytes(U, Tp, K))
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(1 + 10):
        if i == 1: ev[0].record()
        H.call('asr_ctc_beam_search', H.ptr(lp), H.ptr(tlen), U, Tp, a.vocab, K, dec.ctc_cand, Tp, H.ptr(toks), H.ptr(lens), H.ptr(score),
               H.ptr(n), H.ptr(ws), nb, H.stream_ptr())
    ev[1].record(); torch.cuda.synchronize()
    print(json.dumps({'metric': 'CTC prefix beam search, CTC-only model of config 4', 'utterances_per_s': U / dt, 'ms_per_utterance': dt * 1e3 / U,
                      'search_launch_ms': ev[0].elapsed_time(ev[1]) / 10, 'batch_utterances': U, 'frames': T, 'encoder_frames': Tp, 'beam': K,
                      'tokens_extended_per_frame': dec.ctc_cand, 'hyps_first_utt': n_hyp, 'prec': a.prec,
                      'first_hyp_len': len((out[0] if U > 1 else out)[0].outIndex)}))
    sys.exit(0)
print(json.dumps({'metric': 'beam-search decode, config 4', 'utterances_per_s': U / dt, 'ms_per_utterance': dt * 1e3 / U,
                  'decode_positions_per_s': U * steps / dt, 'batch_utterances': U, 'frames': T, 'max_positions': steps, 'beam': a.beam,
                  'ctc_weight': 0.3, 'vocab': a.vocab, 'lm': ('4x1024 tied, %s' % a.lm_module) if with_lm else None, 'lm_weight': 0.3 if with_lm else 0.0, 'path': 'host score table' if a.host else 'device beam step',
                  'hyps_first_utt': n_hyp, 'prec': a.prec, 'decoder_path': 'fast' if dec.fast else 'variant',
                  'attention': '%s x%d' % (mc['attention']['mode'], mc['attention']['num_head']), 'decoder': mc['decoder']['module'],
                  'reference_cpu_note': 'BASELINE.md: ~1.0 s per T=400 utterance, reference on 8 CPU cores'}))
