"""asr_specaug_policy (csrc/specaug_policy.hip) against the draw rule, the float64 restatement, the case table and the derived bound
of tests/test_specaug_policy_reference.py, through the C entry point (src.hipabi); then SpecAugmentPolicy / create_transform with a
mapping against the explicit chain of entry points, Augment against asr_specaug_ws as before, and one Solver step of
config/debug_specaug.yaml.

Conditions on every call: one guard utterance of NaN behind the B that are passed, in `out` and (as the NaN bit pattern) in
`draws_out`, which must come back untouched; a sentinel in the padding rows t >= len of x; x bit-identical after the call; the
padding rows of `out` equal to those of x bit for bit.

Per case: draws_out equals the restatement exactly (device draws, and draws_in through clamp_record).  A first call with all
counts 0 gives the warped batch: bit for bit x where the warp is off or the rule copies (r == 0), elsewhere inside
      |y - y64| <= 2^-24 (|y64| + 3 (1 + 2^-22) (|x_i| + |x_i+1|))
(derived in the reference file from the four roundings, not measured).  A second call with the masks equals the first bit for bit
outside the bands; inside them it is exactly 0 (fill zero) or one value v per utterance, a float32 neighbour of the float64 mean of
the INPUT with |v - mean64| <= 2^-24 |mean64| + n D 2^-53 max|x|.  The `integer` recipe is bit for bit throughout.  Repeating a
call gives the same bits.  The cases `stride-160` and `stride-26` have more (row, vector) pairs per utterance than one pass of the
grid.

Measured on the MI355X, worst error / bound of the warped values: 0.52 over the table (stride-160; 0.37 - 0.51 in the other warped
cases, 0 where nothing is interpolated), 0.48 at worst with caller-supplied draws.  The numpy emulation of the same arithmetic
with a fused multiply-add reaches 0.52 as well (the reference file prints it), without one 0.68."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import test_frontend_reference as FR
import test_specaug_policy_reference as R

gpu = pytest.mark.gpu
ASR_E_ARG = -1
NAN = float('nan')
NAN_BITS = int(np.array([np.nan], dtype=np.float32).view(np.int32)[0])
BEFORE = -7.5                     # what `out` holds before a call


def _H():
    from src import hipabi as H
    return H


def _call(x, lens, B, T, D, p, seed, draws_in=None, want_draws=True, ws_bytes=None, ws_offset=0, null=(), dims=None, override=None,
          out_at=None, shift=0):
    """x (B + 1, T, D) float32 host array, lens (B) -> (rc, out (B + 1, T, D) host, draws_out (B + 1, 82) host or None, x after).
    override: policy fields by name; out_at: byte offset from x at which `out` is claimed to start (overlap refusals);
    shift: both buffers start `shift` floats behind a 16-byte boundary."""
    H = _H()
    flat = torch.empty(x.size + 4, dtype=torch.float32, device='cuda')
    xd = flat[shift:shift + x.size].view(B + 1, T, D)
    xd.copy_(torch.from_numpy(np.array(x)))
    oflat = torch.full((x.size + 4,), BEFORE, dtype=torch.float32, device='cuda')
    od = oflat[shift:shift + x.size].view(B + 1, T, D)
    od[B] = NAN
    ld = torch.tensor(list(lens) + [T], dtype=torch.int64).cuda()
    dd = torch.full((B + 1, R.REC), -1, dtype=torch.int32).cuda() if want_draws else None
    if dd is not None:
        dd[B] = NAN_BITS
    di = None
    if draws_in is not None:
        di = torch.tensor(np.asarray(list(draws_in) + [[NAN_BITS] * R.REC], dtype=np.int64), dtype=torch.int32).cuda()
    need = H.lib().asr_specaug_policy_workspace_bytes(B)
    ws = torch.full((need // 8 + 8,), NAN, dtype=torch.float64, device='cuda')
    wp = ctypes.c_void_p(ws.data_ptr() + ws_offset)
    cB, cT, cD = dims if dims is not None else (B, T, D)
    q = p._asdict()
    q.update(override or {})
    op = H.ptr(od) if out_at is None else ctypes.c_void_p(xd.data_ptr() + out_at)
    rc = H.lib().asr_specaug_policy(None if 'x' in null else H.ptr(xd), None if 'lens' in null else H.ptr(ld), None if 'out' in null else op,
                                    H.ptr(di), H.ptr(dd), cB, cT, cD, q['warp'], q['fm'], q['fw'], q['tm'], q['tw'], q['tr_pm'], q['tc_pm'],
                                    q['fill'], seed, None if 'ws' in null else wp, need if ws_bytes is None else ws_bytes, H.stream_ptr())
    torch.cuda.synchronize()
    return rc, od.cpu().numpy(), None if dd is None else dd.cpu().numpy(), xd.cpu().numpy()


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


def _judge(c, got, recs, fill, what):
    """`got` (B + 1, T, D) against the restatement under the applied records -> worst error / bound of the warped values."""
    x, B, T, D = c['x'], c['B'], c['T'], c['D']
    assert np.isnan(got[B]).all(), (what, 'the guard utterance of out was written')
    worst = 0.0
    for b, n in enumerate(c['n']):
        rec = recs[b]
        assert _same(got[b, n:], x[b, n:]), (what, b, 'padding rows')
        if n == 0:
            continue
        m = R.band_mask(rec, n, T, D)[:n]
        y64 = R.warp64(x[b], n, rec[0], rec[1])
        bd = R.warp_bound(x[b], n, rec[0], rec[1], y64)
        g = got[b, :n]
        err = np.abs(g.astype(np.float64) - y64)
        copied = ~m & (bd == 0.0)
        assert _same(g[copied], y64.astype(np.float32)[copied]), (what, b, 'rows the rule copies')
        sel = ~m & (bd > 0.0)
        if sel.any():
            ratio = float((err[sel] / bd[sel]).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (what, c['name'], b, ratio)
        if not m.any():
            continue
        if fill:
            assert (g[m] == 0.0).all() and not np.signbit(g[m]).any(), (what, b, 'zero fill')
            continue
        vals = np.unique(g[m])
        assert vals.size == 1, (what, b, 'one fill value per utterance', vals[:4])
        v = float(vals[0])
        mean64 = float(x[b, :n].astype(np.float64).sum() / (n * D))
        near = np.float32(mean64)
        assert v in (float(near), float(np.nextafter(near, np.float32(np.inf))), float(np.nextafter(near, np.float32(-np.inf)))), (what, b, v, mean64)
        assert abs(v - mean64) <= 2.0 ** -24 * abs(mean64) + n * D * 2.0 ** -53 * float(np.abs(x[b, :n]).max()), (what, b, v, mean64)
    return worst


@gpu
@pytest.mark.parametrize('name', R.CASE_NAMES)
def test_policy_vs_float64(name):
    c = R.policy_case(name)
    B, T, D, p, seed, x, lens = c['B'], c['T'], c['D'], c['policy'], c['seed'], c['x'], c['lens']
    assert _H().lib().asr_specaug_policy_workspace_bytes(B) == B * 64 * 8
    guard = np.full(R.REC, NAN_BITS, dtype=np.int32)
    # 1: all counts 0 - the warped batch
    rc, warped, dr, xa = _call(x, lens, B, T, D, c['bare'], seed)
    assert rc == 0 and _same(xa, x), 'x was written'
    assert np.array_equal(dr[:B], np.asarray(c['rec_bare'], dtype=np.int32)) and np.array_equal(dr[B], guard)
    worst = _judge(c, warped, c['rec_bare'], p.fill, 'bare')
    print('RATIO specaug_policy %-12s warp: worst err / bound %.4f' % (name, worst))
    for b, n in enumerate(c['n']):
        if c['rec_bare'][b][0] == 0:
            assert _same(warped[b], x[b]), (b, 'warp off: out = x bit for bit')
    # 2: with the masks - the same bits outside the bands
    rc, got, dr, xa = _call(x, lens, B, T, D, p, seed)
    assert rc == 0 and _same(xa, x)
    assert np.array_equal(dr[:B], np.asarray(c['rec'], dtype=np.int32)) and np.array_equal(dr[B], guard)
    _judge(c, got, c['rec'], p.fill, 'masked')
    for b, n in enumerate(c['n']):
        m = R.band_mask(c['rec'][b], n, T, D)
        assert _same(got[b][~m], warped[b][~m]), (b, 'outside the bands')
    if c['recipe'] == 'integer':
        for b in range(B):
            want = R.policy64(x[b], lens[b], c['rec'][b], p.fill)[0].astype(np.float32)
            assert _same(got[b], want), (b, 'integer recipe')
    # 3: again, and without draws_out: the same bits
    rc, again, dr2, _ = _call(x, lens, B, T, D, p, seed)
    assert rc == 0 and _same(again[:B], got[:B]) and np.array_equal(dr2, dr)
    rc, nodr, _, _ = _call(x, lens, B, T, D, p, seed, want_draws=False)
    assert rc == 0 and _same(nodr[:B], got[:B])
    # 4: draws_in - the device's own record fed back, then one that needs every clamp
    rc, fed, dr3, _ = _call(x, lens, B, T, D, p, seed + 1, draws_in=c['rec'])
    assert rc == 0 and _same(fed[:B], got[:B]) and np.array_equal(dr3, dr)
    foreign = [R.foreign_record(c, b) for b in range(B)]
    applied = [R.clamp_record(foreign[b], c['n'][b], D) for b in range(B)]
    rc, got4, dr4, xa = _call(x, lens, B, T, D, p, seed, draws_in=foreign)
    assert rc == 0 and _same(xa, x)
    assert np.array_equal(dr4[:B], np.asarray(applied, dtype=np.int32)) and np.array_equal(dr4[B], guard)
    if c['recipe'] != 'integer':                     # the foreign record warps: the integer recipe is for the exact path only
        w4 = _judge(c, got4, applied, p.fill, 'draws_in')
        print('RATIO specaug_policy %-12s draws_in: worst err / bound %.4f' % (name, w4))


@gpu
def test_policy_unaligned_rows_take_the_scalar_path():
    """D % 4 == 0 with both buffers one float behind a 16-byte boundary: the same bits as the aligned call."""
    c = R.policy_case('w5-40')
    B, T, D, p, seed = c['B'], c['T'], c['D'], c['policy'], c['seed']
    rc, a, da, _ = _call(c['x'], c['lens'], B, T, D, p._replace(fill=0), seed)
    rc2, s, ds, xa = _call(c['x'], c['lens'], B, T, D, p._replace(fill=0), seed, shift=1)
    assert rc == 0 and rc2 == 0 and _same(a[:B], s[:B]) and np.array_equal(da, ds) and _same(xa, c['x']) and np.isnan(s[B]).all()


@gpu
def test_policy_refusals_leave_out_alone():
    c = R.policy_case('w1-8')
    B, T, D, p, seed, x, lens = c['B'], c['T'], c['D'], c['policy'], c['seed'], c['x'], c['lens']
    need = _H().lib().asr_specaug_policy_workspace_bytes(B)
    bad = [{'null': ('x',)}, {'null': ('lens',)}, {'null': ('out',)}, {'null': ('ws',)},
           {'dims': (0, T, D)}, {'dims': (-1, T, D)}, {'dims': (B, 0, D)}, {'dims': (B, -4, D)}, {'dims': (B, T, 0)}, {'dims': (B, T, -1)},
           {'override': {'fm': -1}}, {'override': {'fm': 9}}, {'override': {'tm': -1}}, {'override': {'tm': 33}},
           {'override': {'warp': -1}}, {'override': {'fw': -1}}, {'override': {'tw': -1}},
           {'override': {'tr_pm': -1}}, {'override': {'tr_pm': 1001}}, {'override': {'tc_pm': -1}}, {'override': {'tc_pm': 1001}},
           {'override': {'fill': -1}}, {'override': {'fill': 2}},
           {'out_at': 0}, {'out_at': 16}, {'out_at': T * D * 4},             # out == x, a little behind it, one utterance behind it
           {'ws_bytes': need - 1}, {'ws_bytes': 0}, {'ws_offset': 4}, {'ws_offset': 1},
           {'override': {'fill': 1}, 'ws_offset': 4}, {'override': {'fill': 1}, 'ws_bytes': need - 1}]
    for kw in bad:
        rc, got, dr, xa = _call(x, lens, B, T, D, p, seed, **kw)
        assert rc == ASR_E_ARG, kw
        assert _H().lib().asr_last_error().decode().startswith('asr_specaug_policy:'), kw
        assert (got[:B] == BEFORE).all() and np.isnan(got[B]).all() and (dr[:B] == -1).all() and _same(xa, x), kw
    # what is accepted: a workspace 8 bytes further on, none at all with fill = zero
    rc, got, _, _ = _call(x, lens, B, T, D, p, seed, ws_offset=8)
    assert rc == 0 and not (got[:B] == BEFORE).any()
    rc, gz, _, _ = _call(x, lens, B, T, D, p, seed, override={'fill': 1}, null=('ws',), ws_bytes=0)
    assert rc == 0 and not (gz[:B] == BEFORE).any()
    lib = _H().lib()
    assert lib.asr_specaug_policy_workspace_bytes(0) == 0 and lib.asr_specaug_policy_workspace_bytes(-3) == 0


# ---- module and chain ----------------------------------------------------------------------------------------------------------------
def _waves():
    wlens = [4 * 160 + 1, 30 * 160, 201, 45 * 160 + 7, 1]
    N = max(wlens)
    wav = torch.zeros(len(wlens), N)
    for b, n in enumerate(wlens):
        wav[b, :n] = torch.from_numpy(FR.fbank_signal('tone+noise', b, n, 9))
    return wlens, N, wav


def _stacked(wav, wlens, N):
    """asr_fbank -> asr_delta_stack through the entry points: ((B, T, 120) on the device, frame lengths tensor, frames)."""
    from src.audio import delta_filters
    H = _H()
    nb, T = len(wlens), FR.n_frames(N, 160)
    frames = [FR.n_frames(n, 160) for n in wlens]
    table, fb, window = FR.tables(1025, 400, 40)
    wd, wl = wav.cuda(), torch.tensor(wlens, dtype=torch.int64).cuda()
    mel = torch.full((nb, T, 40), NAN).cuda()
    nbytes = H.lib().asr_fbank_workspace_bytes(nb, T, 400, 1025)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    tb, fbd, wnd = torch.from_numpy(table).cuda(), torch.from_numpy(fb).cuda(), torch.from_numpy(window).cuda()
    H.call('asr_fbank', H.ptr(wd), H.ptr(wl), H.ptr(mel), H.ptr(tb), H.ptr(fbd), H.ptr(wnd), nb, N, T, 400, 160, 1025, 40,
           0.97, 20.0, -100.0, H.ptr(ws), nbytes, H.stream_ptr())
    filt = torch.from_numpy(delta_filters(2, 2)).cuda()
    fl = torch.tensor(frames, dtype=torch.int64).cuda()
    st = torch.full((nb, T, 120), NAN).cuda()
    H.call('asr_delta_stack', H.ptr(mel), H.ptr(fl), H.ptr(st), H.ptr(filt), nb, T, 40, 3, filt.shape[1], H.stream_ptr())
    return st, fl, frames


SMALL_MAP = {'time_warp': 5, 'freq_masks': 2, 'freq_width': 8, 'time_masks': 3, 'time_width': 10, 'time_ratio': 0.5, 'fill': 'mean'}


@gpu
def test_module_and_create_transform_are_the_chain_of_entry_points():
    """create_transform with a mapping: ExtractAudioFeature, Delta, Postprocess, SpecAugmentPolicy; two calls give bit for bit what
    asr_fbank -> asr_delta_stack -> asr_specaug_policy give with the seeds of the first and the second call."""
    from src.audio import SpecAugmentPolicy, create_transform
    H = _H()
    fe, dim = create_transform({'feat_type': 'fbank', 'feat_dim': 40, 'delta_order': 2, 'augment': dict(SMALL_MAP)}, 'train')
    assert [type(s).__name__ for s in fe.stages] == ['ExtractAudioFeature', 'Delta', 'Postprocess', 'SpecAugmentPolicy'] and dim == 120
    fe = fe.cuda()
    wlens, N, wav = _waves()
    st, fl, frames = _stacked(wav, wlens, N)
    nb, T = st.shape[0], st.shape[1]
    kept = st.clone()
    ws = torch.empty(H.lib().asr_specaug_policy_workspace_bytes(nb) // 8, dtype=torch.float64, device='cuda')
    for call in (1, 2):
        feat, flen = fe(wav.cuda(), torch.tensor(wlens).cuda())
        assert flen.cpu().tolist() == frames and feat.shape == (nb, T, 120)
        ref = torch.full((nb, T, 120), NAN).cuda()
        H.call('asr_specaug_policy', H.ptr(st), H.ptr(fl), H.ptr(ref), None, None, nb, T, 120, 5, 2, 8, 3, 10, 500, 0, 0, call, H.ptr(ws),
               ws.numel() * 8, H.stream_ptr())
        torch.cuda.synchronize()
        assert _same(feat.cpu().numpy(), ref.cpu().numpy()), call
        assert torch.equal(st, kept)
    assert fe.stages[-1].calls == 2
    # the module alone, with a seed and with draws
    m = SpecAugmentPolicy(time_warp=5, freq_masks=1, freq_width=8, time_masks=1, time_width=10, fill='zero', seed=3).cuda()
    assert 'time_warp=5' in repr(m) and 'fill=zero' in repr(m) and 'seed=3' in repr(m)
    out, olens = m(st, fl)
    assert out.data_ptr() != st.data_ptr() and olens.cpu().tolist() == frames and torch.equal(st, kept)
    ref = torch.full((nb, T, 120), NAN).cuda()
    rec = torch.full((nb, R.REC), -1, dtype=torch.int32).cuda()
    H.call('asr_specaug_policy', H.ptr(st), H.ptr(fl), H.ptr(ref), None, H.ptr(rec), nb, T, 120, 5, 1, 8, 1, 10, 1000, 0, 1, 3 * 1000003 + 1,
           None, 0, H.stream_ptr())
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), ref.cpu().numpy())
    first = out.clone()
    out2, _ = m(st, fl, draws=rec)                                        # the second call's seed is not used: the record decides
    assert out2.data_ptr() == out.data_ptr() and torch.equal(out2, first), 'the module keeps its output buffer between calls'
    want = [R.policy_draws(b, frames[b], 120, R.Policy(5, 1, 8, 1, 10, 1000, 0, 1), 3 * 1000003 + 1) for b in range(nb)]
    assert rec.cpu().tolist() == want


@gpu
def test_augment_true_is_still_asr_specaug_ws():
    """create_transform(augment=True): the chain ends in Augment and gives bit for bit what asr_specaug_ws gives, in place."""
    from src.audio import create_transform
    H = _H()
    fe, dim = create_transform({'feat_type': 'fbank', 'feat_dim': 40, 'delta_order': 2, 'augment': True}, 'train')
    assert [type(s).__name__ for s in fe.stages] == ['ExtractAudioFeature', 'Delta', 'Postprocess', 'Augment'] and dim == 120
    fe = fe.cuda()
    wlens, N, wav = _waves()
    st, fl, frames = _stacked(wav, wlens, N)
    nb, T = st.shape[0], st.shape[1]
    for call in (1, 2):
        feat, _ = fe(wav.cuda(), torch.tensor(wlens).cuda())
        ref = st.clone()
        aws = torch.zeros(H.lib().asr_specaug_workspace_bytes(nb), dtype=torch.uint8, device='cuda')
        H.call('asr_specaug_ws', H.ptr(ref), H.ptr(fl), None, None, nb, T, 120, 40, 27, call, H.ptr(aws), aws.numel(), H.stream_ptr())
        torch.cuda.synchronize()
        assert _same(feat.cpu().numpy(), ref.cpu().numpy()), call


# ---- one training step ------------------------------------------------------------------------------------------------------------------
@gpu
def test_one_training_step_with_the_debug_policy(tmp_path):
    """config/debug_specaug.yaml on synthetic-wav: one step through the training Solver gives a finite loss; the training chain ends
    in SpecAugmentPolicy, the validation chain has none, and load_dataset names the policy once."""
    import yaml
    from test_checkpoint_interop import _paras
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'e2e-asr-pytorch_amd')
    sys.path.insert(0, pkg)
    from bin.train_asr import Solver
    from src.data import load_dataset
    cfg = yaml.safe_load(open(os.path.join(pkg, 'config', 'debug_specaug.yaml')))
    cfg['data']['corpus'].update(batch_size=4, subset=8)
    cfg['data']['text']['vocab_file'] = os.path.join(pkg, cfg['data']['text']['vocab_file'])
    cfg['hparas'].update(max_step=1, valid_step=1)
    torch.manual_seed(0)
    solver = Solver(cfg, _paras(tmp_path, name='policy'), 'train')
    solver.load_data()
    solver.set_model()
    solver.validate = lambda *a, **k: None
    seen = {}
    write, fetch = solver.write_log, solver.fetch_data

    def record(log, d):
        if log == 'loss' and 'tr_att' in (d or {}):
            seen['loss'] = float(d['tr_att'].detach())
        return write(log, d)

    def fetched(data, train=False):
        out = fetch(data, train=train)
        seen.setdefault('feat', out[0].clone())
        return out
    solver.write_log, solver.fetch_data = record, fetched
    solver.exec()
    torch.cuda.synchronize()
    stages = [type(s).__name__ for s in solver.tr_set.audio_transform.stages]
    assert stages[-1] == 'SpecAugmentPolicy' and 'Augment' not in stages
    assert 'SpecAugmentPolicy' not in [type(s).__name__ for s in solver.dv_set.audio_transform.stages]
    assert solver.tr_set.audio_transform.stages[-1].calls == 1
    assert np.isfinite(seen['loss']) and torch.isfinite(seen['feat']).all()
    print('RATIO one step of debug_specaug.yaml: loss %.6f' % seen['loss'])
    text = dict(cfg['data']['text'])
    for path, count in (('synthetic', 0), ('synthetic-wav', 1)):
        _, _, _, _, _, msg = load_dataset(0, True, False, False, dict(cfg['data']['corpus'], path=path), dict(cfg['data']['audio']), text)
        assert sum('SpecAugment policy' in m for m in msg) == count, msg
    _, _, _, _, _, msg = load_dataset(0, True, False, False, dict(cfg['data']['corpus']), dict(cfg['data']['audio'], augment=True), text)
    assert not any('SpecAugment policy' in m for m in msg)
