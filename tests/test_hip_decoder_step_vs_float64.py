"""asr_att_decoder_keys + asr_att_decoder_step called the way the search calls them, and the greedy loop of
asr_att_decoder_fwd (teacher == NULL), against the float64 restatement of tests/test_decoder_step_reference.py (R), whose
module docstring states every bound used here with its derivation or its source.

THE STEP.  Every state tensor of F._dec_state is filled with a sentinel, then the caller's part is written: tokens[:, t]
and, for t > 0, random hs / cs and a valid attention row (positive below the row's length, summing to one, zero beyond) at
t-1.  Every row has its own encoder output and length; conv is NULL or saved, key16 == enc16 == NULL; d.B may be below the
allocated rows.  Weights, encoder output and the t-1 state are bf16-representable before either side sees them, so in either
precision every product is exact and what is left is fp32 arithmetic.  Per case, precision and conv mode:
  * stage-forced: each stage's float64 reference takes the device's own previous-stage output (rounded to bf16 where bf16
    contraction mode rounds its operand) - keys, query, saved conv, context, gates, logits within R.contraction_bound /
    R.gate_bounds (tests/test_gemm_reference.py::bound), cs / hs within R.cell_bounds and, from the device's own gates,
    within their rounding part, the attention row within R.att_bound, the embedding rows exactly (tokens clamped to [0, V));
  * unforced, fp32: logits and attention row against the float64 step from the same inputs within F32_TOL of
    tests/test_decoder_dims_vs_oracle.py;
  * footprint: only position t of q, att, xin, gates, cs, hs, logits (and conv when saved) of rows below d.B changes and
    every element of it is written; energy may change below d.B; key and tokens do not change; rows at and above d.B are
    untouched everywhere.
t = -1 and t = L return ASR_E_ARG with nothing written.

THE GREEDY LOOP, through F.att_decoder_forward(model, enc, enc_len, 3, None, prec):
  * tokens[:, 0] == 0 and tokens[b, t+1] is the lowest-index arg-max of the device's own logits[b, t], exactly; with two
    identical rows of Wc and equal winning biases the lower index is fed;
  * oracle.att_decoder in float64, teacher := the tokens the device fed, within _bound of
    tests/test_decoder_dims_vs_oracle.py (imported; bf16 inputs rounded first as there).  Two bf16 points of the narrowest
    decoder (R.BF16_NARROW: V2 logits 3.526e-3 against 3.175e-3, V16385 attention row 9.396e-4 against 9.05e-4, both
    measured on the device) exceed it through operand rounding alone - float64 arithmetic on the rounded operands gives the
    same two figures on the CPU, and every stage-forced check of the step passes - so there, and nowhere else, the named
    tensor gets that point's own operand-rounding deviation on top of _bound, and the device is also held, within the plain
    _bound, to the rounded-operand float64 run (R's docstring);
  * fp32: the fed tokens equal the float64 free run's up to the first position whose float64 top-2 gap is below R.GAP
    (R.test_free_run_margins shows that at least 90 % of the positions lie above it).
dec_greedy_kernel keeps no V-sized row in LDS (each wave carries a running (value, index), the four meet in eight words):
V = 16385 - one entry past a 64 KiB row, the most a launch gets - and V = 65536 - more than a CU's 160 KiB - pin that.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import asr_oracle as O
import test_decoder_dims_vs_oracle as DD
import test_decoder_step_reference as R

pytestmark = pytest.mark.gpu

E_ARG = -1
TOKEN_SENTINEL = -12345
POSITIONAL = ('q', 'att', 'xin', 'gates', 'cs', 'hs', 'logits', 'conv')


def _mods():
    H = DD._hipabi()
    from src import functions as F
    return H, F


def _device_weights(sd, NL, dev):
    f = lambda k: sd[k].to(dev, torch.float32).contiguous()
    al = 'attention.att_layer.'
    T = {'Wq': f('attention.proj_q.weight'), 'bq': f('attention.proj_q.bias'), 'Wk': f('attention.proj_k.weight'),
         'bk': f('attention.proj_k.bias'), 'Wconv': f(al + 'loc_conv.weight'), 'Wproj': f(al + 'loc_proj.weight'),
         'wg': f(al + 'gen_energy.weight'), 'bg': f(al + 'gen_energy.bias'), 'emb': f('pre_embed.weight'),
         'Wc': f('decoder.char_trans.weight'), 'bc': f('decoder.char_trans.bias')}
    for n, k in (('Wih', 'weight_ih'), ('Whh', 'weight_hh'), ('bih', 'bias_ih'), ('bhh', 'bias_hh')):
        T[n] = [f('decoder.layers.%s_l%d' % (k, l)) for l in range(NL)]
    return T


def step_inputs(c, tok=None):
    """The caller's side of one step, float64 / int64 numpy, for all allocated rows."""
    seed = R.case_seed(c)
    rng = np.random.default_rng(seed)
    B, Tp, NL, Dd, t = c['B'], c['Tp'], c['NL'], c['Dd'], c['t']
    sd = R.state_dict(c, seed, bf16=True)
    enc = R.r16(rng.standard_normal((B, Tp, c['E'])))
    lens = R.lengths(c, rng)
    tok = rng.integers(0, c['V'], B) if tok is None else np.asarray(tok, dtype=np.int64)
    hp = cp = prev = None
    if t > 0:
        hp = R.r16(rng.uniform(-1, 1, (B, NL, Dd)))
        cp = R.r16(rng.standard_normal((B, NL, Dd)))
        w = np.where(np.arange(Tp)[None, :] < lens[:, None], rng.uniform(0.05, 1.0, (B, Tp)), 0.0)
        prev = (w / w.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    return dict(sd=sd, enc=enc, lens=lens, tok=tok, hp=hp, cp=cp, prev=prev)


def run_step(c, prec, save_conv, inp, t=None):
    """-> (return code of the step, state before the step, state after it) as dicts of CPU tensors"""
    H, F = _mods()
    dev = torch.device('cuda', torch.cuda.current_device())
    t = c['t'] if t is None else t
    st = F._dec_state(R.dims_of(H, c), dev, save_conv=save_conv)
    assert st['key16'] is None and st['enc16'] is None and (st['conv'] is None) == (not save_conv)
    for k, v in st.items():
        if v is not None:
            v.fill_(TOKEN_SENTINEL if k == 'tokens' else R.SENTINEL)
    tc = min(max(t, 0), c['L'] - 1)                      # the refusal calls keep the caller's part at a valid position
    st['tokens'][:, tc] = torch.from_numpy(inp['tok']).to(dev)
    if tc > 0 and inp['hp'] is not None:
        f32 = lambda a: torch.from_numpy(a).to(dev, torch.float32)
        st['hs'][:, tc - 1], st['cs'][:, tc - 1], st['att'][:, tc - 1] = f32(inp['hp']), f32(inp['cp']), f32(inp['prev'])
    enc = torch.from_numpy(inp['enc']).to(dev, torch.float32).contiguous()
    lens = torch.from_numpy(inp['lens']).to(dev)
    wt = _device_weights(inp['sd'], c['NL'], dev)
    w, s, d = H.dec_weights_struct(wt, c['NL']), H.dec_state_struct(st), R.dims_of(H, c, c['live'])
    p, sp = H.BF16 if prec == 'bf16' else H.F32, H.stream_ptr()
    H.call('asr_att_decoder_keys', ctypes.byref(d), ctypes.byref(w), H.ptr(enc), H.ptr(st['key']), p, sp)
    torch.cuda.synchronize()
    before = {k: v.cpu().clone() for k, v in st.items() if v is not None}
    rc = H.lib().asr_att_decoder_step(ctypes.byref(d), ctypes.byref(w), H.ptr(enc), H.ptr(lens), ctypes.byref(s), t, p, sp)
    torch.cuda.synchronize()
    return rc, before, {k: v.cpu() for k, v in st.items() if v is not None}


def footprint(c, before, after, save_conv):
    bad, live, t = [], c['live'], c['t']
    for k, a in after.items():
        b = before[k]
        if not torch.equal(a[live:], b[live:]):
            bad.append('%s: rows at and above d.B changed' % k)
        if k in POSITIONAL:
            m = torch.ones(a.shape[1], dtype=torch.bool)
            m[t] = False
            if not torch.equal(a[:live][:, m], b[:live][:, m]):
                bad.append('%s: a position other than t changed' % k)
            if bool((a[:live, t] == R.SENTINEL).any()):
                bad.append('%s: position t not fully written' % k)
        elif k in ('key', 'tokens') and not torch.equal(a, b):
            bad.append('%s changed' % k)
    assert ('conv' in after) == save_conv
    return bad


def check_step(c, prec, save_conv, inp, after):
    """Stage-forced and (fp32) unforced comparison of one step; -> list of failures, figures printed first."""
    live, t, NL, Dd, L = c['live'], c['t'], c['NL'], c['Dd'], c['L']
    bf = prec == 'bf16'
    W = R.weights(inp['sd'], NL)
    g = lambda k: after[k][:live].double().numpy()
    cut = lambda a: None if a is None else a[:live]
    enc, lens, tok, hp, cp, prev = (cut(inp[k]) for k in ('enc', 'lens', 'tok', 'hp', 'cp', 'prev'))
    key_k, q_k, att_k, xin_k = g('key'), g('q')[:, t], g('att')[:, t], g('xin')[:, t]
    gates_k, cs_k, hs_k, logits_k = g('gates')[:, t], g('cs')[:, t], g('hs')[:, t], g('logits')[:, t]
    bad, fig = [], []

    def hold(name, got, ref, bound):
        err = np.abs(got - ref)
        bound = np.broadcast_to(bound, err.shape)
        ratio = float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf)).max())
        fig.append('%s %.3g' % (name, ratio))
        if not ratio <= 1.0:
            bad.append('%s: largest error / bound %.3g (error %.3e)' % (name, ratio, float(np.abs(got - ref).max())))

    key_r, key_S = R.stage_keys(enc, W)
    hold('keys', key_k, key_r, R.contraction_bound(key_r, key_S, c['E'], act=True))
    o = R.step(W, c, enc, lens, key_k, tok, hp, cp, prev, force={'q': q_k, 'att': att_k, 'ctx': xin_k[:, Dd:], 'hs': hs_k},
               round_x=bf, uniform_f32=True)
    assert o['top_rounded'] == (bf and c['V'] > 2048)
    hold('query', q_k, o['q'], R.contraction_bound(o['q'], o['q_S'], NL * Dd, act=True))
    if save_conv:
        hold('conv', g('conv')[:, t], o['conv'], R.contraction_bound(o['conv'], o['conv_S'], 2 * c['Ks'] + 1))
    hold('att', att_k, o['att'], R.att_bound(c))
    if bool((att_k[np.arange(c['Tp'])[None, :] >= lens[:, None]] != 0).any()):
        bad.append('att: weight beyond a row\'s length')
    hold('ctx', xin_k[:, Dd:], o['ctx'], R.contraction_bound(o['ctx'], o['ctx_S'], c['Tp']))
    if not (xin_k[:, :Dd] == o['emb']).all():
        bad.append('embedding rows differ from emb[clamp(token)]')
    cpz = cp if cp is not None else np.zeros((live, NL, Dd))
    for l, cell in enumerate(o['cells']):
        d_c, d_h = R.cell_bounds(cell, cpz[:, l])
        hold('gates%d' % l, gates_k[:, l], cell['gates'], R.gate_bounds(cell))
        hold('cs%d' % l, cs_k[:, l], cell['c'], d_c)
        hold('hs%d' % l, hs_k[:, l], cell['h'], d_h)
        own = R.cell_from_gates(gates_k[:, l], cpz[:, l])
        t_c, t_h = R.cell_from_gates_bounds(gates_k[:, l], cpz[:, l], own['c'], own['h'])
        hold('cs%d|gates' % l, cs_k[:, l], own['c'], t_c)
        i_, f_, g_, o_ = (gates_k[:, l, k * Dd:(k + 1) * Dd] for k in range(4))
        hold('hs%d|gates,cs' % l, hs_k[:, l], o_ * np.tanh(cs_k[:, l]), t_h)
    hold('logits', logits_k, o['logits'], R.contraction_bound(o['logits'], o['logits_S'], Dd))
    if not bf:
        u = R.step(W, c, enc, lens, key_r, tok, hp, cp, prev)
        rel = float(np.linalg.norm(logits_k - u['logits']) / (np.linalg.norm(u['logits']) + 1e-30))
        da = float(np.abs(att_k - u['att']).max())
        fig.append('unforced logits %.2e att %.2e' % (rel, da))
        if not rel <= DD.F32_TOL['logits']:
            bad.append('unforced logits: %.3e > %.1e' % (rel, DD.F32_TOL['logits']))
        if not da <= DD.F32_TOL['att']:
            bad.append('unforced att: %.3e > %.1e' % (da, DD.F32_TOL['att']))
    print('%s %s conv %s  error/bound: %s' % (c['id'], prec, 'saved' if save_conv else 'NULL', '  '.join(fig)))
    return bad


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', R.STEP_CASES, ids=[c['id'] for c in R.STEP_CASES])
def test_step_vs_float64(case, prec):
    c, inp, report, first = case, step_inputs(case), [], None
    for save_conv in (False, True):
        rc, before, after = run_step(c, prec, save_conv, inp)
        assert rc == 0, rc
        report += ['conv %s: %s' % ('saved' if save_conv else 'NULL', b)
                   for b in footprint(c, before, after, save_conv) + check_step(c, prec, save_conv, inp, after)]
        if first is None:
            first = after
        else:                                            # saving the convolution changes nothing else
            report += ['%s differs between conv NULL and saved' % k for k in first if k != 'energy' and not torch.equal(first[k], after[k])]
    assert not report, '\n'.join(report)


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('cid', ['Tp9_t0_L3', 'Tp1_t1', 'Dd68_V2049'])
def test_step_clamps_tokens(cid, prec):
    """Tokens of -1 and V + 5 embed rows 0 and V - 1; the token table itself is left as the caller wrote it."""
    c = next(x for x in R.STEP_CASES if x['id'] == cid)
    V = c['V']
    tok = np.array(([-1, V + 5, 0, V - 1, V] * 8)[:c['B']], dtype=np.int64)
    inp = step_inputs(c, tok=tok)
    rc, before, after = run_step(c, prec, True, inp)
    assert rc == 0
    emb = inp['sd']['pre_embed.weight']
    want = emb[torch.from_numpy(np.clip(tok, 0, V - 1))]
    assert torch.equal(after['xin'][:c['live'], c['t'], :c['Dd']], want[:c['live']])
    assert torch.equal(after['tokens'], before['tokens']) and (after['tokens'][:, c['t']].numpy() == tok).all()
    bad = footprint(c, before, after, True) + check_step(c, prec, True, inp, after)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('cid', ['Tp9_t0_L3', 'V2049_B40_live23'])
def test_step_refuses_a_position_outside_the_table(cid):
    c = next(x for x in R.STEP_CASES if x['id'] == cid)
    inp = step_inputs(c)
    for t in (-1, c['L']):
        for prec in ('fp32', 'bf16'):
            rc, before, after = run_step(c, prec, True, inp, t=t)
            assert rc == E_ARG, (t, prec, rc)
            assert all(torch.equal(after[k], before[k]) for k in after), (t, prec)


# ---- the greedy loop -----------------------------------------------------------------------------------------------------------
def run_greedy(c, prec):
    H, F = _mods()
    from src.asr import ASR
    bf = prec == 'bf16'
    sd, enc, lens = R.greedy_inputs(c, bf16=bf)
    model = ASR(DD.D_IN, c['V'], c['B'], prec=prec, **R.model_cfg(c))
    model.load_state_dict(sd)
    model = model.cuda().eval()
    with torch.no_grad():
        d, st = F.att_decoder_forward(model, torch.from_numpy(enc).float().cuda(), torch.from_numpy(lens).cuda(), c['L'], None,
                                      H.BF16 if bf else H.F32)
        torch.cuda.synchronize()
    assert (st['key16'] is not None) == (bf and c['E'] % 4 == 0)
    return sd, enc, lens, st['tokens'].cpu().numpy(), st['logits'].double().cpu().numpy(), st['att'].double().cpu().numpy()


GREEDY_RUNS = [(c, p) for c in R.GREEDY_CASES for p in c['precs']]


@pytest.mark.parametrize('case,prec', GREEDY_RUNS, ids=['%s-%s' % (c['id'], p) for c, p in GREEDY_RUNS])
def test_greedy_loop(case, prec):
    c = case
    L = c['L']
    sd, enc, lens, tokens, logits, att = run_greedy(c, prec)
    # the token choice, on the device's own logits
    assert (tokens[:, 0] == 0).all()
    own = np.argmax(logits, axis=2)                      # numpy returns the first of equal maxima
    assert (tokens[:, 1:] == own[:, :L - 1]).all(), np.argwhere(tokens[:, 1:] != own[:, :L - 1])[:4].tolist()
    if c['tie']:
        i, j = c['tie']
        assert (logits[:, :, i] == logits[:, :, j]).all() and (logits.max(axis=2) == logits[:, :, i]).all()
        assert (tokens[:, 1:] == i).all(), tokens.tolist()
    # the teacher-forced oracle on the tokens the device fed
    teacher = np.concatenate([tokens[:, 1:], np.zeros((c['B'], 1), dtype=np.int64)], axis=1)
    P = {k: v.double() for k, v in sd.items()}
    want_l, want_a = O.att_decoder(torch.from_numpy(enc), torch.from_numpy(lens), P, O.ModelCfg(R.model_cfg(c), DD.D_IN, c['V']), L,
                                   teacher=torch.from_numpy(teacher))
    want_l, want_a = want_l.numpy(), want_a[:, 0].numpy()
    rel = float(np.linalg.norm(logits - want_l) / (np.linalg.norm(want_l) + 1e-30))
    da = float(np.abs(att - want_a).max())
    bl, ba = DD._bound(c, prec, 'logits'), DD._bound(c, prec, 'att')
    if prec == 'bf16' and c['id'] in R.BF16_NARROW:
        # operand rounding alone exceeds the bound here (R's docstring): the named tensor gets the point's own rounding
        # deviation on top, and the device is held to the rounded-operand float64 run within the plain bounds
        emu_l, emu_a, own_l, own_a = R.operand_rounding_deviation(c, sd, enc, lens, teacher, want_l, want_a)
        rel_e = float(np.linalg.norm(logits - emu_l) / (np.linalg.norm(emu_l) + 1e-30))
        da_e = float(np.abs(att - emu_a).max())
        print('%s %s: against the rounded-operand float64 run: logits %.3e att %.3e; that run against the exact one: %.3e %.3e'
              % (c['id'], prec, rel_e, da_e, own_l, own_a))
        assert rel_e <= bl and da_e <= ba
        if R.BF16_NARROW[c['id']] == 'logits':
            bl += own_l
        else:
            ba += own_a
    print('%s %s: logits %.3e (bound %.2e)  att %.3e (bound %.2e)' % (c['id'], prec, rel, bl, da, ba))
    assert rel <= bl and da <= ba
    if prec == 'fp32' and not c['tie']:
        free_l, _, free_tok = R.decode(R.weights(sd, c['NL']), c, enc, lens, L)
        gap = R.top2_gap(free_l)
        compared = 0
        for b in range(c['B']):
            for t in range(L - 1):
                if gap[b, t] < R.GAP:
                    break
                compared += 1
                assert tokens[b, t + 1] == free_tok[b, t + 1], (b, t, int(tokens[b, t + 1]), int(free_tok[b, t + 1]), float(gap[b, t]))
        print('%s: %d of %d choices compared with the float64 free run' % (c['id'], compared, c['B'] * (L - 1)))
        assert compared >= R.MARGIN_SHARE * c['B'] * (L - 1)
