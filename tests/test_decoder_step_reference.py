"""One decode position of the attention decoder, restated stage by stage in float64, with the case tables and the bounds that
tests/test_hip_decoder_step_vs_float64.py holds asr_att_decoder_keys / asr_att_decoder_step and the greedy loop of
asr_att_decoder_fwd (teacher == NULL) to.  This file is the CPU half: the restatement is pinned to
oracle.asr_oracle.att_decoder, the tables are asked - through the host query asr_att_decoder_energy_plan, the only thing
taken from the code under test - which forward energy instantiation each case launches, and the float64 free run is shown to
have the arg-max margins that the GPU's arg-max agreement check relies on.

The stages of one position t (csrc/decoder.hip, per-step kernels; written from oracle/asr_oracle.py::attention_keys,
loc_attention_step and lstm_cell):
  keys     key = tanh(enc Wk^T + bk)                                   once per utterance            asr_gemm, act tanh
  embed    xin[:, :Dd] = emb[clamp(token, 0, V-1)]                                                   embed_kernel
  query    q = tanh(hcat_{t-1} Wq^T + bq),  hcat = 0 at t = 0                                        dec_query_kernel
  conv     conv[k, tau] = sum_j Wconv[k, j] prev[tau + j - Ks],  prev = 1/len below len at t = 0     att_energy_kernel
  energy   e[tau] = (wg . tanh(key[tau] + q + tanh(Wproj conv[:, tau])) + bg) / temperature; -inf at tau >= len
  softmax  att = softmax(e)                                                                          att_softmax_ctx_kernel
  context  xin[:, Dd:] = att . enc
  cell l   pre = x Wih^T + bih + h' Whh^T + bhh; (i, f, g, o) = (sig, sig, tanh, sig)(pre); c = f c' + i g; h = o tanh c
  logits   hs_top Wc^T + bc                                                                          dec_logits_kernel / asr_gemm
Every stage function takes its operands as arguments, so a caller can hand it the previous stage's output of another
implementation (stage forcing); `step` chains them and accepts such outputs through `force`.

Where bf16 contraction mode rounds an operand (round_x): the cell's input row x (embedding | context at layer 0, the lower
layer's h above it) and its h', the query's hcat and, above V = 2048 where the step's projection is a contraction, hs_top.
The energy sweep, the softmax, the context sum and the per-row projection at V <= 2048 are fp32 in both modes (the step is
called with key16 == enc16 == NULL).

BOUNDS (u = 2^-24).  With operands that are bf16-representable before either side sees them, every product of a contraction
is exact in fp32 in either mode and what is left is fp32 summation:
  * contraction stages - keys, query, saved conv, context, gate pre-activations, logits: tests/test_gemm_reference.py::bound,
    |got - ref| <= 2 (K + 2) u S per element with S = sum |a b| + |bias|, K the reduction length (E, Q, 2 Ks + 1, T',
    Kx + Dd, Dd), plus its 2e-6 where a tanh follows (keys, query).
  * gates: d_pre = 2 (K + 2) u S.  sigmoid' <= 1/4 and tanh' <= 1, so d_i, d_f, d_o = d_pre / 4 + 2e-6 and d_g = d_pre + 2e-6
    (2e-6: the same allowance for the device's expf / tanhf as that file's).
  * cs: c = f c' + i g with every factor off by its d:
        d_c = d_f |c'| + d_i (|g| + d_g) + d_g |i| + 3 u (|f c'| + |i g|)
    (first-order terms, the one second-order term, and two products and one sum rounded in fp32).
  * hs: h = o tanh c, tanh' <= 1:   d_h = d_o (|tanh c| + d_c) + |o| d_c + 2e-6 + u |h|.
  * from the device's OWN gates (cell_from_gates) the last two shrink to their rounding part: |c - (f c' + i g)| <=
    3 u (|f c'| + |i g|) and, with the device's own c, |h - o tanh c| <= 2e-6 + u |h|.
  * attention row, stage-forced from the device's key and q: F32_TOL['att'] of tests/test_decoder_dims_vs_oracle.py (1e-5,
    max-abs) times max(1, 0.5 / temperature), that file's temperature rule.
  * unforced fp32 step: that file's F32_TOL - logits 1e-4 relative Frobenius, attention row 1e-5 max-abs.
  * the greedy loop against the teacher-forced oracle: that file's _bound, imported.  Its bf16 figures were measured at the
    bench dims, where every contraction sums 300 or more rounded terms.  At the narrowest decoder of the greedy table
    (Dd = 12) two points exceed them through operand rounding alone: `decode(..., bf16_operands=True)` - float64 arithmetic
    on operands rounded where the bf16 loop rounds them, no kernel in it - is off the exact float64 result by
        V2      (B 3,  V 2,     Dd 12)  logits 3.526e-3 relative Frobenius   (bound 3.175e-3; 18 logits in the norm)
        V16385  (B 17, V 16385, Dd 12)  attention row 9.396e-4 max-abs       (bound 9.05e-4)
    and the device measured exactly these figures (3.526e-3, 9.396e-4) while every stage-forced check of the step passes in
    bf16 mode.  BF16_NARROW lists the two points; test_operand_rounding_alone_exceeds_the_bf16_bound_there shows the
    figures on the CPU, and the GPU test holds those two tensors to _bound + that point's own operand-rounding deviation
    (computed, not recorded) and, within _bound, to the rounded-operand float64 run itself.  No other point is widened.

ARG-MAX MARGIN.  The greedy loop's fp32 tokens are compared with the float64 free run's up to the first position whose
float64 top-2 logit gap is below GAP = 1e-3.  A token can differ from the float64 choice only where two logits err by more
than half the gap, 5e-4; the contraction bound of the projection at the largest decoder width of the table (K = 65, S < 10)
is 8e-5 and the unforced fp32 logits are held to 1e-4 of their norm, so 1e-3 is at least five times what a correct kernel can
be off by and a disagreement above it is a defect.  The check would be empty if most positions fell below GAP:
test_free_run_margins shows, on the float64 free run alone, that at least MARGIN_SHARE = 90 % of the (b, t) positions of the
greedy fp32 cases lie above it.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import asr_oracle as O
import test_decoder_dims_vs_oracle as DD
import test_gemm_reference as G

U24 = 2.0 ** -24
ACT_EPS = 2e-6
GAP = 1e-3
MARGIN_SHARE = 0.9
SENTINEL = -32768.0
BF16_NARROW = {'V2': 'logits', 'V16385': 'att'}          # greedy cases whose bf16 operand rounding alone exceeds _bound (docstring)
PAIRS = [(4, 2), (4, 4), (4, 5), (4, 8), (10, 2), (10, 4), (10, 5), (16, 2), (16, 4)]


def r16(x):
    return G.bf16_round(x)


# ---- weights ---------------------------------------------------------------------------------------------------------------
def model_cfg(c):
    return DD._model_cfg(c)


def state_dict(c, seed, bf16=True):
    """Seeded parameters of the case's model (float32 tensors), bf16-representable when asked."""
    sd = O.seeded_state_dict(O.param_shapes(O.ModelCfg(model_cfg(c), DD.D_IN, c['V'])), seed)
    return {k: v.bfloat16().float() for k, v in sd.items()} if bf16 else sd


def weights(sd, NL):
    """state_dict -> the decoder's operands under the names of asr_dec_weights_t, float64 numpy."""
    f = lambda k: sd[k].detach().double().numpy()
    al = 'attention.att_layer.'
    W = {'Wq': f('attention.proj_q.weight'), 'bq': f('attention.proj_q.bias'), 'Wk': f('attention.proj_k.weight'),
         'bk': f('attention.proj_k.bias'), 'Wconv': f(al + 'loc_conv.weight')[:, 0, :], 'Wproj': f(al + 'loc_proj.weight'),
         'wg': f(al + 'gen_energy.weight')[0], 'bg': f(al + 'gen_energy.bias'), 'emb': f('pre_embed.weight'),
         'Wc': f('decoder.char_trans.weight'), 'bc': f('decoder.char_trans.bias')}
    for n, k in (('Wih', 'weight_ih'), ('Whh', 'weight_hh'), ('bih', 'bias_ih'), ('bhh', 'bias_hh')):
        W[n] = [f('decoder.layers.%s_l%d' % (k, l)) for l in range(NL)]
    return W


# ---- the stages ------------------------------------------------------------------------------------------------------------
def stage_keys(enc, W):
    """-> (key (B,T',A), S)"""
    return np.tanh(enc @ W['Wk'].T + W['bk']), np.abs(enc) @ np.abs(W['Wk']).T + np.abs(W['bk'])


def stage_embed(tok, W):
    return W['emb'][np.clip(tok, 0, W['emb'].shape[0] - 1)]


def stage_query(hcat, W):
    """hcat (B,Q): the layers' h of position t-1 side by side (zero at t = 0) -> (q (B,A), S)"""
    return np.tanh(hcat @ W['Wq'].T + W['bq']), np.abs(hcat) @ np.abs(W['Wq']).T + np.abs(W['bq'])


def initial_att(lens, Tp, f32=False):
    """The attention row before position 0: 1/len below the length.  f32: the quotient as the kernel forms it, in float32."""
    inv = (np.float32(1.0) / lens.astype(np.float32)).astype(np.float64) if f32 else 1.0 / lens.astype(np.float64)
    return np.where(np.arange(Tp)[None, :] < lens[:, None], inv[:, None], 0.0)


def stage_conv(prev, W, Ks):
    """prev (B,T') -> (conv (B,Kn,T'), S), zero padding of Ks on both sides"""
    pad = np.pad(prev, ((0, 0), (Ks, Ks)))
    win = np.lib.stride_tricks.sliding_window_view(pad, 2 * Ks + 1, axis=1)              # (B, T', taps)
    return np.einsum('btj,kj->bkt', win, W['Wconv']), np.einsum('btj,kj->bkt', np.abs(win), np.abs(W['Wconv']))


def stage_energy(key, q, conv, W, lens, temperature):
    """-> energies (B,T') after temperature and mask"""
    loc = np.tanh(conv.transpose(0, 2, 1) @ W['Wproj'].T)
    e = (np.tanh(key + q[:, None, :] + loc) @ W['wg'] + W['bg'][0]) / temperature
    return np.where(np.arange(key.shape[1])[None, :] < lens[:, None], e, -np.inf)


def stage_softmax(e):
    x = np.exp(e - e.max(axis=1, keepdims=True))
    return x / x.sum(axis=1, keepdims=True)


def stage_context(att, enc):
    """-> (ctx (B,E), S)"""
    return np.einsum('bt,bte->be', att, enc), np.einsum('bt,bte->be', np.abs(att), np.abs(enc))


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def stage_cell(x, hp, cp, W, l):
    """x (B,Kx), hp / cp (B,Dd) of position t-1 -> dict: pre, S, K, gates (B,4Dd: i f g o, activated), c, h"""
    Wih, Whh, bih, bhh = W['Wih'][l], W['Whh'][l], W['bih'][l], W['bhh'][l]
    pre = x @ Wih.T + bih + hp @ Whh.T + bhh
    S = np.abs(x) @ np.abs(Wih).T + np.abs(bih) + np.abs(hp) @ np.abs(Whh).T + np.abs(bhh)
    Dd = Whh.shape[1]
    gates = np.concatenate([sigmoid(pre[:, :Dd]), sigmoid(pre[:, Dd:2 * Dd]), np.tanh(pre[:, 2 * Dd:3 * Dd]), sigmoid(pre[:, 3 * Dd:])], axis=1)
    out = cell_from_gates(gates, cp)
    out.update(pre=pre, S=S, K=x.shape[1] + Dd, gates=gates)
    return out


def cell_from_gates(gates, cp):
    Dd = cp.shape[1]
    i, f, g, o = (gates[:, k * Dd:(k + 1) * Dd] for k in range(4))
    c = f * cp + i * g
    return {'c': c, 'h': o * np.tanh(c)}


def stage_logits(h, W):
    return h @ W['Wc'].T + W['bc'], np.abs(h) @ np.abs(W['Wc']).T + np.abs(W['bc'])


# ---- the bounds (module docstring) ----------------------------------------------------------------------------------------
def contraction_bound(ref, S, K, act=False):
    return G.bound(ref, S, K, False, act)


def gate_bounds(cell):
    """-> (B,4Dd) bound of the activated gates of a stage_cell result"""
    d_pre = 2.0 * (cell['K'] + 2) * U24 * cell['S']
    Dd = d_pre.shape[1] // 4
    scale = np.concatenate([np.full(Dd, 0.25), np.full(Dd, 0.25), np.full(Dd, 1.0), np.full(Dd, 0.25)])
    return d_pre * scale[None, :] + ACT_EPS


def cell_bounds(cell, cp):
    """-> (d_c, d_h) of a stage_cell result whose gates are off by gate_bounds"""
    Dd = cp.shape[1]
    d = gate_bounds(cell)
    d_i, d_f, d_g, d_o = (d[:, k * Dd:(k + 1) * Dd] for k in range(4))
    i, f, g, o = (np.abs(cell['gates'][:, k * Dd:(k + 1) * Dd]) for k in range(4))
    d_c = d_f * np.abs(cp) + d_i * (g + d_g) + d_g * i + 3 * U24 * (f * np.abs(cp) + i * g)
    d_h = d_o * (np.abs(np.tanh(cell['c'])) + d_c) + o * d_c + ACT_EPS + U24 * np.abs(cell['h'])
    return d_c, d_h


def cell_from_gates_bounds(gates, cp, c, h):
    Dd = cp.shape[1]
    i, f, g, o = (np.abs(gates[:, k * Dd:(k + 1) * Dd]) for k in range(4))
    return 3 * U24 * (f * np.abs(cp) + i * g), ACT_EPS + U24 * np.abs(h)


def att_bound(c):
    return DD.F32_TOL['att'] * max(1.0, DD.BENCH['temp'] / c['temp'])


# ---- one position -----------------------------------------------------------------------------------------------------------
def step(W, c, enc, lens, key, tok, hp, cp, prev, force=None, round_x=False, uniform_f32=False, round_top=None):
    """Position t of the decoder on float64 arrays.  tok (B,) input tokens; hp, cp (B,NL,Dd) and prev (B,T') the state of
    position t-1, None at t = 0.  force: outputs of another implementation - 'q', 'att', 'ctx', 'hs' (B,NL,Dd: layer l-1 feeds
    layer l, the top layer the projection) - that the following stage takes instead of this function's own.  round_x: round
    where bf16 contraction mode does (module docstring); round_top: whether the projection rounds hs_top (default: as
    asr_att_decoder_step does, above V = 2048 in bf16 mode).  -> dict of every stage's output, S and K."""
    force = force or {}
    rx = r16 if round_x else (lambda a: a)
    B, NL, Dd = len(tok), c['NL'], c['Dd']
    if hp is None:
        hp, cp, prev = np.zeros((B, NL, Dd)), np.zeros((B, NL, Dd)), initial_att(lens, c['Tp'], uniform_f32)
    out = {}
    out['q'], out['q_S'] = stage_query(rx(hp.reshape(B, NL * Dd)), W)
    out['conv'], out['conv_S'] = stage_conv(prev, W, c['Ks'])
    out['energy'] = stage_energy(key, force.get('q', out['q']), out['conv'], W, lens, c['temp'])
    out['att'] = stage_softmax(out['energy'])
    out['ctx'], out['ctx_S'] = stage_context(force.get('att', out['att']), enc)
    out['emb'] = stage_embed(tok, W)
    x = rx(np.concatenate([out['emb'], force.get('ctx', out['ctx'])], axis=1))
    out['cells'] = []
    for l in range(NL):
        cell = stage_cell(x, rx(hp[:, l]), cp[:, l], W, l)
        out['cells'].append(cell)
        x = rx(force['hs'][:, l] if 'hs' in force else cell['h'])
    out['top_rounded'] = bool(round_x and c['V'] > 2048) if round_top is None else bool(round_top)
    top = force['hs'][:, NL - 1] if 'hs' in force else out['cells'][-1]['h']
    out['logits'], out['logits_S'] = stage_logits(r16(top) if out['top_rounded'] else top, W)
    return out


def decode(W, c, enc, lens, L, teacher=None, bf16_operands=False):
    """L positions chained from the zero state: teacher (B,L) forced (teacher[:, t] is the input of position t+1, as
    oracle.att_decoder reads it) or, without one, fed with the lowest-index arg-max.  bf16_operands: float64 arithmetic on
    operands rounded where the greedy bf16 loop of asr_att_decoder_fwd rounds them (round_x of `step`; the keys, of which the
    loop reads its bf16 working copy; not hs_top: dec_greedy_kernel projects in fp32 at every V) - what bf16 contraction mode costs by itself, with no kernel in it.  -> logits (B,L,V),
    att (B,L,T'), tokens (B,L) as fed."""
    B = enc.shape[0]
    key, _ = stage_keys(enc, W)
    if bf16_operands:
        key = r16(key)
    tok, hp, cp, prev = np.zeros(B, dtype=np.int64), None, None, None
    logits, att, fed = [], [], []
    for t in range(L):
        o = step(W, c, enc, lens, key, tok, hp, cp, prev, round_x=bf16_operands, round_top=False)
        fed.append(tok)
        logits.append(o['logits'])
        att.append(o['att'])
        hp = np.stack([cell['h'] for cell in o['cells']], axis=1)
        cp = np.stack([cell['c'] for cell in o['cells']], axis=1)
        prev = o['att']
        tok = teacher[:, t] if teacher is not None else np.argmax(o['logits'], axis=1)
    return np.stack(logits, axis=1), np.stack(att, axis=1), np.stack(fed, axis=1)


def top2_gap(logits):
    s = np.sort(logits, axis=-1)
    return s[..., -1] - s[..., -2]


# ---- the tables -------------------------------------------------------------------------------------------------------------
def _step(cid, B, Tp, E, A, Dd, NL, Kn, Ks, temp, V, t, L, lens, live=None):
    return dict(id=cid, B=B, Tp=Tp, E=E, A=A, Dd=Dd, NL=NL, Kn=Kn, Ks=Ks, temp=temp, V=V, t=t, L=L, lens=lens, live=live or B, scale=1.0)


# live: d.B of the call, below the allocated rows B (the search's forward_host sets it to the live hypotheses)
#                                      B   T'    E   A   Dd NL  Kn  Ks  temp  V     t  L  lengths
STEP_CASES = [
    _step('smallest',                  1,  1,    16, 16, 12, 1, 1,  0,  1.0,  2,    0, 1, 'full'),
    _step('Tp1_t1',                    5,  1,    16, 24, 12, 2, 4,  1,  0.5,  31,   1, 3, 'full'),
    _step('Tp9_t0_L3',                 5,  9,    16, 16, 12, 1, 5,  7,  0.5,  31,   0, 3, 'mixed'),
    _step('Ks_wider_than_Tp',          16, 9,    34, 24, 37, 1, 4,  40, 0.25, 31,   1, 3, 'mixed'),
    _step('Ks_wider_than_Tp_t0',       5,  9,    16, 37, 12, 1, 10, 40, 1.0,  31,   0, 1, 'one'),
    _step('Q_not_mult4',               17, 9,    34, 37, 37, 2, 11, 1,  0.5,  31,   2, 3, 'one'),
    _step('NL4_Dd37',                  5,  9,    72, 24, 37, 4, 16, 7,  1.0,  31,   1, 3, 'mixed'),
    _step('NL4_Dd12_t0',               16, 9,    16, 16, 12, 4, 1,  0,  0.5,  2,    0, 3, 'full'),
    _step('Dd64_V2048',                17, 9,    72, 37, 64, 2, 4,  7,  0.5,  2048, 2, 3, 'mixed'),
    _step('Dd68_V2049',                17, 9,    72, 37, 68, 2, 5,  1,  0.5,  2049, 1, 3, 'mixed'),
    _step('V2049_one_row',             1,  9,    16, 16, 12, 1, 4,  1,  1.0,  2049, 0, 1, 'full'),
    _step('V2048_B40',                 40, 9,    16, 16, 12, 1, 4,  1,  0.25, 2048, 1, 3, 'one'),
    _step('V2049_B40_live23',          40, 9,    34, 16, 64, 1, 10, 0,  0.5,  2049, 2, 3, 'mixed', live=23),
    _step('B40_live16',                40, 161,  16, 24, 12, 2, 11, 7,  0.5,  31,   1, 3, 'mixed', live=16),
    _step('B17_live1',                 17, 9,    72, 16, 68, 1, 16, 1,  1.0,  31,   2, 3, 'full', live=1),
    _step('Tp161_ctx_second_trip',     5,  161,  72, 37, 64, 1, 16, 40, 0.5,  31,   1, 3, 'full'),
    _step('Tp161_len1',                16, 161,  34, 16, 12, 1, 5,  7,  0.25, 2,    2, 3, 'one'),
    _step('Tp1025_stage_tail',         5,  1025, 16, 16, 12, 1, 4,  7,  0.5,  31,   1, 3, 'full'),
    _step('Tp1025_mixed_E34',          1,  1025, 34, 24, 37, 1, 10, 40, 1.0,  31,   0, 3, 'full'),
    # the forward energy kernel's tiles at 17 rows (asr_att_decoder_energy_plan is asked in test_step_table_reaches_every_tile)
    _step('tile_4_2',                  17, 161,  16, 16, 12, 1, 4,  1,  0.5,  31,   1, 3, 'mixed'),
    _step('tile_4_4',                  17, 250,  16, 24, 12, 1, 4,  7,  0.5,  31,   1, 3, 'mixed'),
    _step('tile_4_5',                  17, 500,  16, 16, 12, 1, 1,  40, 0.25, 31,   2, 3, 'one'),
    _step('tile_4_8',                  17, 620,  72, 16, 12, 1, 4,  0,  1.0,  31,   1, 3, 'mixed'),
    _step('tile_10_2',                 17, 161,  16, 37, 12, 1, 5,  7,  0.5,  31,   0, 3, 'mixed'),
    _step('tile_10_4',                 17, 250,  34, 16, 12, 1, 10, 1,  0.5,  31,   1, 3, 'full'),
    _step('tile_10_5',                 17, 500,  16, 24, 12, 2, 10, 7,  1.0,  31,   2, 3, 'mixed'),
    _step('tile_10_5_B40',             40, 620,  16, 16, 12, 1, 5,  1,  0.5,  2,    1, 3, 'mixed'),
    _step('tile_16_2',                 17, 161,  16, 16, 12, 1, 11, 40, 0.5,  31,   1, 3, 'one'),
    _step('tile_16_4',                 17, 250,  72, 37, 12, 1, 16, 7,  0.25, 31,   2, 3, 'mixed'),
    _step('tile_16_4_Tp620',           17, 620,  16, 16, 12, 1, 11, 0,  0.5,  31,   0, 1, 'full'),
]
STEP_VALUES = {'B': (1, 5, 16, 17, 40), 'Tp': (1, 9, 161, 250, 500, 620, 1025), 'E': (16, 34, 72), 'A': (16, 24, 37),
               'Dd': (12, 37, 64, 68), 'NL': (1, 2, 4), 'Kn': (1, 4, 5, 10, 11, 16), 'Ks': (0, 1, 7, 40), 'temp': (0.25, 0.5, 1.0),
               'V': (2, 31, 2048, 2049), 'L': (1, 3), 'lens': ('full', 'one', 'mixed')}


def _greedy(cid, B, V, Dd, precs=('fp32', 'bf16'), tie=None, **kw):
    c = dict(id=cid, B=B, Tp=9, E=16, A=16, Dd=Dd, NL=1, Kn=4, Ks=1, temp=0.5, V=V, L=3, lens='mixed', scale=1.0, precs=precs, tie=tie)
    c.update(kw)
    return c


# tie: (i, j) - rows i < j of Wc made identical with equal, winning biases; i is what must be fed
GREEDY_CASES = [
    _greedy('V2', 3, 2, 12),
    _greedy('V2_B17', 17, 2, 65),
    _greedy('V31', 1, 31, 40),
    _greedy('V31_B17_NL2', 17, 31, 12, NL=2),
    _greedy('V31_tie_across_waves', 3, 31, 40, tie=(6, 9)),
    _greedy('V2048', 17, 2048, 65),
    _greedy('V2049', 3, 2049, 12),
    _greedy('V16384', 1, 16384, 40),
    _greedy('V16385', 17, 16385, 12),
    _greedy('V16385_tie_in_one_wave', 3, 16385, 65, tie=(16001, 16381)),
    _greedy('V65536', 3, 65536, 65),
    _greedy('V65536_B17', 17, 65536, 40),
]
# bf16 with the half copies (E % 4 == 0): the nine tiles of the step table
for _c in STEP_CASES:
    if _c['id'] in ('tile_4_2', 'tile_4_4', 'tile_4_5', 'tile_4_8', 'tile_10_2', 'tile_10_4', 'tile_10_5', 'tile_16_2', 'tile_16_4'):
        GREEDY_CASES.append(_greedy('bf16_' + _c['id'], _c['B'], 31, 12, precs=('bf16',), Tp=_c['Tp'], E=_c['E'] if _c['E'] % 4 == 0 else 16,
                                    A=_c['A'], Kn=_c['Kn'], Ks=_c['Ks'], temp=_c['temp'], lens=_c['lens']))
GREEDY_VALUES = {'B': (1, 3, 17), 'V': (2, 31, 2048, 2049, 16384, 16385, 65536), 'Dd': (12, 40, 65)}


def case_seed(c):
    return 100 + [x['id'] for x in STEP_CASES + GREEDY_CASES].index(c['id'])


def lengths(c, rng):
    B, Tp = c['B'], c['Tp']
    if c['lens'] == 'full':
        return np.full(B, Tp, dtype=np.int64)
    lens = rng.integers(max(Tp // 3, 1), Tp + 1, B).astype(np.int64)
    lens[0] = Tp
    if c['lens'] == 'one':
        lens[min(1, B - 1)] = 1
    return lens


def greedy_inputs(c, bf16):
    """-> (state_dict, enc (B,T',E) float64, lens) of a greedy case; bf16: rounded as bf16 contraction mode's inputs are."""
    rng = np.random.default_rng(case_seed(c))
    sd = state_dict(c, case_seed(c), bf16=bf16)
    if c['tie']:
        i, j = c['tie']
        Wc, bc = sd['decoder.char_trans.weight'], sd['decoder.char_trans.bias']
        Wc[j] = Wc[i]
        bc[i] = bc[j] = 48.0
    enc = rng.standard_normal((c['B'], c['Tp'], c['E'])).astype(np.float32)
    enc = r16(enc) if bf16 else enc.astype(np.float64)
    return sd, enc, lengths(c, rng)


# ---- the restatement against the oracle ---------------------------------------------------------------------------------------
def _oracle_cfg(c):
    return O.ModelCfg(model_cfg(c), DD.D_IN, c['V'])


PINNED = ['Tp9_t0_L3', 'Ks_wider_than_Tp', 'NL4_Dd37', 'Dd68_V2049', 'Tp161_len1']


@pytest.mark.parametrize('cid', PINNED)
def test_chained_stages_reproduce_the_oracle(cid):
    """L positions from the zero state, teacher-forced, without forcing any stage: oracle.att_decoder in float64, to rounding."""
    c = dict(next(x for x in STEP_CASES if x['id'] == cid), L=3)
    assert cid != 'NL4_Dd37' or c['NL'] == 4
    assert cid != 'Ks_wider_than_Tp' or c['Ks'] > c['Tp']
    rng = np.random.default_rng(case_seed(c))
    sd = state_dict(c, case_seed(c), bf16=False)
    enc = rng.standard_normal((c['B'], c['Tp'], c['E']))
    lens = lengths(c, rng)
    teacher = rng.integers(0, c['V'], (c['B'], c['L']))
    P = {k: v.double() for k, v in sd.items()}
    want_l, want_a = O.att_decoder(torch.from_numpy(enc), torch.from_numpy(lens), P, _oracle_cfg(c), c['L'], teacher=torch.from_numpy(teacher))
    got_l, got_a, fed = decode(weights(sd, c['NL']), c, enc, lens, c['L'], teacher=teacher)
    assert (fed[:, 0] == 0).all() and (fed[:, 1:] == teacher[:, :-1]).all()
    assert np.abs(got_l - want_l.numpy()).max() <= 1e-12 * max(1.0, np.abs(got_l).max())
    assert np.abs(got_a - want_a[:, 0].numpy()).max() <= 1e-13


def test_free_run_reproduces_the_oracles_greedy_loop():
    c = next(x for x in GREEDY_CASES if x['id'] == 'V31_B17_NL2')
    sd, enc, lens = greedy_inputs(c, bf16=False)
    P = {k: v.double() for k, v in sd.items()}
    want_l, want_a = O.att_decoder(torch.from_numpy(enc), torch.from_numpy(lens), P, _oracle_cfg(c), c['L'])
    got_l, got_a, fed = decode(weights(sd, c['NL']), c, enc, lens, c['L'])
    assert np.abs(got_l - want_l.numpy()).max() <= 1e-12 and np.abs(got_a - want_a[:, 0].numpy()).max() <= 1e-13
    assert (fed[:, 1:] == want_l.numpy().argmax(axis=2)[:, :-1]).all()


def test_forcing_replaces_a_stage_output():
    """A forced output reaches exactly the stages behind it: forcing this function's own outputs changes nothing, forcing q
    moves the attention row and everything after it and leaves q itself and the convolution alone."""
    c = next(x for x in STEP_CASES if x['id'] == 'NL4_Dd37')
    rng = np.random.default_rng(3)
    W = weights(state_dict(c, 3), c['NL'])
    B = c['B']
    enc, lens = r16(rng.standard_normal((B, c['Tp'], c['E']))), lengths(c, rng)
    key, _ = stage_keys(enc, W)
    hp, cp = r16(rng.uniform(-1, 1, (B, c['NL'], c['Dd']))), r16(rng.standard_normal((B, c['NL'], c['Dd'])))
    prev = initial_att(lens, c['Tp'])
    tok = rng.integers(0, c['V'], B)
    a = step(W, c, enc, lens, key, tok, hp, cp, prev)
    own = {'q': a['q'], 'att': a['att'], 'ctx': a['ctx'], 'hs': np.stack([x['h'] for x in a['cells']], axis=1)}
    b = step(W, c, enc, lens, key, tok, hp, cp, prev, force=own)
    assert (b['logits'] == a['logits']).all() and (b['att'] == a['att']).all()
    f = step(W, c, enc, lens, key, tok, hp, cp, prev, force={'q': a['q'] + 0.25})
    assert (f['q'] == a['q']).all() and (f['conv'] == a['conv']).all()
    assert np.abs(f['att'] - a['att']).max() > 1e-4 and np.abs(f['logits'] - a['logits']).max() > 1e-6
    g = step(W, c, enc, lens, key, tok, hp, cp, prev, force={'hs': own['hs'] * 0.5})
    assert (g['cells'][1]['pre'] != a['cells'][1]['pre']).any() and (g['cells'][0]['pre'] == a['cells'][0]['pre']).all()
    assert (g['ctx'] == a['ctx']).all() and (g['logits'] != a['logits']).any()
    # rounding where bf16 contraction mode rounds: the context enters the cell rounded, the attention row is untouched by it
    r = step(W, c, enc, lens, key, tok, hp, cp, prev, round_x=True)
    assert (r['att'] == a['att']).all() and (r['cells'][0]['pre'] != a['cells'][0]['pre']).any()
    x = r16(np.concatenate([a['emb'], a['ctx']], axis=1))
    assert (r['cells'][0]['pre'] == stage_cell(x, hp[:, 0], cp[:, 0], W, 0)['pre']).all()
    assert not r['top_rounded']


def test_token_clamp_and_masks():
    c = next(x for x in STEP_CASES if x['id'] == 'Tp9_t0_L3')
    W = weights(state_dict(c, 5), c['NL'])
    V = c['V']
    assert (stage_embed(np.array([-1, V + 5, 3]), W) == W['emb'][[0, V - 1, 3]]).all()
    lens = np.array([9, 1, 4, 9, 2])
    p0 = initial_att(lens, 9)
    assert np.allclose(p0.sum(axis=1), 1.0) and (p0[1, 1:] == 0).all() and p0[1, 0] == 1.0
    rng = np.random.default_rng(0)
    enc = rng.standard_normal((5, 9, c['E']))
    key, _ = stage_keys(enc, W)
    o = step(W, c, enc, lens, key, np.zeros(5, dtype=np.int64), None, None, None)
    assert (o['att'][np.arange(9)[None, :] >= lens[:, None]] == 0).all() and np.allclose(o['att'].sum(axis=1), 1.0)
    assert o['att'][1, 0] == 1.0


def test_cell_bounds_cover_a_float32_cell():
    """The propagated cs / hs bounds hold for the same cell evaluated in float32 at the widest layer of the step table (numpy's
    float32 matmul and transcendental functions standing in for a correct kernel), and stay below 1e-3 there: a gate that is
    off by 2e-3 stands above them."""
    rng = np.random.default_rng(1)
    B, Kx, Dd = 16, 140, 68
    W = {'Wih': [r16(rng.standard_normal((4 * Dd, Kx)) / np.sqrt(Kx))], 'Whh': [r16(rng.standard_normal((4 * Dd, Dd)) / np.sqrt(Dd))],
         'bih': [r16(rng.standard_normal(4 * Dd) * 0.1)], 'bhh': [r16(rng.standard_normal(4 * Dd) * 0.1)]}
    x, hp, cp = r16(rng.standard_normal((B, Kx))), r16(rng.uniform(-1, 1, (B, Dd))), r16(rng.standard_normal((B, Dd)))
    ref = stage_cell(x, hp, cp, W, 0)
    f = np.float32
    pre = (x.astype(f) @ W['Wih'][0].astype(f).T + W['bih'][0].astype(f)) + (hp.astype(f) @ W['Whh'][0].astype(f).T + W['bhh'][0].astype(f))
    sg = lambda v: (f(1) / (f(1) + np.exp(-v))).astype(f)
    i, fg, g, o = sg(pre[:, :Dd]), sg(pre[:, Dd:2 * Dd]), np.tanh(pre[:, 2 * Dd:3 * Dd]), sg(pre[:, 3 * Dd:])
    c32 = fg * cp.astype(f) + i * g
    h32 = o * np.tanh(c32)
    d_c, d_h = cell_bounds(ref, cp)
    assert (np.abs(np.concatenate([i, fg, g, o], axis=1) - ref['gates']) <= gate_bounds(ref)).all()
    assert (np.abs(c32 - ref['c']) <= d_c).all() and (np.abs(h32 - ref['h']) <= d_h).all()
    print('largest bounds: gates %.2e cs %.2e hs %.2e' % (gate_bounds(ref).max(), d_c.max(), d_h.max()))
    assert d_c.max() < 1e-3 and d_h.max() < 1e-3 and gate_bounds(ref).max() < 1e-3


# ---- which energy instantiation a case launches -------------------------------------------------------------------------------
def dims_of(H, c, rows=None):
    d = H.DecDims()
    d.B, d.Tp, d.E, d.A = rows or c['B'], c['Tp'], c['E'], c['A']
    d.Q, d.Dd, d.NL, d.V = c['Dd'] * c['NL'], c['Dd'], c['NL'], c['V']
    d.Kn, d.Ks, d.L = c['Kn'], c['Ks'], c['L']
    d.temperature = float(c['temp'])
    return d


def energy_tile(H, c, rows=None):
    kn, tpw = ctypes.c_int(-1), ctypes.c_int(-1)
    H.call('asr_att_decoder_energy_plan', ctypes.byref(dims_of(H, c, rows)), ctypes.byref(kn), ctypes.byref(tpw))
    return kn.value, tpw.value


def test_step_table_reaches_every_tile():
    """Every (KNMAX, TPW) instantiation of the forward energy kernel with H16 off (the step is called without the half
    copies), and every value the table is meant to visit."""
    H = DD._hipabi()
    reached = {}
    for c in STEP_CASES:
        reached.setdefault(energy_tile(H, c, c['live']), []).append(c['id'])
    print('H16 off:', {k: v for k, v in sorted(reached.items())})
    assert sorted(reached) == PAIRS, sorted(reached)
    for c in STEP_CASES:
        if c['id'].startswith('tile_'):
            assert energy_tile(H, c, c['live']) == tuple(int(x) for x in c['id'].split('_')[1:3]), c['id']
    for k, vals in STEP_VALUES.items():
        assert {c[k] for c in STEP_CASES} == set(vals), k
    assert {0, 1} <= {c['t'] for c in STEP_CASES} and any(c['t'] == c['L'] - 1 and c['L'] == 3 for c in STEP_CASES)
    assert all(0 <= c['t'] < c['L'] and 1 <= c['live'] <= c['B'] for c in STEP_CASES)
    assert any(c['live'] < c['B'] for c in STEP_CASES) and any(c['Ks'] == 40 and c['Tp'] == 9 for c in STEP_CASES)
    assert len({c['id'] for c in STEP_CASES + GREEDY_CASES}) == len(STEP_CASES) + len(GREEDY_CASES)


def test_greedy_table_reaches_every_tile_with_half_copies():
    """Every (KNMAX, TPW) instantiation with H16 on: bf16 greedy cases with E % 4 == 0 run on the half copies."""
    H = DD._hipabi()
    reached = {}
    for c in GREEDY_CASES:
        if 'bf16' in c['precs'] and c['E'] % 4 == 0:
            reached.setdefault(energy_tile(H, c), []).append(c['id'])
    print('H16 on:', {k: v for k, v in sorted(reached.items())})
    assert sorted(reached) == PAIRS, sorted(reached)
    main = [c for c in GREEDY_CASES if c['precs'] == ('fp32', 'bf16')]
    for k, vals in GREEDY_VALUES.items():
        assert {c[k] for c in main} == set(vals), k
    assert all(c['L'] == 3 for c in GREEDY_CASES)
    assert all(c['E'] == 16 and c['A'] == 16 and c['Tp'] == 9 for c in main if c['V'] > 2049)


def test_energy_plan_query_refuses_what_the_step_refuses():
    H = DD._hipabi()
    c = dict(STEP_CASES[0])
    kn, tpw = ctypes.c_int(-1), ctypes.c_int(-1)
    lib = H.lib()
    assert lib.asr_att_decoder_energy_plan(None, ctypes.byref(kn), ctypes.byref(tpw)) != 0
    assert lib.asr_att_decoder_energy_plan(ctypes.byref(dims_of(H, dict(c, Kn=17))), ctypes.byref(kn), ctypes.byref(tpw)) != 0
    assert (kn.value, tpw.value) == (-1, -1)
    assert lib.asr_att_decoder_energy_plan(ctypes.byref(dims_of(H, dict(c, Kn=16))), ctypes.byref(kn), ctypes.byref(tpw)) == 0
    assert (kn.value, tpw.value) == (16, 2)


# ---- the margins of the float64 free run --------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', [c['id'] for c in GREEDY_CASES if 'fp32' in c['precs'] and not c['tie']])
def test_free_run_margins(cid):
    """The cap on the arg-max agreement check (module docstring): of the positions whose logits choose a fed token
    (t < L - 1), at least MARGIN_SHARE have a float64 top-2 gap above GAP, in every case and so over all of them."""
    c = next(x for x in GREEDY_CASES if x['id'] == cid)
    sd, enc, lens = greedy_inputs(c, bf16=False)
    logits, _, _ = decode(weights(sd, c['NL']), c, enc, lens, c['L'])
    gap = top2_gap(logits[:, :c['L'] - 1])
    share = float((gap > GAP).mean())
    print('%s: %d positions, %.1f %% above %.0e, smallest gap %.2e' % (cid, gap.size, 100 * share, GAP, gap.min()))
    assert share >= MARGIN_SHARE


def operand_rounding_deviation(c, sd, enc, lens, teacher, want_l, want_a):
    """-> (float64 run on bf16-rounded operands: logits, att; its deviation from the exact float64 run: relative Frobenius of
    the logits, max-abs of the attention rows)"""
    emu_l, emu_a, _ = decode(weights(sd, c['NL']), c, enc, lens, c['L'], teacher=teacher, bf16_operands=True)
    return emu_l, emu_a, float(np.linalg.norm(emu_l - want_l) / np.linalg.norm(want_l)), float(np.abs(emu_a - want_a).max())


def test_operand_rounding_alone_exceeds_the_bf16_bound_there():
    """The two documented points, and only they, of the bf16 greedy table: float64 arithmetic on operands rounded as bf16
    contraction mode rounds them already misses the bench-dims bound of tests/test_decoder_dims_vs_oracle.py."""
    over = {}
    for c in GREEDY_CASES:
        if 'bf16' not in c['precs']:
            continue
        sd, enc, lens = greedy_inputs(c, bf16=True)
        W = weights(sd, c['NL'])
        want_l, want_a, tok = decode(W, c, enc, lens, c['L'])
        teacher = np.concatenate([tok[:, 1:], np.zeros((c['B'], 1), dtype=np.int64)], axis=1)
        _, _, dl, da = operand_rounding_deviation(c, sd, enc, lens, teacher, want_l, want_a)
        if dl > DD._bound(c, 'bf16', 'logits'):
            over[c['id']] = 'logits'
            print('%s: logits %.3e > %.3e' % (c['id'], dl, DD._bound(c, 'bf16', 'logits')))
        if da > DD._bound(c, 'bf16', 'att'):
            over[c['id']] = 'att'
            print('%s: att %.3e > %.3e' % (c['id'], da, DD._bound(c, 'bf16', 'att')))
    assert over == BF16_NARROW, over
