"""Float64 restatement of the variant decoder loop and of the GRU encoder layers, their rounded twins, the case tables of
tests/test_hip_variant_decoder_vs_float64.py and the CPU checks of all of them.  Nothing of the code under test is imported here.

What is under test in the GPU file is the chain BETWEEN the kernels of src/variants.py: its autograd Functions, the _Holder /
HoldFn in-place accumulation of the key and value gradients over all steps, the R // Bv groups of AttendFn (the reference's
head-major value.repeat against batch-major rows), the strided batched H.gemm calls of DotEnergyFn and AttendFn, the seqT / bshift
weight-gradient contraction of GRUSeqFn, variant_decoder and gru_layer_forward themselves.  Every kernel they launch is held to
float64 on its own (tests/test_hip_variant_kernels_vs_float64.py, the GEMM and glue files); the chain was held only by
tests/test_variants.py: five fixtures at one shape, fp32 gradients to 1e-4, bf16 gradients to a cosine.

THE FLOAT64 RESTATEMENT.  dec_f64(case, inputs) runs oracle.asr_oracle.att_decoder_variants in float64, teacher-forced with the
tokens that were fed (greedy and sampled cases: teacher := fed tokens, as tests/test_scheduled_sampling.py), dropout through given
{0,1} masks, the backward by autograd from (logits * dlogits).sum() + (att * watt).sum() so that att_seq carries a gradient too.
It returns logits, the attention rows, the decoder states (the top layer's h of every step, recorded at the oracle's own cell
calls), d enc and every gradient of an attention, decoder or embedding parameter.  gru_f64 runs oracle.asr_oracle.encoder with
module GRU the same way and returns out, dx and every layer parameter gradient.

THE ROUNDED TWIN.  A second chain (_dec_forward, _gru_layer), written out stage by stage, which with no rounding equals the
oracle in float64 (test_twin_equals_oracle, test_gru_twin_equals_oracle) and which rounds exactly where the device path does.
WHICH CONTRACTIONS RUN IN bf16, as read from csrc/gemm.hip and csrc/gemm_plan.h: every contraction of the path is one asr_gemm
launch (src/hipabi.gemm / linear_fwd / linear_bwd), asr_gemm has ONE kernel (gemm_kernel) and gemm_plan picks its instantiation
as gemm_kernels[prec == bf16][a_kc][b_kc][fast loaders][0]: the MFMA follows `prec` alone, and M, N, K, batch, strides, seqT and
bshift only choose the loader (fetch_tile_fast or the scalar fetch_tile).  There is no fp32 fall-back by shape.  So in bf16 mode
  * the M = 1 batched rows of DotEnergyFn (q . key) and AttendFn (attn . value), forward and their input gradients,
  * their K = 1 outer-product accumulations into key.grad / value.grad (one rounding of each operand per step, the sum over the
    steps and over AttendFn's groups in fp32),
  * the seqT / bshift weight gradient dW_hh of GRUSeqFn, and dW_ih, dx, the x W_ih^T of the layer,
  * every LinearActFn (proj_k, proj_v, proj_q, loc_proj, merge_head, the cells' W_ih / W_hh, char_trans, the encoder's pj)
all stage both operands as bf16 and accumulate in fp32; in fp32 mode all of them run the f32 MFMA.  Everything else is fp32 in
both modes: loc_conv, the location energy (tanh, gen_energy), the masked softmax, the LSTM / GRU cells, asr_gru_fwd / asr_gru_bwd
(the recurrent product h W_hh^T and its dh are fp32 in the kernel: csrc/variants.hip holds no bf16), LayerNorm, dropout,
down-sampling, the embedding, asr_colsum (bias gradients: sums of unrounded values).  The twin rounds both operands of each of
those launches to bf16 and nothing else, and runs in torch.float32 between them; fp32 mode is the chain run in torch.float32
with nothing rounded.  (Float32 and not float64 between the rounding points in bf16 mode too: "everything else is fp32" on the
device, and tensors that no bf16 rounding reaches - gen_energy.bias's gradient, analytically zero because the softmax Jacobian's
rows sum to zero; char_trans.bias's - are fp32 summation noise there, which a float64 chain does not contain.)  The plan query (asr_gemm_plan) reports the
loaders and the tile counts, not the MFMA; the GPU file asserts with it that the odd shapes are taken, by which loader, and as
one launch of `batch` slices.

THE BOUNDS, by the rule of tests/test_encoder_layer_reference.py.  Per case, metric and precision: E0 = the largest value of the
metric between the twin and the float64 restatement over eight input / weight seeds; bound = 8 x E0, floored at 2^-24 times the
longest sum that feeds the tensor (forward: the widest contraction, T' included; d enc: L steps x NH heads x the wider of the key
and value rows; parameter gradients: B * L * T' rows, the key projection's).  At most 10 % of the (case, metric) bounds sit on
the floor in bf16 mode (test_floor_share; fp32 mode: as the encoder file found, E0 is fp32's own 2 - 4 ulp and most bounds are
the floor by arithmetic; asserted instead: no floored fp32 bound exceeds 2^-24 x the longest sum of the table).

THE METRICS: 'logits', 'att', 'states', 'denc' ('out', 'dx' for the encoder layers), 'grad.<param>' relative Frobenius error (a
gradient's norm floored at 1e-3 of the largest gradient norm of the case); 'proj.<param>' = |<g - r, r>| / |r|^2, which shows a
whole tensor off by a factor at full size.

GREEDY AND SAMPLED CASES.  The float64 side is teacher-forced with the fed tokens.  A greedy case also asserts that every token
the device chose is an argmax of the float64 logits up to the logits bound: with d = bound['logits'] x |logits|_F no element moves
by more than d, so the chosen token's float64 logit is within 2 d of the row's largest.  The run seed of a greedy case
(`run_seed`, found by a CPU search over seeds and pinned in the table) has a float64 top-two gap of at least 4 d at every step:
the reference alone never flips (test_greedy_margin).  A sampled case fixes the teacher / sample decisions; the sampled tokens
are the device's own draws, the bounds are taken at tokens drawn here.

MUTANTS (test_mutants).  Each is a wrong answer derived from the exact restatement; under the named case's own bounds it fails at
least one metric in both precisions:
   1 value rows repeated batch-major (dot_3_F_B2)              2 the key gradient taken from the last step only (dot_1_F)
   3 d enc lacks the value path (dot_1_F)                      4 initial prev_att uniform over T' not enc_len (loc_2_F) 
   5 the query built from the top layer's state only (dot_lstm2)
   6 inter-layer dropout scale missing in the backward (loc_decdrop)
   7 temperature missing in the softmax backward (dot_temp2)   8 the location feature's gradient from head 0 only (loc_2_F)
   9 merge_head's bias gradient times the head count (dot_2_F) 10 GRU dW_hh formed with h_t (g_base)
  11 GRU dW_hh at the first step of a walk reads the neighbouring batch row's end frame (g_T2)
  12 the n gate's b_hh gradient taken without the reset gate (g_base)
"""
import contextlib
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle import asr_oracle as O

F64 = torch.float64
ENC, DIM, V, EIN = 16, 12, 7, 8          # encoder output width, decoder width, vocabulary, the (never run) encoder's input width
MAX_DEC_LAYERS = 4                       # src/hipabi.MAX_DEC_LAYERS, asserted by the GPU file
K_E0, N_SEEDS = 8.0, 8
FLOOR_ULP = 2.0 ** -24
FLOOR_SHARE_CAP = 0.10
PRECS = ('bf16', 'fp32')


# ----------------------------------------------------------------------------------------------------------------------
# the decoder case table (plain data)
# ----------------------------------------------------------------------------------------------------------------------
def _case(cid, mode='dot', NH=1, vp=False, module='LSTM', NL=1, dec_p=0.0, emb_p=0.0, B=3, Tp=9, L=3, lens=None, Ks=2, Kn=3,
          temp=1.0, adim=8, need_denc=True, len_dtype='int64', feed='teacher', decisions=None, run_seed=0):
    """feed: 'teacher' (train mode when a dropout is on, else eval), 'greedy' (teacher None, eval), 'sampled' (train mode,
    `decisions`: True = the teacher's token).  lens: the encoder lengths, the first utterance full by default."""
    if lens is None:
        lens = [Tp, max(1, Tp // 2), max(1, Tp - 2), max(1, Tp // 3)][:B]
    assert len(lens) == B and max(lens) <= Tp and min(lens) >= 1
    return dict(id=cid, mode=mode, NH=NH, vp=vp, module=module, NL=NL, dec_p=dec_p, emb_p=emb_p, B=B, Tp=Tp, L=L, lens=list(lens), Ks=Ks,
                Kn=Kn, temp=temp, adim=adim, need_denc=need_denc, len_dtype=len_dtype, feed=feed, decisions=decisions, run_seed=run_seed,
                train=(dec_p > 0 or emb_p > 0 or feed == 'sampled') and feed != 'greedy')


CASES = [
    # attention (mode, heads, v_proj)
    _case('dot_1_F'),
    _case('dot_1_T', vp=True),
    _case('dot_2_F', NH=2),
    _case('dot_2_T', NH=2, vp=True),
    _case('dot_3_F_B2', NH=3, B=2),                       # the head-major repeat: r % B != r // NH
    _case('loc_2_F', mode='loc', NH=2),
    _case('loc_2_T', mode='loc', NH=2, vp=True),
    _case('loc_3_F_B2', mode='loc', NH=3, B=2),
    # loc / 1 / F leaves the fast path through the decoder alone
    _case('loc_gru1', mode='loc', module='GRU'),
    _case('loc_decdrop', mode='loc', NL=2, dec_p=0.25),
    _case('loc_embdrop', mode='loc', emb_p=0.2),
    _case('loc_lstm5', mode='loc', NL=MAX_DEC_LAYERS + 1),
    # decoder
    _case('dot_lstm2', NL=2),
    _case('dot_lstm3', NL=3),
    _case('dot_gru2', module='GRU', NL=2),
    _case('both_drop_gru2_dot_2_F', NH=2, module='GRU', NL=2, dec_p=0.25, emb_p=0.2),
    # batch and length edges
    _case('loc_2_T_B1', mode='loc', NH=2, vp=True, B=1),
    _case('loc_len1', mode='loc', NH=2, B=2, lens=[1, 9]),
    _case('dot_len1', NH=2, vp=True, B=2, lens=[9, 1]),
    _case('dot_Tp1', Tp=1, B=2),
    _case('loc_Tp1', mode='loc', NH=2, Tp=1, B=2),
    _case('loc_Tp31', mode='loc', NH=2, Tp=31, B=2, lens=[31, 5]),
    _case('loc_Tp32', mode='loc', NH=2, Tp=32, B=2, lens=[32, 31]),
    _case('loc_Tp33', mode='loc', NH=2, Tp=33, B=2, lens=[33, 32]),
    _case('loc_Tp65', mode='loc', module='GRU', Tp=65, B=2, lens=[65, 33]),
    _case('dot_Tp33', NH=2, Tp=33, B=2, lens=[32, 33]),
    _case('loc_Tp257_L2', mode='loc', NH=2, Tp=257, L=2, B=2, lens=[257, 256]),
    _case('dot_Tp257_L2', NH=2, Tp=257, L=2, B=2, lens=[257, 129]),
    _case('loc_L1', mode='loc', NH=2, L=1),
    _case('dot_L1', vp=True, L=1),
    _case('loc_L2', mode='loc', NH=2, vp=True, L=2),
    _case('dot_L5', NH=2, L=5),
    # location kernel half-width
    _case('loc_Ks1', mode='loc', NH=2, Ks=1),
    _case('loc_Ks5_Tp3', mode='loc', NH=2, Ks=5, Tp=3, lens=[3, 1, 2]),
    # temperature, attention dim above the 64 lanes
    _case('dot_temp2', temp=2.0),
    _case('loc_temp05', mode='loc', NH=2, temp=0.5),
    _case('loc_adim65', mode='loc', NH=2, adim=65),
    _case('dot_adim65', vp=True, adim=65),
    # the encoder output without a gradient, int32 lengths
    _case('dot_no_denc', NH=2, need_denc=False),
    _case('loc_no_denc', mode='loc', NH=2, vp=True, need_denc=False),
    _case('loc_int32', mode='loc', NH=2, len_dtype='int32'),
    # greedy (eval) and scheduled sampling with fixed decisions
    _case('dot_greedy', NH=2, B=2, feed='greedy', run_seed=16),
    _case('loc_greedy', mode='loc', module='GRU', B=2, feed='greedy', run_seed=28),
    _case('dot_mh_sampled', NH=2, vp=True, L=5, feed='sampled', decisions=[True, False, False, True, True]),
    _case('loc_gru_sampled', mode='loc', module='GRU', L=5, feed='sampled', decisions=[False, True, False, True, False]),
    # a sampled token's embedding is dropped with a mask of its own, drawn at its step
    _case('loc_embdrop_sampled', mode='loc', emb_p=0.2, L=4, feed='sampled', decisions=[True, False, False, True]),
]
BY_ID = {c['id']: c for c in CASES}
# nothing of the decoder table is refused on the host: every case is launched
REFUSED = []


def model_cfg(c):
    return {'ctc_weight': 0.0, 'emb_drop': c['emb_p'],
            'encoder': {'vgg': 0, 'vgg_freq': -1, 'vgg_low_filt': -1, 'module': 'LSTM', 'bidirection': True, 'dim': [ENC // 2], 'dropout': [0.0],
                        'layer_norm': [False], 'proj': [False], 'sample_rate': [1], 'sample_style': 'drop'},
            'attention': {'mode': c['mode'], 'dim': c['adim'], 'num_head': c['NH'], 'temperature': c['temp'], 'v_proj': c['vp'],
                          'loc_kernel_size': c['Ks'], 'loc_kernel_num': c['Kn']},
            'decoder': {'module': c['module'], 'dim': DIM, 'layer': c['NL'], 'dropout': c['dec_p']}}


def oracle_cfg(c):
    return O.ModelCfg(model_cfg(c), EIN, V)


def leaves_fast_path(c):
    """The choice of ASR.forward, restated: what keeps a model off the persistent decoder kernels."""
    att_fast = c['mode'] == 'loc' and c['NH'] == 1 and not c['vp']
    dec_fast = c['module'] == 'LSTM' and c['dec_p'] == 0 and c['NL'] <= MAX_DEC_LAYERS
    return not (att_fast and dec_fast and c['emb_p'] == 0.0)


def _bf(t):
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def _host_masks(c, rng):
    if not c['train'] or (c['dec_p'] == 0 and c['emb_p'] == 0):
        return None
    B, L, NL = c['B'], c['L'], c['NL']
    draw = lambda shape, p: torch.from_numpy((rng.random(shape) >= p).astype(np.float64))
    return {'emb': draw((B, L, DIM), c['emb_p']) if c['emb_p'] > 0 else None,
            'layer': [[draw((B, DIM), c['dec_p']) for _ in range(NL - 1)] for _ in range(L)],
            'final': [draw((B, DIM), c['dec_p']) for _ in range(L)]}


def greedy_tokens(c, sd, enc, lens):
    """(B, L) tokens the float64 loop feeds when it decodes greedily, <sos> first, and its logits."""
    P = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        logits, _ = O.att_decoder_variants(enc.double(), lens, P, oracle_cfg(c), c['L'], teacher=None)
    fed = torch.zeros(c['B'], c['L'], dtype=torch.int64)
    fed[:, 1:] = logits.argmax(-1)[:, :-1]
    return fed, logits


def inputs(c, seed, prec, masks='host'):
    """Weights, encoder output, lengths, tokens, dlogits, watt (float64 values; in bf16 mode weights and enc are bf16 numbers, as
    both sides see them) and host masks.  'fed' (B, L): what the loop feeds, <sos> first - the teacher's tokens, the float64
    greedy tokens, or for a sampled case tokens drawn here (the device's own replace them in the GPU file)."""
    sd = O.seeded_state_dict(O.param_shapes(oracle_cfg(c)), 1000 + seed)
    g = torch.Generator().manual_seed(17 + seed)
    B, Tp, L = c['B'], c['Tp'], c['L']
    enc = torch.randn(B, Tp, ENC, generator=g, dtype=F64)
    dl = torch.randn(B, L, V, generator=g, dtype=F64).float().double()
    wa = torch.randn(B, c['NH'], L, Tp, generator=g, dtype=F64).float().double()
    teacher = torch.randint(1, V, (B, L), generator=g)
    other = torch.randint(1, V - 1, (B, L), generator=g)
    if prec == 'bf16':
        sd = {k: v.bfloat16().float() for k, v in sd.items()}
        enc = enc.float().bfloat16().double()
    else:
        enc = enc.float().double()
    lens = torch.tensor(c['lens'], dtype=torch.int64)
    fed = torch.zeros(B, L, dtype=torch.int64)
    if c['feed'] == 'greedy':
        fed, _ = greedy_tokens(c, sd, enc, lens)
    else:
        fed[:, 1:] = teacher[:, :-1]
        if c['feed'] == 'sampled':
            for t, use_teacher in enumerate(c['decisions'][:L - 1]):
                if not use_teacher:
                    fed[:, t + 1] = torch.where(other[:, t] >= teacher[:, t], other[:, t] + 1, other[:, t])      # another token than the teacher's
    ms = _host_masks(c, np.random.Generator(np.random.PCG64(99 + seed))) if masks == 'host' else None
    return dict(sd=sd, enc=enc, lens=lens, teacher=teacher, fed=fed, dl=dl, wa=wa, masks=ms)


# ----------------------------------------------------------------------------------------------------------------------
# the chain's building blocks, with their rounding points
# ----------------------------------------------------------------------------------------------------------------------
class _MM(torch.autograd.Function):
    """a (rows, K) @ w (N, K)^T as asr_gemm launches compute it: qf / qx / qw say which of the three contractions (forward, input
    gradient, weight gradient) round both of their operands to bf16."""
    @staticmethod
    def forward(ctx, a, w, qf, qx, qw):
        ctx.q = (qx, qw)
        ctx.save_for_backward(a, w)
        return (_bf(a) @ _bf(w).t()) if qf else a @ w.t()

    @staticmethod
    def backward(ctx, g):
        a, w = ctx.saved_tensors
        qx, qw = ctx.q
        da = (_bf(g) @ _bf(w)) if qx else g @ w
        dw = (_bf(g).t() @ _bf(a)) if qw else g.t() @ a
        return da, dw, None, None, None


class _BMM(torch.autograd.Function):
    """Batched a (R, M, K) @ b (R, K, N): the strided batched asr_gemm of DotEnergyFn / AttendFn and their two gradients."""
    @staticmethod
    def forward(ctx, a, b, q):
        if q:
            a, b = _bf(a), _bf(b)
        ctx.q = q
        ctx.save_for_backward(a, b)
        return torch.bmm(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        if ctx.q:
            g = _bf(g)
        return torch.bmm(g, b.transpose(1, 2)), torch.bmm(a.transpose(1, 2), g), None


class _Drop(torch.autograd.Function):
    """y * mask / (1 - p); a mutant leaves the scale out of the backward."""
    @staticmethod
    def forward(ctx, y, mask, p, no_scale_bwd):
        ctx.k = mask if no_scale_bwd else mask / (1.0 - p)
        return y * mask / (1.0 - p)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.k, None, None, None


class _SoftmaxNoTempBwd(torch.autograd.Function):
    """softmax(e / temperature) whose backward forgets the temperature (mutant 7)."""
    @staticmethod
    def forward(ctx, e, mask, temp):
        a = torch.softmax((e / temp).masked_fill(mask, O.NEG_INF), dim=-1)
        ctx.save_for_backward(a)
        return a

    @staticmethod
    def backward(ctx, g):
        a, = ctx.saved_tensors
        return a * (g - (g * a).sum(-1, keepdim=True)), None, None


def _mm(a, w, q, recurrent=False):
    """recurrent: the product inside asr_gru_fwd / asr_gru_bwd is fp32; only its weight gradient is an asr_gemm launch."""
    qf = qx = q and not recurrent
    return _MM.apply(a.reshape(-1, a.shape[-1]), w, qf, qx, q).view(*a.shape[:-1], w.shape[0])


def _lstm_cell(gx, gh, c):
    i, f, gg, o = (gx + gh).chunk(4, dim=-1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    return torch.sigmoid(o) * torch.tanh(c), c


def _gru_cell(gi, gh, h):
    xr, xz, xn = gi.chunk(3, dim=-1)
    hr, hz, hn = gh.chunk(3, dim=-1)
    r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
    return (1 - z) * torch.tanh(xn + r * hn) + z * h


# ----------------------------------------------------------------------------------------------------------------------
# the decoder chain, stage by stage (src/variants.variant_decoder)
# ----------------------------------------------------------------------------------------------------------------------
def _dec_forward(c, P, enc, lens, fed, masks, q, mut=None):
    """logits (B,L,V), att (B,NH,L,T'), states (B,L,dim); q: the asr_gemm launches round their operands to bf16."""
    B, Tp, Dv = enc.shape
    nh, ad, nl, L, loc_mode = c['NH'], c['adim'], c['NL'], c['L'], c['mode'] == 'loc'
    lin = lambda x, n: _mm(x, P[n + '.weight'], q) + P[n + '.bias']
    valid = torch.arange(Tp)[None, :] < lens[:, None]
    pad_rows = (~valid)[:, None, :].expand(B, nh, Tp).reshape(B * nh, Tp)
    # ---- the memory, once
    key = torch.tanh(lin(enc, 'attention.proj_k'))
    if c['vp']:
        value = torch.tanh(lin(enc, 'attention.proj_v'))
    else:
        value = enc.detach() if mut == 'denc_no_value' else enc
    if nh > 1:
        key = key.view(B, Tp, nh, ad).permute(0, 2, 1, 3).reshape(B * nh, Tp, ad)
        if c['vp']:
            value = value.view(B, Tp, nh, Dv).permute(0, 2, 1, 3).reshape(B * nh, Tp, Dv)
        elif mut == 'batch_major':
            value = value.repeat_interleave(nh, dim=0)
        else:
            value = value.repeat(nh, 1, 1)                     # row r = b * NH + n attends over utterance r % B: AttendFn's groups
    prev = None
    if loc_mode:
        if mut == 'prev_att_T':
            prev = torch.full((B, Tp), 1.0 / Tp, dtype=enc.dtype)
        else:
            prev = torch.where(valid, (1.0 / lens.to(enc.dtype))[:, None].expand(B, Tp), torch.zeros((), dtype=enc.dtype))
        prev = prev[:, None, :].expand(B, nh, Tp)
    E = P['pre_embed.weight']
    h = [enc.new_zeros(B, DIM) for _ in range(nl)]
    cc = [enc.new_zeros(B, DIM) for _ in range(nl)]
    lstm = c['module'] == 'LSTM'
    logits_seq, att_seq, states = [], [], []
    for t in range(L):
        q_in = torch.cat(h, dim=-1)
        if mut == 'query_top':
            q_in = torch.cat([torch.zeros_like(x) for x in h[:-1]] + [h[-1]], dim=-1)
        qv = torch.tanh(lin(q_in, 'attention.proj_q')).view(B * nh, ad)
        k_t = key.detach() if (mut == 'key_last_step' and t + 1 < L) else key
        if not loc_mode:
            energy = _BMM.apply(qv.unsqueeze(1), k_t.transpose(1, 2), q).squeeze(1)
        else:
            conv = Fn.conv1d(prev, P['attention.att_layer.loc_conv.weight'], padding=c['Ks'])
            loc = torch.tanh(_mm(conv.transpose(1, 2), P['attention.att_layer.loc_proj.weight'], q))       # (B,T',ad), shared over heads
            if mut == 'loc_head0':
                loc = torch.stack([loc] + [loc.detach()] * (nh - 1), dim=1)
            else:
                loc = loc.unsqueeze(1).repeat(1, nh, 1, 1)
            u = torch.tanh(k_t + qv.unsqueeze(1) + loc.reshape(B * nh, Tp, ad))
            energy = (u @ P['attention.att_layer.gen_energy.weight'].t()).squeeze(-1) + P['attention.att_layer.gen_energy.bias']
        if mut == 'temp_bwd':
            attn = _SoftmaxNoTempBwd.apply(energy, pad_rows, c['temp'])
        else:
            attn = torch.softmax((energy / c['temp']).masked_fill(pad_rows, O.NEG_INF), dim=-1)
        ctxv = _BMM.apply(attn.unsqueeze(1), value, q).squeeze(1)                                           # (B*NH,Dv)
        attn = attn.view(B, nh, Tp)
        if loc_mode:
            prev = attn
        if nh > 1:
            ctxv = lin(ctxv.view(B, nh * Dv), 'attention.merge_head')
        last = E[fed[:, t]]
        if t > 0 and masks is not None and c['emb_p'] > 0:
            last = last * masks['emb'][:, t - 1].to(last.dtype) / (1.0 - c['emb_p'])
        x = torch.cat([last, ctxv], dim=-1)
        for l in range(nl):
            gx = _mm(x, P['decoder.layers.weight_ih_l%d' % l], q) + P['decoder.layers.bias_ih_l%d' % l]
            gh = _mm(h[l], P['decoder.layers.weight_hh_l%d' % l], q) + P['decoder.layers.bias_hh_l%d' % l]
            if lstm:
                h[l], cc[l] = _lstm_cell(gx, gh, cc[l])
            else:
                h[l] = _gru_cell(gx, gh, h[l])
            x = h[l]
            if l + 1 < nl and masks is not None and c['dec_p'] > 0:
                x = _Drop.apply(x, masks['layer'][t][l].to(x.dtype), c['dec_p'], mut == 'interlayer_scale')
        states.append(x)
        if masks is not None and c['dec_p'] > 0:
            x = _Drop.apply(x, masks['final'][t].to(x.dtype), c['dec_p'], False)
        logits_seq.append(lin(x, 'decoder.char_trans'))
        att_seq.append(attn)
    return torch.stack(logits_seq, dim=1), torch.stack(att_seq, dim=2), torch.stack(states, dim=1)


def _dec_result(c, logits, att, states, enc, P):
    res = {'logits': logits.detach().double(), 'att': att.detach().double(), 'states': states.detach().double(),
           'denc': enc.grad.double() if c['need_denc'] else None}
    for k, p in P.items():
        if not k.startswith('encoder.'):
            res['grad.' + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).double()
    return res


def _dec_chain(c, inp, prec, rounded=True, mut=None):
    dt = torch.float32 if rounded else F64                   # between the rounding points the device path is fp32 in both modes
    P = {k: v.to(dt).clone().requires_grad_(True) for k, v in inp['sd'].items()}
    enc = inp['enc'].to(dt).clone().requires_grad_(c['need_denc'])
    ms = inp['masks']
    logits, att, states = _dec_forward(c, P, enc, inp['lens'], inp['fed'], ms, rounded and prec == 'bf16', mut)
    ((logits * inp['dl'].to(dt)).sum() + (att * inp['wa'].to(dt)).sum()).backward()
    return _dec_result(c, logits, att, states, enc, P)


@contextlib.contextmanager
def _recorded_cells():
    """The oracle's cell calls, in order: the state of step t is the h of its last layer's call."""
    calls, lstm, gru = [], O.lstm_cell, O.gru_cell
    def rec_lstm(*a):
        out = lstm(*a)
        calls.append(out[0])
        return out
    def rec_gru(*a):
        out = gru(*a)
        calls.append(out)
        return out
    O.lstm_cell, O.gru_cell = rec_lstm, rec_gru
    try:
        yield calls
    finally:
        O.lstm_cell, O.gru_cell = lstm, gru


def dec_f64(c, inp, prec=None):
    """prec None: oracle.asr_oracle.att_decoder_variants in float64 - the exact restatement; else the rounded twin."""
    if prec is not None:
        return _dec_chain(c, inp, prec)
    P = {k: v.double().clone().requires_grad_(True) for k, v in inp['sd'].items()}
    enc = inp['enc'].double().clone().requires_grad_(c['need_denc'])
    fed = inp['fed']
    teacher = torch.cat([fed[:, 1:], torch.zeros(c['B'], 1, dtype=torch.int64)], dim=1)      # teacher[:, t] is fed at step t + 1
    with _recorded_cells() as calls:
        logits, att = O.att_decoder_variants(enc, inp['lens'], P, oracle_cfg(c), c['L'], teacher=teacher, masks=inp['masks'])
    assert len(calls) == c['L'] * c['NL']
    states = torch.stack(calls[c['NL'] - 1::c['NL']], dim=1)
    ((logits * inp['dl']).sum() + (att * inp['wa']).sum()).backward()
    return _dec_result(c, logits, att, states, enc, P)


# ----------------------------------------------------------------------------------------------------------------------
# the GRU encoder layer cases and their chain (src/variants.gru_layer_forward through model.encoder)
# ----------------------------------------------------------------------------------------------------------------------
def _GL(rate=1, proj=True, ln=False, p=0.0):
    return dict(rate=rate, proj=proj, ln=ln, p=p)


def _gcase(cid, B=3, T=5, Din=24, H=16, ND=2, style='drop', layers=None, lens=None, **one):
    layers = layers or [_GL(**one)]
    lens = lens or [T, max(1, T - 2), max(1, T // 2), 1][:B]
    return dict(id=cid, B=B, T=T, Din=Din, H=H, ND=ND, style=style, layers=layers, lens=lens, need_dx=True, train=any(l['p'] > 0 for l in layers))


GRU_CASES = [
    _gcase('g_base'),
    _gcase('g_ND1_T1_B1', B=1, T=1, ND=1),
    _gcase('g_T2', T=2),
    _gcase('g_ND1_T2', T=2, ND=1),
    _gcase('g_H48', H=48),
    _gcase('g_ln', ln=True),
    _gcase('g_noproj', proj=False),
    _gcase('g_p25', p=0.25),
    _gcase('g_drop2_T5', rate=2),
    _gcase('g_drop2_T4', T=4, rate=2),
    _gcase('g_concat2_T5', style='concat', rate=2, proj=False),
    _gcase('g_all_on', ln=True, p=0.25, rate=2),
    _gcase('g_B1_ln_p25_concat2', B=1, style='concat', ln=True, p=0.25, rate=2, proj=False),
    _gcase('g_stack2', layers=[_GL(p=0.25), _GL(rate=2, p=0.25, ln=True)]),
]
GRU_BY_ID = {c['id']: c for c in GRU_CASES}


def gru_model_cfg(c, module='GRU'):
    n = len(c['layers'])
    return {'ctc_weight': 1.0,
            'encoder': {'vgg': 0, 'vgg_freq': -1, 'vgg_low_filt': -1, 'module': module, 'bidirection': c['ND'] == 2, 'dim': [c['H']] * n,
                        'dropout': [l['p'] for l in c['layers']], 'layer_norm': [l['ln'] for l in c['layers']],
                        'proj': [l['proj'] for l in c['layers']], 'sample_rate': [l['rate'] for l in c['layers']], 'sample_style': c['style']}}


# what the model refuses on the host, before anything is launched: (case, keyword overrides of the encoder block, error).  The
# encoder block names ONE module for all its layers (as the reference's): a GRU layer below an LSTM layer cannot be stated, a list
# of modules is refused; 'proj' behind 'concat' is refused for GRU layers as for LSTM ones.
GRU_REFUSED = [
    (_gcase('g_gru_below_lstm', layers=[_GL(), _GL()]), {'module': ['GRU', 'LSTM']}, NotImplementedError),
    (_gcase('g_concat2_proj', style='concat', rate=2, proj=False), {'proj': [True]}, ValueError),
]


def gru_oracle_cfg(c):
    return O.ModelCfg(gru_model_cfg(c), c['Din'], V)


def gru_frames(c):
    """[(T, T2, Din, Dz)] per layer."""
    out, T, Din = [], c['T'], c['Din']
    for l in c['layers']:
        D, r = c['ND'] * c['H'], l['rate']
        T2, Dz = (T, D) if r == 1 else (((T + r - 1) // r, D) if c['style'] == 'drop' else (T // r, D * r))
        out.append((T, T2, Din, Dz))
        T, Din = T2, Dz
    return out


def gru_inputs(c, seed, prec, masks='host'):
    sd = O.seeded_state_dict(O.param_shapes(gru_oracle_cfg(c)), 1000 + seed)
    g = torch.Generator().manual_seed(17 + seed)
    fr = gru_frames(c)
    x = torch.randn(c['B'], c['T'], c['Din'], generator=g, dtype=F64)
    dout = torch.randn(c['B'], fr[-1][1], fr[-1][3], generator=g, dtype=F64).float().double()
    if prec == 'bf16':
        sd = {k: v.bfloat16().float() for k, v in sd.items()}
        x = x.float().bfloat16().double()
    else:
        x = x.float().double()
    ms = None
    if masks == 'host':
        rng = np.random.Generator(np.random.PCG64(99 + seed))
        ms = [torch.from_numpy((rng.random((c['B'], f[0], c['ND'] * c['H'])) >= l['p']).astype(np.float64)) if l['p'] > 0 else None
              for f, l in zip(fr, c['layers'])]
    return dict(sd=sd, x=x, dout=dout, masks=ms, lens=torch.tensor(c['lens'], dtype=torch.int64))


def _gru_layer(x, P, pre, c, l, mask, q, keep=None):
    """One GRU RNNLayer: gi = x W_ih^T + b_ih (asr_gemm), the fp32 recurrence (asr_gru_fwd / asr_gru_bwd; dW_hh an asr_gemm over
    the shifted y), [LayerNorm] -> dropout -> down-sampling (fp32 kernels) -> tanh(z W_pj^T + b) (asr_gemm)."""
    Lc = c['layers'][l]
    B, T, _ = x.shape
    Hd, r = c['H'], Lc['rate']
    ys = []
    for d, sfx in enumerate(['', '_reverse'][:c['ND']]):
        w_ih, w_hh, b_ih, b_hh = (P[pre + 'layer.%s_l0%s' % (n, sfx)] for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'))
        gi = _mm(x, w_ih, q) + b_ih
        h, hs = x.new_zeros(B, Hd), [None] * T
        for t in (range(T - 1, -1, -1) if d else range(T)):
            gh = _mm(h, w_hh, q, recurrent=True) + b_hh
            if keep is not None:
                gh.retain_grad()
                keep.setdefault((l, d), [None] * T)[t] = gh
            h = _gru_cell(gi[:, t], gh, h)
            hs[t] = h
        ys.append(torch.stack(hs, dim=1))
    y = torch.cat(ys, dim=-1)
    if keep is not None:
        keep[(l, 'y')] = y
    if Lc['ln']:
        y = Fn.layer_norm(y, (y.shape[-1],), P[pre + 'ln.weight'], P[pre + 'ln.bias'])
    if mask is not None:
        y = _Drop.apply(y, mask.to(y.dtype), Lc['p'], False)
    if r > 1:
        y = y[:, ::r] if c['style'] == 'drop' else y[:, :T - T % r].reshape(B, T // r, -1)
    if Lc['proj']:
        y = torch.tanh(_mm(y, P[pre + 'pj.weight'], q) + P[pre + 'pj.bias'])
    return y


def _gru_result(c, out, x, P):
    res = {'out': out.detach().double(), 'dx': x.grad.double()}
    for k, p in P.items():
        if k.startswith('encoder.'):
            res['grad.' + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).double()
    return res


def _gru_chain(c, inp, prec, rounded=True, keep=None):
    dt = torch.float32 if rounded else F64
    P = {k: v.to(dt).clone().requires_grad_(True) for k, v in inp['sd'].items()}
    x = inp['x'].to(dt).clone().requires_grad_(True)
    h = x
    for l in range(len(c['layers'])):
        h = _gru_layer(h, P, 'encoder.layers.%d.' % l, c, l, None if inp['masks'] is None else inp['masks'][l], rounded and prec == 'bf16', keep)
    (h * inp['dout'].to(dt)).sum().backward()
    return _gru_result(c, h, x, P)


def gru_f64(c, inp, prec=None):
    """prec None: oracle.asr_oracle.encoder (rnn_layer, bigru) in float64; else the rounded twin."""
    if prec is not None:
        return _gru_chain(c, inp, prec)
    P = {k: v.double().clone().requires_grad_(True) for k, v in inp['sd'].items()}
    x = inp['x'].double().clone().requires_grad_(True)
    out, _ = O.encoder(x, inp['lens'], P, gru_oracle_cfg(c), drop_masks=inp['masks'])
    (out * inp['dout']).sum().backward()
    return _gru_result(c, out, x, P)


# ----------------------------------------------------------------------------------------------------------------------
# the whole-model case: GRU encoder layer -> CTC head beside a dot multi-head decoder; the encoder output's gradient has both
# consumers.  Loss = (ctc log-probs * dctc).sum() + (logits * dlogits).sum() + (att * watt).sum()
# ----------------------------------------------------------------------------------------------------------------------
WHOLE = dict(id='whole_gru_ctc_dot_2_F', dec=_case('whole_dec', NH=2, B=3, Tp=9, L=3, lens=[9, 5, 7]),
             enc=_gcase('whole_enc', B=3, T=9, Din=EIN, H=ENC // 2, ND=2, lens=[9, 5, 7]))


def whole_model_cfg():
    cfg = model_cfg(WHOLE['dec'])
    cfg['encoder'] = gru_model_cfg(WHOLE['enc'])['encoder']
    cfg['ctc_weight'] = 0.5
    return cfg


def whole_oracle_cfg():
    return O.ModelCfg(whole_model_cfg(), EIN, V)


def whole_inputs(seed, prec):
    d, e = WHOLE['dec'], WHOLE['enc']
    sd = O.seeded_state_dict(O.param_shapes(whole_oracle_cfg()), 1000 + seed)
    inp = inputs(d, seed, prec, masks=None)
    g = torch.Generator().manual_seed(171 + seed)
    x = torch.randn(e['B'], e['T'], e['Din'], generator=g, dtype=F64).float()
    dctc = torch.randn(e['B'], e['T'], V, generator=g, dtype=F64).float().double()
    if prec == 'bf16':
        sd = {k: v.bfloat16().float() for k, v in sd.items()}
        x = x.bfloat16().float()
    inp.update(sd=sd, x=x.double(), dctc=dctc, enc=None)
    return inp


def whole_f64(inp, prec=None):
    """ctc log-probs, logits, att and the gradient of every parameter; prec None: the oracle's encoder, ctc_head and
    att_decoder_variants in float64, else the twins composed."""
    d, e = WHOLE['dec'], WHOLE['enc']
    rounded = prec is not None
    dt = torch.float32 if rounded else F64
    P = {k: v.to(dt).clone().requires_grad_(True) for k, v in inp['sd'].items()}
    x = inp['x'].to(dt)
    fed = inp['fed']
    if rounded:
        q = prec == 'bf16'
        enc = _gru_layer(x, P, 'encoder.layers.0.', e, 0, None, q)
        ctc = torch.log_softmax(torch.relu(_mm(enc, P['ctc_layer.0.weight'], q) + P['ctc_layer.0.bias']), dim=-1)
        logits, att, _ = _dec_forward(d, P, enc, inp['lens'], fed, None, q)
    else:
        cfg = whole_oracle_cfg()
        enc, lens = O.encoder(x, inp['lens'], P, cfg)
        assert torch.equal(lens, inp['lens'])
        ctc = O.ctc_head(enc, P)
        teacher = torch.cat([fed[:, 1:], torch.zeros(d['B'], 1, dtype=torch.int64)], dim=1)
        logits, att = O.att_decoder_variants(enc, lens, P, cfg, d['L'], teacher=teacher)
    ((ctc * inp['dctc'].to(dt)).sum() + (logits * inp['dl'].to(dt)).sum() + (att * inp['wa'].to(dt)).sum()).backward()
    res = {'ctc': ctc.detach().double(), 'logits': logits.detach().double(), 'att': att.detach().double()}
    for k, p in P.items():
        res['grad.' + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).double()
    return res


# ----------------------------------------------------------------------------------------------------------------------
# metrics and bounds
# ----------------------------------------------------------------------------------------------------------------------
def metrics(got, ref):
    rel = lambda a, b: float((a - b).norm() / (b.norm() + 1e-300))
    m = {k: rel(got[k], ref[k]) for k in ref if not k.startswith('grad.') and ref[k] is not None}
    names = [k for k in ref if k.startswith('grad.')]
    gmax = max(float(ref[k].norm()) for k in names)
    for k in names:
        g, r = got[k], ref[k]
        den = max(float(r.norm()), 1e-3 * gmax)
        m[k] = float((g - r).norm()) / den
        m['proj.' + k[5:]] = abs(float(((g - r) * r).sum())) / den ** 2
    return m


def dec_floors(c):
    """2^-24 x the longest sum that feeds the tensor, by kind of metric."""
    nh = c['NH']
    fwd = max(c['Tp'], DIM + ENC, c['NL'] * DIM, nh * ENC, c['adim'])
    rows = c['B'] * c['L'] * c['Tp']
    f = {k: FLOOR_ULP * fwd for k in ('logits', 'att', 'states')}
    f.update(denc=FLOOR_ULP * c['L'] * nh * max(c['adim'], ENC), grad=FLOOR_ULP * rows, proj=FLOOR_ULP * rows)
    return f


def gru_floors(c):
    D, G = c['ND'] * c['H'], c['ND'] * 3 * c['H']
    fr = gru_frames(c)
    fwd = max(max(f[2], c['H'], f[3]) for f in fr)
    bwd = max(max(3 * c['H'], f[3]) for f in fr)
    rows = c['B'] * c['T']
    return {'out': FLOOR_ULP * fwd, 'dx': FLOOR_ULP * max(G, bwd), 'grad': FLOOR_ULP * rows, 'proj': FLOOR_ULP * rows}


def whole_floors():
    f = dec_floors(WHOLE['dec'])
    f['ctc'] = f['logits']
    return f


def _bound_of(e0, fl):
    bound, floored = {}, set()
    for k, v in e0.items():
        f = fl[k.split('.')[0]]
        bound[k] = max(K_E0 * v, f)
        if K_E0 * v < f:
            floored.add(k)
    return bound, floored, e0


def _e0(run, seeds):
    e0 = {}
    for seed in seeds:
        exact, rounded = run(seed)
        for k, v in metrics(rounded, exact).items():
            e0[k] = max(e0.get(k, 0.0), v)
    return e0


@functools.lru_cache(maxsize=None)
def _bounds(kind, cid, prec):
    if kind == 'dec':
        c = BY_ID[cid]
        def run(seed):
            inp = inputs(c, seed, prec)
            return dec_f64(c, inp), dec_f64(c, inp, prec)
        return _bound_of(_e0(run, range(N_SEEDS)), dec_floors(c))
    if kind == 'gru':
        c = GRU_BY_ID[cid]
        def run(seed):
            inp = gru_inputs(c, seed, prec)
            return gru_f64(c, inp), gru_f64(c, inp, prec)
        return _bound_of(_e0(run, range(N_SEEDS)), gru_floors(c))
    def run(seed):
        inp = whole_inputs(seed, prec)
        return whole_f64(inp), whole_f64(inp, prec)
    return _bound_of(_e0(run, range(N_SEEDS)), whole_floors())


def bounds(c, prec):
    """{metric: bound} of a decoder case in precision `prec`, computed on the CPU from the restatements alone."""
    return _bounds('dec', c['id'], prec)[0]


def gru_bounds(c, prec):
    return _bounds('gru', c['id'], prec)[0]


def whole_bounds(prec):
    return _bounds('whole', WHOLE['id'], prec)[0]


def check(got, ref, bound):
    """[(metric, value, bound, ok)] for every metric of the case."""
    m = metrics(got, ref)
    assert set(m) == set(bound), sorted(set(m) ^ set(bound))
    return [(k, v, bound[k], v <= bound[k]) for k, v in sorted(m.items())]


def greedy_delta(c, prec, ref_logits):
    """The largest move of one logit that the case's logits bound admits."""
    return bounds(c, prec)['logits'] * float(ref_logits.norm())


# ----------------------------------------------------------------------------------------------------------------------
# mutants: wrong answers derived from the exact restatement
# ----------------------------------------------------------------------------------------------------------------------
def _gru_dwhh(c, keep, l, variant):
    """dW_hh of layer l from the exact gradients of gh = h W_hh^T + b_hh and y, rows of y shifted as `variant` says."""
    B, T, Hd = c['B'], len(keep[(l, 0)]), c['H']
    y = keep[(l, 'y')].detach()
    out = []
    for d in range(c['ND']):
        dg = torch.stack([g.grad for g in keep[(l, d)]], dim=1)                       # (B,T,3H)
        yd = y[:, :, d * Hd:(d + 1) * Hd]
        step = 0 if variant == 'same_step' else (-1 if d == 0 else 1)
        flat = torch.cat([yd.new_zeros(1, Hd), yd.reshape(B * T, Hd), yd.new_zeros(1, Hd)])      # rows of (B*T) with a zero row around
        idx = torch.arange(B * T).view(B, T) + step                                  # the neighbouring ROW: crosses into the next batch row
        if variant != 'batch_edge':
            tt = torch.arange(T).view(1, T) + step
            idx = torch.where((tt >= 0) & (tt < T), idx, torch.full_like(idx, -1))    # the zero at the sequence ends
        hprev = flat[(idx + 1).clamp(0, B * T + 1)]
        out.append(torch.einsum('btg,btk->gk', dg, hprev))
    return out


DEC_MUTANTS = [('batch_major', 'dot_3_F_B2'), ('key_last_step', 'dot_1_F'), ('denc_no_value', 'dot_1_F'), ('prev_att_T', 'loc_2_F'),
               ('query_top', 'dot_lstm2'), ('interlayer_scale', 'loc_decdrop'), ('temp_bwd', 'dot_temp2'), ('loc_head0', 'loc_2_F'),
               ('merge_bias_nh', 'dot_2_F')]
GRU_MUTANTS = [('same_step', 'g_base'), ('batch_edge', 'g_T2'), ('n_gate_bhh', 'g_base')]


def dec_mutant(name, c, inp):
    if name == 'merge_bias_nh':
        res = _dec_chain(c, inp, None, rounded=False)
        res['grad.attention.merge_head.bias'] = res['grad.attention.merge_head.bias'] * c['NH']
        return res
    return _dec_chain(c, inp, None, rounded=False, mut=name)


def gru_mutant(name, c, inp):
    keep = {}
    res = _gru_chain(c, inp, None, rounded=False, keep=keep)
    sfxs = ['', '_reverse'][:c['ND']]
    if name in ('same_step', 'batch_edge'):
        exact = _gru_dwhh(c, keep, 0, 'exact')
        for d, w in enumerate(_gru_dwhh(c, keep, 0, name)):
            k = 'grad.encoder.layers.0.layer.weight_hh_l0' + sfxs[d]
            assert float((exact[d] - res[k]).abs().max()) <= 1e-12 * max(1.0, float(res[k].abs().max()))      # the unshifted rule is the oracle's
            res[k] = w
    elif name == 'n_gate_bhh':
        Hd = c['H']
        for s in sfxs:
            # d n_pre reaches b_in directly and b_hn through the reset gate: without the gate b_hn's gradient is b_in's
            res['grad.encoder.layers.0.layer.bias_hh_l0' + s][2 * Hd:] = res['grad.encoder.layers.0.layer.bias_ih_l0' + s][2 * Hd:]
    else:
        raise KeyError(name)
    return res


# ----------------------------------------------------------------------------------------------------------------------
# CPU checks
# ----------------------------------------------------------------------------------------------------------------------
def test_table_covers_the_issue():
    ids = [c['id'] for c in CASES]
    assert len(set(ids)) == len(ids)
    has = lambda **kw: any(all(c[k] == v for k, v in kw.items()) for c in CASES)
    for c in CASES:
        assert leaves_fast_path(c), c['id']
        assert c['Tp'] <= 65 or (c['Tp'] == 257 and c['L'] == 2)
        assert c['L'] <= 5 and c['B'] <= 3 and (c['adim'] == 8 or c['adim'] == 65)
        assert c['feed'] != 'sampled' or (c['dec_p'] == 0 and len(c['decisions']) == c['L'] and not all(c['decisions'][:c['L'] - 1]))
        assert c['feed'] != 'greedy' or not c['train']
    for triple in (('dot', 1, False), ('dot', 1, True), ('dot', 2, False), ('dot', 2, True), ('dot', 3, False), ('loc', 2, False),
                   ('loc', 2, True), ('loc', 3, False)):
        assert has(mode=triple[0], NH=triple[1], vp=triple[2]), triple
    # loc / 1 / F through each way out of the fast path
    one = dict(mode='loc', NH=1, vp=False)
    assert has(module='GRU', **one) and has(dec_p=0.25, module='LSTM', emb_p=0.0, **one) and has(emb_p=0.2, dec_p=0.0, module='LSTM', **one)
    assert has(NL=MAX_DEC_LAYERS + 1, module='LSTM', dec_p=0.0, emb_p=0.0, **one)
    for nl in (1, 2, 3):
        assert has(module='LSTM', NL=nl)
    assert has(module='GRU', NL=1) and has(module='GRU', NL=2)
    assert has(dec_p=0.25, NL=2, emb_p=0.0) and has(emb_p=0.2, dec_p=0.0) and any(c['dec_p'] > 0 and c['emb_p'] > 0 for c in CASES)
    assert has(B=1) and has(B=2, NH=3)
    assert any(1 in c['lens'] and c['Tp'] in c['lens'] and c['Tp'] > 1 for c in CASES)
    for tp in (1, 31, 32, 33, 65):
        assert has(Tp=tp, mode='loc'), tp
    assert has(Tp=257, L=2) and has(L=1, mode='loc') and has(L=1, mode='dot') and has(L=2)
    assert has(Ks=1, mode='loc') and has(Ks=5, Tp=3, mode='loc')
    assert any(c['temp'] != 1 for c in CASES) and has(adim=65)
    assert has(need_denc=False) and has(need_denc=True) and has(len_dtype='int32')
    assert has(feed='greedy', mode='dot') and has(feed='greedy', mode='loc')
    assert any(c['feed'] == 'sampled' and c['mode'] == 'dot' and c['NH'] > 1 for c in CASES)
    assert has(feed='sampled', mode='loc', module='GRU') and any(c['feed'] == 'sampled' and c['emb_p'] > 0 for c in CASES)
    # the GRU encoder layer table
    gids = [c['id'] for c in GRU_CASES]
    assert len(set(gids)) == len(gids)
    ghas = lambda f: any(f(c) for c in GRU_CASES)
    one = lambda c: c['layers'][0]
    assert ghas(lambda c: c['ND'] == 1) and ghas(lambda c: c['ND'] == 2)
    for T in (1, 2, 5):
        assert ghas(lambda c: c['T'] == T)
    assert ghas(lambda c: c['B'] == 1) and ghas(lambda c: c['B'] == 3 and len(set(c['lens'])) > 1)
    assert ghas(lambda c: c['H'] == 16) and ghas(lambda c: c['H'] == 48)
    assert ghas(lambda c: one(c)['ln']) and ghas(lambda c: not one(c)['ln']) and ghas(lambda c: one(c)['p'] == 0.25)
    assert ghas(lambda c: c['style'] == 'drop' and one(c)['rate'] == 2 and c['T'] % 2 == 0)
    assert ghas(lambda c: c['style'] == 'drop' and one(c)['rate'] == 2 and c['T'] % 2 == 1)
    assert ghas(lambda c: c['style'] == 'concat' and one(c)['rate'] == 2 and c['T'] % 2 == 1)
    assert ghas(lambda c: one(c)['proj']) and ghas(lambda c: not one(c)['proj']) and ghas(lambda c: len(c['layers']) == 2)
    assert any(ov.get('module') == ['GRU', 'LSTM'] for _, ov, _ in GRU_REFUSED)
    for c in GRU_CASES:
        assert all(f[1] >= 1 for f in gru_frames(c)) and not any(l['proj'] and l['rate'] > 1 and c['style'] == 'concat' for l in c['layers'])


def _same(got, ref):
    assert set(got) == set(ref)
    for k in ref:
        if ref[k] is None:
            assert got[k] is None, k
        else:
            assert got[k].shape == ref[k].shape and float((got[k] - ref[k]).abs().max()) <= 1e-12 * max(1.0, float(ref[k].abs().max())), k


@pytest.mark.parametrize('case', CASES, ids=[c['id'] for c in CASES])
def test_twin_equals_oracle(case):
    """The stage-by-stage decoder chain with nothing rounded is the oracle's att_decoder_variants: values, states, gradients."""
    inp = inputs(case, case['run_seed'], 'fp32')
    ref = dec_f64(case, inp)
    _same(_dec_chain(case, inp, None, rounded=False), ref)
    assert (ref['denc'] is None) == (not case['need_denc'])
    assert {'grad.' + k for k in inp['sd'] if not k.startswith('encoder.')} == {k for k in ref if k.startswith('grad.')}


@pytest.mark.parametrize('case', GRU_CASES, ids=[c['id'] for c in GRU_CASES])
def test_gru_twin_equals_oracle(case):
    inp = gru_inputs(case, 0, 'fp32')
    ref = gru_f64(case, inp)
    _same(_gru_chain(case, inp, None, rounded=False), ref)
    assert tuple(ref['out'].shape) == (case['B'],) + gru_frames(case)[-1][1::2]
    assert {'grad.' + k for k in inp['sd'] if k.startswith('encoder.')} == {k for k in ref if k.startswith('grad.')}


def test_whole_twin_equals_oracle():
    inp = whole_inputs(0, 'fp32')
    ref = whole_f64(inp)
    P ={k: v.double().clone().requires_grad_(True) for k, v in inp['sd'].items()}
    enc = _gru_layer(inp['x'], P, 'encoder.layers.0.', WHOLE['enc'], 0, None, False)
    ctc = torch.log_softmax(torch.relu(_mm(enc, P['ctc_layer.0.weight'], False) + P['ctc_layer.0.bias']), dim=-1)
    logits, att, _ = _dec_forward(WHOLE['dec'], P, enc, inp['lens'], inp['fed'], None, False)
    ((ctc * inp['dctc']).sum() + (logits * inp['dl']).sum() + (att * inp['wa']).sum()).backward()
    got = {'ctc': ctc.detach(), 'logits': logits.detach(), 'att': att.detach()}
    got.update({'grad.' + k: p.grad for k, p in P.items()})
    _same(got, ref)
    # the encoder output has both consumers: the last encoder layer's gradient is not the decoder path's alone
    only_dec = dict(inp, dctc=torch.zeros_like(inp['dctc']))
    k = 'grad.encoder.layers.0.pj.weight'
    assert float((whole_f64(only_dec)[k] - ref[k]).norm()) > 0.1 * float(ref[k].norm())


def test_twin_rounds():
    """The twin differs from the exact restatement by bf16 rounding in bf16 mode and by fp32 rounding in fp32 mode."""
    for c, run, inp_of in ((BY_ID['loc_2_T'], dec_f64, inputs), (GRU_BY_ID['g_base'], gru_f64, gru_inputs)):
        for prec, lo, hi in (('bf16', 1e-4, 3e-2), ('fp32', 1e-9, 1e-5)):
            inp = inp_of(c, 0, prec)
            m = metrics(run(c, inp, prec), run(c, inp))
            fwd = m['logits'] if 'logits' in m else m['out']
            assert lo < fwd < hi, (c['id'], prec, fwd)


def test_sampled_and_greedy_inputs():
    for c in CASES:
        inp = inputs(c, c['run_seed'], 'bf16')
        fed, teacher = inp['fed'], inp['teacher']
        assert bool((fed[:, 0] == 0).all()) and int(fed.min()) >= 0 and int(fed.max()) < V
        if c['feed'] == 'sampled':
            for t, use_teacher in enumerate(c['decisions'][:c['L'] - 1]):
                assert bool((fed[:, t + 1] == teacher[:, t]).all()) == use_teacher
        elif c['feed'] == 'teacher':
            assert torch.equal(fed[:, 1:], teacher[:, :-1])


@pytest.mark.parametrize('cid', [c['id'] for c in CASES if c['feed'] == 'greedy'])
def test_greedy_margin(cid):
    """At the case's run seed the float64 top-two logit gap at every step is at least 4 x the largest move of a logit that the
    logits bound admits, in both precisions: the reference alone never flips, and a device within the bound feeds its tokens."""
    c = BY_ID[cid]
    for prec in PRECS:
        inp = inputs(c, c['run_seed'], prec)
        fed, logits = greedy_tokens(c, inp['sd'], inp['enc'], inp['lens'])
        assert torch.equal(fed, inp['fed'])
        ref = dec_f64(c, inp)
        assert float((ref['logits'] - logits).abs().max()) <= 1e-12                 # teacher := fed tokens reproduces the greedy run
        top = logits.topk(2, dim=-1).values
        gap, d = float((top[..., 0] - top[..., 1]).min()), greedy_delta(c, prec, ref['logits'])
        print('GREEDY %s %s: smallest top-two gap %.3e, 4 x delta %.3e' % (cid, prec, gap, 4 * d))
        assert gap >= 4 * d, (cid, prec, gap, 4 * d)


def _mutant_fails(name, c, prec, inp_of, mutate, run, bound):
    inp = inp_of(c, 0, prec)
    rep = check(mutate(name, c, inp), run(c, inp), bound)
    bad = [r for r in rep if not r[3]]
    print('MUTANT %s %s %s: %s' % (name, c['id'], prec, ', '.join('%s %.2e > %.2e' % r[:3] for r in bad)))
    assert bad, (name, c['id'], prec)
    # and the unmutated twin passes them, at another seed than the eight
    inp = inp_of(c, N_SEEDS + 1, prec)
    rep = check(run(c, inp, prec), run(c, inp), bound)
    assert all(r[3] for r in rep), [r for r in rep if not r[3]]


@pytest.mark.parametrize('name,cid', DEC_MUTANTS, ids=[m[0] for m in DEC_MUTANTS])
def test_mutants(name, cid):
    c = BY_ID[cid]
    for prec in PRECS:
        _mutant_fails(name, c, prec, inputs, dec_mutant, dec_f64, bounds(c, prec))


@pytest.mark.parametrize('name,cid', GRU_MUTANTS, ids=[m[0] for m in GRU_MUTANTS])
def test_gru_mutants(name, cid):
    c = GRU_BY_ID[cid]
    for prec in PRECS:
        _mutant_fails(name, c, prec, gru_inputs, gru_mutant, gru_f64, gru_bounds(c, prec))


def test_floor_share():
    """At most 10 % of the (case, metric) bounds of both tables and the whole-model case come from the floor rather than from E0 -
    in bf16 mode, where E0 is the error of a rounding model.  In fp32 mode E0 is fp32 arithmetic's own 2 to 4 ulp and the floor is
    n ulp with n the longest sum: most bounds sit on the floor by arithmetic (tests/test_encoder_layer_reference.py found and
    states the same); asserted for fp32 instead: the floor stays a few hundred ulp - no floored fp32 bound exceeds 2^-24 x the
    longest sum of the tables, B * L * T' = 1028 rows of the T' = 257 cases, orders below what any mutant moves (the mutant
    tests reject all twelve in fp32 under these same bounds)."""
    share = {}
    every = [('dec', c['id']) for c in CASES] + [('gru', c['id']) for c in GRU_CASES] + [('whole', WHOLE['id'])]
    for prec in PRECS:
        n = f = 0
        worst = 0.0
        for kind, cid in every:
            b, floored, _ = _bounds(kind, cid, prec)
            n, f = n + len(b), f + len(floored)
            worst = max([worst] + [b[k] for k in floored])
        print('FLOOR %s: %d of %d bounds, largest floored bound %.3e' % (prec, f, n, worst))
        share[prec] = (f, n, worst)
    f, n, _ = share['bf16']
    assert f <= FLOOR_SHARE_CAP * n, ('bf16', f, n)
    longest = max(c['B'] * c['L'] * c['Tp'] for c in CASES)
    assert longest == 1028 and share['fp32'][2] <= FLOOR_ULP * longest, share['fp32']
