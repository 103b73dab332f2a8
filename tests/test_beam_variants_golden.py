"""CPU restatement of the reference's BeamDecoder.forward (src/decode.py:65-183) for every attention / decoder variant, pinned to
the genuine reference's hypotheses (tests/golden/g11_beam_*.npz, tests/golden/gen_beam_variants.py).  The GPU tests of
tests/test_hip_beam_variants.py use this restatement as their oracle for inputs the fixtures do not cover."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from oracle import asr_oracle as O
from oracle import decode_oracle as DO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(p)[len('g11_beam_'):-4] for p in glob.glob(os.path.join(GOLDEN, 'g11_beam_*.npz')))


def load_case(name):
    z = np.load(os.path.join(GOLDEN, 'g11_beam_%s.npz' % name))
    return yaml.safe_load(str(z['meta'])), z


def case_weights(meta):
    """Seeded weights with the fixture's char_trans scale and <eos> bias shift (gen_beam_variants.tweak)."""
    cfg = O.ModelCfg(meta['model'], meta['D'], meta['V'])
    sd = O.seeded_state_dict(O.param_shapes(cfg), meta['wseed'])
    s = float(meta['ct_scale'])
    sd['decoder.char_trans.weight'] = sd['decoder.char_trans.weight'] * s
    b = sd['decoder.char_trans.bias'] * s
    b[1] += float(meta['eos_shift'])
    sd['decoder.char_trans.bias'] = b
    return cfg, sd


def lm_weights(meta):
    from src.lm import RNNLM
    lm = RNNLM(meta['V'], **meta['lm'])
    return O.seeded_state_dict({k: tuple(v.shape) for k, v in lm.state_dict().items()}, meta['lm_wseed'])


class VariantStepCPU(object):
    """One step of the reference's decoder at batch size one (Attention.forward src/asr.py:331-364, Decoder.forward :262-270)
    from the oracle's pieces; enc (T',Dv) of one utterance; state = (h list, c list, prev_att (1,NH,T') or None)."""

    def __init__(self, enc, enc_len, P, cfg):
        self.P, self.cfg = P, cfg
        Tp, Dv = enc.shape
        nh, ad = cfg.num_head, cfg.att_dim
        self.Tp, self.Dv = Tp, Dv
        self.mask = (torch.arange(Tp)[None, :] >= enc_len[:, None]).expand(nh, Tp)
        key = torch.tanh(enc @ P['attention.proj_k.weight'].t() + P['attention.proj_k.bias'])
        self.key = key.view(Tp, nh, ad).permute(1, 0, 2)                                           # (nh,T',ad)
        if cfg.v_proj:
            v = torch.tanh(enc @ P['attention.proj_v.weight'].t() + P['attention.proj_v.bias'])
            self.value = v.view(Tp, nh, Dv).permute(1, 0, 2)                                        # (nh,T',Dv)
        else:
            self.value = enc.expand(nh, Tp, Dv)                                                     # every head: its own utterance
        self.uniform = torch.where(self.mask, torch.zeros(()), 1.0 / enc_len.to(enc.dtype)).view(1, nh, Tp)

    def init_state(self):
        z = [torch.zeros(1, self.cfg.dec_dim) for _ in range(self.cfg.dec_layer)]
        return (z, [t.clone() for t in z], None)

    def __call__(self, state, tok):
        P, cfg = self.P, self.cfg
        h, c, prev_att = state
        nh, ad = cfg.num_head, cfg.att_dim
        q = torch.tanh(torch.cat(h, -1) @ P['attention.proj_q.weight'].t() + P['attention.proj_q.bias']).view(nh, ad)
        if cfg.att_mode == 'dot':
            energy = torch.einsum('ntd,nd->nt', self.key, q)
        else:
            pa = self.uniform if prev_att is None else prev_att
            conv = F.conv1d(pa, P['attention.att_layer.loc_conv.weight'], padding=cfg.loc_kernel_size)               # (1,Kn,T')
            loc = torch.tanh(conv[0].t() @ P['attention.att_layer.loc_proj.weight'].t())                             # (T',ad)
            u = torch.tanh(self.key + q[:, None, :] + loc[None])
            energy = (u @ P['attention.att_layer.gen_energy.weight'].t()).squeeze(-1) + P['attention.att_layer.gen_energy.bias']
        attn = torch.softmax((energy / cfg.att_temperature).masked_fill(self.mask, O.NEG_INF), dim=-1)            # (nh,T')
        ctx = torch.einsum('nt,ntd->nd', attn, self.value)
        if nh > 1:
            ctx = ctx.reshape(1, nh * self.Dv) @ P['attention.merge_head.weight'].t() + P['attention.merge_head.bias']
        else:
            ctx = ctx.view(1, self.Dv)
        x = torch.cat([P['pre_embed.weight'][tok].view(1, -1), ctx], dim=-1)
        h2, c2 = [], []
        for l in range(cfg.dec_layer):
            W = [P['decoder.layers.%s_l%d' % (n, l)] for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
            if cfg.dec_module == 'LSTM':
                hl, cl = O.lstm_cell(x, h[l], c[l], *W)
            else:
                hl, cl = O.gru_cell(x, h[l], *W), c[l]
            h2.append(hl)
            c2.append(cl)
            x = hl
        logits = x @ P['decoder.char_trans.weight'].t() + P['decoder.char_trans.bias']
        return logits, (h2, c2, attn.view(1, nh, self.Tp) if cfg.att_mode == 'loc' else None)


def beam_search_variants(feat, feat_len, P, cfg, beam_size, min_len_ratio, max_len_ratio, ctc_weight=0.0, lm=None, lm_weight=0.0,
                         eos_threshold=1.5):
    """oracle.decode_oracle.beam_search with the decoder step of any variant.  Returns [(tokens, scores)] best first."""
    with torch.no_grad():
        enc, enc_len = O.encoder(feat, feat_len, P, cfg)
        dec = VariantStepCPU(enc[0], enc_len, P, cfg)
        max_len = int(np.ceil(int(feat_len[0]) * max_len_ratio))
        min_len = int(np.ceil(int(feat_len[0]) * min_len_ratio))
        x_ctc, ctc_state0, ctc_beam = None, None, 0
        if ctc_weight > 0:
            x_ctc = O.ctc_head(enc, P)[0].numpy()
            ctc_state0 = DO.ctc_prefix_init(x_ctc)
            ctc_beam = int(DO.CTC_BEAM_RATIO * beam_size)
        prev_top = [DO.Hyp(dec.init_state(), [], [], None, ctc_state0, 0, None)]
        finals, nxt = [], []
        for t in range(max_len):
            for hyp in prev_top:
                tok = hyp.seq[-1] if len(hyp.seq) else 0
                logits, new_state = dec(hyp.dec_state, tok)
                cur = F.log_softmax(logits, dim=-1)
                att_prob = cur[0].clone()
                ctc_state, ctc_prob, cand = None, None, None
                if ctc_weight > 0:
                    cand = cur[0].topk(ctc_beam)[1].tolist()
                    ctc_prob, ctc_state = DO.ctc_prefix_cheap(x_ctc, hyp.seq, hyp.ctc_state, cand)
                    ctc_char = torch.from_numpy(np.asarray(ctc_prob - hyp.ctc_prob, dtype=np.float32))
                    hack = torch.full_like(cur, DO.LOG_ZERO)
                    for i, ch in enumerate(cand):
                        hack[0, ch] = ctc_char[i]
                    cur = (1 - ctc_weight) * cur + ctc_weight * hack
                    cur[0, 0] = DO.LOG_ZERO
                lm_state = None
                if lm is not None and lm_weight > 0:
                    lm_out, lm_state = DO.rnnlm_step(lm[0], lm[1], tok, hyp.lm_state)
                    cur = cur + lm_weight * F.log_softmax(lm_out, dim=-1)
                topv, topi = cur[0].topk(beam_size)
                new, term = [], None
                for i in range(beam_size):
                    ti = int(topi[i])
                    if ti == 1 and float(att_prob[1]) > eos_threshold * float(att_prob[2:].max()):
                        term = float(topv[i])
                        continue
                    cs, cp = None, None
                    if ctc_state is not None:
                        j = cand.index(ti)
                        cs, cp = ctc_state[j], ctc_prob[j]
                    new.append(DO.Hyp(new_state, hyp.seq + [ti], hyp.scores + [float(topv[i])], lm_state, cs, cp, None))
                if term is not None:
                    hyp.seq = hyp.seq + [1]
                    hyp.scores = hyp.scores + [term]
                    if t >= min_len:
                        finals.append(hyp)
                        if beam_size == 1:
                            return [(hyp.seq, hyp.scores)]
                nxt.extend(new)
            nxt.sort(key=lambda o: o.avg(), reverse=True)
            prev_top, nxt = nxt[:beam_size], []
        finals += prev_top
        finals.sort(key=lambda o: o.avg(), reverse=True)
        return [(hh.seq, hh.scores) for hh in finals[:beam_size]]


def test_fixture_set_is_complete():
    assert set(CASES) >= {'dot', 'dot_mh3', 'loc_mh2', 'loc_mh2_vproj', 'gru2', 'gru1_dot', 'lstm5', 'decdrop2', 'beam1'}
    metas = [load_case(c)[0] for c in CASES]
    assert all(m['min_gap'] >= 1e-3 for m in metas)
    # at least one case ends hypotheses with <eos> before max_len
    early = False
    for c in CASES:
        meta, z = load_case(c)
        max_len = int(np.ceil(int(z['feat_len'][0]) * meta['max_len_ratio']))
        for tag, _, _ in meta['modes']:
            early |= any(len(z['%s_seq%d' % (tag, i)]) < max_len for i in range(int(z['n_' + tag])))
    assert early


@pytest.mark.parametrize('name', CASES)
def test_restatement_reproduces_reference(name):
    meta, z = load_case(name)
    cfg, P = case_weights(meta)
    lm = (lm_weights(meta), meta['lm'])
    feat, flen = torch.from_numpy(z['feat']), torch.from_numpy(z['feat_len'])
    for tag, ctc_w, lm_w in meta['modes']:
        got = beam_search_variants(feat, flen, P, cfg, meta['beam'], meta['min_len_ratio'], meta['max_len_ratio'], ctc_weight=ctc_w,
                                   lm=lm if lm_w > 0 else None, lm_weight=lm_w)
        assert len(got) == int(z['n_' + tag]), (name, tag)
        for i, (seq, sc) in enumerate(got):
            assert seq == z['%s_seq%d' % (tag, i)].tolist(), (name, tag, i, seq, z['%s_seq%d' % (tag, i)].tolist())
            np.testing.assert_allclose(np.array(sc, dtype=np.float32), z['%s_score%d' % (tag, i)], rtol=0, atol=1e-5)
            assert abs(sum(sc) / len(sc) - float(z['%s_avg%d' % (tag, i)])) < 1e-5
