"""Beam search for the model variants the fast decode kernels do not cover (GRU decoders, scaled-dot attention, several
heads, value projection, LSTM decoders deeper than H.MAX_DEC_LAYERS): one decoder step for all R = U * beam hypothesis rows
per output position, composed of HIP kernels - the reference's BeamDecoder.forward (src/decode.py:104-116) runs the same
step once per hypothesis at batch size one.

Keys and values are computed once per utterance from its unpadded encoder output and stored (U, NH, T', .) - not per row;
the fused kernel asr_beam_attend (csrc/decode_variants.hip) serves every row of an utterance from them.  Multi-head
attention without a value projection: every head of a hypothesis attends over its own utterance's encoder output (the
reference's batch-size-one semantics, not the head-major repeat of its batched training step, src/variants.py::AttendFn).

The per-row decoder state (h of every layer, c of every LSTM layer, the previous attention of location-aware attention) is
packed into one (R, W) buffer, so that ONE asr_gather_rows re-orders all of it after the bookkeeping has chosen survivors.
The bookkeeping itself (CTC prefix scores, LM step, asr_beam_step, finals) is shared with the fast search (src/decode.py).
"""
import ctypes

import torch

from src import hipabi as H


def _round_up(n, m):
    return (n + m - 1) // m * m


class VariantStep(object):
    """Decoder state and one step of the variant search.  enc (U,T',E) zero-padded fp32, enc_len (U) int64."""

    def __init__(self, asr, enc, enc_len, beam, Lmax):
        att, dec, prec = asr.attention, asr.decoder, asr.prec
        dev, st = enc.device, H.stream_ptr()
        U, Tp, E = enc.shape
        R = U * beam
        NH, A, NL, dim = att.num_head, att.dim, dec.layer, dec.dim
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        self.asr, self.prec, self.R, self.U, self.beam, self.Tp = asr, prec, R, U, beam, Tp
        self.NH, self.A, self.NL, self.dim, self.Dv = NH, A, NL, dim, E
        self.loc, self.lstm = att.mode == 'loc', dec.layers.module == 'LSTM'
        self.kv_bf16 = 1 if prec == H.BF16 else 0
        self.enc_len = enc_len.to(dev, torch.int64).contiguous()
        # ---- memory of the attention, once per utterance (src/asr.py:340-355)
        vw = 8 if self.kv_bf16 else 4                            # elements per 16 bytes: rows padded for vector loads
        enc2 = enc.reshape(U * Tp, E)
        k = f32(U * Tp, NH * A)
        H.linear_fwd(enc2, att.proj_k.weight, att.proj_k.bias, k, act=H.ACT_TANH, prec=prec)
        self.ld_k = _round_up(A, vw)
        key = f32(U, NH, Tp, self.ld_k)
        key[..., :A] = k.view(U, Tp, NH, A).permute(0, 2, 1, 3)
        self.ld_v = _round_up(E, vw)
        if att.v_proj:
            v = f32(U * Tp, NH * E)
            H.linear_fwd(enc2, att.proj_v.weight, att.proj_v.bias, v, act=H.ACT_TANH, prec=prec)
            self.NHv = NH
            value = f32(U, NH, Tp, self.ld_v)
            value[..., :E] = v.view(U, Tp, NH, E).permute(0, 2, 1, 3)
        else:
            self.NHv = 1
            value = f32(U, 1, Tp, self.ld_v)
            value[:, 0, :, :E] = enc
        if self.kv_bf16:
            key, value = self._bf16(key, st), self._bf16(value, st)
        self.key, self.value = key, value
        # ---- per-row state, packed: h_0..h_{NL-1} | c_0..c_{NL-1} (LSTM) | prev_att (NH,T') (loc)
        self.off_c = NL * dim
        self.off_att = self.off_c + (NL * dim if self.lstm else 0)
        self.W = self.off_att + (NH * Tp if self.loc else 0)
        self.state = f32(R, self.W)
        self.pack = f32(R, self.W)
        if self.loc:
            # uniform over the valid frames (LocationAwareAttention, src/module.py:1169-1173), every head
            lens = self.enc_len.repeat_interleave(beam).to(torch.float32).clamp(min=1).view(R, 1, 1)
            ar = torch.arange(Tp, device=dev).view(1, 1, Tp)
            self.state[:, self.off_att:] = torch.where(ar < lens, 1.0 / lens, torch.zeros((), device=dev)).expand(R, NH, Tp).reshape(R, -1)
            Kn = att.att_layer.loc_conv.weight.shape[0]
            self.conv = f32(R, Tp, Kn)
            self.ld_l = _round_up(A, 4)
            self.loc_pre = f32(R, Tp, self.ld_l)
        # ---- step buffers
        self.Xw = dim + E
        self.x = f32(R, self.Xw)
        self.q = f32(R, NH * A)
        self.ctx_heads = f32(R, NH * E) if NH > 1 else None
        self.attn = f32(R, NH * Tp)
        G = 4 if self.lstm else 3
        self.gx, self.gh = f32(R, G * dim), f32(R, G * dim)
        self.cell_scratch = f32(R, 4 * dim)
        self.h_new = [f32(R, dim) for _ in range(NL)]
        self.c_new = [f32(R, dim) for _ in range(NL)] if self.lstm else []
        self.logits = f32(R, asr.vocab_size)
        self.tokens = torch.zeros((R, Lmax + 1), dtype=torch.int64, device=dev)
        self.args = H.BeamAttend()
        a = self.args
        a.key, a.value, a.q, a.enc_len = key.data_ptr(), value.data_ptr(), self.q.data_ptr(), self.enc_len.data_ptr()
        a.attn, a.attn_ld = self.attn.data_ptr(), NH * Tp
        if NH > 1:
            a.ctx, a.ctx_ld = self.ctx_heads.data_ptr(), NH * E
        else:
            a.ctx, a.ctx_ld = self.x[:, dim:].data_ptr(), self.Xw
        a.ld_k, a.ld_v = self.ld_k, self.ld_v
        if self.loc:
            al = att.att_layer
            a.loc, a.ld_l = self.loc_pre.data_ptr(), self.ld_l
            a.wg, a.bg = al.gen_energy.weight.data_ptr(), al.gen_energy.bias.data_ptr()
        a.U, a.rows_per_utt, a.NH, a.NHv, a.Tp, a.A, a.Dv = U, beam, NH, self.NHv, Tp, A, E
        a.mode = H.ATT_LOC if self.loc else H.ATT_DOT
        a.kv_bf16 = self.kv_bf16
        a.temperature = float(att.att_layer.temperature)

    @staticmethod
    def _bf16(t, st):
        out = torch.empty(t.shape, dtype=torch.bfloat16, device=t.device)
        H.call('asr_cast_bf16', H.ptr(t), H.ptr(out), t.numel(), st)
        return out

    def step(self, t):
        """One decoder step of every row at output position t; returns the logits (R,V)."""
        asr, att, dec, prec, st = self.asr, self.asr.attention, self.asr.decoder, self.prec, H.stream_ptr()
        R, NH, A, NL, dim, Tp, W = self.R, self.NH, self.A, self.NL, self.dim, self.Tp, self.W
        s = self.state
        # q = tanh(proj_q(h_0 | ... | h_{NL-1}))  (src/asr.py:251-257,335)
        H.gemm(s, att.proj_q.weight, self.q, R, NH * A, NL * dim, W, NL * dim, NH * A, bias=att.proj_q.bias, act=H.ACT_TANH, prec=prec)
        if self.loc:
            al = att.att_layer
            prev = s[:, self.off_att:].contiguous()
            Kn, _, taps = al.loc_conv.weight.shape
            H.call('asr_loc_conv_fwd', H.ptr(prev), H.ptr(al.loc_conv.weight), R, NH, Tp, Kn, (taps - 1) // 2, H.ptr(self.conv), st)
            H.gemm(self.conv, al.loc_proj.weight, self.loc_pre, R * Tp, A, Kn, Kn, Kn, self.ld_l, act=H.ACT_TANH, prec=prec)
        # embedding of the last token -> x[:, :dim]; context -> x[:, dim:]
        tok = self.tokens[:, t].contiguous()
        V = asr.vocab_size
        H.call('asr_gather_rows', H.ptr(asr.pre_embed.weight), H.ptr(tok), H.ptr(self.x), R, dim, dim, self.Xw, V, st)
        H.call('asr_beam_attend', ctypes.byref(self.args), st)
        if NH > 1:
            E = self.Dv
            H.gemm(self.ctx_heads, att.merge_head.weight, self.x[:, dim:], R, E, NH * E, NH * E, NH * E, self.Xw, bias=att.merge_head.bias,
                   prec=prec)
        # decoder layers (src/asr.py:262-270; dropout is inactive in eval)
        P = dec.layers
        xin, ld_x, K = self.x, self.Xw, self.Xw
        G = self.gx.shape[1]
        for l in range(NL):
            H.gemm(xin, getattr(P, 'weight_ih_l%d' % l), self.gx, R, G, K, ld_x, K, G, bias=getattr(P, 'bias_ih_l%d' % l), prec=prec)
            H.gemm(s[:, l * dim:], getattr(P, 'weight_hh_l%d' % l), self.gh, R, G, dim, W, dim, G, bias=getattr(P, 'bias_hh_l%d' % l), prec=prec)
            if self.lstm:
                c_prev = s[:, self.off_c + l * dim:self.off_c + (l + 1) * dim].contiguous()
                H.call('asr_lstm_cell_fwd', H.ptr(self.gx), H.ptr(self.gh), H.ptr(c_prev), R, dim, H.ptr(self.cell_scratch),
                       H.ptr(self.h_new[l]), H.ptr(self.c_new[l]), st)
            else:
                h_prev = s[:, l * dim:(l + 1) * dim].contiguous()
                H.call('asr_gru_cell_fwd', H.ptr(self.gx), H.ptr(self.gh), H.ptr(h_prev), R, dim, H.ptr(self.cell_scratch),
                       H.ptr(self.h_new[l]), st)
            xin, ld_x, K = self.h_new[l], dim, dim
        H.linear_fwd(self.h_new[-1], dec.char_trans.weight, dec.char_trans.bias, self.logits, prec=prec)
        return self.logits

    def top_state(self, t):
        """(R,dim) hidden state of the top layer just computed (what an embedding-fusing plugin reads)."""
        return self.h_new[-1]

    def reorder(self, t, parent):
        """Row i <- row parent[i] of the state just computed: one gather of the packed state."""
        pieces = self.h_new + self.c_new + ([self.attn] if self.loc else [])
        torch.cat(pieces, dim=1, out=self.pack)
        H.call('asr_gather_rows', H.ptr(self.pack), H.ptr(parent), H.ptr(self.state), self.R, self.W, self.W, self.W, self.R, H.stream_ptr())
