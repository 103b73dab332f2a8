"""Beam-search decoder with the reference's behaviour (src/decode.py:65-281) — hypothesis expansion, the <eos>
threshold rule, joint CTC / RNN-LM scoring, average-score pruning — batched over utterances AND live hypotheses on the
GPU.  `forward` keeps the whole search on the device: per output position one attention+decoder step, one CTC
prefix-score launch, one LM step and ONE bookkeeping kernel (asr_beam_step: fusion, top-k, <eos> rule, pruning, finals)
for all U x beam rows; nothing is copied to the host until the search has ended.  `forward_host` is the first
implementation (score table on the host each step), kept as a cross-check for the shipped decoder.  Models the decode
kernels do not cover (GRU, dot / multi-head attention, v_proj, deep LSTM) take the step of src/decode_variants.py; both
searches share the bookkeeping of _BeamBook.  A CTC-only model (ctc_weight = 1: no attention decoder) is decoded by a CTC
prefix beam search instead, the whole search of all utterances in ONE launch (asr_ctc_beam_search, csrc/ctc_decode.hip); with
an RNN-LM (shallow fusion) by the resumable form of that search, which stops whenever a new prefix needs an LM step
(asr_ctc_beam_lm_advance).  The reference has no counterpart (`# ToDo : implement pure ctc decode`).  A joint model built
with rescore=True is decoded in two passes: that CTC search proposes the n-best list, the attention decoder scores the
hypotheses teacher-forced in one batched pass, and asr_rescore_nbest (csrc/rescore.hip) mixes the scores and re-ranks.  With
lm_rescore=True an RNN-LM scores that list too, teacher-forced by its full-sequence forward (asr_rescore_token_logp,
asr_rescore_rank_lm), and stays out of the first pass."""
import ctypes
import math

import torch
import yaml
from torch import nn

from src import functions as F_hip
from src import hipabi as H
from src import ragged
from src.ctc import CTCPrefixScore
from src.lm import RNNLM

CTC_BEAM_RATIO = 1.5
LOG_ZERO = -10000000.0
EOS = 1
# Two-pass decoding runs the TRAINING forward of the decoder, which keeps its per-step state for a backward pass that never
# comes; the largest piece is the location convolution's output, (rows, L, Kn, T') fp32.  A chunk of hypothesis rows keeps that
# under RESCORE_STATE_BYTES (the sibling of ragged.FRONTEND_ACT_BYTES) and holds at most RESCORE_MAX_ROWS rows, the most the
# streamed decoder plan takes at once (csrc/decoder_plan.h: B <= 64).
RESCORE_STATE_BYTES = 1 << 30
RESCORE_MAX_ROWS = 64
SOS = 0                     # what the LM sees in front of every sequence (RNNLM's convention: _search_ctc_lm starts its rows with it)


def encode_unpadded(asr, audio_feature, feature_len, with_ctc):
    """Encoder (+ CTC log-probs when `with_ctc`) of every utterance on its own, unpadded - the reference decodes one
    utterance at a time (src/decode.py:67) and a padded BiLSTM pass is not equivalent (the reverse direction would start
    inside the padding) - written into zero-padded (U,T'max,.) tensors for a batched search or alignment.  Returns
    (enc, enc_len int64 (U), tlen int32 (U), ctc log-probs or None)."""
    dev = audio_feature.device
    ctx = ragged.eval_ctx(asr)
    U = audio_feature.shape[0]
    encs, lens, ctcs = [], [], []
    for u in range(U):
        n = int(feature_len[u])
        e, el = asr.encoder(audio_feature[u:u + 1, :n].float(), feature_len[u:u + 1].to(dev), ctx)
        e = F_hip.to_f32(e)
        encs.append(e[0])
        lens.append(int(el[0]))
        if with_ctc:
            ctcs.append(F_hip.CTCHeadFn.apply(asr._anchor, e, asr.ctc_layer[0], asr.prec, False, False)[0])
    Tp = max(e.shape[0] for e in encs)
    enc = torch.zeros((U, Tp, encs[0].shape[1]), dtype=torch.float32, device=dev)
    ctc = torch.zeros((U, Tp, asr.vocab_size), dtype=torch.float32, device=dev) if with_ctc else None
    for u in range(U):
        enc[u, :encs[u].shape[0]] = encs[u]
        if ctc is not None:
            ctc[u, :ctcs[u].shape[0]] = ctcs[u]
    # the reference takes T' from the encoder OUTPUT (its masks / CTC scorer see every output frame of the unpadded pass)
    tlen = torch.tensor([e.shape[0] for e in encs], dtype=torch.int32, device=dev)
    return enc, torch.tensor(lens, dtype=torch.int64, device=dev), tlen, ctc


@torch.no_grad()
def encode_batched(asr, audio_feature, feature_len, with_ctc):
    """encode_unpadded's result - same return contract, padding rows of enc and ctc exactly 0 - from ONE pass of the front-end
    (vgg 1..7, when the model has one) and of every encoder layer over the padded batch (src/ragged.py: the data is aligned and
    masked per row, the convolution and recurrence launches are unchanged) and one of the CTC head.  Agrees with
    encode_unpadded to rounding, not bit for bit; tlen and enc_len are equal.  The caller's feature padding is never used,
    nor are the n % time_div trailing frames a conv front-end drops.  More utterances than the recurrence takes at once
    (ragged.max_batch) or than keep the largest front-end activation under ragged.FRONTEND_ACT_BYTES
    (ragged.frontend_max_batch) go in chunks; a model the pass does not cover (ragged.ineligible_reason: GRU layers) is
    encoded by encode_unpadded."""
    if ragged.ineligible_reason(asr) is not None:
        return encode_unpadded(asr, audio_feature, feature_len, with_ctc)
    dev = audio_feature.device
    flen = [int(x) for x in feature_len.reshape(-1).tolist()]
    U, cap = audio_feature.shape[0], min(ragged.max_batch(asr), ragged.frontend_max_batch(asr, max(flen)))
    parts = []
    for u0 in range(0, U, cap):
        fl = flen[u0:u0 + cap]
        parts.append(ragged.encode_chunk(asr, audio_feature[u0:u0 + cap, :max(fl)], fl, with_ctc))
    tl = [n for p in parts for n in p[1]]
    enc_len = torch.tensor([n for p in parts for n in p[2]], dtype=torch.int64, device=dev)
    tlen = torch.tensor(tl, dtype=torch.int32, device=dev)
    if len(parts) == 1:
        return parts[0][0], enc_len, tlen, parts[0][3]
    Tp = max(tl)
    enc = torch.zeros((U, Tp, parts[0][0].shape[2]), dtype=torch.float32, device=dev)
    ctc = torch.zeros((U, Tp, asr.vocab_size), dtype=torch.float32, device=dev) if with_ctc else None
    for i, p in enumerate(parts):
        enc[i * cap:i * cap + p[0].shape[0], :p[0].shape[1]] = p[0]
        if with_ctc:
            ctc[i * cap:i * cap + p[3].shape[0], :p[3].shape[1]] = p[3]
    return enc, enc_len, tlen, ctc


def encoder_pass_msg(asr, batch_encode):
    """The line of create_msg that says which encoder pass a decoder / aligner uses."""
    if not batch_encode:
        return '           |Encoder pass: one utterance at a time, unpadded'
    why = ragged.ineligible_reason(asr)
    if why is not None:
        return '           |Encoder pass: batch_encode asked for, but fell back to one utterance at a time ({})'.format(why)
    return '           |Encoder pass: batched, length-aware (one pass per layer over the padded batch)'


def _masked_rows(dst, src, mask):
    """dst[.., r, :] = src[.., r, :] where mask[r], in place: one asr_masked_copy_rows per (n, width) matrix of an LM table or
    state (a tensor (n, V) / (layers, n, dim), or a tuple of such)."""
    if isinstance(dst, (tuple, list)):
        for d, s_ in zip(dst, src):
            _masked_rows(d, s_, mask)
        return
    n, w = dst.shape[-2], dst.shape[-1]
    for d, s_ in zip(dst.reshape(-1, n, w), src.reshape(-1, n, w)):
        H.call('asr_masked_copy_rows', H.ptr(s_), H.ptr(mask), H.ptr(d), n, w, w, w, H.stream_ptr())


class Hypothesis(object):
    """History of one partial transcript (reference src/decode.py:186-281); `row` = its row in the device state."""

    def __init__(self, row, output_seq, output_scores, ctc_prob=0.0, ctc_idx=None):
        self.row, self.output_seq, self.output_scores = row, output_seq, output_scores
        self.ctc_prob, self.ctc_idx = ctc_prob, ctc_idx

    def avgScore(self):
        assert len(self.output_scores) != 0
        return sum(self.output_scores) / len(self.output_scores)

    @property
    def outIndex(self):
        return [int(i) for i in self.output_seq]

    def addTopk(self, topi, topv, att_prob, ctc_prob=None, ctc_candidates=None, eos_threshold=1.5):
        new_hyps, term_score = [], None
        for i in range(topi.shape[-1]):
            tok = int(topi[i])
            if tok == 1:
                max_score_no_eos = float(att_prob[2:].max())
                if float(att_prob[tok]) > eos_threshold * max_score_no_eos:
                    term_score = float(topv[i])
                    continue
            cp, ci = None, None
            if ctc_prob is not None:
                ci = ctc_candidates.index(tok)
                cp = float(ctc_prob[ci])
            new_hyps.append(Hypothesis(self.row, self.output_seq + [tok], self.output_scores + [float(topv[i])], cp, ci))
        if term_score is not None:
            self.output_seq.append(1)
            self.output_scores.append(term_score)
            return self, new_hyps
        return None, new_hyps


class CTCHypothesis(object):
    """One result of the CTC prefix beam search: the collapsed token sequence (a trailing <eos> included when the model
    emits one) and its score.  CTC gives a sequence no per-token scores, so avgScore() IS the sequence score (not divided by
    the length) - the quantity the search ranks by: the sequence's CTC log-probability `ctc_score`, plus with an LM
    lm_weight * its LM log-probability + len_bonus * its length.  After two-pass decoding (rescore=True) `score` is the mixed
    score the list was re-ranked by and `att_score` the attention decoder's log-probability of the sequence and its <eos>; with
    the LM in the second pass (lm_rescore=True) `lm_score` is the LM's unweighted log-probability of the sequence (no <eos> term),
    otherwise None."""

    def __init__(self, output_seq, score, ctc_score=None, att_score=None, lm_score=None):
        self.output_seq, self.score = output_seq, score
        self.ctc_score = score if ctc_score is None else ctc_score
        self.att_score, self.lm_score = att_score, lm_score

    def avgScore(self):
        return self.score

    @property
    def outIndex(self):
        return [int(i) for i in self.output_seq]


class BeamDecoder(nn.Module):
    def __init__(self, asr, emb_decoder, beam_size, min_len_ratio, max_len_ratio, lm_path='', lm_config='', lm_weight=0.0,
                 ctc_weight=0.0, batch_encode=False, len_bonus=0.0, rescore=False, rescore_rows=None, lm_rescore=False,
                 lm_rescore_rows=None):
        super().__init__()
        # an embedding-fusing plugin (src/plugin.py) replaces log_softmax(logits) of every step by its fused log-probs
        assert emb_decoder is None or hasattr(emb_decoder, 'fuse_rows'), \
            'emb_decoder must be a src.plugin.EmbeddingRegularizer (its fuse_rows scores every step), got %s' % type(emb_decoder).__name__
        self.apply_emb = emb_decoder is not None and bool(getattr(emb_decoder, 'enable', False)) and emb_decoder.apply_fuse
        self.emb_decoder = emb_decoder if self.apply_emb else None
        if self.apply_emb and rescore:
            raise ValueError('rescore=True together with an emb_decoder: two-pass rescoring scores whole hypotheses with the plain '
                             'decoder and has no embedding-fused form; decode with the joint beam search (rescore=False)')
        if self.apply_emb and not asr.enable_att:
            raise ValueError('an emb_decoder fuses the attention decoder\'s distribution, and this model has none (CTC-only, ctc_weight = 1)')
        self.batch_encode = bool(batch_encode)      # opt-in: the batched pass agrees with the per-utterance one to rounding only
        self.beam_size, self.min_len_ratio, self.max_len_ratio, self.asr = beam_size, min_len_ratio, max_len_ratio, asr
        self.ctc_only = not self.asr.enable_att
        self.rescore, self.lm_rescore = bool(rescore), bool(lm_rescore)
        if self.lm_rescore and not self.rescore:
            raise ValueError('lm_rescore=True puts the LM into the second pass of two-pass decoding, and there is none without '
                             'rescore=True: give both, or fuse the LM into the search (lm_weight alone)')
        if self.lm_rescore and lm_rescore_rows is not None and lm_rescore_rows < 1:
            raise ValueError('lm_rescore_rows = %r: a chunk of the LM pass holds at least one hypothesis row' % (lm_rescore_rows,))
        self.lm_rescore_rows = lm_rescore_rows
        if self.rescore:
            # two passes: the CTC search below proposes, the attention decoder rescores - the model needs both halves
            if self.ctc_only:
                raise ValueError('rescore=True needs an attention decoder to rescore with, and this model has none (CTC-only, '
                                 'ctc_weight = 1): decode it without rescore, by the CTC prefix beam search alone')
            if not self.asr.ctc_weight > 0:
                raise ValueError('rescore=True needs a CTC head to propose the n-best list, and this model has none (ctc_weight = 0): '
                                 'decode it without rescore, by the joint beam search')
        if self.ctc_only or self.rescore:
            # no attention decoder to search with: CTC prefix beam search.  Nothing to mix the CTC score with (ctc_weight is
            # ignored), and the frames bound the length (the length ratios are ignored).  With rescore the same search is the
            # first pass, and ctc_weight mixes its score with the attention decoder's in the second
            assert self.asr.ctc_weight > 0, 'ASR was not trained with CTC decoder'
            if lm_weight > 0 and not lm_config:
                raise NotImplementedError('RNN-LM fusion for CTC-only decoding is not built into a decoder that names no LM: '
                                          'give lm_config (and lm_path), or construct with lm_weight = 0 and call set_lm(lm, weight)')
            if not 1 <= beam_size <= H.CTC_BEAM_MAX:
                raise ValueError('the CTC prefix beam search (CTC-only decoding, first pass of rescore) takes a beam of 1..%d, got %d'
                                 % (H.CTC_BEAM_MAX, beam_size))
            self.fast, self.apply_ctc, self.apply_lm = False, True, False
            self.ctc_cand = min(self.asr.vocab_size - 1, int(CTC_BEAM_RATIO * self.beam_size))
            self.len_bonus = float(len_bonus)         # per-token insertion bonus of the fused score; the CTC search alone uses it
            if self.rescore:
                if not 0 <= ctc_weight <= 1:
                    raise ValueError('rescore mixes (1 - ctc_weight) * attention + ctc_weight * CTC: ctc_weight %r is outside 0..1' % (ctc_weight,))
                if rescore_rows is not None and rescore_rows < 1:
                    raise ValueError('rescore_rows = %r: a chunk of the decoder pass holds at least one hypothesis row' % (rescore_rows,))
                self.ctc_w, self.rescore_rows = float(ctc_weight), rescore_rows
                self.phase_hook = None                # called with a phase's name when its launches are issued (tools/bench_decode.py)
            if lm_weight > 0:
                self.set_lm(self._load_lm(lm_config, lm_path), lm_weight)
            return
        # the decode kernels of the shipped decoder (asr_att_decoder_step) cover an LSTM of <= MAX_DEC_LAYERS layers with
        # location-aware single-head attention and no value projection, whatever its dropout (inactive in eval); every other
        # model runs the variant search of src/decode_variants.py
        if self.asr.vocab_size > H.BEAM_WIDE_MAX_V:
            raise ValueError('the joint beam search takes a vocabulary of at most %d tokens (asr_beam_step_wide), this model has %d'
                             % (H.BEAM_WIDE_MAX_V, self.asr.vocab_size))
        self.fast = self.asr.decoder.layers.module == 'LSTM' and self.asr.decoder.layer <= H.MAX_DEC_LAYERS and self.asr.attention.fast
        self.apply_ctc = ctc_weight > 0
        if self.apply_ctc:
            assert self.asr.ctc_weight > 0, 'ASR was not trained with CTC decoder'
            self.ctc_w = ctc_weight
            self.ctc_beam_size = int(CTC_BEAM_RATIO * self.beam_size)
        self.apply_lm = lm_weight > 0
        if self.apply_lm:
            self.lm_w = lm_weight
            if lm_config:
                self.lm = self._load_lm(lm_config, lm_path)

    def _load_lm(self, lm_config, lm_path):
        cfg = yaml.load(open(lm_config, 'r'), Loader=yaml.FullLoader)
        lm = RNNLM(self.asr.vocab_size, **cfg['model'])
        if lm_path:
            lm.load_state_dict(torch.load(lm_path, map_location='cpu')['model'])
        return lm

    def set_lm(self, lm, weight):
        """Fuse `lm` with `weight`.  A CTC-only model takes anything with RNNLM's decoding interface: init_state(n, device),
        step(tokens, state) -> (log-probs (n,V), state) and gather_state(state, index), the state one fp32 (layers, n, dim)
        tensor or a tuple of them.  With lm_rescore=True the LM scores the n-best list in the second pass instead and needs
        RNNLM's full-sequence interface: forward(tokens (B,T) int64 on the device) -> (logits (B,T,V) fp32, anything), position t
        predicting the token behind tokens[:, :t + 1], <sos> = 0 in column 0, from the zero state, one direction only (so that
        what follows a position cannot change it), together with eval() / train() and a settable `prec`; an object without such
        a forward is refused here."""
        if getattr(self, 'lm_rescore', False):
            self._check_lm_forward(lm)
        self.apply_lm, self.lm_w, self.lm = True, weight, lm

    @staticmethod
    def _check_lm_forward(lm):
        fwd = getattr(lm, 'forward', None)
        if not callable(fwd) or getattr(fwd, '__func__', fwd) is nn.Module.forward:
            raise ValueError('lm_rescore=True scores whole hypotheses with the LM\'s full-sequence forward(tokens) -> (logits (B,T,V), _), '
                             'and %s has none (step() alone serves the first-pass fusion only)' % type(lm).__name__)

    def _check_lm_rescore(self):
        """What forward refuses with lm_rescore=True, before anything is launched."""
        if not self.apply_lm or getattr(self, 'lm', None) is None:
            raise ValueError('lm_rescore=True needs an LM to score the n-best list with, and none was given: name one by lm_config '
                             '(and lm_path) with lm_weight > 0, or call set_lm(lm, weight)')
        if not self.lm_w > 0:
            raise ValueError('lm_rescore=True with lm_weight = %r: the LM pass would change nothing; give a weight above 0 or leave '
                             'lm_rescore out' % (self.lm_w,))
        self._check_lm_forward(self.lm)

    def create_msg(self):
        if self.rescore:
            msg = ['Decode spec| Two-pass decoding: CTC prefix beam search, then attention rescoring of its n-best list\t| Beam size = {}'
                   '\t| Tokens extended per frame = {}'.format(self.beam_size, self.ctc_cand),
                   '           |Rescoring score = (1 - w) * attention + w * CTC \t| ctc_weight w = {:.2f}'.format(self.ctc_w),
                   '           |Min/Max len ratio are ignored (the frames bound the length)']
            if self.lm_rescore:
                msg.append('           |LM scores the n-best list in the second pass (none in the first) \t| weight = {:.2f}'
                           '\t| length bonus = {:.2f}'.format(self.lm_w if self.apply_lm else 0.0, self.len_bonus))
            elif self.apply_lm:
                msg.append('           |LM shallow fusion in the first pass, its terms added unweighted in the second \t| weight = {:.2f}'
                           '\t| length bonus = {:.2f}'.format(self.lm_w, self.len_bonus))
            msg.append(encoder_pass_msg(self.asr, self.batch_encode))
            return msg
        if self.ctc_only:
            msg = ['Decode spec| CTC-only model: CTC prefix beam search\t| Beam size = {}\t| Tokens extended per frame = {}'.format(
                       self.beam_size, self.ctc_cand),
                   '           |Min/Max len ratio, ctc_weight are ignored (the frames bound the length; nothing to mix with)']
            if self.apply_lm:
                msg.append('           |LM shallow fusion enabled \t| weight = {:.2f}\t| length bonus = {:.2f}'.format(self.lm_w, self.len_bonus))
            msg.append(encoder_pass_msg(self.asr, self.batch_encode))
            return msg
        msg = ['Decode spec| Beam size = {}\t| Min/Max len ratio = {}/{}'.format(self.beam_size, self.min_len_ratio, self.max_len_ratio)]
        if self.apply_ctc:
            msg.append('           |Joint CTC decoding enabled \t| weight = {:.2f}\t'.format(self.ctc_w))
        if self.apply_lm:
            msg.append('           |Joint LM decoding enabled \t| weight = {:.2f}'.format(self.lm_w))
        if self.apply_emb:
            msg.append('           |Joint Emb. decoding enabled \t| weight = {:.2f}'.format(float(self.emb_decoder.get_weight().mean())))
        msg.append(encoder_pass_msg(self.asr, self.batch_encode))
        return msg

    def _encode(self, audio_feature, feature_len):
        encode = encode_batched if self.batch_encode else encode_unpadded
        return encode(self.asr, audio_feature, feature_len, self.apply_ctc)

    @torch.no_grad()
    def forward(self, audio_feature, feature_len):
        """audio_feature (U,T,D) zero-padded, feature_len (U).  U == 1: the reference's return value (list of <= beam
        Hypothesis, best first); U > 1: a list of such lists.  No device-to-host copy inside the search loop."""
        if self.rescore:
            return self._forward_rescore(audio_feature, feature_len)
        if self.ctc_only:
            return self._forward_ctc(audio_feature, feature_len)
        U = audio_feature.shape[0]
        flens = [int(x) for x in feature_len.reshape(-1).tolist()]
        max_lens = [int(math.ceil(f * self.max_len_ratio)) for f in flens]
        min_lens = [int(math.ceil(f * self.min_len_ratio)) for f in flens]
        Lmax = max(max(max_lens), 1)
        enc, enc_len, tlen, ctc_lp = self._encode(audio_feature, feature_len)
        if self.fast:
            dec = _FastStep(self.asr, enc, enc_len, self.beam_size, Lmax)
        else:
            from src.decode_variants import VariantStep
            dec = VariantStep(self.asr, enc, enc_len, self.beam_size, Lmax)
        book = _BeamBook(self, U, Lmax, min_lens, max_lens, ctc_lp, tlen, dec.tokens)
        for t in range(Lmax):
            logits = dec.step(t)
            parent = book.step(t, logits, dec.top_state(t) if self.apply_emb else None)
            dec.reorder(t, parent)                          # state of the survivors: new row i <- row parent[i]
            if (t & 15) == 15 and book.all_done():          # every 16 positions: stop early when every search has ended
                break
        return book.readout()

    def _forward_ctc(self, audio_feature, feature_len):
        """CTC-only model: one asr_ctc_beam_search launch runs every frame of every utterance; the results are read back
        once, after it.  Returns CTCHypothesis objects in the shape of forward's contract."""
        _, _, tlen, ctc_lp = self._encode(audio_feature, feature_len)
        return self._read_ctc(self._search_ctc_lm(ctc_lp, tlen) if self.apply_lm else self._search_ctc(ctc_lp, tlen))

    def _forward_ctc_lm(self, ctc_lp, tlen, max_frames=0):
        """The resumable search on an encoded batch, read back (tools/bench_decode.py times it)."""
        return self._read_ctc(self._search_ctc_lm(ctc_lp, tlen, max_frames))

    @staticmethod
    def _read_ctc(res):
        """The one read-back of a CTC search: CTCHypothesis objects in the shape of forward's contract."""
        n_c, len_c, tok_c, sc_c = res['n'].cpu(), res['len'].cpu(), res['tokens'].cpu(), res['score'].cpu()
        cs_c = sc_c if res['ctc_score'] is res['score'] else res['ctc_score'].cpu()
        U = n_c.shape[0]
        out = [[CTCHypothesis(tok_c[u, i, :int(len_c[u, i])].tolist(), float(sc_c[u, i]), float(cs_c[u, i])) for i in range(int(n_c[u]))]
               for u in range(U)]
        return out[0] if U == 1 else out

    def _search_ctc(self, ctc_lp, tlen):
        """The one-launch search; its result stays on the device: tokens (U,K,T') int32, len (U,K), n (U), score = ctc_score (U,K)."""
        U, Tp, V = ctc_lp.shape
        K, dev = self.beam_size, ctc_lp.device
        toks = torch.empty((U, K, Tp), dtype=torch.int32, device=dev)
        lens, n = torch.empty((U, K), dtype=torch.int32, device=dev), torch.empty(U, dtype=torch.int32, device=dev)
        score = torch.empty((U, K), dtype=torch.float32, device=dev)
        nbytes = int(H.lib().asr_ctc_beam_search_workspace_bytes(U, Tp, K))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        H.call('asr_ctc_beam_search', H.ptr(ctc_lp), H.ptr(tlen), U, Tp, V, K, self.ctc_cand, Tp, H.ptr(toks), H.ptr(lens), H.ptr(score),
               H.ptr(n), H.ptr(ws), nbytes, H.stream_ptr())
        return {'tokens': toks, 'len': lens, 'n': n, 'score': score, 'ctc_score': score}

    def _search_ctc_lm(self, ctc_lp, tlen, max_frames=0):
        """The search with an LM: the resumable one.  Row u*K + r of the LM table and state belongs to beam slot r of
        utterance u.  Every asr_ctc_beam_lm_advance launch runs frames until some slot of an utterance is a new prefix (at least
        one frame of every unfinished utterance, so T' launches always suffice), then says per slot which row it inherits
        (src_row), with which token the LM has to step it (step_tok) and whether it is new (need); the glue gathers, steps all
        rows and keeps the stepped ones where need.  No device-to-host copy inside the loop except the early-stop check every
        16 launches.  self.launches = the number of advance launches of the last call."""
        U, Tp, V = ctc_lp.shape
        K, dev, st = self.beam_size, ctc_lp.device, H.stream_ptr()
        R = U * K
        lm = self.lm
        lm.prec = self.asr.prec
        i32 = lambda *s_: torch.empty(s_, dtype=torch.int32, device=dev)
        src_row, step_tok = torch.empty(R, dtype=torch.int64, device=dev), torch.empty(R, dtype=torch.int64, device=dev)
        need, frame, done = i32(R), i32(U), i32(U)
        nbytes = int(H.lib().asr_ctc_beam_lm_workspace_bytes(U, Tp, K))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        lm_lp, state = lm.step(torch.zeros(R, dtype=torch.int64, device=dev), lm.init_state(R, dev))         # <sos> = 0
        lm_lp = lm_lp.contiguous()
        H.call('asr_ctc_beam_lm_init', U, Tp, K, H.ptr(ws), nbytes, st)
        self.launches = 0
        for it in range(Tp):
            H.call('asr_ctc_beam_lm_advance', H.ptr(ctc_lp), H.ptr(tlen), H.ptr(lm_lp), U, Tp, V, K, self.ctc_cand, float(self.lm_w),
                   float(self.len_bonus), max_frames, H.ptr(src_row), H.ptr(step_tok), H.ptr(need), H.ptr(frame), H.ptr(done),
                   H.ptr(ws), nbytes, st)
            self.launches += 1
            state_g = lm.gather_state(state, src_row)
            lp_g = torch.empty_like(lm_lp)
            H.call('asr_gather_rows', H.ptr(lm_lp), H.ptr(src_row), H.ptr(lp_g), R, V, V, V, R, st)
            lp_n, state_n = lm.step(step_tok, state_g)
            _masked_rows(lp_g, lp_n.contiguous(), need)
            _masked_rows(state_g, state_n, need)
            lm_lp, state = lp_g, state_g
            if (it & 15) == 15 and bool(done.all()):           # every 16 launches: stop early when every search has ended
                break
        toks, lens, n = i32(U, K, Tp), i32(U, K), i32(U)
        score, ctc_score = torch.empty((U, K), dtype=torch.float32, device=dev), torch.empty((U, K), dtype=torch.float32, device=dev)
        H.call('asr_ctc_beam_lm_readout', U, Tp, K, Tp, H.ptr(toks), H.ptr(lens), H.ptr(score), H.ptr(ctc_score), H.ptr(n), H.ptr(ws),
               nbytes, st)
        return {'tokens': toks, 'len': lens, 'n': n, 'score': score, 'ctc_score': ctc_score}

    def _forward_rescore(self, audio_feature, feature_len):
        """Two passes.  First: the CTC search above on the joint model's CTC log-probs, its n-best list left on the device.
        Second: asr_rescore_pack makes the teacher table, the encoder output is expanded to one row per hypothesis
        (asr_gather_rows), the teacher-forced decoder forward ASR.forward uses runs over the rows in chunks, and ONE
        asr_rescore_nbest launch scores, mixes and ranks.  Host reads: the 4-byte max_len (the decoder's step count is a host
        integer) before the decoder pass, the results after the last launch.  Returns, per utterance, the first pass's
        hypotheses (their sequences untouched: the <eos> the scoring appends is not output) in the new order, score = the mixed
        score, ctc_score as the first pass gave it, att_score the decoder's.
        With lm_rescore the first pass is always the one-launch search without the LM; behind the decoder pass the LM scores the
        same rows (_lm_pass), asr_rescore_nbest still gives att_score (its own total and order are not used) and
        asr_rescore_rank_lm mixes in lm_weight * lm_score + len_bonus * length and ranks.  No further host read before the
        read-back, which brings lm_score along."""
        if self.lm_rescore:
            self._check_lm_rescore()
        asr, K, st = self.asr, self.beam_size, H.stream_ptr()
        phase = self.phase_hook or (lambda name: None)
        enc, enc_len, tlen, ctc_lp = self._encode(audio_feature, feature_len)
        phase('encoder')
        first = self._search_ctc_lm(ctc_lp, tlen) if self.apply_lm and not self.lm_rescore else self._search_ctc(ctc_lp, tlen)
        phase('first_pass')
        U, Tp, E = enc.shape
        V, dev, R, Lr = asr.vocab_size, enc.device, U * K, Tp + 1
        i64 = lambda *s_: torch.empty(s_, dtype=torch.int64, device=dev)
        teacher, row_utt, row_len = i64(R, Lr), i64(R), i64(R)
        tgt_len, max_len = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        H.call('asr_rescore_pack', H.ptr(first['tokens']), H.ptr(first['len']), H.ptr(first['n']), H.ptr(enc_len), U, K, Tp, Lr, EOS,
               H.ptr(teacher), H.ptr(tgt_len), H.ptr(row_utt), H.ptr(row_len), H.ptr(max_len), st)
        L = max(1, int(max_len.item()))
        rows = self._rescore_chunk_rows(L, Tp)
        fast = asr.decoder.fast and asr.attention.fast and asr.emb_drop == 0.0        # the choice of ASR.forward
        ctx = ragged.eval_ctx(asr)
        enc2d = enc.reshape(U, Tp * E)
        logits = None if rows >= R else torch.empty((R, L, V), dtype=torch.float32, device=dev)
        was_training = asr.training
        asr.eval()
        try:
            for r0 in range(0, R, rows):
                r1 = min(R, r0 + rows)
                enc_rows = torch.empty((r1 - r0, Tp, E), dtype=torch.float32, device=dev)
                H.call('asr_gather_rows', H.ptr(enc2d), H.ptr(row_utt[r0:r1]), H.ptr(enc_rows), r1 - r0, Tp * E, Tp * E, Tp * E, U, st)
                if fast:
                    _, dst = F_hip.att_decoder_forward(asr, enc_rows, row_len[r0:r1], L, teacher[r0:r1], asr.prec)
                    out = dst['logits']
                else:
                    from src.variants import variant_decoder
                    out, _, _ = variant_decoder(asr, asr._anchor, enc_rows, row_len[r0:r1], L, teacher[r0:r1, :L].contiguous(), 1.0, ctx)
                    out = out.contiguous()
                if logits is None:
                    logits = out
                else:
                    logits[r0:r1].copy_(out)
        finally:
            asr.train(was_training)
        phase('decoder_pass')
        tok_logp = None
        if self.lm_rescore:
            tok_logp = self._lm_pass(teacher, Lr, first['len'], R, L)
            phase('lm_pass')
        att, total = torch.empty((U, K), dtype=torch.float32, device=dev), torch.empty((U, K), dtype=torch.float32, device=dev)
        order = torch.empty((U, K), dtype=torch.int32, device=dev)
        H.call('asr_rescore_nbest', H.ptr(logits), logits.stride(0), logits.stride(1), H.ptr(teacher), Lr, H.ptr(tgt_len),
               H.ptr(first['ctc_score']), H.ptr(first['score']), H.ptr(first['n']), U, K, L, V, self.ctc_w, H.ptr(att), H.ptr(total),
               H.ptr(order), st)
        lm_c = None
        if self.lm_rescore:
            lm_score = torch.empty((U, K), dtype=torch.float32, device=dev)
            H.call('asr_rescore_rank_lm', H.ptr(att), H.ptr(first['ctc_score']), H.ptr(tok_logp), L, H.ptr(first['len']), H.ptr(first['n']),
                   U, K, L, self.ctc_w, float(self.lm_w), self.len_bonus, H.ptr(lm_score), H.ptr(total), H.ptr(order), st)
        phase('rescore_launch')
        n_c, len_c, tok_c = first['n'].cpu(), first['len'].cpu(), first['tokens'].cpu()
        cs_c, att_c, tot_c, ord_c = first['ctc_score'].cpu(), att.cpu(), total.cpu(), order.cpu()
        if self.lm_rescore:
            lm_c = lm_score.cpu()
        out = []
        for u in range(U):
            slots = [int(i) for i in ord_c[u, :int(n_c[u])]]
            out.append([CTCHypothesis(tok_c[u, i, :int(len_c[u, i])].tolist(), float(tot_c[u, i]), float(cs_c[u, i]), float(att_c[u, i]),
                                      None if lm_c is None else float(lm_c[u, i])) for i in slots])
        phase('read_back')
        return out[0] if U == 1 else out

    def _rescore_chunk_rows(self, L, Tp):
        """Hypothesis rows one decoder pass of L steps takes: at most RESCORE_MAX_ROWS, its saved state under RESCORE_STATE_BYTES,
        and no more than rescore_rows when the constructor gave one; never less than one row."""
        kn = getattr(self.asr.attention.att_layer, 'kernel_num', 1)
        rows = min(RESCORE_MAX_ROWS, max(1, RESCORE_STATE_BYTES // (4 * L * kn * Tp)))
        return rows if self.rescore_rows is None else max(1, min(rows, int(self.rescore_rows)))

    def _lm_pass(self, teacher, Lr, hyp_len, R, L):
        """The LM's log-probability of every token of every hypothesis -> tok_logp (R,L) fp32, 0 behind a hypothesis.
        asr_rescore_lm_input shifts the teacher table into the LM's input (<sos> in front), the LM's full-sequence forward - the
        training forward, only called here: it keeps what a backward pass would need while it runs - goes over chunks of rows in
        eval() with the model's precision, and asr_rescore_token_logp reduces each chunk's logits (rows, L, V) against the
        teacher table (int64, as asr_rescore_pack wrote it) and the first pass's len (int32, as it stands).  Training mode is
        restored afterwards."""
        lm, dev, st = self.lm, teacher.device, H.stream_ptr()
        V = self.asr.vocab_size
        lm_in = torch.empty((R, L), dtype=torch.int64, device=dev)
        H.call('asr_rescore_lm_input', H.ptr(teacher), Lr, R, L, SOS, H.ptr(lm_in), st)
        tok_logp = torch.empty((R, L), dtype=torch.float32, device=dev)
        rows = self._rescore_lm_chunk_rows(L)
        hyp_len = hyp_len.reshape(R)
        lm.prec = self.asr.prec
        was_training = lm.training
        lm.eval()
        try:
            with torch.no_grad():
                for r0 in range(0, R, rows):
                    r1 = min(R, r0 + rows)
                    logits = lm.forward(lm_in[r0:r1])[0]
                    if tuple(logits.shape) != (r1 - r0, L, V) or logits.dtype != torch.float32:
                        raise ValueError('lm_rescore: the LM\'s forward returned logits %s %s for tokens (%d, %d), not fp32 (%d, %d, %d)'
                                         % (tuple(logits.shape), logits.dtype, r1 - r0, L, r1 - r0, L, V))
                    logits = logits.contiguous()
                    H.call('asr_rescore_token_logp', H.ptr(logits), L * V, V, H.ptr(teacher[r0:r1]), Lr, H.ptr(hyp_len[r0:r1]), r1 - r0, L, V,
                           H.ptr(tok_logp[r0:r1]), L, st)
        finally:
            lm.train(was_training)
        return tok_logp

    def _rescore_lm_chunk_rows(self, L):
        """Hypothesis rows one LM pass of L positions takes: the logit block and the forward's transient state under
        RESCORE_STATE_BYTES, no more than lm_rescore_rows when the constructor gave one, never less than one row.  Per row and
        position, in fp32 words: the logits V, a layer's input max(emb_dim, dim), and what its recurrence holds at once - an LSTM
        layer its gates 4 dim, y and c (6 dim), a GRU layer gi 3 dim, y and the saved gates 4 dim (8 dim):
            bytes per row = 4 * L * (V + max(emb_dim, dim) + (6 | 8) * dim)
        A layer's tensors go as the next one runs (no graph is recorded under no_grad), so one layer's count stands for all."""
        lm, V = self.lm, self.asr.vocab_size
        dim = int(getattr(lm, 'dim', 0))
        emb = getattr(getattr(lm, 'emb', None), 'weight', None)
        emb_dim = int(emb.shape[1]) if emb is not None else dim
        per_row = 4 * max(1, int(L)) * (V + max(emb_dim, dim) + (8 if getattr(lm, 'module', 'LSTM') == 'GRU' else 6) * dim)
        rows = max(1, RESCORE_STATE_BYTES // per_row)
        return rows if self.lm_rescore_rows is None else max(1, min(rows, int(self.lm_rescore_rows)))

    @torch.no_grad()
    def forward_host(self, audio_feature, feature_len):
        """First implementation (score table on the host every step), shipped decoder only; kept as a cross-check."""
        if not self.fast:
            raise NotImplementedError('forward_host covers the shipped decoder only (LSTM, location-aware attention, one head); '
                                      'decode this model with forward')
        assert audio_feature.shape[0] == 1, 'Batchsize == 1 is required for beam search'
        asr, dev, st = self.asr, audio_feature.device, H.stream_ptr()
        prec = asr.prec
        flen = int(feature_len.reshape(-1)[0])
        max_len = int(math.ceil(flen * self.max_len_ratio))
        min_len = int(math.ceil(flen * self.min_len_ratio))
        ctx = ragged.eval_ctx(asr)
        enc, enc_len = asr.encoder(audio_feature.float(), feature_len.to(dev), ctx)
        enc = F_hip.to_f32(enc)
        Tp = enc.shape[1]
        nmax = self.beam_size
        L = max(max_len, 1)
        dec = F_hip.DecoderStepper(asr, enc.expand(nmax, Tp, enc.shape[2]).contiguous(),
                                   enc_len.to(dev, torch.int64).expand(nmax).contiguous(), L, prec)
        sd = dec.sd
        ctc_r = None
        if self.apply_ctc:
            ctc_lp = F_hip.CTCHeadFn.apply(asr._anchor, enc, asr.ctc_layer[0], prec, False, False)
            scorer = CTCPrefixScore(ctc_lp)
            ctc_r = scorer.init_state().unsqueeze(0).repeat(nmax, 1, 1).contiguous()
        lm_state = self.lm.init_state(nmax, dev) if self.apply_lm else None
        if self.apply_lm:
            self.lm.prec = prec
        V = asr.vocab_size
        hyps = [Hypothesis(0, [], [], 0.0)]
        finals = []
        for t in range(max_len):
            n = len(hyps)
            toks = torch.tensor([h.output_seq[-1] if h.output_seq else 0 for h in hyps], dtype=torch.int64)
            sd['tokens'][:n, t] = toks.to(dev)
            dec.step(t, live_rows=n)
            logits = sd['logits'][:n, t].contiguous()
            att_lp = torch.empty_like(logits)
            if self.apply_emb:
                self.emb_decoder.fuse_rows(sd['hs'][:n, t, -1, :], logits, out=att_lp)
            else:
                H.call('asr_log_softmax', H.ptr(logits), H.ptr(att_lp), n, V, st)
            att_cpu = att_lp.cpu()
            cur = att_cpu.clone()
            cands, psi_cpu, r_new = None, None, None
            if self.apply_ctc:
                _, cand = att_cpu.topk(self.ctc_beam_size, dim=-1)
                psi, r_new = scorer.score([len(h.output_seq) for h in hyps], [h.output_seq[-1] if h.output_seq else 0 for h in hyps],
                                          ctc_r[:n], cand)
                psi_cpu, cands = psi.cpu(), cand.tolist()
                for i, h in enumerate(hyps):
                    hack = torch.full((V,), LOG_ZERO)
                    hack[cand[i]] = psi_cpu[i] - float(h.ctc_prob)
                    cur[i] = (1 - self.ctc_w) * cur[i] + self.ctc_w * hack
                    cur[i, 0] = LOG_ZERO
            if self.apply_lm:
                lm_lp, lm_new = self.lm.step(toks.to(dev), self.lm.state_rows(lm_state, n))
                cur += self.lm_w * lm_lp.cpu()
            children = []
            for i, h in enumerate(hyps):
                h.row = i
                topv, topi = cur[i].topk(self.beam_size)
                final, new = h.addTopk(topi, topv, att_cpu[i], None if psi_cpu is None else psi_cpu[i], None if cands is None else cands[i])
                if final is not None and t >= min_len:
                    finals.append(final)
                    if self.beam_size == 1:
                        return finals
                children.extend(new)
            children.sort(key=lambda o: o.avgScore(), reverse=True)
            hyps = children[:self.beam_size]
            if not hyps:
                break
            # device state of the survivors: row i <- row parent(i) at step t
            par = torch.tensor([h.row for h in hyps], dtype=torch.int64, device=dev)
            m = len(hyps)
            for name in ('hs', 'cs', 'att'):
                sd[name][:m, t] = sd[name][par, t]
            if self.apply_ctc:
                ci = torch.tensor([h.ctc_idx for h in hyps], dtype=torch.int64, device=dev)
                ctc_r[:m] = r_new[par, ci]
            if self.apply_lm:
                lm_state = self.lm.gather_state(lm_new, par)
        finals += hyps
        finals.sort(key=lambda o: o.avgScore(), reverse=True)
        return finals[:self.beam_size]


class _FastStep(F_hip.DecoderStepper):
    """Decoder state and step of the shipped decoder on the decode kernels: every utterance's rows of enc `beam` times over."""

    def __init__(self, asr, enc, enc_len, beam, Lmax):
        U, Tp, E = enc.shape
        self.R = R = U * beam
        super().__init__(asr, enc.unsqueeze(1).expand(U, beam, Tp, E).reshape(R, Tp, E).contiguous(),
                         enc_len.unsqueeze(1).expand(U, beam).reshape(R).contiguous(), Lmax + 1, asr.prec)
        self.tokens = self.sd['tokens']
        self.tmp = {k: torch.empty_like(self.sd[k][:, 0]) for k in ('hs', 'cs', 'att')}

    def step(self, t):
        super().step(t)
        return self.sd['logits'][:, t].contiguous()

    def top_state(self, t):
        """(R,Dd) hidden state of the top layer at position t (what an embedding-fusing plugin reads)."""
        return self.sd['hs'][:, t, -1, :]

    def reorder(self, t, parent):
        R, st = self.R, H.stream_ptr()
        for name in ('hs', 'cs', 'att'):
            src = self.sd[name][:, t]
            width = src[0].numel()
            H.call('asr_gather_rows', H.ptr(src), H.ptr(parent), H.ptr(self.tmp[name]), R, width, src.stride(0), width, R, st)
            src.copy_(self.tmp[name])


class _BeamBook(object):
    """The bookkeeping of one output position that both searches share (reference src/decode.py:117-177): attention
    log-probs, CTC candidates and prefix scores, the LM step, asr_beam_step (fusion, top-k, <eos> rule, pruning, finals)
    and the re-ordering of the CTC / LM states; the finals are read out once the search has ended.  `tokens` (R, Lmax+1)
    int64 is the decoder's token table: asr_beam_step writes column t+1."""

    def __init__(self, bd, U, Lmax, min_lens, max_lens, ctc_lp, tlen, tokens):
        dev = tokens.device
        beam, V = bd.beam_size, bd.asr.vocab_size
        R = U * beam
        i32 = lambda *s_: torch.zeros(s_, dtype=torch.int32, device=dev)
        f32 = lambda *s_: torch.zeros(s_, dtype=torch.float32, device=dev)
        self.bd, self.U, self.beam, self.V, self.R, self.Lmax, self.tokens = bd, U, beam, V, R, Lmax, tokens
        self.Tp = ctc_lp.shape[1] if ctc_lp is not None else 0
        self.ctc_lp, self.tlen = ctc_lp, tlen
        self.C = bd.ctc_beam_size if bd.apply_ctc else 0
        self.ctc_r = self.ctc_rn = self.cand = self.psi = None
        st = H.stream_ptr()
        if bd.apply_ctc:
            C, Tp = self.C, self.Tp
            self.ctc_r, self.ctc_rn = f32(R, Tp, 2), f32(R, C, Tp, 2)
            self.cand, self.psi = i32(R, C), f32(R, C)
            H.call('asr_ctc_prefix_init_batched', H.ptr(ctc_lp), H.ptr(tlen), H.ptr(self.ctc_r), R, beam, Tp, V, st)
        self.lm_state = None
        if bd.apply_lm:
            bd.lm.prec = bd.asr.prec
            self.lm_state = bd.lm.init_state(R, dev)
        # hypothesis state, double buffered; row u*beam is the empty hypothesis of utterance u
        self.state = [{'alive': i32(R), 'sum': f32(R), 'ctcp': f32(R), 'len': i32(R), 'seq': i32(R, Lmax), 'sc': f32(R, Lmax)} for _ in range(2)]
        self.state[0]['alive'][::beam] = 1
        self.last_tok, self.parent = i32(R), torch.zeros(R, dtype=torch.int64, device=dev)
        self.ctc_index = torch.zeros(R, dtype=torch.int64, device=dev)
        self.min_len_d = torch.tensor(min_lens, dtype=torch.int32, device=dev)
        self.max_len_d = torch.tensor(max_lens, dtype=torch.int32, device=dev)
        self.done = i32(U)
        self.fin_n, self.fin_len, self.fin_avg = i32(U), i32(U, beam), f32(U, beam)
        self.fin_seq, self.fin_sc = i32(U, beam, Lmax + 1), f32(U, beam, Lmax + 1)
        self.att_lp = f32(R, V)
        # above the narrow kernels' vocabulary the row-per-workgroup forms do the same two steps; their shortlists live here
        self.wide = V > H.BEAM_NARROW_MAX_V
        self.wide_ws = None
        if self.wide:
            self.wide_ws = torch.zeros(H.lib().asr_beam_step_wide_workspace_bytes(U, beam), dtype=torch.uint8, device=dev)
        # the step's arguments: everything but the state pointers (swapped per step), lm_logp and t is set here, once
        self.args = args = H.BeamStep()
        for name, ten in (('att_logp', self.att_lp), ('psi', self.psi), ('candidates', self.cand), ('last_token', self.last_tok),
                          ('parent', self.parent), ('ctc_index', self.ctc_index), ('tokens', tokens), ('min_len', self.min_len_d),
                          ('max_len', self.max_len_d), ('done', self.done), ('fin_n', self.fin_n), ('fin_len', self.fin_len),
                          ('fin_avg', self.fin_avg), ('fin_seq', self.fin_seq), ('fin_score', self.fin_sc)):
            setattr(args, name, ten.data_ptr() if ten is not None else None)
        args.tokens_ld = tokens.shape[1]
        args.U, args.beam, args.V, args.C, args.Lmax = U, beam, V, self.C, Lmax
        args.ctc_weight = float(bd.ctc_w) if bd.apply_ctc else 0.0
        args.lm_weight = float(bd.lm_w) if bd.apply_lm else 0.0
        args.eos_threshold = 1.5

    def step(self, t, logits, top_state=None):
        """logits (R,V) of output position t -> parent (R) int64: the source row of every surviving row.  top_state (R,Dd): the
        decoder's top hidden state, given when an embedding-fusing plugin scores the step instead of log_softmax."""
        bd, R, V, C, Tp, st = self.bd, self.R, self.V, self.C, self.Tp, H.stream_ptr()
        a, b = self.state[t & 1], self.state[(t + 1) & 1]
        att_lp = self.att_lp
        if top_state is not None:
            bd.emb_decoder.fuse_rows(top_state, logits, out=att_lp)
        else:
            H.call('asr_log_softmax', H.ptr(logits), H.ptr(att_lp), R, V, st)
        if bd.apply_ctc:
            H.call('asr_beam_candidates_wide' if self.wide else 'asr_beam_candidates', H.ptr(att_lp), H.ptr(self.cand), R, V, C, st)
            H.call('asr_ctc_prefix_score_batched', H.ptr(self.ctc_lp), H.ptr(self.tlen), H.ptr(self.ctc_r), H.ptr(self.cand), H.ptr(a['len']),
                   H.ptr(self.last_tok), H.ptr(self.psi), H.ptr(self.ctc_rn), R, C, Tp, V, self.beam, st)
        lm_lp = lm_new = None
        if bd.apply_lm:
            lm_lp, lm_new = bd.lm.step(self.tokens[:, t].contiguous(), self.lm_state)
        args = self.args
        for key, name in (('alive', 'alive'), ('sum', 'sum'), ('ctcp', 'ctcp'), ('len', 'len'), ('seq', 'seq'), ('sc', 'score')):
            setattr(args, name + '_in', a[key].data_ptr())
            setattr(args, name + '_out', b[key].data_ptr())
        args.lm_logp = lm_lp.data_ptr() if lm_lp is not None else None
        args.t = t
        if self.wide:
            H.call('asr_beam_step_wide', ctypes.byref(args), H.ptr(self.wide_ws), self.wide_ws.numel(), st)
        else:
            H.call('asr_beam_step', ctypes.byref(args), st)
        if bd.apply_ctc:
            H.call('asr_gather_rows', H.ptr(self.ctc_rn), H.ptr(self.ctc_index), H.ptr(self.ctc_r), R, Tp * 2, Tp * 2, Tp * 2, R * C, st)
        if bd.apply_lm:
            self.lm_state = bd.lm.gather_state(lm_new, self.parent)
        return self.parent

    def all_done(self):
        return bool(self.done.all())

    def readout(self):
        n_c, len_c, seq_c, sc_c = self.fin_n.cpu(), self.fin_len.cpu(), self.fin_seq.cpu(), self.fin_sc.cpu()
        out = []
        for u in range(self.U):
            hyps = []
            for i in range(int(n_c[u])):
                l = int(len_c[u, i])
                hyps.append(Hypothesis(i, seq_c[u, i, :l].tolist(), sc_c[u, i, :l].tolist()))
            out.append(hyps)
        return out[0] if self.U == 1 else out
