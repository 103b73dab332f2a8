"""Length-aware batched encoder pass for decoding and alignment: every BiLSTM layer runs ONCE over a padded batch of
utterances of different lengths and computes what the unpadded pass of every utterance computes (to rounding: the GEMM
tiling and the recurrence plan follow the batch's B and T).  The recurrence launches are the training path's, unchanged;
what moves is the data (csrc/ragged.hip):

  1. input projection of the padded batch, as in src/functions.py
  2. asr_ragged_align: direction 0 of the gate pre-activations masked to the row's frames, direction 1 RIGHT-ALIGNED, so the
     reverse walk starts from the zero state on the row's true last frame and meets only zeros after its first one
  3. asr_lstm_fwd / asr_lstm16_fwd
  4. asr_ragged_unalign: direction 1 of y shifted back, exact zeros past the row's length, the time down-sampling taken
  5. [LayerNorm, fp32 storage only, per frame: after the down-sampling it sees the same rows] projection + tanh

Inference only (no autograd, no dropout).  Eligible: an encoder of LSTM layers without a front-end (vgg = 0), any of
LayerNorm / 'drop' / 'concat' / projection, either storage mode - per layer the one src/module.RNNLayer.forward would take."""
import torch

from src import functions as F_hip
from src import hipabi as H


def group_consecutive(items, n):
    """Yields lists of n consecutive items of any iterable: order kept, the last group short."""
    n = max(1, int(n))
    group = []
    for item in items:
        group.append(item)
        if len(group) == n:
            yield group
            group = []
    if group:
        yield group


def ragged_lengths(n, rates, style):
    """Length chain of one utterance of n frames through layers with down-sampling `rates`: (tlen, enc_len).  tlen = the
    frames the unpadded pass produces ('drop' keeps ceil(n/r), 'concat' stacks n // r groups and drops the tail) - the next
    layer runs over all of them; enc_len = the reference's `len // r` chain (src/module.RNNLayer.forward)."""
    tlen, enc_len = int(n), int(n)
    for r in rates:
        if r > 1:
            tlen = (tlen + r - 1) // r if style == 'drop' else tlen // r
            enc_len = enc_len // r
    return tlen, enc_len


def ineligible_reason(asr):
    """None when encode_batched covers this model's encoder, else why not (one phrase for create_msg)."""
    from src.module import RNNLayer
    enc = asr.encoder
    if enc.vgg != 0:
        return 'front-end vgg = %d' % enc.vgg
    for m in enc.layers:
        if not isinstance(m, RNNLayer) or m.module != 'LSTM':
            return '%s encoder layer' % getattr(m, 'module', type(m).__name__)
    return None


def max_batch(asr):
    """Rows one pass takes: the bf16 recurrence holds B <= 16 * (8 / directions); fp32 storage has no such bound."""
    if asr.prec != H.BF16 or not H.fast16_enabled():
        return 1 << 30
    return min(16 * (8 // m.nd) for m in asr.encoder.layers)


def _unalign(y, bstride, off, z, lens, B, T, layer, T2, esize):
    style = 0 if layer.sample_style == 'drop' else 1
    H.call('asr_ragged_unalign', H.ptr(y), bstride, off, H.ptr(z), H.ptr(lens), B, T, layer.nd, layer.dim, T2, layer.sample_rate, style,
           esize, H.stream_ptr())


def ragged_layer(layer, x, lens, prec):
    """One encoder layer over the padded batch x (B,T,Din), fp32 or bf16, rows at t >= lens[b] arbitrary (never used).
    lens int64 (B) on the device, max(lens) == T.  Returns (B,T2,Dz) in the storage mode RNNLayer.forward would choose; its
    rows past the layer's output length hold tanh(bias) when the layer projects (the NEXT align ignores them), else zeros."""
    B, T, Din = x.shape
    Hd, ND = layer.dim, layer.nd
    G, D = ND * 4 * Hd, ND * Hd
    T2, segs = F_hip.out_frames(layer, T)
    Dz = D * segs
    st = H.stream_ptr()
    if T2 == 0:
        raise ValueError("every utterance is shorter than the 'concat' rate %d of an encoder layer: no frame comes out" % layer.sample_rate)
    if F_hip.rnn_fast_ok(layer, x, prec):
        x16 = F_hip.to_bf16(x)
        pk = F_hip._packed16(layer)
        raw = F_hip._empty16((B, T, ND, Hd, 4), x16)
        H.gemm16(x16, pk['wih'], raw, B * T, G, Din, Din, Din, G, 1, 1, bias=pk['bias'])
        gates = torch.empty_like(raw)
        H.call('asr_ragged_align', H.ptr(raw), H.ptr(gates), H.ptr(lens), B, T, ND, 4 * Hd, 2, st)
        y, _c = F_hip.lstm16_rec(layer, gates, B, T, 0)
        z = F_hip._empty16((B, T2, Dz), x16)
        _unalign(y, (T + 2) * D, D, z, lens, B, T, layer, T2, 2)
        if not layer.proj:
            return z
        out = F_hip._empty16((B, T2, Dz), x16)
        H.gemm16(z, pk['pj'], out, B * T2, D, D, D, D, D, 1, 1, bias=layer.pj.bias, act=H.ACT_TANH)
        return out
    x = F_hip.to_f32(x)
    raw = F_hip._empty((B, T, ND, 4 * Hd), x)
    H.gemm(x, layer.w_ih_cat, raw, B * T, G, Din, Din, Din, G, 1, 1, bias=layer.b_ih_cat, prec=prec)
    gates = torch.empty_like(raw)
    H.call('asr_ragged_align', H.ptr(raw), H.ptr(gates), H.ptr(lens), B, T, ND, 4 * Hd, 4, st)
    y, _c = F_hip.lstm_rec(layer, gates, B, T, prec)
    z = F_hip._empty((B, T2, Dz), x)
    _unalign(y, T * D, 0, z, lens, B, T, layer, T2, 4)
    if layer.layer_norm:
        # per frame, so the frames that survive the down-sampling are normalised as the unpadded pass normalises them;
        # a 'concat' row is `segs` frames side by side.  Padding rows become the LayerNorm bias: masked by the next align
        zn, stats = torch.empty_like(z), F_hip._empty((B * T2 * segs, 2), x)
        H.call('asr_layernorm_fwd', H.ptr(z), H.ptr(layer.ln.weight), H.ptr(layer.ln.bias), H.ptr(zn), H.ptr(stats), B * T2 * segs, D, 1e-5, 0, st)
        z = zn
    if not layer.proj:
        return z
    out = F_hip._empty((B, T2, Dz), x)
    H.linear_fwd(z.view(B * T2, Dz), layer.pj.weight, layer.pj.bias, out.view(B * T2, Dz), act=H.ACT_TANH, prec=prec)
    return out


def masked_copy(x, lens):
    """Copy of x (B,T,D) with exact zeros at t >= lens[b]; the source rows there are never read."""
    x = x.contiguous()
    B, T, D = x.shape
    out = torch.empty_like(x)
    H.call('asr_ragged_unalign', H.ptr(x), T * D, 0, H.ptr(out), H.ptr(lens), B, T, 1, D, T, 1, 0, x.element_size(), H.stream_ptr())
    return out


@torch.no_grad()
def encode_chunk(asr, feat, flen, with_ctc):
    """One pass over feat (B,T,D), T == max(flen) > 0, B <= max_batch(asr).  flen: list of ints.
    Returns (enc fp32 (B,T',E) with zero padding, tlen list, enc_len list, ctc (B,T',V) with zero padding or None)."""
    from src.module import RNNLayer
    dev = feat.device
    enc_m = asr.encoder
    H.begin_forward()
    H.configure_rec_units([m.dim for m in enc_m.layers if isinstance(m, RNNLayer)] or [320])
    lens = torch.tensor(flen, dtype=torch.int64, device=dev)
    # the caller's padding is not trusted: what the first projection reads there is zeros of our own
    x = masked_copy(feat.float(), lens)
    tl, el = list(flen), list(flen)
    for layer in enc_m.layers:
        x = ragged_layer(layer, x, lens, asr.prec)
        tl = [F_hip.out_frames(layer, n)[0] for n in tl]
        el = [e // layer.sample_rate if layer.sample_rate > 1 else e for e in el]
        lens = torch.tensor(tl, dtype=torch.int64, device=dev)
    enc = masked_copy(F_hip.to_f32(x), lens)
    ctc = None
    if with_ctc:
        ctc = masked_copy(F_hip.CTCHeadFn.apply(asr._anchor, enc, asr.ctc_layer[0], asr.prec, False), lens)
    return enc, tl, el, ctc
