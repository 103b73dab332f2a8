"""Length-aware batched encoder pass for decoding and alignment: the front-end and every BiLSTM layer run ONCE over a padded
batch of utterances of different lengths and compute what the unpadded pass of every utterance computes (to rounding: the GEMM
tiling and the recurrence plan follow the batch's B and T).  The recurrence launches are the training path's, unchanged;
what moves is the data (csrc/ragged.hip):

  0. front-end, when the encoder has one (vgg 1..7), once over the batch:
       conv extractors (vgg 1..5): the unpadded pass drops n % time_div trailing frames, so row b has n' = n - n % time_div valid
         frames, the batch runs at T = max n' and the features are masked at n'; src/vgg.forward_lens runs the conv stack with
         the tail of every convolution's activation zeroed in place (asr_ragged_zero_tail) - the zero padding in time the
         unpadded pass's next convolution reads at t = n' - and halves the lengths at each time pooling
       vgg 6 (every 4th frame) and vgg 7 (one Linear) work per frame: their own kernels on the masked features
  1..5. every BiLSTM layer through the training path's loop, src/functions.layer_forward with the lengths: input projection
     of the padded batch; asr_ragged_align (direction 0 of the gate pre-activations masked to the row's frames, direction 1
     RIGHT-ALIGNED, so the reverse walk starts from the zero state on the row's true last frame and meets only zeros after its
     first one); asr_lstm_fwd / asr_lstm16_fwd; asr_ragged_unalign (direction 1 of y shifted back, exact zeros past the row's
     length, the time down-sampling taken); [LayerNorm, fp32 storage only, per frame: after the down-sampling it sees the same
     rows] projection + tanh

Inference only (no autograd, no dropout).  Eligible: an encoder of LSTM layers behind any front-end the config accepts
(vgg = 0..7), any of LayerNorm / 'drop' / 'concat' / projection, either storage mode - per layer the one
src/module.RNNLayer.forward would take, per extractor the layout its forward would take.  GRU layers are not covered."""
import torch

from src import functions as F_hip
from src import hipabi as H


def eval_ctx(asr):
    """Stand-in for the per-forward context (src/asr.py:_RunCtx) where a layer runs outside ASR.forward, in evaluation."""
    return type('C', (), {'anchor': asr._anchor, 'prec': asr.prec, 'next_seed': lambda s: 0})()


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


def frontend_lengths(ext, n):
    """Length chain of one utterance of n frames through front-end `ext` (enc.layers[0] when it is no RNNLayer): (tlen,
    enc_len).  tlen = the frames the unpadded pass produces, enc_len = the length the module returns.  Conv extractors drop
    n % time_div frames and fold time_div into one: both n // time_div.  The down-sampler (vgg 6) keeps frames 0, 4, ..:
    ceil(n / 4) come out, it reports n // 4.  The feature embedding (vgg 7) is per frame."""
    from src.module import Downsampler
    from src.vgg import conv_time_div
    n = int(n)
    div = conv_time_div(ext)
    if div is not None:
        return n // div, n // div
    if isinstance(ext, Downsampler):
        return (n + ext.sample_rate - 1) // ext.sample_rate, n // ext.sample_rate
    return n, n


def _frontend(enc):
    from src.module import RNNLayer
    return None if isinstance(enc.layers[0], RNNLayer) else enc.layers[0]


def ineligible_reason(asr):
    """None when encode_batched covers this model's encoder, else why not (one phrase for create_msg)."""
    from src.module import RNNLayer
    enc = asr.encoder
    for m in list(enc.layers)[0 if _frontend(enc) is None else 1:]:
        if not isinstance(m, RNNLayer) or m.module != 'LSTM':
            return '%s encoder layer' % getattr(m, 'module', type(m).__name__)
    return None


def max_batch(asr):
    """Rows one pass takes: the bf16 recurrence holds B <= 16 * (8 / directions); fp32 storage has no such bound."""
    from src.module import RNNLayer
    if asr.prec != H.BF16 or not H.fast16_enabled():
        return 1 << 30
    return min(16 * (8 // m.nd) for m in asr.encoder.layers if isinstance(m, RNNLayer))


# Byte budget of the largest single activation of a conv front-end over one chunk of the batch.  asr_conv3x3_16 addresses
# its bf16 input image by 32-bit byte offsets that must stay below 2^31, one 2 K-byte read-ahead (K = 9 C <= 2304) included
# (csrc/gemm16.hip: gemm16_nt_plan), and every image a convolution reads is at most as large as the largest activation of
# the stack; 2^31 - 2^16 keeps them all addressable.  The fp32-operand path (asr_conv3x3: < 2^31 pixels) is inside the same
# bound.  At most five such tensors are alive at once (input, pre-activation, activation, pooled, pooling index).
FRONTEND_ACT_BYTES = (1 << 31) - (1 << 16)


def frontend_max_batch(asr, T):
    """Rows of T frames whose largest front-end activation stays under FRONTEND_ACT_BYTES (at least 1); unbounded without a
    conv extractor.  Sibling of max_batch: encode_batched takes the smaller of the two."""
    from src.vgg import conv_time_div, largest_activation_bytes
    ext = _frontend(asr.encoder)
    if ext is None or conv_time_div(ext) is None:
        return 1 << 30
    return max(1, FRONTEND_ACT_BYTES // largest_activation_bytes(ext, max(1, int(T)), asr.prec))


def masked_copy(x, lens):
    """Copy of x (B,T,D) with exact zeros at t >= lens[b]; the source rows there are never read."""
    x = x.contiguous()
    B, T, D = x.shape
    out = torch.empty_like(x)
    H.call('asr_ragged_unalign', H.ptr(x), T * D, 0, H.ptr(out), H.ptr(lens), B, T, 1, D, T, 1, 0, x.element_size(), H.stream_ptr())
    return out


def run_frontend(asr, ext, feat, flen):
    """Front-end `ext` once over feat (B,T,D), T == max(flen) -> (x (B,T',D') whose rows past a row's output length are never
    used, tlen list, enc_len list).  Raises ValueError before any launch when no row yields a frame."""
    from src.vgg import conv_time_div, forward_lens
    dev = feat.device
    chain = [frontend_lengths(ext, n) for n in flen]
    tl, el = [c[0] for c in chain], [c[1] for c in chain]
    div = conv_time_div(ext)
    if max(tl) == 0:
        raise ValueError('every utterance is shorter than the %d frames the front-end folds into one: no frame comes out' % (div or 1))
    if div is not None:
        # what the unpadded pass drops (n % time_div trailing frames) must not be seen: mask at n', run at T = max n'
        valid = [n - n % div for n in flen]
        x = masked_copy(feat[:, :max(valid)].float(), torch.tensor(valid, dtype=torch.int64, device=dev))
        x, out_lens = forward_lens(ext, x, valid, asr.prec)
        assert out_lens == tl
        return x, tl, el
    # per-frame front-ends on features whose padding is zeros of our own
    x = masked_copy(feat.float(), torch.tensor(flen, dtype=torch.int64, device=dev))
    ctx = eval_ctx(asr)
    x, _ = ext(x, torch.tensor(flen, dtype=torch.int64, device=dev), ctx)
    return x, tl, el


@torch.no_grad()
def encode_chunk(asr, feat, flen, with_ctc):
    """One pass over feat (B,T,D), T == max(flen) > 0, B <= max_batch(asr).  flen: list of ints.
    Returns (enc fp32 (B,T',E) with zero padding, tlen list, enc_len list, ctc (B,T',V) with zero padding or None).  A row
    that yields no frame (shorter than a conv front-end's time_div, or than a 'concat' rate) is allowed beside others."""
    from src.module import RNNLayer
    dev = feat.device
    enc_m = asr.encoder
    ext = _frontend(enc_m)
    H.begin_forward([m.dim for m in enc_m.layers if isinstance(m, RNNLayer)] or [320])
    if ext is None:
        # the caller's padding is not trusted: what the first projection reads there is zeros of our own
        x = masked_copy(feat.float(), torch.tensor(flen, dtype=torch.int64, device=dev))
        tl, el = list(flen), list(flen)
    else:
        x, tl, el = run_frontend(asr, ext, feat, flen)
    lens = torch.tensor(tl, dtype=torch.int64, device=dev)
    for layer in list(enc_m.layers)[0 if ext is None else 1:]:
        storage = F_hip.LayerBF16 if F_hip.rnn_fast_ok(layer, x, asr.prec) else F_hip.LayerF32      # as RNNLayer.forward chooses
        x = F_hip.layer_forward(storage(layer, asr.prec, x.shape), x, lens=lens)
        tl = [F_hip.out_frames(layer, n)[0] for n in tl]
        el = [e // layer.sample_rate if layer.sample_rate > 1 else e for e in el]
        lens = torch.tensor(tl, dtype=torch.int64, device=dev)
    enc = masked_copy(F_hip.to_f32(x), lens)
    ctc = None
    if with_ctc:
        ctc = masked_copy(F_hip.CTCHeadFn.apply(asr._anchor, enc, asr.ctc_layer[0], asr.prec, False, False), lens)
    return enc, tl, el, ctc
