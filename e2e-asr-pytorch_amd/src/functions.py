"""Autograd bookkeeping around the HIP kernels (libasr_hip.so).

Each torch.autograd.Function below covers one coarse stage of the reference graph and calls the C ABI
for all arithmetic.  Parameter gradients are accumulated by the kernels directly into the model's flat
gradient buffer (the views held in `param.grad`); the Functions therefore return gradients only for
activations.  `anchor` is a dummy requires-grad tensor that keeps autograd calling `backward` even when
the acoustic features themselves need no gradient.
"""
import contextlib
import ctypes
import weakref

import torch

from src import hipabi as H


def _empty(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


# --------------------------------------------------------------------------------------------------
# encoder RNN layer: input projection -> BiLSTM -> [LayerNorm] -> dropout -> time down-sampling -> tanh(Linear)
# (reference RNNLayer.forward, src/module.py:1040-1081).  Activations live in one of two storages, and a storage class owns every
# launch of the layer: LayerF32 (fp32 tensors, any LayerNorm / down-sampling style; also the LM's LSTM stack) and LayerBF16 (the
# encoder's working point in bf16 contraction mode: gate-minor bf16 gates, time-padded bf16 h, packed bf16 weights, batch-sliced
# persistent recurrence of csrc/lstm_persist3.hip).  One loop in each direction (layer_forward, layer_backward) walks the stages,
# for training (RNNLayerFn) and for inference over a padded batch (src/ragged.encode_chunk); rnn_fast_ok picks the storage.
# --------------------------------------------------------------------------------------------------
def out_frames(layer, T):
    """(T2, segs) of the layer's time down-sampling: 'drop' keeps ceil(T / rate) frames, 'concat' stacks T // rate groups of
    segs = rate frames side by side and drops the tail."""
    r = layer.sample_rate
    if r == 1:
        return T, 1
    return ((T + r - 1) // r, 1) if layer.sample_style == 'drop' else (T // r, r)


def _empty16(shape, like):
    return torch.empty(shape, dtype=torch.bfloat16, device=like.device)


def to_bf16(x):
    """fp32 -> bf16 copy through asr_cast_bf16 (bf16 tensors pass through)."""
    if x.dtype == torch.bfloat16:
        return x.contiguous()
    x = x.contiguous()
    out = _empty16(x.shape, x)
    H.call('asr_cast_bf16', H.ptr(x), H.ptr(out), x.numel(), H.stream_ptr())
    return out


def to_f32(x):
    if x.dtype == torch.float32:
        return x.contiguous()
    x = x.contiguous()
    out = _empty(x.shape, x)
    H.call('asr_cast_f32', H.ptr(x), H.ptr(out), x.numel(), 0, H.stream_ptr())
    return out


class CastF32Fn(torch.autograd.Function):
    """bf16 encoder output -> fp32 for the CTC head and the decoder; the gradient goes back as bf16."""
    @staticmethod
    def forward(ctx, x):
        return to_f32(x)

    @staticmethod
    def backward(ctx, g):
        return to_bf16(g)


def to_f32_fn(x):
    """Differentiable fp32 view of a layer input (no-op for fp32 tensors)."""
    return CastF32Fn.apply(x) if x.dtype == torch.bfloat16 else x


def fast16_layer_ok(layer, B, Din):
    """What the bf16 storage asks of a layer: LSTM cell, H % 16 == 0 <= 512, no LayerNorm, 'drop' down-sampling (or none),
    input width a multiple of 8, B <= 16 * (8 / directions)."""
    if layer.layer_norm or (layer.sample_rate > 1 and layer.sample_style != 'drop'):
        return False
    if Din % 8 != 0 or (layer.nd * layer.dim) % 8 != 0:
        return False
    return int(H.lib().asr_lstm16_workspace_bytes(B, layer.dim, layer.nd, 0)) > 0


def rnn_fast_ok(layer, x, prec):
    """LayerBF16 covers: bf16 contractions and the layers of fast16_layer_ok; everything else runs on LayerF32."""
    return prec == H.BF16 and H.fast16_enabled() and fast16_layer_ok(layer, x.shape[0], x.shape[2])


class _LayerStorage(object):
    """One layer at one input shape (B,T,Din): the shape arithmetic every stage shares, and the stages that differ between the
    storages only in the element size, in the `pad` zero frames around y and in the entry point's name."""

    def __init__(self, layer, prec, shape):
        self.layer, self.prec = layer, prec
        self.B, self.T, self.Din = shape
        self.Hd, self.ND = layer.dim, layer.nd
        self.G, self.D = self.ND * 4 * self.Hd, self.ND * self.Hd
        self.T2, self.segs = out_frames(layer, self.T)
        self.Dz = self.D * self.segs
        self.style = 0 if layer.sample_style == 'drop' else 1
        self.y_bstride, self.y_off = (self.T + 2 * self.pad) * self.D, self.pad * self.D       # frame 0 of y sits behind the leading pad

    def inputs(self, x):
        return self.cast(x)

    def align(self, raw, lens):
        """Direction 0 of the gate pre-activations masked to the row's frames, direction 1 right-aligned."""
        gates = torch.empty_like(raw)
        H.call('asr_ragged_align', H.ptr(raw), H.ptr(gates), H.ptr(lens), self.B, self.T, self.ND, 4 * self.Hd, self.esize, H.stream_ptr())
        return gates

    def unalign(self, y, lens):
        """Direction 1 of y shifted back, exact zeros past the row's length, the time down-sampling taken."""
        z = self.new((self.B, self.T2, self.Dz), y)
        H.call('asr_ragged_unalign', H.ptr(y), self.y_bstride, self.y_off, H.ptr(z), H.ptr(lens), self.B, self.T, self.ND, self.Hd, self.T2,
               self.layer.sample_rate, self.style, self.esize, H.stream_ptr())
        return z

    def act_bwd(self, dout, out):
        dpre = self.new((self.B * self.T2, self.Dz), out)
        H.call(self.act_bwd_entry, H.ptr(dout), H.ptr(out), H.ptr(dpre), dpre.numel(), H.ACT_TANH, H.stream_ptr())
        return dpre


class LayerF32(_LayerStorage):
    """fp32 tensors: gates (B,T,ND,4H), y (B,T,D); the contractions round their operands to `prec` when they stage them.  Never
    defers its parameter gradients and never runs its recurrence beside them: measured, the fp32 contractions beside the
    recurrence slow it and each other and the step gains nothing."""
    overlaps, esize, pad, act_bwd_entry = False, 4, 0, 'asr_act_bwd'
    new, cast = staticmethod(_empty), staticmethod(to_f32)

    def project(self, x):
        gates = _empty((self.B, self.T, self.ND, 4 * self.Hd), x)
        H.gemm(x, self.layer.w_ih_cat, gates, self.B * self.T, self.G, self.Din, self.Din, self.Din, self.G, 1, 1,
               bias=self.layer.b_ih_cat, prec=self.prec)
        return gates

    def _rec_workspace(self, gates):
        """A pool area for this one launch (it goes back to the pool once its abort word has been collected) and the
        arguments both recurrence entry points end with."""
        nbytes = H.lib().asr_lstm_workspace_bytes(self.B, self.Hd, self.ND)
        ws = H.handoff_acquire(nbytes, gates.device)
        return ws, (self.B, self.T, self.Hd, self.ND, self.prec, H.ptr(ws), nbytes, H.stream_ptr())

    def rec_fwd(self, gates, reserved=0):
        """`reserved` is not used: the fp32 recurrence kernels take no CU reservation."""
        layer = self.layer
        ws, tail = self._rec_workspace(gates)
        y, c = _empty((self.B, self.T, self.D), gates), _empty((self.B, self.T, self.ND, self.Hd), gates)
        H.call('asr_lstm_fwd', H.ptr(gates), H.ptr(layer.w_hh_cat), H.ptr(layer.b_hh_cat), H.ptr(y), H.ptr(c), *tail)
        H.watch_abort(ws, release=True)
        return y, c

    def rec_bwd(self, gates, dy, c, reserved=0, beside=False):
        """`gates` becomes the gradient wrt the gate pre-activations.  Always in line on the current stream (`reserved` and `beside`
        are LayerBF16's and not used here); what the layers above, the decoder and the CTC head deferred starts with it."""
        ws, tail = self._rec_workspace(gates)
        pre = torch.cuda.Event()
        pre.record(torch.cuda.current_stream())
        H.call('asr_lstm_bwd', H.ptr(gates), H.ptr(self.layer.w_hh_cat), H.ptr(dy), H.ptr(c), *tail)
        H.watch_abort(ws, release=True)
        H.flush_side(after=pre)

    def layer_norm(self, y, rows):
        ln = self.layer.ln
        yn, stats = torch.empty_like(y), _empty((rows, 2), y)
        H.call('asr_layernorm_fwd', H.ptr(y), H.ptr(ln.weight), H.ptr(ln.bias), H.ptr(yn), H.ptr(stats), rows, self.D, 1e-5, 0, H.stream_ptr())
        return yn, stats

    def layer_norm_bwd(self, dyn, y, stats):
        ln = self.layer.ln
        dy = torch.empty_like(y)
        H.call('asr_layernorm_bwd', H.ptr(dyn), H.ptr(y), H.ptr(ln.weight), H.ptr(ln.bias), H.ptr(stats), H.ptr(dy), H.ptr(ln.weight.grad),
               H.ptr(ln.bias.grad), self.B * self.T, self.D, 0, H.stream_ptr())
        return dy

    def downsample(self, yn, p, seed):
        """Dropout + time down-sampling; with neither, z IS yn and nothing is launched (in either direction)."""
        if self.layer.sample_rate == 1 and p == 0.0:
            return yn
        z = _empty((self.B, self.T2, self.Dz), yn)
        H.call('asr_dropout_downsample_fwd', H.ptr(yn), H.ptr(z), self.B, self.T, self.D, self.T2, self.layer.sample_rate, self.style, p, seed,
               H.stream_ptr())
        return z

    def downsample_bwd(self, dz, p, seed):
        if self.layer.sample_rate == 1 and p == 0.0:
            return dz
        dyn = _empty((self.B, self.T, self.D), dz)
        H.call('asr_dropout_downsample_bwd', H.ptr(dz), H.ptr(dyn), self.B, self.T, self.D, self.T2, self.layer.sample_rate, self.style, p, seed,
               H.stream_ptr())
        return dyn

    def out_proj(self, z):
        pj, rows = self.layer.pj, self.B * self.T2
        out = _empty((self.B, self.T2, self.Dz), z)
        H.linear_fwd(z.view(rows, self.Dz), pj.weight, pj.bias, out.view(rows, self.Dz), act=H.ACT_TANH, prec=self.prec)
        return out

    def pj_grads(self, dpre, z):
        pj = self.layer.pj
        H.linear_bwd(z.view(self.B * self.T2, self.Dz), pj.weight, dpre, pj.weight.grad, pj.bias.grad, None, prec=self.prec)

    def pj_input_grad(self, dpre):
        dz = _empty((self.B, self.T2, self.Dz), dpre)
        H.linear_bwd_input(self.layer.pj.weight, dpre, dz.view(self.B * self.T2, self.Dz), prec=self.prec)
        return dz

    def input_grad(self, gates):
        dx, rows = _empty((self.B, self.T, self.Din), gates), self.B * self.T
        H.gemm(gates.view(rows, self.G), self.layer.w_ih_cat, dx, rows, self.Din, self.G, self.G, self.Din, self.Din, 1, 0, prec=self.prec)
        return dx

    def weight_grads(self, gates, x, y):
        layer, rows, Hd, G, D, Din = self.layer, self.B * self.T, self.Hd, self.G, self.D, self.Din
        g2, x2, y2 = gates.view(rows, G), x.view(rows, Din), y.view(rows, D)
        H.gemm(g2, x2, layer.g_w_ih_cat, G, Din, rows, G, Din, Din, 0, 0, accum=1, splits=H.wgrad_splits(rows, G, Din), prec=self.prec)
        H.call('asr_colsum2', H.ptr(g2), G, rows, G, H.ptr(layer.g_b_ih_cat), H.ptr(layer.g_b_hh_cat), H.stream_ptr())
        splits_hh = H.wgrad_splits(rows, 4 * Hd, Hd)
        for d in range(self.ND):       # dW_hh = sum_t dgates_t^T h_{t -+ 1}: rows of y shifted one step against the direction's walk
            H.gemm(g2[:, d * 4 * Hd:], y2[:, d * Hd:], layer.g_w_hh_cat[d], 4 * Hd, Hd, rows, G, D, Hd, 0, 0,
                   accum=1, splits=splits_hh, seqT=self.T, bshift=(-1 if d == 0 else 1), prec=self.prec)


class LayerBF16(_LayerStorage):
    """bf16 tensors: gates gate-minor (B,T,ND,H,4), y time-padded (B,T+2,D) with zero rows 0 and T+1 (written by the recurrence
    kernel), contraction operands packed to bf16 (`packed`); c and the parameter gradients stay fp32.  No LayerNorm and no
    'concat' (fast16_layer_ok).  Its parameter gradients may be deferred to the side stream and its backward recurrence may run
    beside them on the complementary CU mask (layer_backward).  `pk`, the packed weights, is set by the first stage, `inputs`, and
    read by every contraction behind it, the backward's included."""
    overlaps, esize, pad, act_bwd_entry = True, 2, 1, 'asr_act_bwd16'
    new, cast = staticmethod(_empty16), staticmethod(to_bf16)

    @staticmethod
    def packed(layer, side=False):
        """bf16 operand copies of the layer's contraction weights, rebuilt from the fp32 master by ONE kernel per call."""
        Hd, ND = layer.dim, layer.nd
        G, Din, D = ND * 4 * Hd, layer.w_ih_cat.shape[1], ND * Hd
        dev = layer.w_ih_cat.device
        pk = layer.__dict__.get('_pack16')
        if pk is None or pk['wih'].device != dev:
            b16 = lambda *s_: torch.empty(s_, dtype=torch.bfloat16, device=dev)
            pk = {'wih': b16(G, Din), 'wihT': b16(Din, G), 'bias': torch.empty(G, dtype=torch.float32, device=dev),
                  'pj': b16(D, D) if layer.proj else None, 'pjT': b16(D, D) if layer.proj else None}
            layer.__dict__['_pack16'] = pk
        ev = layer.__dict__.pop('_pack16_ev', None)
        if ev is not None and not side:
            torch.cuda.current_stream().wait_event(ev)       # packed ahead on the side stream (prepack16) in this forward
            return pk
        H.call('asr_rnn_pack_weights', H.ptr(layer.w_ih_cat), H.ptr(layer.b_ih_cat), H.ptr(layer.b_hh_cat),
               H.ptr(layer.pj.weight) if layer.proj else None, H.ptr(pk['wih']), H.ptr(pk['wihT']), H.ptr(pk['bias']),
               H.ptr(pk['pj']), H.ptr(pk['pjT']), Hd, ND, Din, D, H.stream_ptr())
        return pk

    def inputs(self, x):
        x16 = self.cast(x)
        self.pk = self.packed(self.layer)       # kept with the storage object from forward to backward
        return x16

    def project(self, x16):
        gates = _empty16((self.B, self.T, self.ND, self.Hd, 4), x16)
        H.gemm16(x16, self.pk['wih'], gates, self.B * self.T, self.G, self.Din, self.Din, self.Din, self.G, 1, 1, bias=self.pk['bias'])
        return gates

    def _workspace(self, bwd):
        """Persistent, zero-initialised workspace of the recurrence per (layer, batch, pass) + its launch counter."""
        layer, key = self.layer, (self.B, bwd)
        cache = layer.__dict__.setdefault('_ws16_cache', {})
        dev = layer.w_hh_cat.device
        if key not in cache or cache[key][0].device != dev:
            n = int(H.lib().asr_lstm16_workspace_bytes(self.B, self.Hd, self.ND, bwd))
            ws = H.handoff_acquire(n, dev)                    # pool area: scrubbed from every XCD, never returned to the allocator
            weakref.finalize(layer, H.handoff_release, ws)    # the layer's areas go back to the POOL when the layer dies
            cache[key] = [ws, 0]
        ent = cache[key]
        ent[1] += 1
        return ent[0], ent[1]

    def _rec(self, bwd, gates, buf, c, reserved, beside):
        """One recurrence launch.  Owns the layer's persistent workspace and its abort words: two status blocks by launch parity
        (include/asr_hip.h), this launch reports in block epoch & 1 and clears the other one.  beside=True: launched on the
        CU-masked recurrence stream, and the deferred side-stream work is flushed to start with it."""
        ws, epoch = self._workspace(int(bwd))
        H.abort_guard(ws, ((epoch + 1) & 1) * 1024)
        pre = torch.cuda.Event() if beside else None
        if beside:
            pre.record(torch.cuda.current_stream())
        with (H.on_rec_stream() if beside else contextlib.nullcontext()):
            H.call('asr_lstm16_bwd' if bwd else 'asr_lstm16_fwd', H.ptr(gates), H.ptr(self.layer.w_hh_cat), H.ptr(buf), H.ptr(c),
                   self.B, self.T, self.Hd, self.ND, H.ptr(ws), ws.numel(), epoch, reserved, H.stream_ptr())
        if beside:
            H.flush_side(after=pre)       # the deferred gradients (layer above, this layer's projection) start with this recurrence
        H.watch_abort(ws, (epoch & 1) * 1024)

    def rec_fwd(self, gates, reserved=0):
        y, c = _empty16((self.B, self.T + 2 * self.pad, self.D), gates), _empty((self.B, self.T, self.ND, self.Hd), gates)
        self._rec(False, gates, y, c, reserved, False)
        return y, c

    def rec_bwd(self, gates, dy, c, reserved=0, beside=False):
        """`gates` becomes the gradient wrt the gate pre-activations (gate-minor)."""
        self._rec(True, gates, dy, c, reserved, beside)

    def downsample(self, y, p, seed):
        z = _empty16((self.B, self.T2, self.D), y)
        H.call('asr_dropout_downsample16_fwd', H.ptr(y), self.y_bstride, self.y_off, H.ptr(z), self.B, self.T, self.D, self.T2,
               self.layer.sample_rate, 0, p, seed, H.stream_ptr())
        return z

    def downsample_bwd(self, dz, p, seed):
        dy = _empty16((self.B, self.T, self.D), dz)
        H.call('asr_dropout_downsample16_bwd', H.ptr(dz), H.ptr(dy), self.B, self.T, self.D, self.T2, self.layer.sample_rate, 0, p, seed,
               H.stream_ptr())
        return dy

    def out_proj(self, z):
        D, out = self.D, _empty16((self.B, self.T2, self.D), z)
        H.gemm16(z, self.pk['pj'], out, self.B * self.T2, D, D, D, D, D, 1, 1, bias=self.layer.pj.bias, act=H.ACT_TANH)
        return out

    def pj_grads(self, dpre, z):
        pj, D, rows = self.layer.pj, self.D, self.B * self.T2
        H.gemm16(dpre, z, pj.weight.grad, D, D, rows, D, D, D, 0, 0, accum=1, splits=H.wgrad_splits(rows, D, D))
        H.call('asr_colsum16', H.ptr(dpre), D, rows, D, H.ptr(pj.bias.grad), None, 0, H.stream_ptr())

    def pj_input_grad(self, dpre):
        D, dz = self.D, _empty16((self.B, self.T2, self.D), dpre)
        H.gemm16(dpre, self.pk['pjT'], dz, self.B * self.T2, D, D, D, D, D, 1, 1)
        return dz

    def input_grad(self, gates):
        dx = _empty16((self.B, self.T, self.Din), gates)
        H.gemm16(gates, self.pk['wihT'], dx, self.B * self.T, self.Din, self.G, self.G, self.G, self.Din, 1, 1)
        return dx

    def weight_grads(self, gates, x16, y):
        """Parameter gradients in reference row order (perm_h undoes the gate-minor layout)."""
        layer, rows, Hd, G, D, Din = self.layer, self.B * self.T, self.Hd, self.G, self.D, self.Din
        H.gemm16(gates, x16, layer.g_w_ih_cat, G, Din, rows, G, Din, Din, 0, 0, accum=1, splits=H.wgrad_splits(rows, G, Din), perm_h=Hd)
        H.call('asr_colsum16', H.ptr(gates), G, rows, G, H.ptr(layer.g_b_ih_cat), H.ptr(layer.g_b_hh_cat), Hd, H.stream_ptr())
        splits_hh = H.wgrad_splits(rows, 4 * Hd, Hd)
        for d in range(self.ND):
            H.gemm16(gates, y, layer.g_w_hh_cat[d], 4 * Hd, Hd, rows, G, D, Hd, 0, 0, accum=1, splits=splits_hh,
                     perm_h=Hd, seqT=self.T, bshift=(-1 if d == 0 else 1), b_time_padded=1, a_off=d * 4 * Hd, b_off=d * Hd)


def layer_forward(s, x, train=False, seed=0, lens=None, save=None):
    """Forward of one layer on the storage object `s` (made for x's shape): x (B,T,Din), fp32 or bf16 -> (B,T2,Dz) in s's storage.

    save: a dict that receives what layer_backward reads (training).

    lens: inference over a padded batch - int64 (B) on the device, max(lens) == T, rows of x at t >= lens[b] arbitrary (never
    used).  Row b comes out as the unpadded pass of its lens[b] frames (to rounding): the gate pre-activations are aligned
    behind the projection (the reverse walk starts from the zero state on the row's true last frame), asr_ragged_unalign takes
    the place of dropout + down-sampling, and the LayerNorm, per frame, follows it over the B * T2 * segs frames that survive
    (a 'concat' row is `segs` frames side by side).  Rows past the layer's output length hold tanh(bias) when the layer projects,
    the LayerNorm bias behind a LayerNorm, else zeros: the NEXT align ignores them.  Nothing is kept."""
    layer = s.layer
    if lens is not None and s.T2 == 0:
        raise ValueError("every utterance is shorter than the 'concat' rate %d of an encoder layer: no frame comes out" % layer.sample_rate)
    x = s.inputs(x)
    gates = s.project(x)
    if lens is not None:
        gates = s.align(gates, lens)
    # training under data parallelism: 64 compute units stay with the all-reduce kernels
    reserved = 64 if (lens is None and layer.dp is not None and layer.dp.world > 1) else 0
    y, c = s.rec_fwd(gates, reserved)
    p, stats = float(layer.dropout) if train else 0.0, None
    if lens is not None:
        z = s.unalign(y, lens)
        if layer.layer_norm:
            z = s.layer_norm(z, s.B * s.T2 * s.segs)[0]
    else:
        yn = y
        if layer.layer_norm:
            yn, stats = s.layer_norm(y, s.B * s.T)
        z = s.downsample(yn, p, seed)
    out = s.out_proj(z) if layer.proj else z
    if save is not None:
        save.update(tensors=(x, gates, c, y, z, out) + (() if stats is None else (stats,)), p=p, seed=seed, reserved=reserved)
    return out


def layer_backward(s, tensors, kept, dout, need_dx, in_dtype):
    """dout (B,T2,Dz), the gradient of layer_forward's output, walked back through what it saved: returns the gradient of its
    input (None without need_dx; fp32 when the input came in as fp32, else in s's storage); the parameter gradients go into
    the layer's flat gradient views."""
    layer, dp = s.layer, s.layer.dp
    x, gates, c, y, z, out = tensors[:6]
    # Parameter gradients are off the critical path (only the optimizer reads them).  On a storage that `overlaps` they are
    # deferred to the CU-masked side stream and start together with the NEXT recurrence of the backward pass, which then runs on
    # the complementary CU mask (H.on_rec_stream: 8 * REC_UNITS compute units, the others reserved) - unless ASR_OVERLAP=0, or
    # under data parallelism without ASR_OVERLAP_DP=1.  A gradient bucket may be signalled only when everything that writes into
    # it has been issued: in line the signals stay where they were; deferred, they are deferred too, FIFO behind the work they
    # depend on, and fire on the side stream.  A storage that does not overlap first runs in line whatever the decoder and the
    # layers above deferred (H.join_side), since their buckets are signalled here.
    defer = s.overlaps and H.step_overlaps(dp)
    later = H.defer_side if defer else (lambda fn, *keep: fn())
    dout = s.cast(dout)
    if dp is not None:
        # every consumer of this layer's output has finished its backward: the buckets of the heads / decoder / upper layers can go
        if not s.overlaps:
            H.join_side()
        def earlier_buckets():
            for i in range(layer.bucket):
                dp.bucket_ready(i)
        later(earlier_buckets)
    if layer.proj:
        dpre = s.act_bwd(dout, out)
        later(lambda: s.pj_grads(dpre, z), dpre, z)
        dz = s.pj_input_grad(dpre)
    else:
        dz = dout
    dy = s.downsample_bwd(dz, kept['p'], kept['seed'])
    if layer.layer_norm:
        dy = s.layer_norm_bwd(dy, y, tensors[6])
    s.rec_bwd(gates, dy, c, 256 - 8 * H.REC_UNITS if defer else kept['reserved'], beside=defer)
    # gates now holds the gradient wrt the gate pre-activations; the input gradient continues the chain
    dx = None
    if need_dx:
        dx = s.input_grad(gates)
        if in_dtype == torch.float32:
            dx = to_f32(dx)
    later(lambda: s.weight_grads(gates, x, y), gates, x, y)
    if dp is not None:
        later(lambda: dp.bucket_ready(layer.bucket))
    return dx


class RNNLayerFn(torch.autograd.Function):
    """Training pass of one layer on the storage class `storage`: x fp32 for LayerF32, fp32 or bf16 for LayerBF16."""

    @staticmethod
    def forward(ctx, anchor, x, layer, train, seed, prec, storage):
        ctx.store, ctx.kept = storage(layer, prec, x.shape), {}
        ctx.need_dx, ctx.in_dtype = x.requires_grad, x.dtype
        out = layer_forward(ctx.store, x, train, seed, save=ctx.kept)
        ctx.save_for_backward(*ctx.kept.pop('tensors'))
        return out

    @staticmethod
    def backward(ctx, dout):
        dx = layer_backward(ctx.store, ctx.saved_tensors, ctx.kept, dout, ctx.need_dx, ctx.in_dtype)
        return None, dx, None, None, None, None, None


def prepack16(layers, B, prec):
    """The bf16 weight copies of the later encoder layers, made on the side stream beside the first layer's projection and
    recurrence instead of in front of their own (4 x 13 us of small launches on the step's critical path).  Called once per
    forward by the Encoder, before the first layer; a marker left behind by a forward that never reached its layer is
    dropped here."""
    for l in layers:
        l.__dict__.pop('_pack16_ev', None)
    dp = next((l.dp for l in layers if getattr(l, 'dp', None) is not None), None)
    # data parallel: no CU-masked stream beside RCCL's kernels until that has been run
    if not (H.step_overlaps(dp) and prec == H.BF16 and H.fast16_enabled() and torch.is_grad_enabled()):
        return
    todo = [l for l in layers[1:] if fast16_layer_ok(l, B, l.w_ih_cat.shape[1])]
    if not todo:
        return
    for l in todo:
        if l.__dict__.get('_pack16') is None:
            return                                        # first step: the copies are allocated on the layers' own stream
    with H.on_side_stream(None):
        for l in todo:
            LayerBF16.packed(l, side=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            l.__dict__['_pack16_ev'] = ev


# --------------------------------------------------------------------------------------------------
# CTC head: log_softmax(ReLU(Linear(enc)))   (src/asr.py:29-32,116-120)
# --------------------------------------------------------------------------------------------------
class CTCHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, enc, lin, prec, get_logit, defer):
        enc = enc.contiguous()
        B, T, E = enc.shape
        V = lin.weight.shape[0]
        act = _empty((B, T, V), enc)
        H.linear_fwd(enc.view(B * T, E), lin.weight, lin.bias, act.view(B * T, V), act=H.ACT_RELU, prec=prec)
        ctx.lin, ctx.prec, ctx.get_logit, ctx.defer = lin, prec, get_logit, defer
        if get_logit:
            ctx.save_for_backward(enc, act)
            return act
        logp = _empty((B, T, V), enc)
        H.call('asr_log_softmax', H.ptr(act), H.ptr(logp), B * T, V, H.stream_ptr())
        ctx.save_for_backward(enc, act, logp)
        return logp

    @staticmethod
    def backward(ctx, g):
        lin, prec = ctx.lin, ctx.prec
        g = g.contiguous()
        if ctx.get_logit:
            enc, act = ctx.saved_tensors
            B, T, E = enc.shape
            V = act.shape[-1]
            dpre = _empty((B * T, V), enc)
            H.call('asr_act_bwd', H.ptr(g), H.ptr(act), H.ptr(dpre), B * T * V, H.ACT_RELU, H.stream_ptr())
        else:
            enc, act, logp = ctx.saved_tensors
            B, T, E = enc.shape
            V = act.shape[-1]
            dpre = _empty((B * T, V), enc)
            H.call('asr_logsoftmax_relu_bwd', H.ptr(g), H.ptr(logp), H.ptr(act), H.ptr(dpre), B * T, V, H.stream_ptr())
        denc = _empty((B, T, E), enc)
        if ctx.defer:
            # input gradient now; the head's own gradients (a split reduction over B*T rows + a column sum) go to the side
            # stream beside the encoder's BPTT, like the decoder's (AttDecoderFn.backward)
            H.linear_bwd_input(lin.weight, dpre, denc.view(B * T, E), prec=prec)
            x2d = enc.view(B * T, E)
            H.defer_side(lambda: H.linear_bwd(x2d, lin.weight, dpre, lin.weight.grad, lin.bias.grad, None, prec=prec), x2d, dpre)
        else:
            H.linear_bwd(enc.view(B * T, E), lin.weight, dpre, lin.weight.grad, lin.bias.grad, denc.view(B * T, E), prec=prec)
        return None, denc, None, None, None, None


def scale_by_device_scalar(x, alpha):
    """x * alpha with alpha a one-element device tensor (the grad_output of a loss): asr_scale_dev."""
    x = x.contiguous()
    out = torch.empty_like(x)
    a = alpha.reshape(1).to(torch.float32).contiguous()
    H.call('asr_scale_dev', H.ptr(x), H.ptr(out), x.numel(), H.ptr(a), H.stream_ptr())
    return out


_LOSS_W = {}


def loss_weight(value, device):
    """A cached one-element device tensor holding a host constant (loss weights)."""
    key = (float(value), str(device))
    if key not in _LOSS_W:
        _LOSS_W[key] = torch.full((1,), float(value), dtype=torch.float32, device=device)
    return _LOSS_W[key]


class LossMixFn(torch.autograd.Function):
    """total = wa a + wb b (bin/train_asr.py:238,246) with the weights as one-element device tensors (under data parallelism the
    attention weight comes out of an all-reduce); forward and backward are the one-thread kernel asr_loss_mix."""

    @staticmethod
    def forward(ctx, a, wa, b, wb):
        out = torch.empty((), dtype=torch.float32, device=a.device)
        H.call('asr_loss_mix', H.ptr(a), H.ptr(wa), H.ptr(b), H.ptr(wb) if b is not None else None, H.ptr(out), H.stream_ptr())
        ctx.has_b = b is not None
        ctx.save_for_backward(wa, *( [wb] if b is not None else []))
        return out

    @staticmethod
    def backward(ctx, g):
        sv = ctx.saved_tensors
        g = g.reshape(1).to(torch.float32).contiguous()
        ga = torch.empty((), dtype=torch.float32, device=g.device)
        H.call('asr_loss_mix', H.ptr(g), H.ptr(sv[0]), None, None, H.ptr(ga), H.stream_ptr())
        gb = None
        if ctx.has_b:
            gb = torch.empty((), dtype=torch.float32, device=g.device)
            H.call('asr_loss_mix', H.ptr(g), H.ptr(sv[1]), None, None, H.ptr(gb), H.stream_ptr())
        return ga, None, gb, None


# --------------------------------------------------------------------------------------------------
# CTC loss (torch.nn.CTCLoss(blank=0, zero_infinity=False), bin/train_asr.py:135,237)
# --------------------------------------------------------------------------------------------------
class CTCLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp_btv, targets, input_len, target_len):
        logp = logp_btv.contiguous()
        B, T, V = logp.shape
        targets = targets.contiguous()
        L = targets.shape[1]
        if 2 * L + 1 > 1024:
            # the kernel holds the 2L+1 lattice states of an utterance in one workgroup; what counts is the longest TARGET, not
            # the padded width of the batch (one device read-back, on this rare path only)
            L = max(1, int(target_len.max()))
            targets = targets[:, :L].contiguous()
        dev = logp.device
        nll = torch.empty(B, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        grad = _empty((B, T, V), logp)
        nbytes = H.lib().asr_ctc_loss_workspace_bytes(B, T, L)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        # locals keep the converted tensors alive until the kernel has been enqueued on this stream
        targets = targets.to(dev, torch.int64)
        il = input_len.to(dev, torch.int64).contiguous()
        tl = target_len.to(dev, torch.int64).contiguous()
        H.call('asr_ctc_loss', H.ptr(logp), H.ptr(targets), H.ptr(il), H.ptr(tl), H.ptr(nll), H.ptr(loss), H.ptr(grad),
               B, T, V, L, 1.0, H.ptr(ws), nbytes, H.stream_ptr())
        ctx.save_for_backward(grad)
        ctx.nll = nll
        return loss

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        return scale_by_device_scalar(grad, gout), None, None, None


# --------------------------------------------------------------------------------------------------
# sequence loss on decoder logits (CrossEntropyLoss(ignore_index=0) / LabelSmoothingLoss)
# --------------------------------------------------------------------------------------------------
class SeqLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits_rv, target_r, mode, classes, smoothing):
        logits = logits_rv.contiguous()
        R, V = logits.shape
        tgt = target_r.to(logits_rv.device, torch.int64).contiguous()
        dev = logits.device
        dl = _empty((R, V), logits)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        acc = torch.empty(4, dtype=torch.float32, device=dev)
        H.call('asr_xent', H.ptr(logits), H.ptr(tgt), R, H.ptr(dl), H.ptr(loss), H.ptr(acc), 1, R, V, mode, classes,
               smoothing, 1.0, H.stream_ptr())
        ctx.save_for_backward(dl)
        return loss

    @staticmethod
    def backward(ctx, gout):
        (dl,) = ctx.saved_tensors
        return scale_by_device_scalar(dl, gout), None, None, None, None


# --------------------------------------------------------------------------------------------------
# attention decoder loop (src/asr.py:123-175)
# --------------------------------------------------------------------------------------------------
def _dec_dims(model, B, Tp, L):
    att, dec = model.attention, model.decoder
    d = H.DecDims()
    d.B, d.Tp, d.E = B, Tp, model.encoder.out_dim
    d.A, d.Q = att.dim, dec.dim * dec.layer
    d.Dd, d.NL, d.V = dec.dim, dec.layer, model.vocab_size
    d.Kn, d.Ks = att.att_layer.kernel_num, att.att_layer.kernel_size
    d.L = L
    d.temperature = float(att.att_layer.temperature)
    return d


def _dec_tensors(model, grads):
    att, dec, al = model.attention, model.decoder, model.attention.att_layer
    g = (lambda p: p.grad) if grads else (lambda p: p)
    nl = dec.layer
    return {
        'Wq': g(att.proj_q.weight), 'bq': g(att.proj_q.bias), 'Wk': g(att.proj_k.weight), 'bk': g(att.proj_k.bias),
        'Wconv': g(al.loc_conv.weight), 'Wproj': g(al.loc_proj.weight), 'wg': g(al.gen_energy.weight), 'bg': g(al.gen_energy.bias),
        'emb': g(model.pre_embed.weight),
        'Wih': [g(getattr(dec.layers, 'weight_ih_l%d' % l)) for l in range(nl)],
        'Whh': [g(getattr(dec.layers, 'weight_hh_l%d' % l)) for l in range(nl)],
        'bih': [g(getattr(dec.layers, 'bias_ih_l%d' % l)) for l in range(nl)],
        'bhh': [g(getattr(dec.layers, 'bias_hh_l%d' % l)) for l in range(nl)],
        'Wc': g(dec.char_trans.weight), 'bc': g(dec.char_trans.bias),
    }


def _dec_state(d, dev, save_conv=True, half_copies=False):
    """save_conv: keep the location-convolution output of every step (B,L,Kn,Tp) for the backward pass.
    half_copies: bf16 working copies of key and enc for the step kernels (bf16 contraction mode, E % 4 == 0)."""
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    h = lambda *s: torch.empty(s, dtype=torch.bfloat16, device=dev)
    return {
        'conv': f(d.B, d.L, d.Kn, d.Tp) if save_conv else None,
        'key16': h(d.B, d.Tp, d.A) if half_copies else None,
        'enc16': h(d.B, d.Tp, d.E) if half_copies else None,
        'key': f(d.B, d.Tp, d.A), 'att': f(d.B, d.L, d.Tp), 'q': f(d.B, d.L, d.A), 'xin': f(d.B, d.L, d.Dd + d.E),
        'gates': f(d.B, d.L, d.NL, 4 * d.Dd), 'cs': f(d.B, d.L, d.NL, d.Dd), 'hs': f(d.B, d.L, d.NL, d.Dd),
        'logits': f(d.B, d.L, d.V), 'energy': f(d.B, d.Tp),
        'tokens': torch.empty((d.B, d.L), dtype=torch.int64, device=dev),
    }


class DecoderStepper(object):
    """The per-step C-ABI calls over dims `d` and state dict `sd` (tokens zeroed); the key projection runs on construction.
    The caller writes sd['tokens'][:, t] and, for t > 0, the step t-1 rows of hs / cs / att, then calls step(t)."""

    def __init__(self, model, enc, enc_len, L, prec, save_conv=False):
        self.enc, self.enc_len, self.prec = enc, enc_len, prec
        self.d = _dec_dims(model, enc.shape[0], enc.shape[1], L)
        self.sd = _dec_state(self.d, enc.device, save_conv=save_conv, half_copies=False)
        self.sd['tokens'].zero_()
        self.w = H.dec_weights_struct(_dec_tensors(model, False), self.d.NL)
        self.s = H.dec_state_struct(self.sd)
        H.call('asr_att_decoder_keys', ctypes.byref(self.d), ctypes.byref(self.w), H.ptr(enc), H.ptr(self.sd['key']), prec, H.stream_ptr())

    def step(self, t, live_rows=None):
        self.d.B = self.enc.shape[0] if live_rows is None else live_rows
        H.call('asr_att_decoder_step', ctypes.byref(self.d), ctypes.byref(self.w), H.ptr(self.enc), H.ptr(self.enc_len),
               ctypes.byref(self.s), t, self.prec, H.stream_ptr())


def att_decoder_forward_sampled(model, enc, enc_len, L, teacher, prec, tf_rate, decisions=None):
    """Scheduled sampling (reference src/asr.py:145-158): after every step ONE uniform draw decides for the whole batch
    whether the next input token is the teacher's (probability tf_rate) or a sample from softmax(logits) of this step.
    The loop runs through the per-step C-ABI call; the token table records what was fed, so the backward pass (tokens
    are data) is the ordinary one.  decisions: optional list of booleans (True = teacher) replacing the host draws (tests)."""
    dec = DecoderStepper(model, enc, enc_len, L, prec, save_conv=True)
    d, st = dec.d, dec.sd
    teacher = teacher.contiguous()
    model._ss_counter = getattr(model, '_ss_counter', 0)
    st['tf_decisions'] = []
    for t in range(L):
        dec.step(t)
        if t + 1 < L:
            use_teacher = bool(decisions[t]) if decisions is not None else (tf_rate == 1 or torch.rand(1).item() <= tf_rate)
            st['tf_decisions'].append(use_teacher)
            if use_teacher:
                st['tokens'][:, t + 1] = teacher[:, t]
            else:
                model._ss_counter += 1
                seed = (model.seed * 7919 + model._ss_counter) & 0xFFFFFFFFFFFF
                H.call('asr_sample_tokens', H.ptr(st['logits'][:, t]), st['logits'].stride(0), H.ptr(st['tokens'][:, t + 1]),
                       st['tokens'].stride(0), d.B, d.V, seed, H.stream_ptr())
    return d, st


@torch.no_grad()
def att_decoder_forward_fused(model, enc, enc_len, L, prec, emb_decoder):
    """Greedy decoding through an embedding-fusing plugin (reference src/asr.py:167-172 with emb_decoder): every step runs the
    per-step C-ABI call, the plugin fuses the step's logits with its embedding distribution (asr_emb_fuse_fwd) and the kernel's
    argmax of the fused row is the next step's token.  Returns (dims, state, fused log-probs (B,L,V))."""
    dec = DecoderStepper(model, enc, enc_len, L, prec)
    d, st = dec.d, dec.sd
    fused = torch.empty((d.B, L, d.V), dtype=torch.float32, device=enc.device)
    scratch = torch.empty(d.B, dtype=torch.int64, device=enc.device)
    for t in range(L):
        dec.step(t)
        nxt, ld = (st['tokens'][:, t + 1], st['tokens'].stride(0)) if t + 1 < L else (scratch, 1)
        row = emb_decoder.fuse_rows(st['hs'][:, t, -1, :], st['logits'][:, t], argmax=nxt, argmax_ld=ld)
        fused[:, t].copy_(row)
    return d, st, fused


_DEC_WS = {}          # (kind, decoder dims, device) -> uint8 tensor; process-wide, LRU of 32 shapes per pass


def _dec_workspace(model, kind, key, nbytes, device):
    """Workspaces of the persistent decoder launches live for the whole PROCESS, one per (pass, decoder dimensions, shape):
    fixed address ranges instead of recycled allocator blocks.  On a recycled block an exchange granule of ANY earlier launch
    of the process can sit at a polled address with a matching 6-bit tag (4-bit launch epoch + step sequence); in an XCD's L2
    it survives the host memset, and the producers' own clear covers only clusters that land on the same XCD again.  With a
    fixed range and the per-range launch epoch of csrc/decoder_persist.hip (`next_epoch`) the only older tags a slot can hold are
    those of the previous launch on that range, whose epoch differs by one.  Keyed by shape, not by model: tests build and drop
    many models of the same shape, which is exactly the recycling this avoids.  Concurrent use by two models of the same shape
    cannot happen on one stream: a launch has finished with the range when the next one starts, except the backward's
    parameter half on the side stream - joined before the next backward is issued (src/step.py, engine callback)."""
    dd = _dec_dims(model, *key)
    k = (kind, tuple(getattr(dd, f) for f, _ in dd._fields_), str(device))
    ws = _DEC_WS.pop(k, None)
    if ws is not None and ws.numel() < nbytes:
        H.handoff_release(ws)
        ws = None
    if ws is None:
        while len(_DEC_WS) >= 64:                  # variable-length training: keep the 32 most recent shapes (x 2 passes)
            H.handoff_release(_DEC_WS.pop(next(iter(_DEC_WS))))      # evicted areas go back to the hand-off POOL, not to the allocator
        ws = H.handoff_acquire(nbytes, device)     # zeroed + scrubbed from every XCD whenever an area changes hands
    _DEC_WS[k] = ws                                # most recently used last
    return ws


def att_decoder_forward(model, enc, enc_len, L, teacher, prec):
    """Runs the decode loop; returns (dims, state dict)."""
    B, Tp, _ = enc.shape
    d = _dec_dims(model, B, Tp, L)
    st = _dec_state(d, enc.device, half_copies=(prec == H.BF16 and d.E % 4 == 0))
    if prec == H.BF16 and teacher is not None:
        nwork = int(H.lib().asr_att_decoder_fwd_work_bytes(ctypes.byref(d)))     # 0: no single-launch plan for this shape
        if nwork:
            st['work'] = _dec_workspace(model, 'fwd', (d.B, d.Tp, d.L), nwork, enc.device)
            H.abort_guard(st['work'])
    w = H.dec_weights_struct(_dec_tensors(model, False), d.NL)
    s = H.dec_state_struct(st)
    t_ptr, t_ld = (None, 0)
    if teacher is not None:
        teacher = teacher.contiguous()
        assert teacher.shape[1] >= L - 1
        t_ptr, t_ld = H.ptr(teacher), teacher.shape[1]
    H.call('asr_att_decoder_fwd', ctypes.byref(d), ctypes.byref(w), H.ptr(enc), H.ptr(enc_len), t_ptr, t_ld,
           ctypes.byref(s), prec, H.stream_ptr())
    H.watch_abort(st.get('work'))
    return d, st


class AttDecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, enc, enc_len, teacher, L, model, prec, tf_rate=1.0):
        enc = enc.contiguous()
        enc_len = enc_len.to(enc.device, torch.int64).contiguous()
        if teacher is not None and tf_rate != 1:
            d, st = att_decoder_forward_sampled(model, enc, enc_len, L, teacher, prec, tf_rate, getattr(model, '_tf_decisions', None))
            model._last_tokens = st['tokens']
        else:
            d, st = att_decoder_forward(model, enc, enc_len, L, teacher, prec)
        ctx.model, ctx.prec, ctx.d, ctx.st = model, prec, d, st
        ctx.save_for_backward(enc, enc_len)
        att_seq = st['att'].view(d.B, 1, d.L, d.Tp)
        ctx.mark_non_differentiable(att_seq)
        ctx.set_materialize_grads(False)         # an unused output arrives as None in backward, not as a tensor of zeros
        return st['logits'], att_seq, st['hs']

    @staticmethod
    def backward(ctx, dlogits, _datt, dhs):
        model, prec, d, st = ctx.model, ctx.prec, ctx.d, ctx.st
        enc, enc_len = ctx.saved_tensors
        dlogits = torch.zeros_like(st['logits']) if dlogits is None else dlogits.contiguous()
        # a gradient on the decoder states (the embedding regulariser reads the top layer's h_t, src/plugin.py): the top layer's
        # slice joins dh_top inside the call; without one this is asr_att_decoder_bwd_ex, launch for launch
        dhs_top = dhs[:, :, -1, :].contiguous() if dhs is not None else None
        denc = torch.zeros_like(enc)
        w = H.dec_weights_struct(_dec_tensors(model, False), d.NL)
        g = H.dec_weights_struct(_dec_tensors(model, True), d.NL)
        s = H.dec_state_struct(st)
        nbytes = H.lib().asr_att_decoder_bwd_workspace_bytes(ctypes.byref(d))
        ws = _dec_workspace(model, 'bwd', (d.B, d.Tp, d.L), nbytes, enc.device)
        model._last_dec_bwd_ws = ws          # kept for diagnostics (tools/diag_dec.py)
        persistent = int(H.lib().asr_att_decoder_bwd_persistent_tiles(ctypes.byref(d))) > 0
        status_off = int(H.lib().asr_att_decoder_bwd_status_offset(ctypes.byref(d))) if persistent else 0
        if persistent:
            H.abort_guard(ws, status_off)
        overlap = H.step_overlaps(getattr(model, '_dp', None))
        looped = ctypes.c_int(0)
        if dhs_top is None:
            H.call('asr_att_decoder_bwd_ex', ctypes.byref(d), ctypes.byref(w), ctypes.byref(g), H.ptr(enc), H.ptr(enc_len),
                   ctypes.byref(s), H.ptr(dlogits), H.ptr(denc), H.ptr(ws), nbytes, prec, 1 if overlap else 0, ctypes.byref(looped),
                   H.stream_ptr())
        else:
            H.call('asr_att_decoder_bwd_hs', ctypes.byref(d), ctypes.byref(w), ctypes.byref(g), H.ptr(enc), H.ptr(enc_len),
                   ctypes.byref(s), H.ptr(dlogits), H.ptr(dhs_top), H.ptr(denc), H.ptr(ws), nbytes, prec, 1 if overlap else 0,
                   ctypes.byref(looped), H.stream_ptr())
        if persistent:
            H.watch_abort(ws, status_off)
        if overlap:
            # the decoder's parameter gradients (15 launches, ~0.7 ms) are off the path to the encoder gradient: they run on the
            # CU-masked side stream beside the encoder's BPTT (issued at its first recurrence, layer_backward)
            keep = [t for t in st.values() if torch.is_tensor(t)]

            def param_grads():
                H.call('asr_att_decoder_bwd_params', ctypes.byref(d), ctypes.byref(w), ctypes.byref(g), H.ptr(enc), H.ptr(enc_len),
                       ctypes.byref(s), H.ptr(dlogits), H.ptr(ws), nbytes, looped.value, prec, H.stream_ptr())
            H.defer_side(param_grads, enc, enc_len, dlogits, ws, *keep)
        ctx.st = None
        return None, denc, None, None, None, None, None, None


# --------------------------------------------------------------------------------------------------
# RNN language model, training forward/backward (reference src/lm.py:27-38): embedding -> dropout -> LSTM stack -> dropout ->
# output projection.  The LSTM layers go through RNNLayerFn (one direction, dropout on each layer's output: nn.LSTM's
# inter-layer dropout plus the model's dp2 on the last layer).
# --------------------------------------------------------------------------------------------------
class EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, tokens, emb):
        tok = tokens.reshape(-1).contiguous()
        V, D = emb.weight.shape
        out = torch.empty((tok.numel(), D), dtype=torch.float32, device=tok.device)
        H.call('asr_gather_rows', H.ptr(emb.weight), H.ptr(tok), H.ptr(out), tok.numel(), D, D, D, V, H.stream_ptr())
        ctx.emb = emb
        ctx.save_for_backward(tok)
        return out.view(*tokens.shape, D)

    @staticmethod
    def backward(ctx, dout):
        (tok,) = ctx.saved_tensors
        emb = ctx.emb
        V, D = emb.weight.shape
        dout = dout.contiguous().view(-1, D)
        H.call('asr_embedding_bwd', H.ptr(dout), D, H.ptr(tok), H.ptr(emb.weight.grad), tok.numel(), D, V, H.stream_ptr())
        return None, None, None


class DropoutFn(torch.autograd.Function):
    """nn.Dropout on a (B,T,D) tensor with the counter-based generator of the encoder layers (mask = f(seed, index))."""

    @staticmethod
    def forward(ctx, x, p, seed):
        x = x.contiguous()
        B, T, D = x.shape
        z = torch.empty_like(x)
        H.call('asr_dropout_downsample_fwd', H.ptr(x), H.ptr(z), B, T, D, T, 1, 0, float(p), int(seed), H.stream_ptr())
        ctx.meta = (B, T, D, float(p), int(seed))
        return z

    @staticmethod
    def backward(ctx, dz):
        B, T, D, p, seed = ctx.meta
        dz = dz.contiguous()
        dx = torch.empty_like(dz)
        H.call('asr_dropout_downsample_bwd', H.ptr(dz), H.ptr(dx), B, T, D, T, 1, 0, p, seed, H.stream_ptr())
        return dx, None, None


class LinearFn(torch.autograd.Function):
    """y = x W^T + b with the parameter gradients accumulated into W.grad / b.grad (flat storage); b may be None."""

    @staticmethod
    def forward(ctx, anchor, x, weight, bias, prec):
        x = x.contiguous()
        K = x.shape[-1]
        x2 = x.view(-1, K)
        N = weight.shape[0]
        out = torch.empty((x2.shape[0], N), dtype=torch.float32, device=x.device)
        H.linear_fwd(x2, weight, bias, out, prec=prec)
        ctx.weight, ctx.bias, ctx.prec = weight, bias, prec
        ctx.need_dx = x.requires_grad
        ctx.save_for_backward(x2)
        return out.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dout):
        (x2,) = ctx.saved_tensors
        weight, bias, prec = ctx.weight, ctx.bias, ctx.prec
        N = weight.shape[0]
        dy = dout.contiguous().view(-1, N)
        dx = torch.empty_like(x2) if ctx.need_dx else None
        H.linear_bwd(x2, weight, dy, weight.grad, bias.grad if bias is not None else None, dx, prec=prec)
        return None, (dx.view(*dout.shape[:-1], x2.shape[1]) if dx is not None else None), None, None, None
