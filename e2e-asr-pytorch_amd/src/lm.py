"""RNN language model for shallow fusion (reference src/lm.py:5-38): parameter container with the same names
(`emb`, `rnn.weight_ih_l*`, `trans`) and a one-token `step` batched over hypotheses on the HIP path.  module 'LSTM' runs the
encoder-layer LSTM kernels; module 'GRU' runs the single-direction GRU recurrence of csrc/gru_rec.hip (GRULayerFn)."""
import torch
import torch.nn as nn

from src import hipabi as H
from src.module import LSTMParams
from src.variants import RNNParams

GRU_MAX_DIM = 2048          # asr_gru_rec_fwd / _bwd refuse a larger hidden size (include/asr_hip.h)


class _LayerView(object):
    """What RNNLayerFn reads of an encoder layer, for one LM layer (views into the flat buffers)."""


class GRULayerFn(torch.autograd.Function):
    """One nn.GRU layer of the LM over a whole (B,T,Din) sequence from the zero state.  Forward: gi = x W_ih^T + b_ih (asr_gemm),
    then asr_gru_rec_fwd.  Backward: asr_gru_rec_bwd, then the parameter gradients as GRUSeqFn.backward forms them (src/variants.py),
    accumulated into the flat gradient views of `layer`."""

    @staticmethod
    def forward(ctx, anchor, x, layer, prec):
        x = x.contiguous()
        B, T, Din = x.shape
        Hd = layer.dim
        G = 3 * Hd
        gi = torch.empty((B, T, G), dtype=torch.float32, device=x.device)
        H.gemm(x, layer.w_ih, gi, B * T, G, Din, Din, Din, G, 1, 1, bias=layer.b_ih, prec=prec)
        y = torch.empty((B, T, Hd), dtype=torch.float32, device=x.device)
        saved = torch.empty((B, T, 4 * Hd), dtype=torch.float32, device=x.device)
        H.call('asr_gru_rec_fwd', H.ptr(gi), H.ptr(layer.w_hh), H.ptr(layer.b_hh), None, B, T, Hd, prec, H.ptr(y), H.ptr(saved),
               H.stream_ptr())
        ctx.layer, ctx.prec = layer, prec
        ctx.need_dx = x.requires_grad
        ctx.save_for_backward(x, y, saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        layer, prec = ctx.layer, ctx.prec
        x, y, saved = ctx.saved_tensors
        B, T, Din = x.shape
        Hd = layer.dim
        G = 3 * Hd
        st = H.stream_ptr()
        dgi = torch.empty((B * T, G), dtype=torch.float32, device=x.device)
        dgh = torch.empty_like(dgi)
        nbytes = H.lib().asr_gru_rec_workspace_bytes(B, Hd)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        H.call('asr_gru_rec_bwd', H.ptr(dy.contiguous()), H.ptr(y), H.ptr(saved), None, H.ptr(layer.w_hh), B, T, Hd, prec,
               H.ptr(dgi), H.ptr(dgh), None, H.ptr(ws), nbytes, st)
        x2, y2 = x.view(B * T, Din), y.view(B * T, Hd)
        H.gemm(dgi, x2, layer.g_w_ih, G, Din, B * T, G, Din, Din, 0, 0, accum=1, splits=H.wgrad_splits(B * T, G, Din), prec=prec)
        H.call('asr_colsum', H.ptr(dgi), G, B * T, G, H.ptr(layer.g_b_ih), st)
        H.call('asr_colsum', H.ptr(dgh), G, B * T, G, H.ptr(layer.g_b_hh), st)
        # dW_hh = sum_t dgh_t^T h_{t-1}: rows of y shifted one step back in time, zero at t = 0
        H.gemm(dgh, y2, layer.g_w_hh, G, Hd, B * T, G, Hd, Hd, 0, 0, accum=1, splits=H.wgrad_splits(B * T, G, Hd), seqT=T, bshift=-1,
               prec=prec)
        dx = None
        if ctx.need_dx:
            dx = torch.empty((B, T, Din), dtype=torch.float32, device=x.device)
            H.gemm(dgi, layer.w_ih, dx, B * T, Din, G, G, Din, Din, 1, 0, prec=prec)
        return None, dx, None, None


class RNNLM(nn.Module):
    def __init__(self, vocab_size, emb_tying, emb_dim, module, dim, n_layers, dropout):
        super().__init__()
        self.module = module.upper()
        if self.module not in ('LSTM', 'GRU'):
            raise NotImplementedError('HIP path implements the LSTM and GRU language models, not %r' % module)
        if self.module == 'GRU' and not 1 <= dim <= GRU_MAX_DIM:
            raise NotImplementedError('GRU language model: dim %d outside 1..%d (asr_gru_rec_fwd)' % (dim, GRU_MAX_DIM))
        self.dim, self.n_layers, self.emb_tying, self.vocab_size = dim, n_layers, emb_tying, vocab_size
        self.dropout = float(dropout)
        if emb_tying:
            assert emb_dim == dim, 'Output dim of RNN should be identical to embedding if using weight tying.'
        elif emb_dim != dim:
            # the reference builds trans = nn.Linear(emb_dim, vocab) and feeds it the RNN's outputs of width dim (src/lm.py:20,37):
            # its first forward raises.  Here the contraction would take K = dim from its input and the row stride emb_dim from
            # trans.weight, and return numbers (emb_dim > dim) or read past the weight's rows (emb_dim < dim).
            raise NotImplementedError('untied language model with emb_dim %d != dim %d: the reference applies trans = nn.Linear(emb_dim, '
                                      'vocab) to outputs of width dim and fails at its first forward' % (emb_dim, dim))
        self.emb = nn.Embedding(vocab_size, emb_dim)
        if self.module == 'LSTM':
            self.rnn = LSTMParams(emb_dim, dim, False, num_layers=n_layers)
        else:
            self.rnn = RNNParams('GRU', emb_dim, dim, False, num_layers=n_layers)
        if not emb_tying:
            self.trans = nn.Linear(emb_dim, vocab_size)
        self.prec = H.BF16
        # nn.LSTM's / nn.GRU's default initialisation (the reference's RNNLM keeps PyTorch's defaults, src/lm.py:14-21): U(-1/sqrt(dim),
        # 1/sqrt(dim)); LSTMParams / RNNParams allocate with torch.empty, so without this an untrained LM would run on uninitialised memory
        k = 1.0 / (dim ** 0.5)
        for p_ in self.rnn.parameters():
            nn.init.uniform_(p_, -k, k)

    # ---- training / full-sequence forward (reference src/lm.py:27-38) ------------------------------------------------
    def flatten(self):
        """All parameters in ONE flat fp32 buffer, gradients in another (what the fused optimizer kernels and the encoder-layer
        functions expect); per-layer adaptors expose the views RNNLayerFn reads."""
        params = list(self.parameters())
        dev = params[0].device
        ALIGN = 64
        offs, off = {}, 0
        for p in params:
            off = (off + ALIGN - 1) // ALIGN * ALIGN
            offs[id(p)] = off
            off += p.numel()
        total = (off + ALIGN - 1) // ALIGN * ALIGN
        flat = torch.zeros(total, dtype=torch.float32, device=dev)
        grad = torch.zeros(total, dtype=torch.float32, device=dev)
        for p in params:
            o, n = offs[id(p)], p.numel()
            flat[o:o + n].copy_(p.data.reshape(-1))
            p.data = flat[o:o + n].view(p.shape)
            p.grad = grad[o:o + n].view(p.shape)
            p._asr_flat = (flat, grad, offs)
        self.flat_param, self.flat_grad = flat, grad
        self._anchor = torch.zeros(1, dtype=torch.float32, device=dev, requires_grad=True)
        self._layers = []
        for l in range(self.n_layers):
            wih, whh = getattr(self.rnn, 'weight_ih_l%d' % l), getattr(self.rnn, 'weight_hh_l%d' % l)
            bih, bhh = getattr(self.rnn, 'bias_ih_l%d' % l), getattr(self.rnn, 'bias_hh_l%d' % l)
            a = _LayerView()
            if self.module == 'GRU':
                # what GRULayerFn reads: the layer's parameters and their gradients, views into the flat buffers
                a.dim = self.dim
                a.w_ih, a.w_hh, a.b_ih, a.b_hh = wih.data, whh.data, bih.data, bhh.data
                a.g_w_ih, a.g_w_hh, a.g_b_ih, a.g_b_hh = wih.grad, whh.grad, bih.grad, bhh.grad
                self._layers.append(a)
                continue
            a.dim, a.nd, a.dropout, a.layer_norm, a.sample_rate, a.sample_style, a.proj = self.dim, 1, self.dropout, False, 1, 'drop', False
            a.w_ih_cat, a.w_hh_cat, a.b_ih_cat, a.b_hh_cat = wih.data, whh.data.view(1, 4 * self.dim, self.dim), bih.data, bhh.data
            a.g_w_ih_cat, a.g_w_hh_cat, a.g_b_ih_cat, a.g_b_hh_cat = wih.grad, whh.grad.view(1, 4 * self.dim, self.dim), bih.grad, bhh.grad
            a.dp, a.bucket = None, None
            self._layers.append(a)
        self._flat_dev = dev

    def _apply(self, fn, *a, **kw):
        r = super()._apply(fn, *a, **kw)
        self.__dict__.pop('_layers', None)           # moved / cast: the flat views are rebuilt on first use
        return r

    def forward(self, x, lens=None, hidden=None):
        """x (B,T) int64 tokens -> (logits (B,T,V), None).  The reference packs by `lens`; one direction only, so the outputs
        at valid positions do not depend on the padding and the padded positions are ignored by the loss (ignore_index 0)."""
        from src import functions as F_
        if hidden is not None:
            raise NotImplementedError('training forward starts from the zero state; use step() for incremental decoding')
        if '_layers' not in self.__dict__ or self._flat_dev != self.emb.weight.device:
            self.flatten()
        train = self.training and self.dropout > 0
        self._seed = getattr(self, '_seed', 12345) + 7919
        h = F_.EmbeddingFn.apply(self._anchor, x, self.emb)
        if train:
            h = F_.DropoutFn.apply(h, self.dropout, self._seed)
        for l, layer in enumerate(self._layers):
            if self.module == 'GRU':
                h = GRULayerFn.apply(self._anchor, h, layer, self.prec)
                if train:
                    h = F_.DropoutFn.apply(h, self.dropout, self._seed + 1 + l)
            else:
                h = F_.RNNLayerFn.apply(self._anchor, h, layer, train, self._seed + 1 + l, self.prec, F_.LayerF32)
        if self.emb_tying:
            out = F_.LinearFn.apply(self._anchor, h, self.emb.weight, None, self.prec)
        else:
            out = F_.LinearFn.apply(self._anchor, h, self.trans.weight, self.trans.bias, self.prec)
        return out, None

    def create_msg(self):
        return ['Model spec.| RNNLM weight tying = {}, # of layers = {}, dim = {}'.format(self.emb_tying, self.n_layers, self.dim)]

    def init_state(self, n, device):
        """The zero state of n hypotheses: (h, c) each (layers, n, dim) for an LSTM, ONE (layers, n, dim) tensor for a GRU
        (the reference's two state kinds, src/decode.py:198-204)."""
        z = lambda: torch.zeros((self.n_layers, n, self.dim), dtype=torch.float32, device=device)
        return (z(), z()) if self.module == 'LSTM' else z()

    def _parts(self, state):
        return tuple(state) if self.module == 'LSTM' else (state,)

    def _pack(self, parts):
        return tuple(parts) if self.module == 'LSTM' else parts[0]

    def state_rows(self, state, n):
        """The first n hypotheses of `state`, contiguous."""
        return self._pack([s[:, :n].contiguous() for s in self._parts(state)])

    def gather_state(self, state, index):
        """New state whose row i is row index[i] of `state` (index int64 on the device): one asr_gather_rows per layer and
        state tensor, whatever the module."""
        R, st = index.shape[0], H.stream_ptr()
        parts = self._parts(state)
        out = [torch.empty((self.n_layers, R, self.dim), dtype=torch.float32, device=s.device) for s in parts]
        for l in range(self.n_layers):
            for s, o in zip(parts, out):
                H.call('asr_gather_rows', H.ptr(s[l]), H.ptr(index), H.ptr(o[l]), R, self.dim, self.dim, self.dim, s.shape[1], st)
        return self._pack(out)

    @torch.no_grad()
    def step(self, tokens, state):
        """tokens (n) int64 on the device, state = init_state's kind with n rows -> (log-probs (n,V), new state)."""
        n = tokens.shape[0]
        dev = tokens.device
        st = H.stream_ptr()
        x = torch.empty((n, self.emb.weight.shape[1]), dtype=torch.float32, device=dev)
        tok = tokens.contiguous()
        H.call('asr_gather_rows', H.ptr(self.emb.weight), H.ptr(tok), H.ptr(x), n, x.shape[1], x.shape[1], x.shape[1],
               self.vocab_size, st)
        if self.module == 'GRU':
            h_new = torch.empty_like(state)
            for l in range(self.n_layers):
                wih, whh = getattr(self.rnn, 'weight_ih_l%d' % l), getattr(self.rnn, 'weight_hh_l%d' % l)
                gi = torch.empty((n, 3 * self.dim), dtype=torch.float32, device=dev)
                H.gemm(x, wih, gi, n, 3 * self.dim, x.shape[1], x.shape[1], wih.shape[1], 3 * self.dim, 1, 1,
                       bias=getattr(self.rnn, 'bias_ih_l%d' % l), prec=self.prec)
                hp = state[l].contiguous()
                H.call('asr_gru_rec_fwd', H.ptr(gi), H.ptr(whh), H.ptr(getattr(self.rnn, 'bias_hh_l%d' % l)), H.ptr(hp), n, 1, self.dim,
                       self.prec, H.ptr(h_new[l]), None, st)
                x = h_new[l]
            return self._output(x, n, st), h_new
        h_prev, c_prev = state
        h_new, c_new = torch.empty_like(h_prev), torch.empty_like(c_prev)
        for l in range(self.n_layers):
            wih, whh = getattr(self.rnn, 'weight_ih_l%d' % l), getattr(self.rnn, 'weight_hh_l%d' % l)
            pre = torch.empty((n, 4 * self.dim), dtype=torch.float32, device=dev)
            H.gemm(x, wih, pre, n, 4 * self.dim, x.shape[1], x.shape[1], wih.shape[1], 4 * self.dim, 1, 1, prec=self.prec)
            hp = h_prev[l].contiguous()
            H.gemm(hp, whh, pre, n, 4 * self.dim, self.dim, self.dim, self.dim, 4 * self.dim, 1, 1, accum=1, prec=self.prec)
            cp = c_prev[l].contiguous()
            H.call('asr_lstm_cell', H.ptr(pre), H.ptr(getattr(self.rnn, 'bias_ih_l%d' % l)), H.ptr(getattr(self.rnn, 'bias_hh_l%d' % l)),
                   H.ptr(cp), H.ptr(h_new[l]), H.ptr(c_new[l]), n, self.dim, st)
            x = h_new[l]
        return self._output(x, n, st), (h_new, c_new)

    def _output(self, x, n, st):
        """Output projection (tied embedding or `trans`) and log-softmax of the last layer's h (n, dim)."""
        dev = x.device
        logits = torch.empty((n, self.vocab_size), dtype=torch.float32, device=dev)
        if self.emb_tying:
            H.gemm(x, self.emb.weight, logits, n, self.vocab_size, self.dim, self.dim, self.dim, self.vocab_size, 1, 1, prec=self.prec)
        else:
            H.gemm(x, self.trans.weight, logits, n, self.vocab_size, self.dim, self.dim, self.dim, self.vocab_size, 1, 1,
                   bias=self.trans.bias, prec=self.prec)
        logp = torch.empty_like(logits)
        H.call('asr_log_softmax', H.ptr(logits), H.ptr(logp), n, self.vocab_size, st)
        return logp
