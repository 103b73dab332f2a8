"""Word-embedding regulariser and embedding-fused decoding with the reference's surface (src/plugin.py:7-160):
`EmbeddingRegularizer(tokenizer, dec_dim, enable, src, distance, weight, fuse, temperature, freeze, fuse_normalize, dropout,
bert)`, `.create_msg()`, `.get_weight()`, `.get_temp()`, `.fuse_prob(x_emb, dec_logit)`, `.forward(dec_state, dec_logit, label,
return_loss) -> (loss, log_fused_prob)`, and its state_dict keys (emb_table.weight, emb_net.{0,2}.{weight,bias}, fuse_lambda,
temp).  Everything runs in libasr_hip.so: the two linear layers and the table contraction through asr_gemm at the model's
precision, dropout through the Philox kernel, the loss, the fusion and F.normalize through csrc/emb_fuse.hip.

Refused at construction, because the reference cannot run them either: `bert` (needs a downloaded model), distance 'MSE' (its
loss.view(b, t) fails on the (N * E) tensor).  check_emb_config refuses fusion together with scheduled sampling (the reference
hands log-probabilities to Categorical) and a CTC-only model.

lambda and temp.  fuse > 0: constant lambda = fuse (buffer); fuse = -1: sigmoid of a learnable scalar (initial raw value 0.5);
fuse = -2: sigmoid of a learnable value per token.  temperature > 0: constant (buffer); -1 / -2: learnable scalar / per token
(initial 1); relu is applied to the raw value inside the kernel, so temp <= 0 gives a uniform embedding distribution."""
import torch
from torch import nn

from src import functions as F_hip
from src import hipabi as H
from src.util import load_embedding
from src.variants import LinearActFn

ALIGN = 64


def check_emb_config(emb_cfg, model_cfg, hparas):
    """What a training run refuses before it builds the plugin (bin/train_asr.py)."""
    if not emb_cfg or not emb_cfg.get('enable', False):
        return
    if float(model_cfg.get('ctc_weight', 0.0)) >= 1.0:
        raise ValueError('emb.enable needs an attention decoder to regularise, and this model has none (CTC-only, ctc_weight = 1)')
    if emb_cfg.get('fuse', 0) != 0 and (hparas.get('tf_end', 1) < 1 or hparas.get('tf_start', 1) < 1):
        raise ValueError('embedding fusion (emb.fuse != 0) cannot be combined with scheduled sampling (tf_start / tf_end < 1): the '
                         'fused output is a log-probability, which the reference hands to Categorical as logits and fails')


class EmbCosLossFn(torch.autograd.Function):
    """asr_emb_cos_loss: loss and both gradients in the forward launch; backward scales them by the incoming device scalar."""

    @staticmethod
    def forward(ctx, x_emb, table, label):
        B, L = label.shape
        V, E = table.shape
        x = x_emb.contiguous()
        lab = label.to(x.device, torch.int64).contiguous()
        dev = x.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        dx = torch.empty((B * L, E), dtype=torch.float32, device=dev)
        dy = torch.empty((B * L, E), dtype=torch.float32, device=dev) if table.requires_grad else None
        row = torch.empty(B * L, dtype=torch.float32, device=dev)
        H.call('asr_emb_cos_loss', H.ptr(x), H.ptr(table), H.ptr(lab), L, H.ptr(loss), H.ptr(dx), H.ptr(dy), H.ptr(row), B, L, E, V,
               H.stream_ptr())
        ctx.table, ctx.shape = table, x_emb.shape
        ctx.save_for_backward(dx, dy, lab)
        return loss

    @staticmethod
    def backward(ctx, gout):
        dx, dy, lab = ctx.saved_tensors
        table = ctx.table
        if dy is not None:
            V, E = table.shape
            dyg = F_hip.scale_by_device_scalar(dy, gout)
            H.call('asr_embedding_bwd', H.ptr(dyg), E, H.ptr(lab), H.ptr(table.grad), dyg.shape[0], E, V, H.stream_ptr())
        return F_hip.scale_by_device_scalar(dx, gout).view(ctx.shape), None, None


class RowNormalizeFn(torch.autograd.Function):
    """F.normalize(x, dim=-1) on (N,E): asr_row_normalize_fwd / _bwd."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y = torch.empty_like(x)
        H.call('asr_row_normalize_fwd', H.ptr(x), H.ptr(y), x.shape[0], x.shape[1], H.stream_ptr())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        H.call('asr_row_normalize_bwd', H.ptr(dy), H.ptr(x), H.ptr(dx), x.shape[0], x.shape[1], H.stream_ptr())
        return dx


class TableLogitFn(torch.autograd.Function):
    """emb_logit (N,V) = x (N,E) table (V,E)^T; the table's gradient is formed only when it is trained."""

    @staticmethod
    def forward(ctx, x, table, prec):
        x, table = x.contiguous(), table.contiguous()
        N, E = x.shape
        V = table.shape[0]
        out = torch.empty((N, V), dtype=torch.float32, device=x.device)
        H.gemm(x, table, out, N, V, E, E, E, V, 1, 1, prec=prec)
        ctx.prec = prec
        ctx.save_for_backward(x, table)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, table = ctx.saved_tensors
        N, E = x.shape
        V = table.shape[0]
        dout = dout.contiguous()
        dx = dt = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            H.gemm(dout, table, dx, N, E, V, V, E, E, 1, 0, prec=ctx.prec)
        if ctx.needs_input_grad[1]:
            dt = torch.zeros_like(table)
            H.gemm(dout, x, dt, V, E, N, V, E, E, 0, 0, accum=1, splits=1, prec=ctx.prec)
        return dx, dt, None


class EmbFuseFn(torch.autograd.Function):
    """asr_emb_fuse_fwd / _bwd on dec_logit (..., V) and emb_logit (N,V); temp / lam: the raw parameters (1 or V entries)."""

    @staticmethod
    def forward(ctx, dec_logit, emb_logit, temp, lam, lam_sigmoid):
        V = dec_logit.shape[-1]
        dec = dec_logit.contiguous().view(-1, V)
        emb = emb_logit.contiguous()
        N = dec.shape[0]
        out = torch.empty((N, V), dtype=torch.float32, device=dec.device)
        stats = torch.empty((N, 2), dtype=torch.float32, device=dec.device)
        H.call('asr_emb_fuse_fwd', H.ptr(dec), V, H.ptr(emb), H.ptr(temp), 1 if temp.numel() > 1 else 0, H.ptr(lam),
               1 if lam.numel() > 1 else 0, 1 if lam_sigmoid else 0, H.ptr(out), H.ptr(stats), None, 1, N, V, H.stream_ptr())
        ctx.lam_sigmoid, ctx.shape = lam_sigmoid, dec_logit.shape
        ctx.save_for_backward(dec, emb, temp, lam, stats)
        return out.view(dec_logit.shape)

    @staticmethod
    def backward(ctx, dout):
        dec, emb, temp, lam, stats = ctx.saved_tensors
        N, V = dec.shape
        dout = dout.contiguous().view(N, V)
        dev = dec.device
        d_dec, d_emb = torch.empty_like(dec), torch.empty_like(emb)
        need_t, need_l = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        d_temp = torch.empty_like(temp) if need_t else None
        d_lam = torch.empty_like(lam) if need_l else None
        n_work = (N * (V if temp.numel() > 1 else 1) if need_t else 0) + (N * (V if lam.numel() > 1 else 1) if need_l else 0)
        work = torch.empty(n_work, dtype=torch.float32, device=dev) if n_work else None
        H.call('asr_emb_fuse_bwd', H.ptr(dout), H.ptr(dec), V, H.ptr(emb), H.ptr(temp), 1 if temp.numel() > 1 else 0, H.ptr(lam),
               1 if lam.numel() > 1 else 0, 1 if ctx.lam_sigmoid else 0, H.ptr(stats), H.ptr(d_dec), H.ptr(d_emb), H.ptr(d_temp),
               H.ptr(d_lam), H.ptr(work), N, V, H.stream_ptr())
        return d_dec.view(ctx.shape), d_emb, d_temp, d_lam, None


class EmbeddingRegularizer(nn.Module):
    ''' Perform word embedding regularization training for ASR'''

    def __init__(self, tokenizer, dec_dim, enable, src, distance, weight, fuse, temperature,
                 freeze=True, fuse_normalize=False, dropout=0.0, bert=None, prec='bf16', seed=0):
        super().__init__()
        self.enable = enable
        self.prec = H.BF16 if prec == 'bf16' else H.F32
        self.seed, self._drop_counter = int(seed), 0
        self.flat_param = self.flat_grad = self._anchor = None
        self._mode_word = {}
        if not enable:
            return
        if bert is not None:
            raise NotImplementedError('emb.bert = %r: the BERT embedding predictor needs from_pretrained of a downloaded model, which '
                                      'is outside this build; use the fastText-table variant (emb.src)' % (bert,))
        if distance == 'MSE':
            raise NotImplementedError("emb.distance = 'MSE' cannot run in the reference either (its loss.view(b, t) fails on the "
                                      "(N * E) tensor of nn.MSELoss(reduction='none')); use 'CosEmb'")
        if distance != 'CosEmb':
            raise NotImplementedError('emb.distance = %r' % (distance,))
        self.use_bert = False
        vectors = torch.as_tensor(load_embedding(tokenizer, src), dtype=torch.float32)
        vocab_size, self.dim = vectors.shape
        # the table under the reference's key `emb_table.weight`: padding_idx 0, the file's rows as they are, trained only on request
        self.emb_table = nn.Embedding(vocab_size, self.dim, padding_idx=0)
        with torch.no_grad():
            self.emb_table.weight.copy_(vectors)
        self.emb_table.weight.requires_grad_(not freeze)
        hidden = (self.dim + dec_dim) // 2
        self.emb_net = nn.Sequential(nn.Linear(dec_dim, hidden), nn.ReLU(), nn.Linear(hidden, self.dim))      # keys emb_net.0.* / emb_net.2.*
        self.weight, self.distance, self.fuse_normalize = weight, distance, bool(fuse_normalize)
        self.drop_p = float(dropout)
        self.apply_dropout = self.drop_p > 0
        self.apply_fuse = fuse != 0
        self.fuse_learnable = False
        if self.apply_fuse:
            # name of the tensor, config value, initial raw value when learnt, create_msg's word for the scalar / per-token form
            for name, value, init, words in (('fuse_lambda', fuse, 0.5, ('learnable', 'vocab-wise learnable')),
                                             ('temp', temperature, 1.0, ('learnable', 'elementwise'))):
                learnt = value in (-1, -2)
                if learnt:
                    self.register_parameter(name, nn.Parameter(torch.full((vocab_size if value == -2 else 1,), init)))
                else:
                    self.register_buffer(name, torch.tensor([float(value)]))
                self._mode_word[name] = words[0 if value == -1 else 1] if learnt else str(value)
                if name == 'fuse_lambda':
                    self.fuse_learnable = learnt
            self.eps = 1e-8
        self._flatten()

    # ---- flat storage of the trainable parameters (the fused optimizer kernels step one buffer, src/optim.py) ----------
    def _flatten(self):
        params = [p for p in self.parameters() if p.requires_grad]
        if not params:
            return
        dev = params[0].device
        offs, off = {}, 0
        for p in params:
            offs[id(p)] = off
            off = (off + p.numel() + ALIGN - 1) // ALIGN * ALIGN
        flat = torch.zeros(off, dtype=torch.float32, device=dev)
        grad = torch.zeros(off, dtype=torch.float32, device=dev)
        for p in params:
            o, n = offs[id(p)], p.numel()
            flat[o:o + n].copy_(p.data.reshape(-1))
            p.data = flat[o:o + n].view(p.shape)
            p.grad = grad[o:o + n].view(p.shape)
            p._asr_flat = (flat, grad, offs)
        self.flat_param, self.flat_grad, self._offsets = flat, grad, offs
        self._anchor = torch.zeros(1, dtype=torch.float32, device=dev, requires_grad=True)

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        if self.enable:
            self._flatten()
        return self

    def trainable_parameters(self):
        """What an optimizer steps: the parameters in flat storage (a frozen table is not among them)."""
        return [p for p in self.parameters() if p.requires_grad]

    def zero_grad(self, set_to_none=False):
        if self.flat_grad is not None:
            self.flat_grad.zero_()

    # ---- reference surface ------------------------------------------------------------------------------------------
    def create_msg(self):
        """The two lines the reference prints for the plugin."""
        lines = ['Plugin.    | Word embedding regularization enabled (type:%s, weight:%s)' % (self.distance, self.weight)]
        if self.apply_fuse:
            lines += ['           | Embedding-fusion decoder enabled ( temp. = %s, lambda = %s )'
                      % (self._mode_word['temp'], self._mode_word['fuse_lambda'])]
        return lines

    def get_weight(self):
        """lambda for the log: the mean of sigmoid(raw) when it is learnt (a host scalar), the constant's buffer otherwise."""
        lam = self.fuse_lambda.detach()
        return lam.sigmoid().mean().cpu() if self.fuse_learnable else lam

    def get_temp(self):
        """The temperature in effect for the log: mean of relu(raw)."""
        return self.temp.detach().clamp(min=0).mean()

    def _embed(self, dec_state):
        """x_emb = emb_net(dropout(dec_state)): (..., Dd) -> (..., E)."""
        x = dec_state.contiguous()         # (a tracked copy: the Functions below look at requires_grad of a contiguous input)
        if self.apply_dropout and self.training:
            self._drop_counter += 1
            x3 = x.reshape(1, -1, x.shape[-1])
            x = F_hip.DropoutFn.apply(x3, self.drop_p, (self.seed * 1000003 + self._drop_counter) & 0xFFFFFFFFFFFF).view(x.shape)
        l0, l2 = self.emb_net[0], self.emb_net[2]
        h = LinearActFn.apply(self._anchor, x, l0.weight, l0.bias, H.ACT_RELU, self.prec)
        return LinearActFn.apply(self._anchor, h, l2.weight, l2.bias, H.ACT_NONE, self.prec)

    def _emb_logit(self, x_emb):
        xe, tab = x_emb.reshape(-1, self.dim), self.emb_table.weight
        if self.fuse_normalize:
            xe, tab = RowNormalizeFn.apply(xe), RowNormalizeFn.apply(tab)
        return TableLogitFn.apply(xe, tab, self.prec)

    def fuse_prob(self, x_emb, dec_logit):
        ''' Takes context and decoder logit to perform word embedding fusion '''
        return EmbFuseFn.apply(dec_logit, self._emb_logit(x_emb), self.temp, self.fuse_lambda, self.fuse_learnable)

    @torch.no_grad()
    def fuse_rows(self, dec_state, dec_logit, out=None, argmax=None, argmax_ld=1):
        """Decoding step (greedy validation, beam search): dec_state (R,Dd), dec_logit (R,V) with unit column stride (rows may
        be strided) -> fused log-probs (R,V) written into `out`; argmax: int64 tensor (view) whose element r * argmax_ld gets the
        best token of row r (the token table of the next step)."""
        R, V = dec_logit.shape
        assert dec_logit.stride(1) == 1 and dec_logit.stride(0) >= V
        emb = self._emb_logit(self._embed(dec_state.contiguous())).contiguous()
        if out is None:
            out = torch.empty((R, V), dtype=torch.float32, device=dec_logit.device)
        stats = torch.empty((R, 2), dtype=torch.float32, device=dec_logit.device)
        H.call('asr_emb_fuse_fwd', H.ptr(dec_logit), dec_logit.stride(0), H.ptr(emb), H.ptr(self.temp), 1 if self.temp.numel() > 1 else 0,
               H.ptr(self.fuse_lambda), 1 if self.fuse_lambda.numel() > 1 else 0, 1 if self.fuse_learnable else 0, H.ptr(out),
               H.ptr(stats), H.ptr(argmax), argmax_ld, R, V, H.stream_ptr())
        return out

    def forward(self, dec_state, dec_logit, label=None, return_loss=True):
        if not dec_state.is_cuda:
            raise RuntimeError('EmbeddingRegularizer (HIP path) needs CUDA tensors; there is no CPU fallback')
        log_fused_prob, loss = None, None
        x_emb = self._embed(dec_state)
        if return_loss:
            b, t = label.shape
            loss = EmbCosLossFn.apply(x_emb.reshape(b, t, self.dim), self.emb_table.weight, label)
        if self.apply_fuse:
            log_fused_prob = self.fuse_prob(x_emb, dec_logit)
        return loss, log_fused_prob
