"""VGG front-ends of the encoder on the HIP path, with the reference's module/parameter names
(VGGExtractor src/module.py:659-716, VGGExtractor_LN src/module.py:582-657; `extractor.<i>.weight` keys).

Activations are channel-last images in one of two layouts, and a layout class owns every launch for its images: _Plain32
(unbordered fp32 (B,T,F,C): asr_conv3x3, implicit GEMM on MFMA - forward, input gradient with the flipped weight copy, weight
gradient - and the HBM-bound pooling / LayerNorm-over-frequency kernels of csrc/vgg.hip) and _Bordered16 (zero-bordered bf16
(B,T+2,F+2,C), csrc/vgg16.hip).  One loop in each direction (conv_stack, conv_stack_bwd) walks the convolutions of an
extractor, for training (_ConvStackFn) and for inference over a padded batch (forward_lens); layout_of picks the layout."""
import os

import torch
import torch.nn as nn

from src import hipabi as H

FBANK_SIZE = 40


class CNNLayerNorm(nn.Module):
    def __init__(self, n_feats):
        super().__init__()
        self.layer_norm = nn.LayerNorm(n_feats)


def vgg16_ok(mod, prec):
    """The bf16 front-end (csrc/vgg16.hip) covers bf16 contraction mode with channel counts that are multiples of 64 behind the
    first layer (both reference extractors: 128/256 and 64/128) and at most 4 input channels per tap group (9*Cin <= 40)."""
    if prec != H.BF16 or os.environ.get('ASR_VGG16', '1') == '0':
        return False
    return mod.init_dim % 64 == 0 and mod.hide_dim % 64 == 0 and 9 * mod.in_channel <= 40


# ---- the two image layouts: every launch of a front-end entry point ------------------------------------------------------------
class _Layout(object):
    """The forward methods fill `rec`, the record of one convolution that the backward methods read (None for inference,
    which keeps nothing alive): x the convolution's input, pre / stats the CNNLayerNorm's input and statistics (None without
    one), act the activation, pool = (idx, t2, f2, freq_only) behind a pooling."""

    def __init__(self, prec, dev):
        self.prec, self.dev, self.st, self._lens = prec, dev, H.stream_ptr(), {}

    def new(self, shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=self.dev)

    def lens_dev(self, lens):
        key = tuple(lens)
        if key not in self._lens:
            self._lens[key] = torch.tensor(lens, dtype=torch.int64, device=self.dev)
        return self._lens[key]


class _Plain32(_Layout):
    """Unbordered fp32 images (B,t,f,C); the contractions round their operands to `prec` when they stage them."""

    @staticmethod
    def image_bytes(T, F, C, ln):
        return T * F * C * 4

    def first(self, feature, B, T, Cin, F):
        x = self.new((B, T, F, Cin))
        H.call('asr_permute_last2', H.ptr(feature), H.ptr(x), B * T, Cin, F, self.st)              # (.., C, F) -> (.., F, C)
        return x

    def conv(self, li, cur, conv, ln, B, t, f, rec=None):
        Co, Ci = conv.weight.shape[0], conv.weight.shape[1]
        wf = self.new((Co, 9 * Ci))
        H.call('asr_conv_weight_permute', H.ptr(conv.weight), H.ptr(wf), Co, Ci, 0, self.st)
        act, pre, stats = self.new((B, t, f, Co)), None, None
        H.call('asr_conv3x3', H.ptr(cur), H.ptr(wf), H.ptr(act), H.ptr(conv.bias), B, t, f, Ci, Co, 0,
               H.ACT_RELU if ln is None else H.ACT_NONE, 0, self.prec, self.st)
        if ln is not None:
            pre, act, stats = act, self.new((B, t, f, Co)), self.new((B * t * Co, 2))
            H.call('asr_ln_freq_fwd', H.ptr(pre), H.ptr(ln.weight), H.ptr(ln.bias), H.ptr(act), H.ptr(stats), B * t, f, Co, 1e-5, 1, self.st)
        if rec is not None:
            rec.update(x=cur, pre=pre, stats=stats, act=act)
        return act

    def zero_tail(self, act, lens, B, t, f, Co):
        H.call('asr_ragged_zero_tail', H.ptr(act), H.ptr(self.lens_dev(lens)), B, t, t, 0, f * Co, 4, self.st)

    @staticmethod
    def _pool_dims(B, t, t2, freq_only):
        """(images, rows, pooled rows): MaxPool2d((1, 2)) is the 2 x 2 kernel on the image seen as B*t images of ONE row."""
        return (B * t, 1, 1) if freq_only else (B, t, t2)

    def pool(self, act, B, t, f, Co, t2, f2, freq_only, rec=None):
        pooled, idx = self.new((B, t2, f2, Co)), self.new((B, t2, f2, Co), torch.uint8)
        n, r, r2 = self._pool_dims(B, t, t2, freq_only)
        H.call('asr_maxpool2x2_fwd', H.ptr(act), H.ptr(pooled), H.ptr(idx), n, r, f, Co, r2, f2, self.st)
        if rec is not None:
            rec['pool'] = (idx, t2, f2, freq_only)
        return pooled

    def output(self, cur, B, t, f, Co):
        out = self.new((B, t, Co * f))
        H.call('asr_permute_last2', H.ptr(cur), H.ptr(out), B * t, f, Co, self.st)                  # (.., F, C) -> (.., C, F)
        return out

    def output_bwd(self, dout, B, t, f, Co):
        g = self.new((B, t, f, Co))
        H.call('asr_permute_last2', H.ptr(dout), H.ptr(g), B * t, Co, f, self.st)                   # (.., C, F) -> (.., F, C)
        return g

    def pool_bwd(self, g, B, t, f, Co, idx, t2, f2, freq_only):
        gp = self.new((B, t, f, Co))
        n, r, r2 = self._pool_dims(B, t, t2, freq_only)
        H.call('asr_maxpool2x2_bwd', H.ptr(g), H.ptr(idx), H.ptr(gp), n, r, f, Co, r2, f2, self.st)
        return gp

    def act_bwd(self, g, rec, conv, ln, B, t, f):
        Co = conv.weight.shape[0]
        dpre = self.new((B, t, f, Co))
        if ln is None:
            H.call('asr_act_bwd', H.ptr(g), H.ptr(rec['act']), H.ptr(dpre), g.numel(), H.ACT_RELU, self.st)
        else:
            H.call('asr_ln_freq_bwd', H.ptr(g), H.ptr(rec['pre']), H.ptr(ln.weight), H.ptr(ln.bias), H.ptr(rec['stats']),
                   H.ptr(dpre), H.ptr(ln.weight.grad), H.ptr(ln.bias.grad), B * t, f, Co, 1, self.st)
        return dpre

    def param_grads(self, li, x, dpre, conv, ln, B, t, f):
        Co, Ci = conv.weight.shape[0], conv.weight.shape[1]
        dwf = torch.zeros((Co, 9 * Ci), dtype=torch.float32, device=self.dev)
        H.call('asr_conv3x3', H.ptr(x), H.ptr(dpre), H.ptr(dwf), None, B, t, f, Ci, Co, 1, H.ACT_NONE, 1, self.prec, self.st)
        H.call('asr_conv_weight_permute', H.ptr(dwf), H.ptr(conv.weight.grad), Co, Ci, 2, self.st)
        H.call('asr_colsum', H.ptr(dpre), Co, B * t * f, Co, H.ptr(conv.bias.grad), self.st)

    def input_grad(self, dpre, conv, B, t, f):
        Co, Ci = conv.weight.shape[0], conv.weight.shape[1]
        wd, gin = self.new((Ci, 9 * Co)), self.new((B, t, f, Ci))
        H.call('asr_conv_weight_permute', H.ptr(conv.weight), H.ptr(wd), Co, Ci, 1, self.st)
        H.call('asr_conv3x3', H.ptr(dpre), H.ptr(wd), H.ptr(gin), None, B, t, f, Co, Ci, 0, H.ACT_NONE, 0, self.prec, self.st)
        return gin


class _Bordered16(_Layout):
    """Zero-bordered bf16 images P(t,f,C) = (B, t+2, f+2, C), held as (B (t+2) (f+2), C): every convolution is an implicit GEMM
    on the direct-to-LDS bf16 contraction kernel (asr_conv3x3_16), the first one on its patch matrix (K1p columns: 9 Cin padded
    to a multiple of 8), the weight gradient one launch of nine shifted-row TN contractions; pooling / CNNLayerNorm / layout
    changes run on the bordered images (reference src/module.py:582-716)."""

    @staticmethod
    def image_bytes(T, F, C, ln):
        return (T + 2) * (F + 2) * C * (4 if ln else 2)

    def first(self, feature, B, T, Cin, F):
        return feature                             # the first convolution reads its patch matrix straight off the features

    def conv(self, li, cur, conv, ln, B, t, f, rec=None):
        Co, Ci = conv.weight.shape[0], conv.weight.shape[1]
        Mp = B * (t + 2) * (f + 2)
        if li == 0:
            K = (9 * Ci + 7) // 8 * 8
            x = self.new((Mp, K), torch.bfloat16)
            H.call('asr_vgg16_im2col', H.ptr(cur), H.ptr(x), B, t, f, Ci, K, self.st)
        else:
            K, x = 9 * Ci, cur
        w16 = self.new((Co, K), torch.bfloat16)
        H.call('asr_conv_weight_pack16', H.ptr(conv.weight), H.ptr(w16), Co, Ci, K, 0, self.st)
        # pre-activations of a CNNLayerNorm stay fp32 (see asr_conv3x3_16)
        act, pre, stats = self.new((Mp, Co), torch.bfloat16 if ln is None else torch.float32), None, None
        H.call('asr_conv3x3_16', H.ptr(x), H.ptr(w16), H.ptr(act), H.ptr(conv.bias), B, t, f, Ci, Co, K, 0 if li == 0 else 1,
               H.ACT_RELU if ln is None else H.ACT_NONE, 0 if ln is None else 1, self.st)
        if ln is not None:
            pre, act, stats = act, self.new((Mp, Co), torch.bfloat16), self.new((B * (t + 2) * Co, 2))
            H.call('asr_ln_freq16_fwd', H.ptr(pre), H.ptr(ln.weight), H.ptr(ln.bias), H.ptr(act), H.ptr(stats), B, t, f, Co, 1e-5, 1, self.st)
        if rec is not None:
            rec.update(x=x, pre=pre, stats=stats, act=act)
        return act

    def zero_tail(self, act, lens, B, t, f, Co):
        H.call('asr_ragged_zero_tail', H.ptr(act), H.ptr(self.lens_dev(lens)), B, t, t + 2, 1, (f + 2) * Co, 2, self.st)

    def pool(self, act, B, t, f, Co, t2, f2, freq_only, rec=None):
        if freq_only:
            raise NotImplementedError('frequency-only pooling has no kernel on the bordered bf16 images')
        Mp2 = B * (t2 + 2) * (f2 + 2)
        pooled, idx = self.new((Mp2, Co), torch.bfloat16), self.new((Mp2, Co), torch.uint8)
        H.call('asr_maxpool2x2_16_fwd', H.ptr(act), H.ptr(pooled), H.ptr(idx), B, t, f, Co, t2, f2, self.st)
        if rec is not None:
            rec['pool'] = (idx, t2, f2, freq_only)
        return pooled

    def output(self, cur, B, t, f, Co):
        out = self.new((B, t, Co * f), torch.bfloat16)
        H.call('asr_vgg16_output', H.ptr(cur), H.ptr(out), B, t, f, Co, self.st)
        return out

    def output_bwd(self, dout, B, t, f, Co):
        if dout.dtype != torch.bfloat16:
            d16 = self.new(tuple(dout.shape), torch.bfloat16)
            H.call('asr_cast_bf16', H.ptr(dout), H.ptr(d16), dout.numel(), self.st)
            dout = d16
        g = self.new((B * (t + 2) * (f + 2), Co), torch.bfloat16)
        H.call('asr_vgg16_output_bwd', H.ptr(dout), H.ptr(g), B, t, f, Co, self.st)
        return g

    def pool_bwd(self, g, B, t, f, Co, idx, t2, f2, freq_only):
        gp = self.new((B * (t + 2) * (f + 2), Co), torch.bfloat16)
        H.call('asr_maxpool2x2_16_bwd', H.ptr(g), H.ptr(idx), H.ptr(gp), B, t, f, Co, t2, f2, self.st)
        return gp

    def act_bwd(self, g, rec, conv, ln, B, t, f):
        Co, Mp = conv.weight.shape[0], B * (t + 2) * (f + 2)
        dpre = self.new((Mp, Co), torch.bfloat16)
        if ln is None:
            H.call('asr_act_bwd16', H.ptr(g), H.ptr(rec['act']), H.ptr(dpre), Mp * Co, H.ACT_RELU, self.st)
        else:
            H.call('asr_ln_freq16_bwd', H.ptr(g), H.ptr(rec['pre']), H.ptr(ln.weight), H.ptr(ln.bias), H.ptr(rec['stats']),
                   H.ptr(dpre), H.ptr(ln.weight.grad), H.ptr(ln.bias.grad), H.ptr(conv.bias.grad), B, t, f, Co, 1, self.st)
        return dpre

    def param_grads(self, li, x, dpre, conv, ln, B, t, f):
        Co, Ci = conv.weight.shape[0], conv.weight.shape[1]
        Mp = B * (t + 2) * (f + 2)
        K = x.shape[1] if li == 0 else 9 * Ci      # the columns of the patch matrix / the nine taps of the image
        dwf = torch.zeros((Co, K), dtype=torch.float32, device=self.dev)
        if li == 0:
            H.gemm16(dpre, x, dwf, Co, K, Mp, Co, K, K, 0, 0, accum=1, splits=min(64, max(1, Mp // 4096)))
        else:
            tiles = ((Co + 127) // 128) * ((Ci + 127) // 128)
            splits = max(1, min(Mp // 2048, 96 // tiles))          # x 9 taps: ~800 workgroups per launch
            H.call('asr_conv3x3_16_wgrad', H.ptr(x), H.ptr(dpre), H.ptr(dwf), B, t, f, Ci, Co, K, splits, self.st)
        H.call('asr_conv_weight_fold', H.ptr(dwf), H.ptr(conv.weight.grad), Co, Ci, K, self.st)
        if ln is None:         # (behind a CNNLayerNorm the bias gradient comes out of asr_ln_freq16_bwd, in fp32)
            H.call('asr_colsum16', H.ptr(dpre), Co, Mp, Co, H.ptr(conv.bias.grad), None, 0, self.st)

    def input_grad(self, dpre, conv, B, t, f):
        Co, Ci = conv.weight.shape[0], conv.weight.shape[1]
        wd, gin = self.new((Ci, 9 * Co), torch.bfloat16), self.new((B * (t + 2) * (f + 2), Ci), torch.bfloat16)
        H.call('asr_conv_weight_pack16', H.ptr(conv.weight), H.ptr(wd), Co, Ci, 9 * Co, 1, self.st)
        H.call('asr_conv3x3_16', H.ptr(dpre), H.ptr(wd), H.ptr(gin), None, B, t, f, Co, Ci, 9 * Co, 1, H.ACT_NONE, 0, self.st)
        return gin


# ---- one loop over the convolutions in each direction ---------------------------------------------------------------------------
def conv_stack(mod, lay, feature, lens=None, save=None):
    """Forward of one conv stack `mod` (an extractor, or one band of a frequency-split one) in the layout `lay`: a pooling behind
    convolutions 1 and 3, the second one frequency-only for `pool2_freq_only`.  feature (B,T,D) with T % time_div == 0.
    Returns (out (B, T / time_div, C*F), lens / time_div or None).

    save: a list that receives one record per convolution for conv_stack_bwd (training).

    lens: inference over a padded batch - ints, multiples of time_div, max(lens) == T, and feature holds exact zeros at
    t >= lens[b].  Row b comes out as the unpadded pass of its lens[b] frames (to rounding): that pass's 3 x 3 convolutions read
    zero padding at t = lens[b], where the padded batch holds ReLU(bias + taps that reach into valid frames) (or the
    CNNLayerNorm of it) - so the tail of EVERY convolution's activation is zeroed in place (asr_ragged_zero_tail) before
    anything reads it.  Pooling windows never straddle a row's end (lengths are multiples of time_div) and pooling a zero tail
    gives zeros; a time pooling halves the lengths, a frequency-only one does not; out has zero tails."""
    B, T = feature.shape[0], feature.shape[1]
    fs = getattr(mod, 'freq_slice', None)
    if fs is not None:                           # one band of a frequency-split extractor: columns f0..f1 of every channel (a copy)
        feature = feature.reshape(B, T, mod.in_channel, -1)[..., fs[0]:fs[1]]
    cur, t, f = lay.first(feature.contiguous().float(), B, T, mod.in_channel, mod.freq_dim), T, mod.freq_dim
    lens = None if lens is None else list(lens)
    for li, (conv, ln) in enumerate(mod.conv_layers()):
        Co = conv.weight.shape[0]
        rec = None if save is None else {'dims': (t, f), 'pool': None}
        cur = lay.conv(li, cur, conv, ln, B, t, f, rec)
        if lens is not None and min(lens) < t:
            lay.zero_tail(cur, lens, B, t, f, Co)
        if li in (1, 3):
            freq_only = li == 3 and mod.pool2_freq_only
            if freq_only:
                t2, f2 = t, f // 2
            else:
                t2, f2 = ((t + 1) // 2, (f + 1) // 2) if mod.ceil_mode else (t // 2, f // 2)
                lens = None if lens is None else [n // 2 for n in lens]
            cur, t, f = lay.pool(cur, B, t, f, Co, t2, f2, freq_only, rec), t2, f2
        if save is not None:
            save.append(rec)
    return lay.output(cur, B, t, f, Co), lens


def conv_stack_bwd(mod, lay, saved, dout):
    """dout (B, t, C*f), the gradient of conv_stack's output, walked back through the records `saved`: the gradients of the
    convolutions and CNNLayerNorms go into their `.grad` (the features are data: no input gradient at the first convolution)."""
    layers = mod.conv_layers()
    B, t, Co = dout.shape[0], dout.shape[1], layers[-1][0].weight.shape[0]
    g = lay.output_bwd(dout.contiguous(), B, t, dout.shape[2] // Co, Co)
    for li in range(len(layers) - 1, -1, -1):
        (conv, ln), rec = layers[li], saved[li]
        t, f = rec['dims']
        if rec['pool'] is not None:
            g = lay.pool_bwd(g, B, t, f, conv.weight.shape[0], *rec['pool'])
        dpre = lay.act_bwd(g, rec, conv, ln, B, t, f)
        lay.param_grads(li, rec['x'], dpre, conv, ln, B, t, f)
        if li > 0:
            g = lay.input_grad(dpre, conv, B, t, f)


class _ConvStackFn(torch.autograd.Function):
    """Training pass of one conv stack in the layout class `layout`; drops the T % time_div trailing frames first."""

    @staticmethod
    def forward(ctx, anchor, feature, mod, prec, layout):
        div = mod.time_div
        if feature.shape[1] % div != 0:
            feature = feature[:, :-(feature.shape[1] % div), :]
        ctx.mod, ctx.prec, ctx.layout, ctx.saved = mod, prec, layout, []
        return conv_stack(mod, layout(prec, feature.device), feature, save=ctx.saved)[0]

    @staticmethod
    def backward(ctx, dout):
        mod = ctx.mod
        conv_stack_bwd(mod, ctx.layout(ctx.prec, dout.device), ctx.saved, dout)
        owner = getattr(mod, 'owner', None)
        if owner is not None:                    # a band of a frequency-split extractor: the bucket goes when both bands are done
            owner._bands_done += 1
            if owner._bands_done == 2 and owner.dp is not None:
                owner.dp.bucket_ready(owner.bucket)
        elif mod.dp is not None:
            mod.dp.bucket_ready(mod.bucket)
        ctx.saved = None
        return None, None, None, None, None


class _VGGFn(object):
    """_ConvStackFn with the layout in the name, for callers that run one extractor in both (tests/test_hip_vgg_kernels.py)."""
    layout = _Plain32

    @classmethod
    def apply(cls, anchor, feature, mod, prec):
        return _ConvStackFn.apply(anchor, feature, mod, prec, cls.layout)


class _VGG16Fn(_VGGFn):
    layout = _Bordered16


# ---- the extractors ----------------------------------------------------------------------------------------------------------------
class _VGGBase(nn.Module):
    time_div, pool2_freq_only = 4, False

    def check_dim(self, input_dim):
        if input_dim % FBANK_SIZE != 0:
            raise ValueError('HIP VGG front-end expects 40-bin fbank channels (input dim %d)' % input_dim)
        return input_dim // FBANK_SIZE, FBANK_SIZE, (FBANK_SIZE // 4) * self.hide_dim

    def forward(self, feature, feat_len, ctx=None):
        out = _ConvStackFn.apply(ctx.anchor, feature, self, ctx.prec, layout_of(self, ctx.prec))
        return out, feat_len // self.time_div


class VGGExtractor(_VGGBase):
    ''' VGG extractor (reference src/module.py:659-716): 2x(conv3x3+ReLU) -> maxpool(ceil) -> 2x(conv3x3+ReLU) -> maxpool(ceil) '''

    def __init__(self, input_dim):
        super().__init__()
        self.init_dim, self.hide_dim, self.ceil_mode = 128, 256, True
        self.in_channel, self.freq_dim, self.out_dim = self.check_dim(input_dim)
        self.dp, self.bucket = None, None
        self.extractor = nn.Sequential(
            nn.Conv2d(self.in_channel, self.init_dim, 3, stride=1, padding=1), nn.ReLU(),
            nn.Conv2d(self.init_dim, self.init_dim, 3, stride=1, padding=1), nn.ReLU(),
            nn.MaxPool2d(2, stride=2, ceil_mode=True),
            nn.Conv2d(self.init_dim, self.hide_dim, 3, stride=1, padding=1), nn.ReLU(),
            nn.Conv2d(self.hide_dim, self.hide_dim, 3, stride=1, padding=1), nn.ReLU(),
            nn.MaxPool2d(2, stride=2, ceil_mode=True))

    def conv_layers(self):
        return [(self.extractor[i], None) for i in (0, 2, 5, 7)]


class VGGExtractor_LN(_VGGBase):
    ''' VGG + LayerNorm over frequency (reference src/module.py:582-657), floor-mode pooling '''

    def __init__(self, input_dim):
        super().__init__()
        self.init_dim, self.hide_dim, self.ceil_mode = 64, 128, False
        self.in_channel, self.freq_dim, self.out_dim = self.check_dim(input_dim)
        self.upstream = False
        self.dp, self.bucket = None, None
        n = FBANK_SIZE
        self.extractor = nn.Sequential(
            nn.Conv2d(self.in_channel, self.init_dim, 3, stride=1, padding=1), CNNLayerNorm(n), nn.ReLU(),
            nn.Conv2d(self.init_dim, self.init_dim, 3, stride=1, padding=1), CNNLayerNorm(n), nn.ReLU(),
            nn.MaxPool2d(2, stride=2),
            nn.Conv2d(self.init_dim, self.hide_dim, 3, stride=1, padding=1), CNNLayerNorm(n // 2), nn.ReLU(),
            nn.Conv2d(self.hide_dim, self.hide_dim, 3, stride=1, padding=1), CNNLayerNorm(n // 2), nn.ReLU(),
            nn.MaxPool2d(2, stride=2))

    def conv_layers(self):
        return [(self.extractor[i], self.extractor[i + 1].layer_norm) for i in (0, 3, 7, 10)]


class VGGExtractor2(_VGGBase):
    """VGG extractor that halves time once (reference src/module.py:843-905): 64 / 128 channels, floor-mode 2 x 2 pooling,
    then MaxPool2d((1, 2)) - frequency only."""

    def __init__(self, input_dim):
        super().__init__()
        self.init_dim, self.hide_dim, self.ceil_mode = 64, 128, False
        self.time_div, self.pool2_freq_only = 2, True
        self.in_channel, self.freq_dim, self.out_dim = self.check_dim(input_dim)
        self.dp, self.bucket = None, None
        self.extractor = nn.Sequential(
            nn.Conv2d(self.in_channel, self.init_dim, 3, stride=1, padding=1), nn.ReLU(),
            nn.Conv2d(self.init_dim, self.init_dim, 3, stride=1, padding=1), nn.ReLU(),
            nn.MaxPool2d(2, stride=2),
            nn.Conv2d(self.init_dim, self.hide_dim, 3, stride=1, padding=1), nn.ReLU(),
            nn.Conv2d(self.hide_dim, self.hide_dim, 3, stride=1, padding=1), nn.ReLU(),
            nn.MaxPool2d((1, 2), stride=(1, 2)))

    def conv_layers(self):
        return [(self.extractor[i], None) for i in (0, 2, 5, 7)]


class _Band(object):
    """One band (low / high frequencies) of a frequency-split extractor as conv_stack sees it."""

    def __init__(self, owner, seq, in_channel, f0, f1, time_div, pool2_freq_only):
        self.owner, self.seq, self.in_channel, self.freq_slice, self.freq_dim = owner, seq, in_channel, (f0, f1), f1 - f0
        self.time_div, self.pool2_freq_only, self.ceil_mode, self.dp, self.bucket = time_div, pool2_freq_only, False, None, None

    def conv_layers(self):
        return [(self.seq[i], None) for i in (0, 2, 5, 7)]


class FreqVGGExtractor(nn.Module):
    """Frequency-split VGG (reference src/module.py:746-841; `pool2_freq_only` = FreqVGGExtractor2, :907-1001): the bins below
    `split_freq` go through a narrow stack (low_dim, 2 low_dim channels), the rest through a wide one (64 - low_dim,
    128 - 2 low_dim); the two outputs are concatenated."""

    def __init__(self, input_dim, split_freq, low_dim=4, pool2_freq_only=False):
        super().__init__()
        if input_dim % FBANK_SIZE != 0:
            raise ValueError('HIP VGG front-end expects 40-bin fbank channels (input dim %d)' % input_dim)
        self.split_freq, self.in_channel, self.freq_dim = split_freq, input_dim // FBANK_SIZE, FBANK_SIZE
        assert split_freq % 4 == 0 and 0 < split_freq < self.freq_dim
        li, lh, hi, hh = low_dim, 2 * low_dim, 64 - low_dim, 128 - 2 * low_dim
        self.low_out_dim, self.high_out_dim = split_freq // 4 * lh, (self.freq_dim - split_freq) // 4 * hh
        self.out_dim = self.low_out_dim + self.high_out_dim
        self.time_div = 2 if pool2_freq_only else 4
        self.dp, self.bucket, self._bands_done = None, None, 0
        last = (lambda: nn.MaxPool2d((1, 2), stride=(1, 2))) if pool2_freq_only else (lambda: nn.MaxPool2d(2, stride=2))

        def stack(c1, c2):
            return nn.Sequential(nn.Conv2d(self.in_channel, c1, 3, stride=1, padding=1), nn.ReLU(),
                                 nn.Conv2d(c1, c1, 3, stride=1, padding=1), nn.ReLU(), nn.MaxPool2d(2, stride=2),
                                 nn.Conv2d(c1, c2, 3, stride=1, padding=1), nn.ReLU(),
                                 nn.Conv2d(c2, c2, 3, stride=1, padding=1), nn.ReLU(), last())
        self.low_extractor, self.high_extractor = stack(li, lh), stack(hi, hh)
        self._bands = (_Band(self, self.low_extractor, self.in_channel, 0, split_freq, self.time_div, pool2_freq_only),
                       _Band(self, self.high_extractor, self.in_channel, split_freq, self.freq_dim, self.time_div, pool2_freq_only))

    def forward(self, feature, feat_len, ctx=None):
        self._bands_done = 0
        lo, hi = [_ConvStackFn.apply(ctx.anchor, feature, b, ctx.prec, layout_of(self, ctx.prec)) for b in self._bands]
        return torch.cat((lo, hi), dim=-1), feat_len // self.time_div


class FreqVGGExtractor2(FreqVGGExtractor):
    def __init__(self, input_dim, split_freq, low_dim=4):
        super().__init__(input_dim, split_freq, low_dim, pool2_freq_only=True)


def layout_of(ext, prec):
    """The layout class an extractor runs in at this precision: the bordered bf16 images where csrc/vgg16.hip covers the
    extractor (vgg16_ok; it has no frequency-only pooling, and the narrow band of a frequency-split extractor is below its
    channel counts), the plain fp32 images otherwise."""
    if isinstance(ext, FreqVGGExtractor) or ext.pool2_freq_only or not vgg16_ok(ext, prec):
        return _Plain32
    return _Bordered16


def conv_time_div(ext):
    """Frames a conv extractor folds into one (it drops n % time_div trailing frames first), None for any other front-end."""
    if isinstance(ext, (_VGGBase, FreqVGGExtractor)):
        return ext.time_div
    return None


def forward_lens(ext, feature, lens, prec):
    """Inference-only pass of a conv extractor over a padded batch: conv_stack with `lens` in the layout ext.forward takes for
    this precision, both bands and the concatenation for a frequency-split extractor.  Arguments and result as conv_stack."""
    lay = layout_of(ext, prec)(prec, feature.device)
    if isinstance(ext, FreqVGGExtractor):
        (lo, out_lens), (hi, _) = [conv_stack(b, lay, feature, lens) for b in ext._bands]
        return torch.cat((lo, hi), dim=-1), out_lens
    return conv_stack(ext, lay, feature, lens)


def largest_activation_bytes(ext, T, prec):
    """Bytes of the largest single tensor forward_lens holds for ONE batch row of T frames: the first two convolutions'
    outputs (full resolution, init_dim channels; the later ones have twice the channels on a quarter of the pixels) - fp32
    (T,F,C) unbordered, bf16 (T+2,F+2,C) bordered, the latter's CNNLayerNorm pre-activations fp32."""
    lay = layout_of(ext, prec)

    def first_conv_bytes(stack):
        conv, ln = stack.conv_layers()[0]
        return lay.image_bytes(T, stack.freq_dim, conv.weight.shape[0], ln is not None)
    return max(first_conv_bytes(s) for s in (ext._bands if isinstance(ext, FreqVGGExtractor) else (ext,)))
