"""One training step on the HIP path: forward -> CTC + attention losses -> backward -> [gradient all-reduce] -> global-norm clip
+ NaN guard + Adadelta, the sequence bin/train_asr.py:200-253 + src/solver.py:88-106 of the reference runs.  bench.py runs it as
train_step; the Solver runs its halves, forward_losses and backward_update, with its timer between (bin/train_asr.py)."""
import torch


def train_step(model, optimizer, ctc_crit, att_crit, feat, feat_len, txt, decode_step, tf_rate=1.0, dp=None,
               clip=5.0, txt_len=None, optimize=True, emb_decoder=None, emb_optimizer=None):
    """Returns dict(total_loss, ctc_loss, att_loss, grad_normsq (device float64 scalar)).  No host sync.
    emb_decoder: an enabled src.plugin.EmbeddingRegularizer - its loss joins the total with its weight and, when it fuses, its
    output replaces the decoder's in the sequence loss (reference bin/train_asr.py:215-222); emb_optimizer steps its parameters."""
    from src import hipabi as H
    cur = torch.cuda.current_stream()
    if not (feat.is_cuda and H.step_overlaps(dp)) or cur != torch.cuda.default_stream():
        return _train_step(model, optimizer, ctc_crit, att_crit, feat, feat_len, txt, decode_step, tf_rate, dp, clip, txt_len, optimize,
                           emb_decoder, emb_optimizer)
    with H.on_work_stream():           # see work_stream's docstring: the CU-masked streams serialise against the default stream
        out = _train_step(model, optimizer, ctc_crit, att_crit, feat, feat_len, txt, decode_step, tf_rate, dp, clip, txt_len, optimize,
                          emb_decoder, emb_optimizer)
    for v in out.values():
        if torch.is_tensor(v):
            v.record_stream(cur)
    return out


def step_emb_optimizer(emb_optimizer, model_normsq, grad_mul=1.0):
    """The plugin's parameters step beside the model's: the reference clips the MODEL's gradient norm only and skips the whole
    update when that norm is not finite (src/solver.py:97-103), so the plugin's fused step reads the model's norm for the NaN
    guard and does not clip."""
    eo = emb_optimizer.opt if hasattr(emb_optimizer, 'opt') else emb_optimizer
    eo.normsq = model_normsq
    eo.step(clip=0.0, grad_mul=grad_mul, use_norm=True)


def scale_weight(w_dev, k):
    """k * w_dev for a one-element device tensor (asr_loss_mix with a host constant as the second factor)."""
    from src import hipabi as H
    from src.functions import loss_weight
    if not torch.is_tensor(w_dev):
        return loss_weight(float(w_dev) * k, torch.device('cuda', torch.cuda.current_device()))
    w = w_dev.reshape(1).to(torch.float32).contiguous()
    out = torch.empty(1, dtype=torch.float32, device=w.device)
    H.call('asr_loss_mix', H.ptr(w), H.ptr(loss_weight(k, w.device)), None, None, H.ptr(out), H.stream_ptr())
    return out


def _train_step(model, optimizer, ctc_crit, att_crit, feat, feat_len, txt, decode_step, tf_rate=1.0, dp=None,
                clip=5.0, txt_len=None, optimize=True, emb_decoder=None, emb_optimizer=None):
    opt = optimizer.opt if hasattr(optimizer, 'opt') else optimizer
    opt.zero_grad()
    if txt_len is None:
        txt_len = torch.sum(txt != 0, dim=-1)
    if emb_decoder is not None:
        emb_decoder.zero_grad()
    out = forward_losses(model, ctc_crit, att_crit, feat, feat_len, txt, decode_step, tf_rate, dp, txt_len, emb_decoder)
    normsq, grad_mul = backward_update(out['total_loss'], opt, dp, clip, optimize, emb_optimizer)
    out.update(total_loss=out['total_loss'].detach(), grad_normsq=normsq, grad_mul=grad_mul)
    return out


def forward_losses(model, ctc_crit, att_crit, feat, feat_len, txt, decode_step, tf_rate, dp, txt_len, emb_decoder=None):
    """Model call, the losses and their mix.  Returns dict(total_loss - still attached to its graph, for backward_update -
    ctc_loss, att_loss, emb_loss, ctc_output, att_output - the plugin's when it fuses - att_align, encode_len).  Zeroes no gradient."""
    from src import hipabi as H
    if emb_decoder is None:
        ctc_output, encode_len, att_output, att_align, _ = model(feat, feat_len, decode_step, tf_rate=tf_rate, teacher=txt, ctc_async=True)
        emb_loss = None
    else:
        if getattr(emb_decoder, 'apply_fuse', False) and tf_rate != 1:
            raise ValueError('embedding fusion cannot be combined with scheduled sampling (tf_rate = %r < 1): the fused output is a '
                             'log-probability, which the reference hands to Categorical as logits and fails' % (tf_rate,))
        ctc_output, encode_len, att_output, att_align, dec_state = model(feat, feat_len, decode_step, tf_rate=tf_rate, teacher=txt,
                                                                         ctc_async=True, get_dec_state=True)
        emb_loss, fuse_output = emb_decoder(dec_state, att_output, label=txt[:, :att_output.shape[1]])
        if fuse_output is not None:
            att_output = fuse_output
    total, ctc_loss, att_loss = None, None, None
    from src.functions import LossMixFn, loss_weight
    dev = feat.device
    if ctc_output is not None:
        if getattr(ctc_output, '_asr_side', False):       # the CTC branch lives on the side stream (ASR.forward): loss there too
            with H.side_branch(False, txt, txt_len):
                ctc_loss = ctc_crit(ctc_output.transpose(0, 1), txt, encode_len, txt_len)
            H.join_branch(ctc_loss, ctc_output)
        else:
            ctc_loss = ctc_crit(ctc_output.transpose(0, 1), txt, encode_len, txt_len)
    w_att = None
    if att_output is not None:
        b, t, _ = att_output.shape
        att_loss = att_crit(att_output.view(b * t, -1), txt[:, :t].reshape(-1))
        if dp is not None and dp.world > 1:
            # exact global token-mean under data parallelism: the factor is a device scalar out of an all-reduce
            w_att = scale_weight(dp.ce_weight(txt_len.sum()), 1 - model.ctc_weight)
        else:
            w_att = loss_weight(1 - model.ctc_weight, dev)
    # total = w ctc + (1 - w) att (bin/train_asr.py:238,246): one one-thread kernel forward, one per branch backward
    if ctc_loss is not None and att_loss is not None:
        total = LossMixFn.apply(ctc_loss, loss_weight(model.ctc_weight, dev), att_loss, w_att)
    elif ctc_loss is not None:
        total = LossMixFn.apply(ctc_loss, loss_weight(model.ctc_weight, dev), None, None)
    else:
        total = LossMixFn.apply(att_loss, w_att, None, None)
    if emb_loss is not None:                # total += emb.weight * emb_loss (bin/train_asr.py:218)
        total = LossMixFn.apply(total, loss_weight(1.0, dev), emb_loss, loss_weight(emb_decoder.weight, dev))
    return {'total_loss': total, 'ctc_loss': ctc_loss, 'att_loss': att_loss, 'emb_loss': emb_loss, 'ctc_output': ctc_output,
            'att_output': att_output, 'att_align': att_align, 'encode_len': encode_len}


def backward_update(total, opt, dp=None, clip=5.0, optimize=True, emb_optimizer=None):
    """total.backward(), the joins, [gradient all-reduce], the gradient norm and - with `optimize` - the fused step of `opt` (the
    flat optimizer itself, src/optim.py) and of the plugin's.  Returns (normsq - a device float64 scalar - , grad_mul)."""
    from src import hipabi as H
    total.backward()
    H.join_side()          # side-stream work of the step (parameter gradients, CTC branch): a no-op when the engine callback ran
    grad_mul = 1.0
    if dp is not None:
        dp.finish()
        grad_mul = dp.grad_mul
    normsq = opt.grad_norm()
    if optimize:
        opt.step(clip=clip, grad_mul=grad_mul, use_norm=True)
        if emb_optimizer is not None:
            step_emb_optimizer(emb_optimizer, normsq, grad_mul)
    return normsq, grad_mul
