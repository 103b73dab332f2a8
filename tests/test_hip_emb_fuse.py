"""The embedding-regulariser kernels (csrc/emb_fuse.hip: asr_emb_fuse_fwd / _bwd, asr_emb_cos_loss, asr_row_normalize_fwd / _bwd)
on the GPU against the float64 restatements of tests/test_emb_fuse_reference.py, at its case tables.

Every output lives between two 64-element canary borders that must come back untouched; outputs start as NaN (the entry points
write, they do not accumulate) and the padding of a strided input row is NaN, so a read or a write outside a row shows.

Bounds.  Integer-valued statements are exact: the argmax (the lowest index of the largest value the kernel itself wrote, and the
known index of a constructed tie), the zero rows, the masked rows, gradients that a factor of exactly 0 removes (lambda 0 / 1,
temp <= 0).  On random inputs each output is held to
    err_kernel <= 8 * e32 + 4 * 2^-23 * max |reference|,   e32 = max |torch float32 on the CPU - float64| on the same inputs
- the factor covers a tree reduction and the device's exp / log against torch's sequential libm path - and every case prints a
RATIO line before it asserts.  The cosine gradients of a zero prediction are 1e6 times those of the other rows (1 / sqrt(1e-12)):
that row is judged on its own scale."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from test_emb_fuse_reference import (COS_CASES, FUSE_CASES, NORM_CASES, cos_inputs, cos_loss_ref, fuse_bwd_ref, fuse_case_id,
                                     fuse_fwd_ref, fuse_inputs, norm_inputs, normalize_bwd_ref, normalize_fwd_ref)

gpu = pytest.mark.gpu

ULP32 = 2.0 ** -23
K, FLOOR = 8, 4 * ULP32
CAN, SENT = 64, -777.25
F64, F32 = torch.float64, torch.float32
E_ARG = -1


def _buf(shape, dtype=F32, fill=float('nan')):
    """(whole device buffer, payload view): CAN sentinels, the payload filled with `fill`, CAN sentinels."""
    n = math.prod(shape)
    t = torch.full((n + 2 * CAN,), SENT if dtype.is_floating_point else int(SENT), dtype=dtype)
    t[CAN:CAN + n] = fill
    d = t.cuda()
    return d, d[CAN:CAN + n].view(shape)


def _back(d, shape, dtype=F64):
    c = d.cpu()
    sent = SENT if c.dtype.is_floating_point else int(SENT)
    assert (c[:CAN] == sent).all() and (c[-CAN:] == sent).all(), 'a canary border of an output was overwritten'
    return c[CAN:-CAN].view(shape).to(dtype)


def _judge(name, what, got, ref64, ref32, keep=None):
    keep = torch.ones(ref64.shape, dtype=torch.bool) if keep is None else keep.expand(ref64.shape)
    assert not torch.isnan(got).any(), '%s %s: NaN in an output the kernel must write' % (name, what)
    if not bool(keep.any()):
        return
    scale = float(ref64[keep].abs().max())
    e32 = float((ref32.double() - ref64)[keep].abs().max())
    err = float((got - ref64)[keep].abs().max())
    print('RATIO %-44s %-8s err %.3e e32 %.3e ratio %7.2f scale %.3g' % (name, what, err, e32, err / max(e32, 1e-300), scale))
    assert err <= K * e32 + FLOOR * scale, (name, what, err, e32, scale)


# ---------------------------------------------------------------------------------------------------------------------
# fusion
# ---------------------------------------------------------------------------------------------------------------------
def _fuse_torch32(dec, emb, t_raw, l_raw, sig, dout):
    d, e, t, l = (v.clone().requires_grad_(True) for v in (dec, emb, t_raw, l_raw))
    lam = torch.sigmoid(l) if sig else l
    out = ((1 - lam) * d.softmax(-1) + lam * (F.relu(t) * e).softmax(-1) + 1e-8).log()
    (out * dout).sum().backward()
    stats = torch.stack([torch.logsumexp(dec, -1), torch.logsumexp(F.relu(t_raw) * emb, -1)], -1)
    return out.detach(), stats, d.grad, e.grad, t.grad, l.grad


def _strided(x, pad):
    """x (N,V) as rows of a (N, V + pad) device matrix whose padding is NaN."""
    N, V = x.shape
    m = torch.full((N, V + pad), float('nan'))
    m[:, :V] = x
    return m.cuda()


def _run_fuse_fwd(H, dec_d, ld, emb_d, t_d, l_d, c, N, V, amax_ld=3):
    out, out_v = _buf((N, V))
    stats, stats_v = _buf((N, 2))
    amax, amax_v = _buf((N * amax_ld,), torch.int64, -5)
    H.call('asr_emb_fuse_fwd', H.ptr(dec_d), ld, H.ptr(emb_d), H.ptr(t_d), 1 if c['vec'] else 0, H.ptr(l_d), 1 if c['vec'] else 0,
           1 if c['sig'] else 0, H.ptr(out_v), H.ptr(stats_v), H.ptr(amax_v), amax_ld, N, V, H.stream_ptr())
    torch.cuda.synchronize()
    return out, stats, amax, stats_v


@gpu
@pytest.mark.parametrize('c', FUSE_CASES, ids=fuse_case_id)
def test_fuse_fwd_and_bwd(c):
    from src import hipabi as H
    name = fuse_case_id(c)
    N, V = c['N'], c['V']
    dec, emb, t_raw, l_raw, dout = fuse_inputs(c)
    ld = V + c['pad']
    dec_d, emb_d, t_d, l_d = _strided(dec, c['pad']), emb.cuda(), t_raw.cuda(), l_raw.cuda()
    out, stats, amax, stats_v = _run_fuse_fwd(H, dec_d, ld, emb_d, t_d, l_d, c, N, V)
    r_out, r_stats, _ = fuse_fwd_ref(dec, emb, t_raw, l_raw, c['sig'])
    t32 = _fuse_torch32(dec, emb, t_raw, l_raw, c['sig'], dout)
    got_out = _back(out, (N, V))
    _judge(name, 'out', got_out, r_out, t32[0])
    _judge(name, 'stats', _back(stats, (N, 2)), r_stats, t32[1])
    # argmax: the lowest index of the largest value the kernel wrote; the slots between the strided entries stay untouched
    am = _back(amax, (N, 3), torch.int64)
    top = got_out.max(-1, keepdim=True).values
    want = torch.where(got_out == top, torch.arange(V).expand(N, V), torch.full((N, V), V)).min(-1).values
    assert torch.equal(am[:, 0], want) and bool((am[:, 1:] == -5).all())
    if c['lam'] == 0.0 and not c['sig']:
        # lambda = 0: log(p_dec + 1e-8) as computed - nothing of p_emb reaches it
        c0 = dict(c, temp=-1.0, vec=False)
        out0 = _run_fuse_fwd(H, dec_d, ld, emb_d, torch.full((1,), -1.0).cuda(), l_d, c0, N, V)[0]
        assert torch.equal(_back(out0, (N, V)), got_out)

    # backward, both parameter gradients asked for
    nt, nl = (V, V) if c['vec'] else (1, 1)
    ddec, ddec_v = _buf((N, V))
    demb, demb_v = _buf((N, V))
    dtemp, dtemp_v = _buf((nt,))
    dlam, dlam_v = _buf((nl,))
    work, work_v = _buf((N * nt + N * nl,))
    dout_d = dout.cuda()
    H.call('asr_emb_fuse_bwd', H.ptr(dout_d), H.ptr(dec_d), ld, H.ptr(emb_d), H.ptr(t_d), 1 if c['vec'] else 0, H.ptr(l_d),
           1 if c['vec'] else 0, 1 if c['sig'] else 0, H.ptr(stats_v), H.ptr(ddec_v), H.ptr(demb_v), H.ptr(dtemp_v), H.ptr(dlam_v),
           H.ptr(work_v), N, V, H.stream_ptr())
    torch.cuda.synchronize()
    r = fuse_bwd_ref(dout, dec, emb, t_raw, l_raw, c['sig'])
    got = [_back(ddec, (N, V)), _back(demb, (N, V)), _back(dtemp, (nt,)), _back(dlam, (nl,))]
    _back(work, (N * nt + N * nl,), F32)
    for what, g_, r_, t_ in zip(('d_dec', 'd_emb', 'd_temp', 'd_lam'), got, r, t32[2:]):
        _judge(name, what, g_, r_, t_)
    if c['temp'] <= 0 and not c['vec']:
        assert float(got[1].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0
    if c['lam'] == 0.0 and not c['sig']:
        assert float(got[1].abs().max()) == 0.0
    if c['lam'] == 1.0 and not c['sig']:
        assert float(got[0].abs().max()) == 0.0

    # without the parameter gradients (NULL, NULL, no work area) the two logit gradients are the same bits
    ddec2, ddec2_v = _buf((N, V))
    demb2, demb2_v = _buf((N, V))
    H.call('asr_emb_fuse_bwd', H.ptr(dout_d), H.ptr(dec_d), ld, H.ptr(emb_d), H.ptr(t_d), 1 if c['vec'] else 0, H.ptr(l_d),
           1 if c['vec'] else 0, 1 if c['sig'] else 0, H.ptr(stats_v), H.ptr(ddec2_v), H.ptr(demb2_v), None, None, None, N, V,
           H.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_back(ddec2, (N, V)), got[0]) and torch.equal(_back(demb2, (N, V)), got[1])


@gpu
@pytest.mark.parametrize('V', [31, 2049])
def test_fuse_argmax_on_an_exact_tie(V):
    """Integer logits, lambda = 0: tokens 7 and 19 carry the same largest logit (and V - 1 the same in the second row) - equal
    inputs give equal outputs, so the tie is exact and the lower index must win in both kernels."""
    from src import hipabi as H
    N = 2
    dec = torch.zeros(N, V)
    dec[0, 19] = dec[0, 7] = 3.0
    dec[1, V - 1] = dec[1, 19] = 5.0
    emb = torch.randn(N, V, generator=torch.Generator().manual_seed(5))
    c = dict(vec=False, sig=False)
    out, _, amax, _ = _run_fuse_fwd(H, dec.cuda(), V, emb.cuda(), torch.ones(1).cuda(), torch.zeros(1).cuda(), c, N, V, amax_ld=1)
    assert _back(amax, (N,), torch.int64).tolist() == [7, 19]
    got = _back(out, (N, V))
    assert float(got[0, 7]) == float(got[0, 19]) and float(got[1, 19]) == float(got[1, V - 1])


@gpu
def test_fuse_refusals_write_nothing():
    from src import hipabi as H
    L = H.lib()
    N, V = 3, 31
    x = torch.randn(N, V).cuda()
    one = torch.ones(1).cuda()
    out, out_v = _buf((N, V))
    stats, stats_v = _buf((N, 2))
    sp = H.stream_ptr()
    p = H.ptr

    def fwd(dec=x, ld=V, emb=x, temp=one, lam=one, o=out_v, s=stats_v, n=N, v=V, ts=0):
        return L.asr_emb_fuse_fwd(p(dec), ld, p(emb), p(temp), ts, p(lam), 0, 0, p(o), p(s), None, 1, n, v, sp)

    def bwd(dout=x, dec=x, ld=V, emb=x, temp=one, lam=one, s=x, dd=out_v, de=out_v, dt=None, wk=None, n=N, v=V):
        return L.asr_emb_fuse_bwd(p(dout), p(dec), ld, p(emb), p(temp), 0, p(lam), 0, 0, p(s), p(dd), p(de), p(dt), None, p(wk), n, v, sp)

    for kw in (dict(dec=None), dict(emb=None), dict(temp=None), dict(lam=None), dict(o=None), dict(s=None), dict(v=1), dict(v=65537),
               dict(n=0), dict(ld=V - 1), dict(ts=2)):
        assert fwd(**kw) == E_ARG, kw
    for kw in (dict(dout=None), dict(dec=None), dict(s=None), dict(dd=None), dict(de=None), dict(v=1), dict(v=65537), dict(n=0),
               dict(ld=V - 1), dict(dt=one, wk=None)):
        assert bwd(**kw) == E_ARG, kw
    assert b'asr_emb_fuse_bwd' in L.asr_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(_back(out, (N, V))).all() and torch.isnan(_back(stats, (N, 2))).all()


# ---------------------------------------------------------------------------------------------------------------------
# cosine embedding loss
# ---------------------------------------------------------------------------------------------------------------------
def _cos_torch32(x, table, label):
    B, L = label.shape
    E = x.shape[-1]
    xt = x.clone().requires_grad_(True)
    yt = table[label].clone().requires_grad_(True)
    per = F.cosine_embedding_loss(xt.view(-1, E), yt.view(-1, E), torch.ones(1), reduction='none').view(B, L)
    per = torch.where(label != 0, per, torch.zeros_like(per))
    cnt = (label != 0).sum(-1)
    keep = cnt > 0
    loss = (per.sum(-1)[keep] / cnt[keep].float()).sum() / B
    loss.backward()
    return loss.detach(), xt.grad, yt.grad


@gpu
@pytest.mark.parametrize('B,L,E,V', COS_CASES)
def test_cos_loss(B, L, E, V):
    from src import hipabi as H
    name = 'cos B%d L%d E%d V%d' % (B, L, E, V)
    x, table, label = cos_inputs(B, L, E, V)
    ld = L + 2                                         # a label matrix wider than L
    lab = torch.full((B, ld), 3, dtype=torch.int64)
    lab[:, :L] = label
    xd, td, labd = x.cuda(), table.cuda(), lab.cuda()
    r_loss, r_dx, r_dy = cos_loss_ref(x, table, label)
    t_loss, t_dx, t_dy = _cos_torch32(x, table, label)
    zero_x = (x == 0).all(-1, keepdim=True)
    for with_dy in (True, False):
        loss, loss_v = _buf((1,))
        dx, dx_v = _buf((B, L, E))
        dy, dy_v = _buf((B, L, E))
        rl, rl_v = _buf((B * L,))
        H.call('asr_emb_cos_loss', H.ptr(xd), H.ptr(td), H.ptr(labd), ld, H.ptr(loss_v), H.ptr(dx_v), H.ptr(dy_v) if with_dy else None,
               H.ptr(rl_v), B, L, E, V, H.stream_ptr())
        torch.cuda.synchronize()
        _back(rl, (B * L,), F32)
        _judge(name, 'loss', _back(loss, (1,)), r_loss.reshape(1), t_loss.reshape(1))
        g_dx = _back(dx, (B, L, E))
        _judge(name, 'dx', g_dx, r_dx, t_dx, ~zero_x)
        _judge(name, 'dx zero', g_dx, r_dx, t_dx, zero_x)
        # the utterance without a label and the pad position: exactly zero
        assert float(g_dx[B - 1].abs().max()) == 0.0 and float(g_dx[0, L - 1].abs().max()) == 0.0
        if with_dy:
            g_dy = _back(dy, (B, L, E))
            _judge(name, 'dy', g_dy, r_dy, t_dy)
            assert float(g_dy[B - 1].abs().max()) == 0.0 and float(g_dy[0, L - 1].abs().max()) == 0.0
            # two rows carry the same label: asr_embedding_bwd adds both into the table's row, on top of what is there
            init = torch.randn(V, E, generator=torch.Generator().manual_seed(9))
            dtab, dtab_v = _buf((V, E), fill=0.0)
            dtab_v.copy_(init)
            H.call('asr_embedding_bwd', H.ptr(dy_v), E, H.ptr(labd[:, :L].contiguous()), H.ptr(dtab_v), B * L, E, V, H.stream_ptr())
            torch.cuda.synchronize()
            want = init.double().index_add(0, label.reshape(-1), g_dy.reshape(-1, E))
            got = _back(dtab, (V, E))
            assert int((label == label[0, 0]).sum()) >= 2
            assert float((got - want).abs().max()) <= 4 * ULP32 * max(1.0, float(want.abs().max()))
        else:
            assert torch.isnan(_back(dy, (B, L, E))).all()


@gpu
def test_cos_loss_refusals_write_nothing():
    from src import hipabi as H
    L_ = H.lib()
    B, L, E, V = 2, 3, 7, 11
    x, tab, lab = torch.randn(B * L, E).cuda(), torch.randn(V, E).cuda(), torch.ones(B, L, dtype=torch.int64).cuda()
    loss, loss_v = _buf((1,))
    dx, dx_v = _buf((B * L, E))
    rl, rl_v = _buf((B * L,))
    p, sp = H.ptr, H.stream_ptr()

    def run(x_=x, t=tab, l=lab, ld=L, lo=loss_v, d=dx_v, r=rl_v, b=B, ll=L, e=E, v=V):
        return L_.asr_emb_cos_loss(p(x_), p(t), p(l), ld, p(lo), p(d), None, p(r), b, ll, e, v, sp)

    for kw in (dict(x_=None), dict(t=None), dict(l=None), dict(lo=None), dict(d=None), dict(r=None), dict(e=0), dict(b=0), dict(ll=0),
               dict(v=1), dict(v=65537), dict(ld=L - 1)):
        assert run(**kw) == E_ARG, kw
    torch.cuda.synchronize()
    assert torch.isnan(_back(loss, (1,))).all() and torch.isnan(_back(dx, (B * L, E))).all() and torch.isnan(_back(rl, (B * L,))).all()


# ---------------------------------------------------------------------------------------------------------------------
# row normalisation
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('N,E', NORM_CASES)
def test_row_normalize(N, E):
    from src import hipabi as H
    name = 'normalize N%d E%d' % (N, E)
    x, dy = norm_inputs(N, E)
    xd, dyd = x.cuda(), dy.cuda()
    y, y_v = _buf((N, E))
    dx, dx_v = _buf((N, E))
    H.call('asr_row_normalize_fwd', H.ptr(xd), H.ptr(y_v), N, E, H.stream_ptr())
    H.call('asr_row_normalize_bwd', H.ptr(dyd), H.ptr(xd), H.ptr(dx_v), N, E, H.stream_ptr())
    torch.cuda.synchronize()
    xt = x.clone().requires_grad_(True)
    t_y = F.normalize(xt, dim=-1)
    (t_y * dy).sum().backward()
    zero = (x == 0).all(-1, keepdim=True)
    tiny = torch.zeros(N, 1, dtype=torch.bool)
    tiny[2] = True
    g_y, g_dx = _back(y, (N, E)), _back(dx, (N, E))
    _judge(name, 'y', g_y, normalize_fwd_ref(x), t_y.detach(), ~tiny)
    _judge(name, 'dx', g_dx, normalize_bwd_ref(dy, x), xt.grad, ~(zero | tiny))
    # the zero row stays zero and gets a zero gradient; the row of norm 1e-20 is x / 1e-12 with dx = dy / 1e-12: one rounding
    assert float(g_y[1].abs().max()) == 0.0 and float(g_dx[1].abs().max()) == 0.0
    eps32 = float(torch.tensor(1e-12, dtype=F32))
    assert float((g_y[2] - x[2].double() / eps32).abs().max()) <= ULP32 * 1e-8
    assert float((g_dx[2] - dy[2].double() / eps32).abs().max()) <= ULP32 * float(dy[2].abs().max()) / eps32


@gpu
def test_row_normalize_refusals_write_nothing():
    from src import hipabi as H
    L_ = H.lib()
    x = torch.randn(4, 7).cuda()
    y, y_v = _buf((4, 7))
    p, sp = H.ptr, H.stream_ptr()
    assert L_.asr_row_normalize_fwd(None, p(y_v), 4, 7, sp) == E_ARG and L_.asr_row_normalize_fwd(p(x), None, 4, 7, sp) == E_ARG
    assert L_.asr_row_normalize_fwd(p(x), p(y_v), 0, 7, sp) == E_ARG and L_.asr_row_normalize_fwd(p(x), p(y_v), 4, 0, sp) == E_ARG
    assert L_.asr_row_normalize_bwd(None, p(x), p(y_v), 4, 7, sp) == E_ARG and L_.asr_row_normalize_bwd(p(x), None, p(y_v), 4, 7, sp) == E_ARG
    assert L_.asr_row_normalize_bwd(p(x), p(x), None, 4, 7, sp) == E_ARG and L_.asr_row_normalize_bwd(p(x), p(x), p(y_v), 4, 0, sp) == E_ARG
    assert L_.asr_row_normalize_bwd(p(x), p(x), p(y_v), 0, 7, sp) == E_ARG
    torch.cuda.synchronize()
    assert torch.isnan(_back(y, (4, 7))).all()
