"""asr_conv3x3 - the implicit-GEMM 3x3 convolution over unbordered fp32 channel-last images (conv_tap and the conv branch of
fetch_tile in csrc/gemm.hip) - held element by element to the float64 restatement of tests/test_conv3x3_reference.py at its
tap, seam, k-step, tile and slice edges, through the C entry point.

Each case asserts first, through asr_conv3x3_plan on the REAL device addresses, the tiles, slices and loaders its table entry
names.  A written output starts as NaN, an accumulated one as its integer C0, with a guard row of a sentinel above and below;
the image has NaN guard pixels before and after it (a tap that leaves the image in t must read nothing), the second operand
NaN before and after, and the slack in front of a base that is offset from a 16-byte boundary is NaN too - and the WHOLE output
buffer is compared, so a store outside the matrix fails like a wrong element inside.  Exact cases must equal the reference;
rounded cases are held to the per-element bound of the reference module and print the largest error / bound as a RATIO line.
Both precisions run every case.

Then one layer through src/vgg.py::_Plain32 (conv, act_bwd, param_grads, input_grad) on the integer recipe against float64
conv2d + ReLU and its autograd - equal for y, dx, dW and db, which fixes the wiring of the three weight-permute modes to the
three calls - and the refusals of the entry point: return code, asr_last_error naming asr_conv3x3, output still all-sentinel.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as tF

import test_conv3x3_reference as R
from test_gemm_reference import BF16, F32, NONE, RELU, SENTINEL

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = -1, -3


def run_case(c):
    """Runs one case on the GPU.  Returns (None or a description of the failure, largest error / bound of a rounded case)."""
    from src import hipabi as H
    img, op2, bias, out0, ref, tol, S = R.expected(c)
    up = lambda a: torch.tensor(a, dtype=torch.float32).cuda()
    it, ot, ct = up(img), up(op2), up(out0)
    bt = up(bias) if bias is not None else None
    ptrs = (it.data_ptr(), ot.data_ptr(), ct.data_ptr(), bt.data_ptr() if bt is not None else 0)
    assert all(p % 16 == 0 for p in ptrs)
    bad = R.plan_mismatch(c, ptrs)
    if bad:
        return 'plan ' + bad, 0.0
    H.call('asr_conv3x3', *R.abi_args(c, *ptrs), H.stream_ptr())
    torch.cuda.synchronize()
    got = ct.cpu().double().numpy()
    assert np.isfinite(ref).all(), R.cid(c)
    if tol is None:
        wrong, ratio = ~(got == ref), 0.0
    else:
        err = np.abs(got - ref)
        wrong = ~(err <= tol)
        ratio = float(np.nanmax(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), 0.0)))
    if not wrong.any():
        return None, ratio
    g = R.geometry(c)
    idx, ld = np.flatnonzero(wrong), g['out_shape'][1]
    where = ['[row %d col %d] got %r want %r%s' % ((int(f) - g['out_base']) // ld, (int(f) - g['out_base']) % ld, float(got[f]), float(ref[f]),
                                                  '' if tol is None else ' bound %.3g' % tol[f]) for f in idx[:6]]
    return '%s: %d wrong of %d (rows/cols relative to the output; outside the matrix = guard): %s' % (R.cid(c), idx.size, got.size, '; '.join(where)), ratio


def _check(c):
    bad, ratio = run_case(c)
    if not c.exact:
        print('RATIO asr_conv3x3 %s %.4f' % (R.cid(c), ratio))
    assert bad is None, bad


def _table(name):
    return dict(argvalues=R.TABLES[name], ids=R.ids(R.TABLES[name]))


@pytest.mark.parametrize('c', **_table('taps'))
def test_taps_and_seams(c):
    _check(c)


@pytest.mark.parametrize('c', **_table('channels'))
def test_channels(c):
    _check(c)


@pytest.mark.parametrize('c', **_table('outputs'))
def test_output_channels(c):
    _check(c)


@pytest.mark.parametrize('c', **_table('epilogue'))
def test_forward_epilogue(c):
    _check(c)


@pytest.mark.parametrize('c', **_table('dgrad'))
def test_input_gradient_form(c):
    _check(c)


@pytest.mark.parametrize('c', **_table('wgrad'))
def test_weight_gradient_and_its_slices(c):
    _check(c)


@pytest.mark.parametrize('c', **_table('alignment'))
def test_bases_off_a_16_byte_boundary(c):
    _check(c)


# ---- one layer through _Plain32 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', [F32, BF16])
@pytest.mark.parametrize('Ci,Co', [(3, 7), (4, 8)])
def test_plain32_layer_is_conv2d_relu_and_its_autograd(Ci, Co, prec):
    """conv -> act_bwd -> param_grads / input_grad of src/vgg.py::_Plain32 for one nn.Conv2d(Ci, Co) + ReLU on integers: y, dx,
    dW and db equal float64 autograd (integers up to 3 * 3 * 9 Ci + 8 forward, sums over 70 pixels backward: far below 2^24)."""
    from src import vgg
    B, T, Fq = 2, 5, 7
    g = torch.Generator().manual_seed(31 * Ci + Co)
    ints = lambda shape, lim: torch.randint(-lim, lim + 1, shape, generator=g).double()
    x, w, b, gy = ints((B, Ci, T, Fq), 3), ints((Co, Ci, 3, 3), 3), ints((Co,), 8), ints((B, Co, T, Fq), 3)
    x64, w64, b64 = (t.clone().requires_grad_(True) for t in (x, w, b))
    y64 = torch.relu(tF.conv2d(x64, w64, b64, padding=1))
    (y64 * gy).sum().backward()
    assert float((y64 == 0).double().mean()) > 0.2 and float((y64 > 0).double().mean()) > 0.2     # the ReLU gate does both

    conv = torch.nn.Conv2d(Ci, Co, 3, padding=1).cuda()
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    conv.weight.grad, conv.bias.grad = torch.zeros_like(conv.weight), torch.zeros_like(conv.bias)
    cl = lambda t: t.permute(0, 2, 3, 1).contiguous().float().cuda()
    lay = vgg._Plain32(prec, torch.device('cuda'))
    rec = {}
    x_cl = cl(x)
    y = lay.conv(0, x_cl, conv, None, B, T, Fq, rec)
    dpre = lay.act_bwd(cl(gy), rec, conv, None, B, T, Fq)
    lay.param_grads(0, rec['x'], dpre, conv, None, B, T, Fq)
    dx = lay.input_grad(dpre, conv, B, T, Fq)
    torch.cuda.synchronize()
    back = lambda t: t.cpu().double().permute(0, 3, 1, 2)
    assert torch.equal(back(y), y64.detach()), 'y'
    assert torch.equal(back(dx), x64.grad), 'dx'
    assert torch.equal(conv.weight.grad.cpu().double(), w64.grad), 'dW'
    assert torch.equal(conv.bias.grad.cpu().double(), b64.grad), 'db'


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _refusal_buffers():
    sent = lambda n: torch.full((n,), SENTINEL, dtype=torch.float32).cuda()
    return dict(img=torch.ones(2 * 5 * 7 * 4).cuda(), op2=torch.ones(70 * 8).cuda(), out=sent(70 * 8 + 16), bias=torch.ones(8).cuda())


REFUSALS = [
    ('mode2', dict(mode=2), E_ARG), ('mode-1', dict(mode=-1), E_ARG), ('prec5', dict(prec=5), E_ARG), ('act7', dict(act=7), E_ARG),
    ('accum2', dict(accum=2), E_ARG),
    ('wgrad_accum0', dict(mode=1, accum=0, bias=None), E_ARG), ('wgrad_act', dict(mode=1, accum=1, act=RELU, bias=None), E_ARG),
    ('wgrad_bias', dict(mode=1, accum=1), E_ARG),
    ('null_img', dict(img=None), E_ARG), ('null_w', dict(op2=None), E_ARG), ('zero_T', dict(T=0), E_ARG), ('zero_C', dict(C=0), E_ARG),
    ('zero_N', dict(N=0), E_ARG),
    # one-element buffers would do: the pixel count is checked in 64-bit arithmetic in front of the plan and the launch
    ('2^31_pixels', dict(B=32768, T=32768, F=2), E_UNSUPPORTED),
]


@pytest.mark.parametrize('name,change,code', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_launch_nothing(name, change, code):
    from src import hipabi as H
    lib = H.lib()
    buf = _refusal_buffers()
    a = dict(img=buf['img'], op2=buf['op2'], out=buf['out'], bias=buf['bias'], B=2, T=5, F=7, C=4, N=8, mode=0, act=NONE, accum=0, prec=F32)
    a.update(change)
    args = [H.ptr(a[k]) for k in ('img', 'op2', 'out', 'bias')] + [a[k] for k in ('B', 'T', 'F', 'C', 'N', 'mode', 'act', 'accum', 'prec')]
    plan = (ctypes.c_int * 8)(*([-7] * 8))
    assert lib.asr_conv3x3_plan(*args, plan) == code and list(plan) == [-7] * 8
    rc = lib.asr_conv3x3(*args, H.stream_ptr())
    last = lib.asr_last_error().decode()
    torch.cuda.synchronize()
    assert rc == code, (rc, last)
    assert 'asr_conv3x3' in last, last
    assert bool((buf['out'].cpu() == SENTINEL).all()), 'the refused call wrote its output'


def test_null_output_is_refused():
    from src import hipabi as H
    buf = _refusal_buffers()
    rc = H.lib().asr_conv3x3(H.ptr(buf['img']), H.ptr(buf['op2']), None, H.ptr(buf['bias']), 2, 5, 7, 4, 8, 0, NONE, 0, F32, H.stream_ptr())
    assert rc == E_ARG and 'asr_conv3x3' in H.lib().asr_last_error().decode()
