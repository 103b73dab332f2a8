"""Float64 restatement, operands and case table of asr_conv3x3 - the implicit-GEMM 3x3 convolution over unbordered fp32
channel-last images (conv_tap and the conv branch of fetch_tile in csrc/gemm.hip, driven by src/vgg.py::_Plain32) - and the CPU
half of its test.  tests/test_hip_conv3x3_vs_float64.py runs the same table on the GPU.

The contract (include/asr_hip.h), img (B,T,F,C), tap = 3 (dt+1) + (df+1), a tap that leaves the image in t or f reads zero:
  mode 0   out[(b,t,f), n] (+)= act( sum_{tap,ci} img[(b,t+dt,f+df), ci] w[n][tap*C+ci] + bias[n] ), accumulation order C0 + act(..)
  mode 1   dw[n][tap*C+ci] += sum_pixels dout[pixel, n] img[pixel + tap, ci]
conv_reference says that with a zero-padded numpy image and nine shifted slices, knows nothing of the kernel, and is checked
here against float64 torch.nn.functional.conv2d and its autograd through the weight copies of asr_conv_weight_permute
(test_vgg16_kernels_reference.pack_unrounded for modes 0 and 1, unpack_mode0 for the way back, mode 2): the three calls a layer
makes are nn.Conv2d's forward, input gradient and weight gradient.

Operands and bounds are those of tests/test_gemm_reference.py (bf16_round, bound, SENTINEL are imported, nothing is derived
anew):
  EXACT    image, weights and dout integers in {-3..3}, bias and C0 integers in [-8, 8]: every partial sum is an integer below
           2^24 (max S asserted per case), so fp32 accumulation in any order, atomics included, is exact and the kernel must
           EQUAL the reference in both precisions.
  ROUNDED  standard normals, the second operand (weights; dout for mode 1) scaled by K^-1/2, K the reduction length (9 C for mode
           0, B T F for mode 1); |got - ref| <= 2 (K+2) 2^-24 S (+ 2e-6 where tanh is applied), with S = sum|terms| + |bias| +
           |C0| and, in BF16 mode, ref the product of bf16_round of the fp32 operands.  K <= 640, that module's limit: a lost
           8-element chunk must stand ten times above the bound, which is asserted here on the reference alone by dropping one.
           Reduction slices above 640 pixels are therefore EXACT only.

Every case names the plan it expects - asr_conv3x3_plan is the only thing this file takes from the code under test: nx, ny, nz,
the convolution operand on the masked loader (fastA = 0 for mode 0, fastB = 0 for mode 1) and the other operand on the
unconditional 16-byte loader exactly when its base is 16-byte aligned and its contiguous extent a multiple of 4.
"""
import collections
import ctypes
import functools
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as tF

import test_vgg16_kernels_reference as V
from test_gemm_reference import BF16, F32, LIB_PATH, NONE, RELU, SENTINEL, TANH, bf16_round, bound

TAPS = [(dt, df) for dt in (-1, 0, 1) for df in (-1, 0, 1)]          # tap = 3 (dt+1) + (df+1)
PRECS = [F32, BF16]
PLAN_KEYS = ('fastA', 'fastB', 'plain_order', 'nx', 'ny', 'nz', 'gx', 'ngx')
FAKE = {'img': 0x10000000, 'op2': 0x20000000, 'out': 0x30000000, 'bias': 0x40000000}   # device allocations are 256-byte aligned


# ---- the float64 restatement -------------------------------------------------------------------------------------------
def patches(img):
    """(B,T,F,C) -> (B*T*F, 9C)[pixel][tap*C+ci]: nine shifted slices of the zero-padded image."""
    B, T, F, C = img.shape
    pad = np.zeros((B, T + 2, F + 2, C))
    pad[:, 1:T + 1, 1:F + 1] = img
    return np.concatenate([pad[:, 1 + dt:1 + dt + T, 1 + df:1 + df + F].reshape(B * T * F, C) for dt, df in TAPS], axis=1)


def conv_reference(img, op2, out0, bias, mode, act=NONE, accum=0, drop=None):
    """The whole contract in float64.  img (B,T,F,C) holds the exact values the kernel multiplies; mode 0: op2 = w (N, 9C),
    out0 (B*T*F, N); mode 1: op2 = dout (B*T*F, N), out0 = dw before the call (N, 9C).  Returns (result, S) with
    S = sum|terms| + |bias| + |C0|.  drop = (lo, hi): those indices of the reduction are left out (the dropped-chunk check)."""
    P = patches(img)
    if mode == 0:
        a, b = P, op2.T                        # (rows, K) (K, N)
    else:
        a, b = op2.T, P                        # (N, rows) (rows, 9C)
    if drop is not None:
        a = a.copy()
        a[:, drop[0]:drop[1]] = 0.0
    s, mag = a @ b, np.abs(a) @ np.abs(b)
    if bias is not None:
        s, mag = s + bias[None, :], mag + np.abs(bias)[None, :]
    if act == TANH:
        s = np.tanh(s)
    elif act == RELU:
        s = np.maximum(s, 0.0)
    if accum:
        s, mag = out0 + s, mag + np.abs(out0)
    return s, mag


# ---- cases -------------------------------------------------------------------------------------------------------------
_FIELDS = dict(name='', B=1, T=1, F=1, C=4, N=8, mode=0, prec=BF16, act=NONE, bias=1, accum=0, exact=1, img_off=0, op2_off=0,
               dgrad=0, nz=1)
Case = collections.namedtuple('Case', list(_FIELDS))


def mk(**kw):
    d = dict(_FIELDS)
    d.update(kw)
    if d['mode'] == 1:
        d.update(bias=0, accum=1)
    return Case(**d)


def cid(c):
    return '%s_%s_p%d' % (c.name, 'x' if c.exact else 'r', c.prec)


def reduction(c):
    return 9 * c.C if c.mode == 0 else c.B * c.T * c.F


def want_plan(c):
    """The plan entries the case's arguments must lead to (module docstring)."""
    rows, K9 = c.B * c.T * c.F, 9 * c.C
    if c.mode == 0:
        other = int(c.op2_off == 0 and K9 % 4 == 0)                       # w (N, 9C), reduction index contiguous
        return dict(fastA=0, fastB=other, nx=-(-c.N // 128), ny=-(-rows // 128), nz=1)
    other = int(c.op2_off == 0 and c.N % 4 == 0)                          # dout (rows, N), output row index contiguous
    return dict(fastA=other, fastB=0, nx=-(-K9 // 128), ny=-(-c.N // 128), nz=c.nz)


def geometry(c):
    """Element positions in the three flat buffers.  Image: guard pixels (a row of the image and two more) before and after,
    the base `img_off` floats behind a 16-byte boundary.  Second operand: eight floats before and after, base `op2_off` floats
    behind a 16-byte boundary.  Output: a guard row above and below."""
    rows, K9 = c.B * c.T * c.F, 9 * c.C
    g = dict(rows=rows, K9=K9)
    gi = -(-(c.F + 2) * c.C // 4) * 4
    g['img_base'], g['n_img'] = gi + c.img_off, gi + c.img_off + rows * c.C + gi
    g['op2_shape'] = (c.N, K9) if c.mode == 0 else (rows, c.N)
    g['op2_base'], g['n_op2'] = 8 + c.op2_off, 8 + c.op2_off + g['op2_shape'][0] * g['op2_shape'][1] + 8
    g['out_shape'] = (rows, c.N) if c.mode == 0 else (c.N, K9)
    guard = -(-g['out_shape'][1] // 8) * 8
    g['out_base'], g['n_out'] = guard, guard + g['out_shape'][0] * g['out_shape'][1] + guard
    return g


def operands(c):
    """The flat float64 buffers of a case AS UPLOADED: image and second operand (NaN wherever the call must not read), bias
    (or None) and the output before the call (SENTINEL guards; inside NaN, or the integer C0 of an accumulating call).  The
    values are fp32 values; in BF16 mode the rounded ones are not bf16-representable, so the kernel's own conversion is under
    test.  dgrad: the weights are the mode-1 copy (pack_unrounded) of a (Co = C, Ci = N, 3, 3) tensor."""
    g = geometry(c)
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    K = reduction(c)
    if c.exact:
        d1 = d2 = lambda shape: rng.integers(-3, 4, shape).astype(np.float64)
    else:
        d1 = lambda shape: rng.standard_normal(shape).astype(np.float32).astype(np.float64)
        d2 = lambda shape: (rng.standard_normal(shape) * K ** -0.5).astype(np.float32).astype(np.float64)
    img, op2 = np.full(g['n_img'], np.nan), np.full(g['n_op2'], np.nan)
    img[g['img_base']:g['img_base'] + g['rows'] * c.C] = d1(g['rows'] * c.C)
    if c.dgrad:
        w4 = d2((c.C, c.N, 3, 3))                                               # (Co, Ci, 3, 3) of the layer
        second = V.pack_unrounded(torch.from_numpy(w4), 1).numpy()               # (Ci, 9 Co) = (N, 9 C)
    else:
        second = d2(g['op2_shape'])
    op2[g['op2_base']:g['op2_base'] + second.size] = second.reshape(-1)
    bias = None
    if c.bias:
        bias = rng.integers(-8, 9, c.N).astype(np.float64) if c.exact else rng.standard_normal(c.N).astype(np.float32).astype(np.float64)
    out = np.full(g['n_out'], SENTINEL)
    n = g['out_shape'][0] * g['out_shape'][1]
    out[g['out_base']:g['out_base'] + n] = rng.integers(-8, 9, n) if c.accum else np.nan
    return img, op2, bias, out


def views(c, img, op2, out):
    g = geometry(c)
    n2, no = g['op2_shape'][0] * g['op2_shape'][1], g['out_shape'][0] * g['out_shape'][1]
    return (img[g['img_base']:g['img_base'] + g['rows'] * c.C].reshape(c.B, c.T, c.F, c.C),
            op2[g['op2_base']:g['op2_base'] + n2].reshape(g['op2_shape']),
            out[g['out_base']:g['out_base'] + no].reshape(g['out_shape']))


def multiplied(c, x):
    """The exact values the kernel multiplies: in BF16 mode the round-to-nearest-even bf16 of the fp32 operands."""
    return bf16_round(x) if c.prec == BF16 else x


_EXPECTED = {}


def expected(c, drop=None):
    """(img, op2, bias, out0, ref, tol, S) as flat buffers, computed once and shared (read-only).  tol is None for an exact
    case; ref holds SENTINEL and tol / S hold 0 outside the matrix."""
    key = c._replace(prec=F32) if c.exact else c              # integers are bf16 values: both precisions share one reference
    if drop is None and key in _EXPECTED:
        return _EXPECTED[key]
    g = geometry(c)
    img, op2, bias, out0 = operands(c)
    vi, v2, vo = views(c, img, op2, out0)
    s, mag = conv_reference(multiplied(c, vi), multiplied(c, v2), vo, bias, c.mode, c.act, c.accum, drop)
    ref, S = out0.copy(), np.zeros_like(out0)
    ref[g['out_base']:g['out_base'] + s.size], S[g['out_base']:g['out_base'] + s.size] = s.reshape(-1), mag.reshape(-1)
    tol = None if c.exact else bound(ref, S, reduction(c), False, c.act == TANH)
    res = (img, op2, bias, out0, ref, tol, S)
    for a in res:
        if a is not None:
            a.setflags(write=False)
    if drop is None:
        _EXPECTED[key] = res
    return res


def abi_args(c, p_img, p_op2, p_out, p_bias):
    """Arguments of asr_conv3x3 / asr_conv3x3_plan without the last one, from the BASE addresses of the four buffers."""
    g = geometry(c)
    return (p_img + 4 * g['img_base'], p_op2 + 4 * g['op2_base'], p_out + 4 * g['out_base'], p_bias if c.bias else None,
            c.B, c.T, c.F, c.C, c.N, c.mode, c.act, c.accum, c.prec)


# ---- the table ---------------------------------------------------------------------------------------------------------
def _both(**kw):
    """A base case in both recipes; tanh is rounded only, reductions above 640 exact only."""
    probe = mk(**kw)
    out = []
    if probe.act != TANH:
        out.append(probe)
    if reduction(probe) <= 640:
        out.append(probe._replace(exact=0))
    return out


def _taps():
    shapes = [(1, 1, 1), (1, 1, 5), (1, 3, 1), (2, 2, 2), (3, 5, 7), (1, 43, 3), (1, 32, 4)]
    return [c for B, T, F in shapes for c in _both(name='tap_%d_%d_%d' % (B, T, F), B=B, T=T, F=F, C=4, N=8, act=RELU)]


def _channels():
    out = []
    for C in (1, 3, 6, 4, 7, 8, 64):
        out += _both(name='ch_%d' % C, B=2, T=5, F=7, C=C, N=8, act=RELU)
    for C in (128, 256):
        out += _both(name='ch_%d' % C, B=1, T=3, F=5, C=C, N=8, act=RELU)
    return out


def _outputs():
    return [c for N in (1, 7, 128, 130, 256) for c in _both(name='n_%d' % N, B=2, T=5, F=7, C=4, N=N)]


def _epilogue():
    out = []
    for act in (NONE, RELU, TANH):
        for bias in (1, 0):
            for accum in (0, 1):
                out += _both(name='ep_a%d_b%d_c%d' % (act, bias, accum), B=2, T=5, F=7, C=3, N=7, act=act, bias=bias, accum=accum)
    return out


def _dgrad():
    # the input-gradient call of a Conv2d(Ci, Co): mode 0 over dout with C and N exchanged and the flipped weight copy
    return [c for Ci, Co in ((1, 128), (3, 7), (128, 256))
            for c in _both(name='dg_%d_%d' % (Ci, Co), B=2, T=4, F=5, C=Co, N=Ci, bias=0, dgrad=1)]


def _wgrad():
    out = []
    for C, N in ((1, 7), (3, 7), (4, 8), (16, 8), (16, 130)):
        out += _both(name='wg_%d_%d' % (C, N), B=2, T=5, F=7, C=C, N=N, mode=1)
    slices = [(1, 63, 65, 1), (1, 64, 64, 8), (1, 41, 100, 8), (1, 257, 255, 8), (1, 256, 256, 32), (1, 1640, 40, 32)]
    for B, T, F, nz in slices:
        out.append(mk(name='wg_px%d' % (B * T * F), B=B, T=T, F=F, C=4, N=8, mode=1, nz=nz))
    out.append(mk(name='wg_px65600_3_7', B=1, T=1640, F=40, C=3, N=7, mode=1, nz=32))
    out.append(mk(name='wg_px630', B=2, T=9, F=35, C=4, N=8, mode=1, exact=0))
    return out


def _alignment():
    out = []
    for C in (4, 8):
        for mode in (0, 1):
            for io, oo in ((1, 0), (0, 1), (1, 1)):
                out += _both(name='al_c%d_m%d_%d%d' % (C, mode, io, oo), B=2, T=5, F=7, C=C, N=8, mode=mode, img_off=io, op2_off=oo,
                             act=NONE if mode else RELU)
    return out


def _precs(cases):
    return [c._replace(prec=p) for c in cases for p in PRECS]


TABLES = {'taps': _precs(_taps()), 'channels': _precs(_channels()), 'outputs': _precs(_outputs()), 'epilogue': _precs(_epilogue()),
          'dgrad': _precs(_dgrad()), 'wgrad': _precs(_wgrad()), 'alignment': _precs(_alignment())}
ALL = [c for t in TABLES.values() for c in t]
ROUNDED = [c for c in ALL if not c.exact]
EXACT_ONCE = [c for c in ALL if c.exact and c.prec == F32]


def ids(cases):
    return [cid(c) for c in cases]


# ---- the query ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lib():
    if not os.path.exists(LIB_PATH):
        pytest.skip('libasr_hip.so is not built: run `python -c "import __graft_entry__ as g; g.build()"` first')
    lib = ctypes.CDLL(LIB_PATH)
    lib.asr_conv3x3_plan.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 9 + [ctypes.POINTER(ctypes.c_int)]
    return lib


def query(c, p_img=FAKE['img'], p_op2=FAKE['op2'], p_out=FAKE['out'], p_bias=FAKE['bias']):
    """The eight plan entries asr_conv3x3_plan gives for the case.  Host arithmetic only - the addresses are never followed."""
    out = (ctypes.c_int * 8)()
    rc = _lib().asr_conv3x3_plan(*abi_args(c, p_img, p_op2, p_out, p_bias), out)
    assert rc == 0, (cid(c), rc)
    return dict(zip(PLAN_KEYS, out))


def plan_mismatch(c, ptrs=()):
    """None when the case reaches the plan it names, else a description.  ptrs: the base addresses of real buffers."""
    got, want = query(c, *ptrs), want_plan(c)
    bad = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    return None if not bad else '%s: (got, want) %s' % (cid(c), bad)


# ---- CPU tests ---------------------------------------------------------------------------------------------------------
def test_case_names_are_unique():
    assert len(set(ids(ALL))) == len(ALL)


def _loops(img, op2, out0, bias, mode, act, accum):
    B, T, F, C = img.shape
    out = out0.copy()
    N = op2.shape[0] if mode == 0 else op2.shape[1]
    for n in range(N):
        if mode == 0:
            for b in range(B):
                for t in range(T):
                    for f in range(F):
                        s = 0.0
                        for tap, (dt, df) in enumerate(TAPS):
                            if 0 <= t + dt < T and 0 <= f + df < F:
                                for ci in range(C):
                                    s += img[b, t + dt, f + df, ci] * op2[n, tap * C + ci]
                        if bias is not None:
                            s += bias[n]
                        s = np.tanh(s) if act == TANH else (max(s, 0.0) if act == RELU else s)
                        p = (b * T + t) * F + f
                        out[p, n] = (out0[p, n] if accum else 0.0) + s
        else:
            for tap, (dt, df) in enumerate(TAPS):
                for ci in range(C):
                    s = 0.0
                    for b in range(B):
                        for t in range(T):
                            for f in range(F):
                                if 0 <= t + dt < T and 0 <= f + df < F:
                                    s += op2[(b * T + t) * F + f, n] * img[b, t + dt, f + df, ci]
                    out[n, tap * C + ci] = out0[n, tap * C + ci] + s
    return out


@pytest.mark.parametrize('B,T,F,C,N,mode,act,bias,accum', [(2, 3, 2, 2, 3, 0, TANH, 1, 1), (1, 1, 1, 3, 2, 0, RELU, 1, 0),
                                                           (2, 1, 3, 1, 2, 0, NONE, 0, 0), (2, 3, 2, 2, 3, 1, NONE, 0, 1),
                                                           (1, 1, 4, 3, 1, 1, NONE, 0, 1)])
def test_reference_against_loops(B, T, F, C, N, mode, act, bias, accum):
    rng = np.random.default_rng(7 + B + T + F + C + N)
    img = rng.standard_normal((B, T, F, C))
    op2 = rng.standard_normal((N, 9 * C) if mode == 0 else (B * T * F, N))
    out0 = rng.standard_normal((B * T * F, N) if mode == 0 else (N, 9 * C))
    bv = rng.standard_normal(N) if bias else None
    got, S = conv_reference(img, op2, out0, bv, mode, act, accum)
    assert np.allclose(got, _loops(img, op2, out0, bv, mode, act, accum), rtol=1e-13, atol=1e-13)
    absed, _ = conv_reference(np.abs(img), np.abs(op2), np.abs(out0), None if bv is None else np.abs(bv), mode, NONE, accum)
    assert np.allclose(S, absed, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize('B,T,F,Ci,Co', [(1, 1, 1, 1, 1), (2, 3, 4, 3, 7), (2, 1, 5, 4, 2), (3, 4, 1, 2, 5), (1, 5, 6, 8, 3)])
def test_three_calls_are_conv2d_forward_input_gradient_and_weight_gradient(B, T, F, Ci, Co):
    """With the copies asr_conv_weight_permute makes (modes 0, 1 and back by 2), the restatement of the three calls a layer makes
    is float64 nn.Conv2d: forward, input gradient (this pins the flip of the mode-1 copy) and weight gradient."""
    g = V.gen(900 + B + T + F + Ci + Co)
    x = torch.randn(B, Ci, T, F, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(Co, Ci, 3, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    bias = torch.randn(Co, generator=g, dtype=torch.float64)
    dy = torch.randn(B, Co, T, F, generator=g, dtype=torch.float64)
    y = tF.conv2d(x, w, bias, padding=1)
    (y * dy).sum().backward()
    cl = lambda t: t.detach().permute(0, 2, 3, 1).contiguous().numpy()          # (B, C, T, F) -> channel-last
    rows = B * T * F
    fwd, _ = conv_reference(cl(x), V.pack_unrounded(w.detach(), 0).numpy(), np.zeros((rows, Co)), bias.numpy(), 0)
    assert np.allclose(fwd, cl(y).reshape(rows, Co), rtol=1e-12, atol=1e-12)
    dx, _ = conv_reference(cl(dy), V.pack_unrounded(w.detach(), 1).numpy(), np.zeros((rows, Ci)), None, 0)
    assert np.allclose(dx, cl(x.grad).reshape(rows, Ci), rtol=1e-12, atol=1e-12)
    dw, _ = conv_reference(cl(x), cl(dy).reshape(rows, Co), np.zeros((Co, 9 * Ci)), None, 1)
    assert np.allclose(V.unpack_mode0(torch.from_numpy(dw), Co, Ci).numpy(), w.grad.numpy(), rtol=1e-12, atol=1e-12)
    if (B, T, F) != (1, 1, 1) and (T > 1 and F > 1):
        # an unflipped copy is NOT the input gradient: the check above can tell
        unflipped = V.pack_unrounded(w.detach().flip(2, 3), 1).numpy()
        bad, _ = conv_reference(cl(dy), unflipped, np.zeros((rows, Ci)), None, 0)
        assert not np.allclose(bad, cl(x.grad).reshape(rows, Ci), rtol=1e-6, atol=1e-6)


DGRAD_SMALL = [c for c in TABLES['dgrad'] if c.prec == F32 and c.exact]


@pytest.mark.parametrize('c', DGRAD_SMALL, ids=ids(DGRAD_SMALL))
def test_dgrad_cases_are_input_gradients(c):
    """The table's input-gradient cases carry the mode-1 copy: their reference is conv2d's input gradient for the layer's
    (Co, Ci, 3, 3) weight, recovered from the copy by the inverse of the documented rule."""
    img, op2, bias, out0, ref, tol, S = expected(c)
    vi, v2, vo = views(c, img, op2, ref)
    Co, Ci = c.C, c.N
    w4 = torch.from_numpy(v2.copy()).reshape(Ci, 3, 3, Co).permute(3, 0, 1, 2).flip(2, 3).contiguous()       # [co][ci][kh][kw]
    assert torch.equal(V.pack_unrounded(w4, 1), torch.from_numpy(v2.copy()))
    x = torch.zeros(c.B, Ci, c.T, c.F, dtype=torch.float64, requires_grad=True)
    dy = torch.from_numpy(vi.copy()).permute(0, 3, 1, 2)
    (tF.conv2d(x, w4, None, padding=1) * dy).sum().backward()
    assert np.array_equal(vo, x.grad.permute(0, 2, 3, 1).reshape(-1, Ci).numpy())


@pytest.mark.parametrize('c', ALL, ids=ids(ALL))
def test_case_reaches_the_plan_it_names(c):
    assert plan_mismatch(c) is None, plan_mismatch(c)


@pytest.mark.parametrize('c', ALL, ids=ids(ALL))
def test_reference_of_every_case_is_finite_and_confined(c):
    """No NaN of the guards reaches the reference, and it writes the matrix and nothing else."""
    img, op2, bias, out0, ref, tol, S = expected(c)
    assert np.isfinite(ref).all()
    assert ((ref == SENTINEL) == (out0 == SENTINEL)).all()
    assert tol is None or (np.isfinite(tol).all() and ((tol == 0) == (out0 == SENTINEL)).all())
    g = geometry(c)
    assert np.isnan(img[:g['img_base']]).all() and np.isnan(img[g['img_base'] + g['rows'] * c.C:]).all()
    assert g['img_base'] - c.img_off >= (c.F + 1) * c.C and g['img_base'] % 4 == c.img_off and g['op2_base'] % 4 == c.op2_off


@pytest.mark.parametrize('c', EXACT_ONCE, ids=ids(EXACT_ONCE))
def test_exact_cases_stay_exact_in_fp32(c):
    img, op2, bias, out0, ref, tol, S = expected(c)
    assert c.act != TANH and S.max() < 2 ** 24
    assert np.array_equal(ref, np.round(ref))


def chunk_to_drop(c):
    """Eight consecutive reduction indices every case has terms in: mode 0 the chunk that holds the centre tap's first
    channel, mode 1 eight pixels from the middle of the batch."""
    K = reduction(c)
    lo = (4 * c.C) // 8 * 8 if c.mode == 0 else (K // 2) // 8 * 8
    return lo, min(lo + 8, K)


@pytest.mark.parametrize('c', ROUNDED, ids=ids(ROUNDED))
def test_a_dropped_chunk_stands_above_the_bound(c):
    """K <= 640, and on the reference alone: leaving one 8-element chunk out of the reduction moves the outputs it has terms
    in - the median of them - more than ten times further than the bound allows.  The chunk has terms in every output of a
    case (chunk_to_drop), so without a ReLU more than half of the outputs move; a ReLU hides the loss wherever both results
    are clipped, which only has to leave some."""
    assert reduction(c) <= 640
    img, op2, bias, out0, ref, tol, S = expected(c)
    bad = expected(c, drop=chunk_to_drop(c))[4]
    written = out0 != SENTINEL
    moved = written & (bad != ref)
    assert moved.any() and (c.act == RELU or moved[written].mean() > 0.5)
    assert np.median(np.abs(bad - ref)[moved] / tol[moved]) > 10


BF16_ROUNDED = [c for c in ROUNDED if c.prec == BF16 and c.name in ('ch_64', 'wg_px630', 'n_130')]


@pytest.mark.parametrize('c', BF16_ROUNDED, ids=ids(BF16_ROUNDED))
def test_bf16_mode_operands_put_the_conversion_under_test(c):
    """The fp32 operands of a BF16-mode rounded case are not bf16 values, and a kernel that multiplied them unrounded (or
    truncated) would stand above the bound."""
    img, op2, bias, out0, ref, tol, S = expected(c)
    vi, v2, vo = views(c, img, op2, out0)
    assert (bf16_round(vi) != vi).mean() > 0.9
    unrounded = expected(c._replace(prec=F32))[4]
    assert (np.abs(unrounded - ref) > tol).mean() > 0.25


def test_table_covers_what_the_kernel_branches_on():
    m0 = [c for c in ALL if c.mode == 0]
    m1 = [c for c in ALL if c.mode == 1]
    assert {(c.B, c.T, c.F) for c in TABLES['taps']} >= {(1, 1, 1), (1, 1, 5), (1, 3, 1), (2, 2, 2), (3, 5, 7), (1, 43, 3), (1, 32, 4)}
    assert {c.C for c in m0 if not c.dgrad} >= {1, 3, 4, 6, 7, 8, 64, 128, 256}
    assert {c.N for c in m0 if not c.dgrad} >= {1, 7, 128, 130, 256}
    assert {(c.act, c.bias, c.accum) for c in TABLES['epilogue']} == {(a, b, k) for a in (NONE, RELU, TANH) for b in (0, 1) for k in (0, 1)}
    assert {(c.B * c.T * c.F, c.nz) for c in m1 if c.name.startswith('wg_px')} >= {(4095, 1), (4096, 8), (4100, 8), (65535, 8), (65536, 32),
                                                                                    (65600, 32), (630, 1)}
    assert {(c.C, c.mode, c.img_off, c.op2_off) for c in TABLES['alignment']} == {(C, m, i, o) for C in (4, 8) for m in (0, 1)
                                                                                 for i, o in ((1, 0), (0, 1), (1, 1))}
    # tap 8 of dw starts at column 128, the second column tile, and the ragged output row tile sits beside it
    assert {(c.C, c.N) for c in m1 if c.name.startswith('wg_') and 8 * c.C == 128} >= {(16, 8), (16, 130)}
    assert all(c.exact for c in ALL if reduction(c) > 640) and all(reduction(c) <= 640 for c in ROUNDED)


def test_refused_arguments_answer_like_the_launch():
    """asr_conv3x3_plan runs the checks of asr_conv3x3 (host only): what the issue's table lists is refused with its code and
    the plan is left alone."""
    lib = _lib()
    lib.asr_last_error.restype = ctypes.c_char_p
    base = dict(zip(('img', 'op2', 'out', 'bias', 'B', 'T', 'F', 'C', 'N', 'mode', 'act', 'accum', 'prec'),
                    (FAKE['img'], FAKE['op2'], FAKE['out'], None, 2, 5, 7, 4, 8, 0, NONE, 0, F32)))
    refused = [(dict(mode=2), -1), (dict(mode=-1), -1), (dict(prec=5), -1), (dict(act=7), -1), (dict(accum=2), -1), (dict(accum=-1), -1),
               (dict(mode=1, accum=0), -1), (dict(mode=1, accum=1, act=RELU), -1), (dict(mode=1, accum=1, bias=FAKE['bias']), -1),
               (dict(img=None), -1), (dict(op2=None), -1), (dict(out=None), -1), (dict(B=0), -1), (dict(T=0), -1), (dict(F=-1), -1),
               (dict(C=0), -1), (dict(N=0), -1), (dict(B=32768, T=32768, F=2), -3), (dict(B=65536, T=65536, F=1), -3),
               (dict(C=238609295), -3)]                                         # 9 C = 2^31 + 7
    for change, code in refused:
        a = dict(base)
        a.update(change)
        out = (ctypes.c_int * 8)(*([-7] * 8))
        assert lib.asr_conv3x3_plan(*a.values(), out) == code, change
        assert b'asr_conv3x3' in lib.asr_last_error() and list(out) == [-7] * 8, change
    out = (ctypes.c_int * 8)()
    assert lib.asr_conv3x3_plan(*dict(base, B=32768, T=32768, F=1, C=1, N=1).values(), out) == 0       # 2^30 pixels are taken
    assert lib.asr_conv3x3_plan(*base.values(), None) == -1
