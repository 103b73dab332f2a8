"""Float64 reference, operands and case tables of the contraction kernels (asr_gemm, asr_gemm16), and the CPU half of their
test: the reference is checked against explicit loops, and every case of the tables is asked - through the host queries
asr_gemm_plan / asr_gemm16_route / asr_gemm16_plan, the only things this file takes from the code under test - whether it reaches the kernel,
loader pair, tile order and tile / slice counts its entry names.  tests/test_hip_gemm_vs_float64.py runs the same tables on
the GPU.

The contract (include/asr_hip.h):  C[i,j] (+)= act( sum_r opA(i,r) opB(r,j) + bias[j] ), accumulation order
C0 + act(AB + bias); a_kc / b_kc choose which index of an operand is contiguous; lda / ldb / ldc, element offsets and batch
strides place the matrices; reduction slices (`splits`) never change the result; seqT / bshift read row r = (b,t) of B at row
r + bshift and as zero where t + bshift leaves [0, T), or - time-padded - at row b*(T+2) + t + 1 + bshift of a buffer that
holds the border rows; perm_h = H stores output row i at (i / 4H)*4H + (i & 3)*H + ((i % 4H) >> 2).

Two kinds of operands.
  EXACT: small integers - every product is an integer and every partial sum stays below 2^24, so fp32 accumulation in any
  order, atomics included, is exact and the kernel must EQUAL the reference (-0.0 == 0.0).  fp32 output: operands in
  {-3..3}, bias and C0 integers in [-8, 8].  bf16 output: operands in {-1, 0, 1}, bias in [-8, 8], and max|ref| <= 256
  (asserted here per case), integers up to 256 being exact in bf16.  Any dropped, doubled or misplaced product changes an
  integer.
  ROUNDED: standard-normal operands, weights scaled by K^-1/2, held per element:
      |got - ref| <= 2 (K+2) 2^-24 S   (+ 2^-8 |ref| for a bf16 output)   (+ 2e-6 where tanh is applied)
  with ref the float64 product of the exact values the kernel multiplies (bf16 operands as they are, fp32 operands as they
  are in F32 mode, their round-to-nearest-even bf16 in BF16 mode) and S = sum|a b| + |bias| + |C0|.  (K+2) 2^-24 S is the
  worst case of fp32 summation in any order; the factor 2 on it is an allowance for the MFMA's internal adds, of which
  nobody has measured whether they round as IEEE adds do.  2^-8 |ref| is one round-to-nearest to bf16.  2e-6 is the error
  the comment of tanh_fast (csrc/gemm16.hip) states, also unmeasured.  Rounded cases keep K <= 640, where a lost 8-element
  chunk stands more than ten times above the bound.
"""
import collections
import ctypes
import functools
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the library src/hipabi.py launches from (ASR_HIP_LIB: A/B builds), so that the queries are asked of the code that runs
LIB_PATH = os.environ.get('ASR_HIP_LIB') or os.path.join(ROOT, 'e2e-asr-pytorch_amd', 'lib', 'libasr_hip.so')

F32, BF16 = 0, 1
NONE, TANH, RELU = 0, 1, 2
SENTINEL = -32768.0            # exact in bf16 and fp32, out of reach of every exact result
GENERIC, NT128, TN, NT256 = 0, 1, 2, 3


# ---- the float64 reference ---------------------------------------------------------------------------------------------
def bf16_round(x):
    """Round-to-nearest-even of float values to bf16, returned as float64."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def perm_rows(i, H):
    return (i // (4 * H)) * (4 * H) + (i & 3) * H + ((i % (4 * H)) >> 2)


def reference(A, B, C, bias, M, N, K, lda, ldb, ldc, a_kc, b_kc, act=NONE, accum=0, splits=1, batch=1, sA=0, sB=0, sC=0,
              seqT=0, bshift=0, padded=0, perm_h=0, a_off=0, b_off=0, c_off=0, bias_off=0):
    """The whole contract on flat float64 buffers.  A, B hold the exact values the kernel multiplies, C the output buffer
    before the call; returns (C after the call, S) with S = sum|a b| + |bias| + |C0| at the written elements, 0 elsewhere.
    `splits` is accepted and ignored: slices of the reduction never change the result."""
    out, S = C.copy(), np.zeros_like(C)
    i, j, r = np.arange(M), np.arange(N), np.arange(K)
    for z in range(batch):
        ia = a_off + z * sA + (i[:, None] * lda + r[None, :] if a_kc else r[None, :] * lda + i[:, None])
        a = A[ia]                                                                   # (M, K)
        if b_kc:
            b = B[b_off + z * sB + j[None, :] * ldb + r[:, None]]                   # (K, N)
        else:
            rows, valid = r, np.ones(K, bool)
            if seqT > 0 and padded:
                rows = (r // seqT) * (seqT + 2) + r % seqT + 1 + bshift
            elif seqT > 0:
                t = r % seqT + bshift
                valid = (t >= 0) & (t < seqT)
                rows = np.where(valid, r + bshift, 0)
            b = np.where(valid[:, None], B[b_off + z * sB + rows[:, None] * ldb + j[None, :]], 0.0)
        s, mag = a @ b, np.abs(a) @ np.abs(b)
        if bias is not None:
            s, mag = s + bias[bias_off + j][None, :], mag + np.abs(bias[bias_off + j])[None, :]
        if act == TANH:
            s = np.tanh(s)
        elif act == RELU:
            s = np.maximum(s, 0.0)
        io = perm_rows(i, perm_h) if perm_h > 0 else i
        ic = c_off + z * sC + io[:, None] * ldc + j[None, :]
        if accum:
            s, mag = C[ic] + s, mag + np.abs(C[ic])
        out[ic], S[ic] = s, mag
    return out, S


def bound(ref, S, K, bf16_out, tanh):
    """Per-element bound of a rounded case (module docstring); 0 where nothing is written."""
    b = 2.0 * (K + 2) * 2.0 ** -24 * S
    if bf16_out:
        b = b + np.where(S > 0, 2.0 ** -8 * np.abs(ref), 0.0)
    if tanh:
        b = b + np.where(S > 0, 2e-6, 0.0)
    return b


# ---- cases -------------------------------------------------------------------------------------------------------------
_FIELDS = dict(api='gemm', name='', M=1, N=1, K=1, a_kc=1, b_kc=1, prec=BF16, lda_pad=0, ldb_pad=0, ldc_pad=0, a_off=0, b_off=0,
               c_off=0, bias_off=0, batch=1, sA_gap=0, sB_gap=0, sC_gap=0, bias=0, act=NONE, accum=0, splits=1, seqT=0, bshift=0,
               padded=0, perm_h=0, c16=0, exact=1, route=None, plan=None)
Case = collections.namedtuple('Case', list(_FIELDS))


def mk(**kw):
    d = dict(_FIELDS)
    d.update(kw)
    return Case(**d)


def geometry(c):
    """Rows, leading dimensions, batch strides and buffer sizes of a case's three matrices."""
    g = {}
    brows = c.K
    if c.seqT > 0 and c.padded:
        brows = (c.K // c.seqT) * (c.seqT + 2)
    g['ar'], g['ac'] = (c.M, c.K) if c.a_kc else (c.K, c.M)
    g['br'], g['bc'] = (c.N, c.K) if c.b_kc else (brows, c.N)
    g['lda'], g['ldb'], g['ldc'] = g['ac'] + c.lda_pad, g['bc'] + c.ldb_pad, c.N + c.ldc_pad
    one = c.batch == 1
    g['sA'] = 0 if one else g['ar'] * g['lda'] + c.sA_gap
    g['sB'] = 0 if one else g['br'] * g['ldb'] + c.sB_gap
    g['sC'] = 0 if one else c.M * g['ldc'] + c.sC_gap
    g['guard'] = (g['ldc'] + 7) // 8 * 8                    # one guard row above C (a multiple of 8: keeps the alignment)
    g['c_base'] = g['guard'] + c.c_off
    g['nA'] = c.a_off + (c.batch - 1) * g['sA'] + g['ar'] * g['lda']
    g['nB'] = c.b_off + (c.batch - 1) * g['sB'] + g['br'] * g['ldb']
    g['nC'] = g['c_base'] + (c.batch - 1) * g['sC'] + c.M * g['ldc'] + g['guard']
    g['nbias'] = c.bias_off + c.N
    return g


def _fill(rng, buf, off, nb, stride, rows, ld, cols, draw):
    for z in range(nb):
        idx = off + z * stride + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
        buf[idx] = draw(rows, cols)


def operands(c):
    """Flat float64 buffers of a case AS UPLOADED: A, B (NaN outside the matrices), bias (or None) and the initial C
    (SENTINEL outside the matrix; inside NaN, or the integer C0 of an accumulating call).  bf16 storage (asr_gemm16) holds
    bf16 values; asr_gemm gets fp32 values in both modes - in BF16 mode the rounded cases are NOT bf16-representable, so the
    kernel's own fp32 -> bf16 conversion is under test (multiplied() gives the values it must arrive at)."""
    g = geometry(c)
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    io16 = c.api == 'gemm16'
    if c.exact:
        lim = 1 if (io16 and c.c16) else 3
        da = db = lambda r, k: rng.integers(-lim, lim + 1, (r, k)).astype(np.float64)
    else:
        rnd = bf16_round if io16 else (lambda x: np.asarray(x, np.float32).astype(np.float64))
        da = lambda r, k: rnd(rng.standard_normal((r, k)))
        db = lambda r, k: rnd(rng.standard_normal((r, k)) * c.K ** -0.5)
    A, B = np.full(g['nA'], np.nan), np.full(g['nB'], np.nan)
    _fill(rng, A, c.a_off, c.batch, g['sA'], g['ar'], g['lda'], g['ac'], da)
    _fill(rng, B, c.b_off, c.batch, g['sB'], g['br'], g['ldb'], g['bc'], db)
    bias = None
    if c.bias:
        bias = np.full(g['nbias'], np.nan)
        bias[c.bias_off:] = rng.integers(-8, 9, c.N) if c.exact else np.asarray(rng.standard_normal(c.N), np.float32)
    C = np.full(g['nC'], SENTINEL)
    c0 = (lambda r, k: rng.integers(-8, 9, (r, k)).astype(np.float64)) if c.accum else (lambda r, k: np.full((r, k), np.nan))
    _fill(rng, C, g['c_base'], c.batch, g['sC'], c.M, g['ldc'], c.N, c0)
    return A, B, bias, C


_EXPECTED = {}


def expected(c):
    """(A, B, bias, C0, ref, tol) of a case, computed once and shared (callers must not write into them).  tol is None for
    an exact case."""
    key = tuple(v for v in c if not isinstance(v, dict))
    if key not in _EXPECTED:
        _EXPECTED[key] = _expected(c)
        for a in _EXPECTED[key]:
            if a is not None:
                a.setflags(write=False)
    return _EXPECTED[key]


def multiplied(c, X):
    """The exact values the kernel multiplies for an uploaded operand: asr_gemm in BF16 mode rounds its fp32 operands to
    nearest-even bf16 on the way into LDS, everything else multiplies what is stored."""
    return bf16_round(X) if (c.api == 'gemm' and c.prec == BF16) else X


def _expected(c):
    g = geometry(c)
    A, B, bias, C = operands(c)
    ref, S = reference(multiplied(c, A), multiplied(c, B), C, bias, c.M, c.N, c.K, g['lda'], g['ldb'], g['ldc'], c.a_kc, c.b_kc, c.act, c.accum, c.splits,
                       c.batch, g['sA'], g['sB'], g['sC'], c.seqT, c.bshift, c.padded, c.perm_h, c.a_off, c.b_off, g['c_base'],
                       c.bias_off)
    tol = None if c.exact else bound(ref, S, c.K, c.api == 'gemm16' and c.c16, c.act == TANH)
    return A, B, bias, C, ref, tol


def abi_args(c, pA, pB, pC, pbias):
    """Arguments of asr_gemm / asr_gemm16 (and of their queries) without the stream, from the BASE addresses of the four
    buffers: the case's element offsets are applied here."""
    g = geometry(c)
    es = 2 if c.api == 'gemm16' else 4
    a, b = pA + es * c.a_off, pB + es * c.b_off
    cc = pC + (2 if (c.api == 'gemm16' and c.c16) else 4) * g['c_base']
    bi = (pbias + 4 * c.bias_off) if c.bias else None
    if c.api == 'gemm':
        return (a, b, cc, bi, c.M, c.N, c.K, g['lda'], g['ldb'], g['ldc'], c.a_kc, c.b_kc, c.act, c.accum, c.splits, c.batch,
                g['sA'], g['sB'], g['sC'], c.seqT, c.bshift, c.prec)
    return (a, b, cc, bi, c.M, c.N, c.K, g['lda'], g['ldb'], g['ldc'], c.a_kc, c.b_kc, c.act, c.accum, c.splits, c.c16,
            c.perm_h, c.seqT, c.bshift, c.padded)


# ---- tables ------------------------------------------------------------------------------------------------------------
LAYOUTS = [(1, 1), (1, 0), (0, 0), (0, 1)]
PRECS = [F32, BF16]


def _gemm_extents():
    ext = [(1, 1, 1), (127, 129, 3), (128, 128, 4), (129, 127, 31), (257, 1, 32), (1, 257, 33), (128, 257, 68), (129, 129, 32),
           (257, 128, 31), (127, 128, 68)]
    out = []
    for n, (M, N, K) in enumerate(ext):
        for a_kc, b_kc in LAYOUTS:
            for prec in PRECS:
                # contiguous matrices: an operand is fast exactly when its contiguous extent is a positive multiple of 4
                fa, fb = ((K if a_kc else M) % 4 == 0), ((K if b_kc else N) % 4 == 0)
                out.append(mk(name='ext%d_%d%d_p%d' % (n, a_kc, b_kc, prec), M=M, N=N, K=K, a_kc=a_kc, b_kc=b_kc, prec=prec,
                              bias=n & 1, act=RELU if n % 3 == 0 else NONE, ldc_pad=n % 3,
                              plan=dict(fastA=int(fa), fastB=int(fb), nx=-(-N // 128), ny=-(-M // 128), nz=1)))
    return out


def _gemm_loaders():
    ways = [
        # (name, overrides, fastA, fastB)
        ('ff', dict(a_kc=1, b_kc=1, M=129, N=130, K=32), 1, 1),
        ('sA_off', dict(a_kc=1, b_kc=1, M=129, N=130, K=32, a_off=1), 0, 1),
        ('sA_ld', dict(a_kc=1, b_kc=1, M=129, N=130, K=32, lda_pad=1), 0, 1),
        ('sA_ext', dict(a_kc=1, b_kc=0, M=129, N=132, K=33, lda_pad=3), 0, 1),
        ('sA_stride', dict(a_kc=1, b_kc=1, M=129, N=130, K=32, batch=2, sA_gap=2), 0, 1),
        ('sB_off', dict(a_kc=1, b_kc=1, M=129, N=130, K=32, b_off=1), 1, 0),
        ('sB_ld', dict(a_kc=0, b_kc=0, M=132, N=128, K=33, ldb_pad=1), 1, 0),
        ('sB_ext', dict(a_kc=0, b_kc=0, M=132, N=129, K=33, ldb_pad=3), 1, 0),
        ('sB_stride', dict(a_kc=0, b_kc=0, M=132, N=128, K=33, batch=2, sB_gap=2), 1, 0),
        ('ss_off_ld', dict(a_kc=1, b_kc=1, M=129, N=130, K=32, a_off=1, ldb_pad=1), 0, 0),
        ('ss_ext_stride', dict(a_kc=0, b_kc=0, M=129, N=128, K=33, lda_pad=3, batch=2, sB_gap=2), 0, 0),
    ]
    return [mk(name='ld_%s_p%d' % (n, prec), prec=prec, bias=1, plan=dict(fastA=fa, fastB=fb), **kw)
            for n, kw, fa, fb in ways for prec in PRECS]


def _gemm_slices():
    out = []
    for prec in PRECS:
        for a_kc, b_kc in ((0, 0), (1, 1)):
            tag = '%d%d_p%d' % (a_kc, b_kc, prec)
            base = dict(M=132, N=136, a_kc=a_kc, b_kc=b_kc, prec=prec, accum=1)
            # ktiles = ceil(K / 32): 68 -> 3, 130 -> 5
            out += [mk(name='sl2_' + tag, K=68, splits=2, plan=dict(nz=2, plain_order=1), **base),           # 3 % 2 != 0: slices of 2 and 1
                    mk(name='sl3_' + tag, K=130, splits=3, plan=dict(nz=3, plain_order=1), **base),          # slices of 2, 2, 1
                    mk(name='sl7_' + tag, K=68, splits=7, plan=dict(nz=7, plain_order=1), **base),           # more slices than k-tiles
                    mk(name='sl3bias_' + tag, K=130, splits=3, bias=1, plan=dict(nz=3), **base),            # bias: first slice only
                    mk(name='acc_' + tag, K=68, plan=dict(nz=1), **base),
                    mk(name='accrelu_' + tag, K=68, act=RELU, bias=1, plan=dict(nz=1), **base),             # C0 + relu(AB + bias)
                    mk(name='b3s2_' + tag, K=68, splits=2, batch=3, sC_gap=8, plan=dict(nz=6, plain_order=1), **base)]
    return out


def _gemm_shifts():
    out = []
    for prec in PRECS:
        for T in (1, 5, 37):
            for Bb in (1, 3):
                for sh in (-1, 1):
                    for fast in (1, 0):
                        out.append(mk(name='sh_T%d_B%d_%+d_f%d_p%d' % (T, Bb, sh, fast, prec), M=36, N=132 if fast else 129, K=Bb * T,
                                      a_kc=0, b_kc=0, prec=prec, accum=1, splits=3 if (T == 37 and Bb == 3) else 1, seqT=T, bshift=sh,
                                      plan=dict(fastA=1, fastB=fast)))
    return out


def _gemm_order():
    out = []
    for prec in PRECS:
        out += [mk(name='ord_plain_p%d' % prec, M=130, N=1160, K=40, prec=prec, bias=1,
                   plan=dict(plain_order=1, nx=10, ny=2, nz=1)),
                mk(name='ord_groups_p%d' % prec, M=130, N=1000, K=1000, prec=prec,
                   plan=dict(plain_order=0, nx=8, ny=2, nz=1, gx=5, ngx=2)),                       # groups of 5 and 3 column tiles
                mk(name='ord_band_p%d' % prec, M=1153, N=40, K=8, prec=prec, act=RELU,
                   plan=dict(plain_order=0, nx=1, ny=10, nz=1, gx=1, ngx=1))]                      # 2 rows per band: XCDs 5..7 idle
    return out


def _gemm_rounded():
    out = []
    for prec in PRECS:
        for a_kc, b_kc in LAYOUTS:
            out.append(mk(name='rnd_%d%d_p%d' % (a_kc, b_kc, prec), M=132, N=136, K=200, a_kc=a_kc, b_kc=b_kc, prec=prec, bias=1, exact=0))
        for act in (NONE, TANH, RELU):
            out.append(mk(name='rnd_act%d_p%d' % (act, prec), M=129, N=130, K=640, prec=prec, bias=1, act=act, exact=0))
        out.append(mk(name='rnd_acctanh_p%d' % prec, M=129, N=130, K=68, prec=prec, bias=1, act=TANH, accum=1, exact=0))
    return out


def _g16(**kw):
    return mk(api='gemm16', **kw)


def _generic16():
    o = []
    nt = dict(a_kc=1, b_kc=1, c16=1, route=GENERIC)
    o += [_g16(name='g_nmod8', M=136, N=132, K=40, bias=1, act=RELU, **nt),
          _g16(name='g_ldc', M=8, N=136, K=72, ldc_pad=4, bias=1, **nt),
          _g16(name='g_coff', M=264, N=128, K=8, c_off=4, **nt),
          _g16(name='g_biasoff', M=136, N=128, K=72, bias=1, bias_off=1, **nt),
          _g16(name='g_nt_f32', M=136, N=136, K=72, a_kc=1, b_kc=1, bias=1, route=GENERIC),                  # fp32 output, written
          _g16(name='g_nt_f32acc', M=136, N=136, K=72, a_kc=1, b_kc=1, accum=1, act=RELU, route=GENERIC),
          _g16(name='g_10_c16', M=136, N=136, K=72, a_kc=1, b_kc=0, c16=1, bias=1, route=GENERIC),
          _g16(name='g_10_f32', M=264, N=8, K=40, a_kc=1, b_kc=0, route=GENERIC),
          _g16(name='g_01_c16', M=136, N=132, K=72, a_kc=0, b_kc=1, c16=1, act=RELU, route=GENERIC),
          _g16(name='g_01_f32', M=8, N=136, K=8, a_kc=0, b_kc=1, accum=1, route=GENERIC),
          _g16(name='g_tn_bias', M=136, N=136, K=72, a_kc=0, b_kc=0, accum=1, bias=1, route=GENERIC),
          _g16(name='g_tn_bias_s3', M=136, N=136, K=130, a_kc=0, b_kc=0, accum=1, bias=1, splits=3, route=GENERIC),
          _g16(name='g_tn_write', M=264, N=136, K=40, a_kc=0, b_kc=0, accum=0, route=GENERIC),
          _g16(name='g_tn_perm', M=320, N=40, K=72, a_kc=0, b_kc=0, accum=0, perm_h=40, route=GENERIC),       # ND = 2, 4H = 160
          # banded order, two column groups: a column tile's B slice is 128 x 2560 bf16 = 655360 B, 2.5 MB hold 4 of them, nx = 8
          _g16(name='g_banded', M=136, N=1000, K=2560, ldc_pad=4, bias=1, plan=dict(plain_order=0, nx=8, ny=2, gx=4, ngx=2), **nt)]
    for sh in (-1, 1):
        o += [_g16(name='g_tn_mask%+d' % sh, M=136, N=136, K=3 * 17, a_kc=0, b_kc=0, accum=1, seqT=17, bshift=sh, route=GENERIC),
              _g16(name='g_tn_mask40%+d' % sh, M=8, N=136, K=2 * 40, a_kc=0, b_kc=0, accum=1, splits=2, seqT=40, bshift=sh, route=GENERIC),
              _g16(name='g_tn_padwrite%+d' % sh, M=136, N=8, K=3 * 17, a_kc=0, b_kc=0, accum=0, seqT=17, bshift=sh, padded=1, route=GENERIC)]
    return o


def _nt16(big=False):
    route = NT256 if big else NT128
    shapes = [(1, 8, 8), (127, 120, 56), (128, 128, 64), (129, 136, 72), (300, 264, 128), (300, 136, 200), (1, 264, 200),
              (128, 120, 72), (129, 8, 128), (127, 264, 64), (300, 128, 56), (128, 136, 8),
              (1, 888, 8), (129, 504, 8), (1153, 648, 8)]                          # 7, 8 and 60 tiles (1 and 9 are above)
    if big:
        shapes += [(255, 248, 64), (256, 256, 72), (257, 264, 128), (256, 248, 200), (257, 256, 56), (255, 264, 8)]
    o = []
    for n, (M, N, K) in enumerate(shapes):
        o.append(_g16(name='nt%s_%d' % ('b' if big else '', n), M=M, N=N, K=K, c16=1, bias=n & 1, act=RELU if n % 3 else NONE,
                      lda_pad=8 * (n % 2), ldb_pad=16 * (n % 3 == 1), ldc_pad=8 * (n % 4 == 2), route=route))
    return o


def _nt16_rounded():
    return [_g16(name='ntr_%d' % n, M=M, N=N, K=K, c16=1, bias=1, act=act, exact=0, route=NT128)
            for n, (M, N, K, act) in enumerate([(129, 136, 200, NONE), (129, 136, 200, TANH), (300, 264, 640, TANH), (127, 120, 72, NONE)])]


def _tn16():
    base = dict(a_kc=0, b_kc=0, accum=1, route=TN)
    shapes = [(8, 8, 1), (120, 128, 63), (128, 136, 64), (136, 264, 65), (264, 8, 130), (264, 264, 330), (8, 136, 330),
              (128, 128, 130), (120, 264, 64), (136, 8, 63)]
    o = [_g16(name='tn_%d' % n, M=I, N=J, K=R, lda_pad=16 * (n % 2), a_off=8 * (n % 2), ldb_pad=8 * (n % 3 == 1), b_off=8 * (n % 3 == 1),
              ldc_pad=4 * (n % 3), **base) for n, (I, J, R) in enumerate(shapes)]
    # reduction slices: nk = ceil(R / 64)
    o += [_g16(name='tn_s2', M=136, N=136, K=330, splits=2, plan=dict(splits=2, per=3, wgs=8), **base),                  # nk = 6: 3 + 3
          _g16(name='tn_s3', M=136, N=136, K=300, splits=3, plan=dict(splits=3, per=2, wgs=12), **base),                  # nk = 5: 2 + 2 + 1
          _g16(name='tn_s4_empty', M=136, N=136, K=300, splits=4, plan=dict(splits=4, per=2, wgs=16), **base),            # nk = 5: 2 + 2 + 1 + 0
          _g16(name='tn_s9_clip', M=136, N=136, K=100, splits=9, plan=dict(splits=2, per=1, wgs=8), **base),             # nk = 2: clipped to 2 slices
          _g16(name='tn_perm', M=320, N=136, K=130, splits=2, perm_h=40, ldc_pad=8, **base)]   # ND = 2, 4H = 160: straddles row 128
    for Bb in (1, 3):
        for T in (1, 17, 64, 65):
            for sh in (-1, 1):
                o.append(_g16(name='tn_pad_B%d_T%d_%+d' % (Bb, T, sh), M=136, N=8 if T == 1 else 136, K=Bb * T, seqT=T, bshift=sh, padded=1,
                              ldb_pad=8, b_off=8 * (Bb == 3), splits=2 if T == 65 else 1, perm_h=34 if T == 17 else 0, **base))
    return o


def _tn16_rounded():
    return [_g16(name='tnr_0', M=136, N=136, K=330, a_kc=0, b_kc=0, accum=1, splits=2, exact=0, route=TN),
            _g16(name='tnr_1', M=320, N=40, K=3 * 65, a_kc=0, b_kc=0, accum=1, seqT=65, bshift=-1, padded=1, perm_h=40, exact=0, route=TN)]


def _generic16_rounded():
    return [_g16(name='gr_%d%d_%d' % (a, b, c16), M=136, N=132 if b else 136, K=200, a_kc=a, b_kc=b, c16=c16, bias=1, act=TANH if c16 else NONE,
                 exact=0, route=GENERIC) for a, b in LAYOUTS for c16 in (1, 0)]


TABLES = {
    'gemm_extents': _gemm_extents(), 'gemm_loaders': _gemm_loaders(), 'gemm_slices': _gemm_slices(), 'gemm_shifts': _gemm_shifts(),
    'gemm_order': _gemm_order(), 'gemm_rounded': _gemm_rounded(),
    'generic16': _generic16(), 'generic16_rounded': _generic16_rounded(),
    'nt16': _nt16(), 'nt16_rounded': _nt16_rounded(), 'tn16': _tn16(), 'tn16_rounded': _tn16_rounded(),
}
ALL = [c for t in TABLES.values() for c in t]

# The switches: environment variable -> value -> (cases, what every case's query must answer under it).  Each is read once
# per process, so only a fresh process reaches it.
SWITCHES = {
    'ASR_GEMM16_NT=0': (TABLES['nt16'] + TABLES['tn16'], dict(route=GENERIC)),
    'ASR_GEMM16_BIG=1': (_nt16(big=True), dict(route=NT256)),
    'ASR_GEMM16_TN_STAGES=2': (TABLES['tn16'], dict(route=TN, stages=2)),
    'ASR_GEMM16_TN_STAGES=4': (TABLES['tn16'], dict(route=TN, stages=4)),
    'ASR_GEMM_PLAIN_ORDER=1': (TABLES['gemm_order'] + TABLES['gemm_slices'], dict(plain_order=1)),
}


# ---- the queries -------------------------------------------------------------------------------------------------------
PLAN_KEYS = ('fastA', 'fastB', 'plain_order', 'nx', 'ny', 'nz', 'gx', 'ngx')
PLAN16_KEYS = {GENERIC: PLAN_KEYS, NT128: ('ntx', 'nty', 'bm', 'bn'), NT256: ('ntx', 'nty', 'bm', 'bn'),
               TN: ('nti', 'ntj', 'splits', 'per', 'stages', 'wgs')}
FAKE = {'A': 0x10000000, 'B': 0x20000000, 'C': 0x30000000, 'bias': 0x40000000}        # device allocations are 256-byte aligned


@functools.lru_cache(maxsize=None)
def _lib():
    assert os.path.exists(LIB_PATH), 'run `python -c "import __graft_entry__ as g; g.build()"` first'
    lib = ctypes.CDLL(LIB_PATH)
    vp, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    lib.asr_gemm_plan.argtypes = [vp] * 4 + [i] * 3 + [l] * 3 + [i] * 6 + [l] * 3 + [i] * 3 + [ctypes.POINTER(i)]
    lib.asr_gemm16_route.argtypes = [vp] * 4 + [i] * 3 + [l] * 3 + [i] * 10
    lib.asr_gemm16_plan.argtypes = lib.asr_gemm16_route.argtypes + [ctypes.POINTER(i)]
    return lib


def query(c, pA=FAKE['A'], pB=FAKE['B'], pC=FAKE['C'], pbias=FAKE['bias']):
    """What the library says a call of this case takes: the eight plan entries for asr_gemm; for asr_gemm16 the route and
    the entries asr_gemm16_plan gives for that route.  Host arithmetic only - the addresses are never followed."""
    args = abi_args(c, pA, pB, pC, pbias)
    out = (ctypes.c_int * 8)()
    if c.api == 'gemm16':
        route = _lib().asr_gemm16_route(*args)
        assert _lib().asr_gemm16_plan(*args, out) == route, c.name
        got = {'route': route}
        got.update(zip(PLAN16_KEYS.get(route, ()), out))
        return got
    rc = _lib().asr_gemm_plan(*args, out)
    assert rc == 0, (c.name, rc)
    return dict(zip(PLAN_KEYS, out))


def route_mismatch(c, override=None, ptrs=()):
    """None when the case reaches what its table entry (or a switch's override) names, else a description.  ptrs: the base
    addresses of real buffers (A, B, C, bias) instead of the 256-byte aligned stand-ins."""
    got = query(c, *ptrs)
    override = dict(override or {})
    if c.api == 'gemm16':
        want = {'route': override.get('route', c.route)}
        if want['route'] == c.route:                       # the entry's plan describes the kernel it names
            want.update(c.plan or {})
        if want['route'] == TN:
            want.setdefault('stages', 1)
            want.setdefault('nti', -(-c.M // 128))
            want.setdefault('ntj', -(-c.N // 128))
        elif want['route'] in (NT128, NT256):
            bm = 256 if want['route'] == NT256 else 128
            want.update(bm=bm, bn=bm, ntx=-(-c.N // bm), nty=-(-c.M // bm))
        else:
            want.update(nx=-(-c.N // 128), ny=-(-c.M // 128), nz=c.splits, fastA=1, fastB=1)
    else:
        want = dict(c.plan or {})
        want.setdefault('nx', -(-c.N // 128))
        want.setdefault('ny', -(-c.M // 128))
        want.setdefault('nz', c.batch * c.splits)
    for k, v in override.items():
        if k in got:
            want[k] = v
    assert set(want) <= set(got) or got.get('route') != want.get('route'), (c.name, want, got)
    bad = {k: (got.get(k), v) for k, v in want.items() if got.get(k) != v}
    return None if not bad else '%s: (got, want) %s' % (c.name, bad)


# ---- CPU tests ---------------------------------------------------------------------------------------------------------
def _ids(cases):
    return [c.name for c in cases]


def test_case_names_are_unique():
    names = [c.name for c in ALL] + [c.name for c in _nt16(big=True)]
    assert len(set(names)) == len(names)


def test_bf16_round():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 257.0, 3.0e-40, 0.0], np.float32)
    #             exact, tie -> even (down), tie -> even (up), sign, 257 -> 256 (tie to even), ...
    got = bf16_round(x)
    assert got[0] == 1.0 and got[1] == 1.0 and got[2] == 1.015625 and got[3] == -1.0 and got[4] == 256.0 and got[6] == 0.0
    import torch
    y = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    assert np.array_equal(bf16_round(y), torch.from_numpy(y).to(torch.bfloat16).double().numpy())


def _loops(A, B, C, bias, M, N, K, lda, ldb, ldc, a_kc, b_kc, act, accum, batch, sA, sB, sC, seqT, bshift, padded, perm_h, a_off, b_off,
           c_off, bias_off):
    out = C.copy()
    for z in range(batch):
        for i in range(M):
            for j in range(N):
                s = 0.0
                for r in range(K):
                    a = A[a_off + z * sA + (i * lda + r if a_kc else r * lda + i)]
                    if b_kc:
                        b = B[b_off + z * sB + j * ldb + r]
                    elif seqT > 0 and padded:
                        bb, t = divmod(r, seqT)
                        b = B[b_off + z * sB + (bb * (seqT + 2) + t + 1 + bshift) * ldb + j]
                    elif seqT > 0:
                        t = r % seqT + bshift
                        b = B[b_off + z * sB + (r + bshift) * ldb + j] if 0 <= t < seqT else 0.0
                    else:
                        b = B[b_off + z * sB + r * ldb + j]
                    s += a * b
                if bias is not None:
                    s += bias[bias_off + j]
                s = np.tanh(s) if act == TANH else (max(s, 0.0) if act == RELU else s)
                io = i
                if perm_h:
                    blk, rr = divmod(i, 4 * perm_h)
                    io = blk * 4 * perm_h + (rr % 4) * perm_h + rr // 4
                at = c_off + z * sC + io * ldc + j
                out[at] = (C[at] if accum else 0.0) + s
    return out


TINY = [mk(name='t0', M=3, N=5, K=4, a_kc=1, b_kc=1, lda_pad=2, ldb_pad=1, ldc_pad=3, a_off=1, b_off=2, c_off=1, bias=1, bias_off=2, act=TANH,
           exact=0),
        mk(name='t1', M=4, N=3, K=6, a_kc=1, b_kc=0, batch=2, sA_gap=3, sB_gap=1, sC_gap=2, accum=1, act=RELU, bias=1),
        mk(name='t2', M=5, N=4, K=6, a_kc=0, b_kc=0, accum=1, seqT=3, bshift=-1, ldb_pad=2, splits=2),
        mk(name='t3', M=5, N=4, K=6, a_kc=0, b_kc=0, accum=1, seqT=3, bshift=1, lda_pad=1),
        mk(name='t4', M=2, N=3, K=5, a_kc=0, b_kc=1, exact=0),
        mk(name='t5', M=3, N=2, K=1, a_kc=0, b_kc=0, accum=1, seqT=1, bshift=1),
        _g16(name='t6', M=16, N=3, K=6, a_kc=0, b_kc=0, accum=1, seqT=3, bshift=-1, padded=1, perm_h=2, ldb_pad=1, b_off=1),
        _g16(name='t7', M=8, N=2, K=4, a_kc=0, b_kc=0, accum=0, seqT=2, bshift=1, padded=1, perm_h=2)]


@pytest.mark.parametrize('c', TINY, ids=_ids(TINY))
def test_reference_against_loops(c):
    g = geometry(c)
    A, B, bias, C, ref, tol = expected(c)
    want = _loops(multiplied(c, A), multiplied(c, B), C, bias, c.M, c.N, c.K, g['lda'], g['ldb'], g['ldc'], c.a_kc, c.b_kc, c.act, c.accum, c.batch, g['sA'], g['sB'], g['sC'],
                  c.seqT, c.bshift, c.padded, c.perm_h, c.a_off, c.b_off, g['c_base'], c.bias_off)
    assert np.isfinite(want[want != SENTINEL]).all() and np.allclose(ref, want, rtol=1e-13, atol=1e-13)
    assert ((ref == SENTINEL) == (C == SENTINEL)).all()              # exactly the matrix is written
    if c.name == 't5':                                                  # T = 1: every shifted row is outside, C0 stays
        assert np.array_equal(ref, C)


def test_reference_against_einsum_and_permutation():
    rng = np.random.default_rng(1)
    a, b, c0 = rng.standard_normal((2, 7, 5)), rng.standard_normal((2, 5, 6)), rng.standard_normal((2, 7, 6))
    ref, S = reference(a.ravel(), b.ravel(), c0.ravel(), None, 7, 6, 5, 5, 6, 6, 1, 0, accum=1, batch=2, sA=35, sB=30, sC=42, splits=3)
    assert np.allclose(ref.reshape(2, 7, 6), c0 + np.einsum('zir,zrj->zij', a, b), rtol=1e-13, atol=1e-13)
    assert np.allclose(S.reshape(2, 7, 6), np.abs(c0) + np.einsum('zir,zrj->zij', np.abs(a), np.abs(b)))
    ref, _ = reference(a[0].ravel(), b[0].T.copy().ravel(), np.zeros(42), None, 7, 6, 5, 5, 5, 6, 1, 1)
    assert np.allclose(ref.reshape(7, 6), a[0] @ b[0])
    # the row permutation is the gate-minor -> [gate][unit] map of an (ND, H, 4) -> (ND, 4, H) weight gradient
    H, ND = 3, 2
    i = np.arange(ND * 4 * H)
    want = np.arange(ND * 4 * H).reshape(ND, 4, H).transpose(0, 2, 1).reshape(-1)      # gate-minor position -> reference row
    assert np.array_equal(perm_rows(i, H), want)


@pytest.mark.parametrize('c', ALL, ids=_ids(ALL))
def test_case_reaches_what_its_entry_names(c):
    assert route_mismatch(c) is None, route_mismatch(c)


BF16_OUT_EXACT = [c for c in ALL + _nt16(big=True) if c.exact and c.api == 'gemm16' and c.c16]


@pytest.mark.parametrize('c', BF16_OUT_EXACT, ids=_ids(BF16_OUT_EXACT))
def test_exact_bf16_output_stays_representable(c):
    ref = expected(c)[4]
    assert np.abs(ref[ref != SENTINEL]).max() <= 256


@pytest.mark.parametrize('c', ALL, ids=_ids(ALL))
def test_reference_of_every_case_is_finite_and_confined(c):
    """No NaN of the operand padding reaches the reference, and it writes the matrix and nothing else."""
    A, B, bias, C, ref, tol = expected(c)
    assert np.isfinite(ref).all()
    assert ((ref == SENTINEL) == (C == SENTINEL)).all()
    assert tol is None or (np.isfinite(tol).all() and ((tol == 0) == (C == SENTINEL)).all())


BF16_MODE_ROUNDED = [c for c in TABLES['gemm_rounded'] if c.prec == BF16]


@pytest.mark.parametrize('c', BF16_MODE_ROUNDED, ids=_ids(BF16_MODE_ROUNDED))
def test_bf16_mode_operands_put_the_conversion_under_test(c):
    """The uploaded fp32 operands of a BF16-mode rounded case are not bf16-representable, and a kernel that truncated them
    instead of rounding to nearest even would stand above the bound."""
    g = geometry(c)
    A, B, bias, C, ref, tol = expected(c)
    ok = np.isfinite(A)
    assert (bf16_round(A)[ok] != A[ok]).mean() > 0.9

    def trunc(x):
        u = np.asarray(x, np.float32).view(np.uint32) & np.uint32(0xffff0000)
        return u.view(np.float32).astype(np.float64)
    bad, _ = reference(trunc(A), trunc(B), C, bias, c.M, c.N, c.K, g['lda'], g['ldb'], g['ldc'], c.a_kc, c.b_kc, c.act, c.accum, c.splits,
                       c.batch, g['sA'], g['sB'], g['sC'], c.seqT, c.bshift, c.padded, c.perm_h, c.a_off, c.b_off, g['c_base'], c.bias_off)
    assert (np.abs(bad - ref) > tol).mean() > 0.25


def test_exact_cases_stay_exact_in_fp32():
    for c in ALL:
        if c.exact:
            lim = 1 if (c.api == 'gemm16' and c.c16) else 3
            assert lim * lim * c.K + 16 < 2 ** 24 and c.act != TANH, c.name
        else:
            assert c.K <= 640, c.name


def test_tables_cover_what_they_claim():
    plans = {c.name: query(c) for c in ALL if c.api == 'gemm'}
    pairs = {(p['fastA'], p['fastB']) for p in plans.values()}
    assert pairs == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for prec in PRECS:
        for tbl in ('gemm_extents', 'gemm_rounded'):
            assert {(c.a_kc, c.b_kc) for c in TABLES[tbl] if c.prec == prec} == set(LAYOUTS)
    # XCD run remap of the NT kernel with and without a remainder
    assert {1, 7, 8, 9, 60} <= {-(-c.M // 128) * -(-c.N // 128) for c in TABLES['nt16']}
    assert {c.K for c in TABLES['nt16']} >= {8, 56, 64, 72, 128, 200}
    assert {c.K for c in TABLES['tn16'] if not c.seqT} >= {1, 63, 64, 65, 130, 330}
    assert {(c.a_kc, c.b_kc) for c in TABLES['generic16']} == set(LAYOUTS)


def _child_env(setting):
    env = {k: v for k, v in os.environ.items() if not k.startswith('ASR_GEMM')}
    k, v = setting.split('=')
    env[k] = v
    return env


@pytest.mark.parametrize('setting', list(SWITCHES))
def test_switch_routes_in_a_fresh_process(setting):
    """The switches are read once per process: a fresh child with the variable set asks the queries (no GPU involved)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), setting], env=_child_env(setting), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert json.loads(r.stdout.strip().splitlines()[-1]) == []


if __name__ == '__main__':
    cases, override = SWITCHES[sys.argv[1]]
    bad = [m for m in (route_mismatch(c, override) for c in cases) if m]
    print(json.dumps(bad))
    sys.exit(1 if bad else 0)
