"""The seven entry points of the bf16 encoder glue (csrc/elementwise16.hip) and the three fp32 dropout entry points
(csrc/elementwise.hip), each called through the C ABI and held to the restatements of tests/test_encoder_glue_reference.py, which
also owns the case tables and the input recipes.

Conditions on every case: outputs the kernel must write fully start as NaN (bf16: the pattern 0x7fc0), accumulated outputs
(asr_cast_f32 with accum = 1, out / out2 of asr_colsum16) start from random values and must equal init + contribution, every output
buffer carries a 64-element sentinel tail that must survive, and inputs the kernel must not read - time rows the down-sampling
does not select, rows behind T2, the pad rows and everything else outside the addressed rows of the bf16 y, columns past N of a
column-sum operand - hold NaN.

BIT FOR BIT (the raw patterns are compared, so -0 / +0 and a NaN left over both show):
  asr_cast_bf16, asr_cast_f32 (accum = 1: the float32 sum init + value); NaN inputs are judged by isnan alone
  asr_dropout_mask against Philox4x32-10 itself (keep_mask), seeds with and without a high word
  asr_dropout_downsample_fwd / _bwd and asr_dropout_downsample16_fwd / _bwd against downsample_ref / downsample_bwd_ref; the fp32
      kernels on buffers offset by one float (the scalar kernel) must give the aligned (vec4) result
  all five outputs of asr_rnn_pack_weights
  asr_act_bwd16, tanh and ReLU
  asr_colsum16 on the integer recipe: every partial sum is an integer below 2^24 (asserted per case), so fp32 accumulation and
      atomics are exact in any order
BOUNDED: asr_colsum16 on bf16 normals, n 2^-24 sum|terms| per output element, n = M + 1 terms with the start value (any order of
summation).  Every (case, lda, recipe) prints one SUM line with the worst err / bound of its runs.

Grid stride: every kernel here runs once with more work than its grid capped at 4096 x 256 threads (the casts at n = 8 388 608 and
above, asr_act_bwd16 at 8 x 1 048 576 + 8 x 257, the three dropout kernels, the mask), the pack with 2000 jobs against its 1024
workgroups.  Block indices >= 2^32 of the device Philox would need a 64 GB tensor and are not run here; philox_blocks covers them
on the CPU only.

Subnormals.  asr_cast_bf16 rounds float32 subnormals to nearest-even like every other value (it does not flush them): measured on
the MI355X, stated in include/asr_hip.h and asserted here with the rest of the special values.

Two findings of this module, fixed in csrc/:
  asr_cast_f32     with accum = 0 the n & 7 tail computed 0.f + value, which turns -0 into +0, while the 8-wide body copies the
                   bit pattern: the same input gave a different sign depending on where in the vector it stood.  Failing cases
                   with the old tail: test_cast_f32[1-0] and [7-0] (source -0 in the tail).  The tail now stores the value itself.
  host checks      asr_dropout_downsample_bwd / asr_dropout_downsample16_bwd accepted p = 1 (an infinite scale), asr_dropout_mask any
                   p, no dropout entry point looked at `style` (anything but 0 meant 1) or at a T2 beyond the frames that exist (rows
                   of z left unwritten, the backward reading past dz).  All refused now, as include/asr_hip.h states.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_encoder_glue_reference as R
from test_encoder_glue_reference import ACT_RELU, ACT_TANH, F32

gpu = pytest.mark.gpu

U24 = 2.0 ** -24
TAIL = 64
SENT = -776.0                                    # a bf16 value
SENT16 = int(R.bf16_bits(np.array([SENT], dtype=F32))[0])
NAN16 = 0x7fc0
E_ARG, E_UNSUPPORTED = -1, -3


# ---------------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------------
def _H():
    from src import hipabi as H
    return H


def _rc(name, *args):
    """The raw return code (H.call raises on anything but 0)."""
    return getattr(_H().lib(), name)(*args)


def _at(t, nbytes=0):
    return ctypes.c_void_p(t.data_ptr() + nbytes)


def _t16(bits):
    """uint16 numpy patterns -> int16 torch tensor."""
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16))


def _dev16(bits):
    return _t16(np.asarray(bits).reshape(-1)).cuda()


def _dev32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32).reshape(-1)).cuda()


def _out16(n, lead=0):
    """bf16 output of n elements behind `lead` untouched ones: NaN patterns, then the sentinel tail."""
    b = np.full(lead + n + TAIL, SENT16, dtype=np.uint16)
    b[lead:lead + n] = NAN16
    return _dev16(b)


def _out32(n, init=None, lead=0):
    b = np.full(lead + n + TAIL, SENT, dtype=F32)
    b[lead:lead + n] = np.nan if init is None else np.asarray(init, dtype=F32).reshape(-1)
    return _dev32(b)


def _back16(buf, n, lead=0):
    c = buf.cpu().numpy().view(np.uint16)
    assert (c[:lead] == SENT16).all() and (c[lead + n:] == SENT16).all(), 'the sentinel around the output was overwritten'
    return c[lead:lead + n]


def _back32(buf, n, lead=0):
    c = buf.cpu().numpy()
    assert (c[:lead] == SENT).all() and (c[lead + n:] == SENT).all(), 'the sentinel around the output was overwritten'
    return c[lead:lead + n]


def _same32(got, want):
    return np.array_equal(np.ascontiguousarray(got, dtype=F32).reshape(-1).view(np.uint32), np.ascontiguousarray(want, dtype=F32).reshape(-1).view(np.uint32))


def _untouched16(buf):
    c = buf.cpu().numpy().view(np.uint16)
    return bool((c[:-TAIL] == NAN16).all() and (c[-TAIL:] == SENT16).all())


def _untouched32(buf):
    c = buf.cpu().numpy()
    return bool(np.isnan(c[:-TAIL]).all() and (c[-TAIL:] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------
# casts
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('n', R.CAST_N)
def test_cast_bf16(n):
    """Eight elements per thread and an n & 7 tail; ties, overflow to infinity, signed zeros, subnormals and NaN sit in the body
    and in the tail.  The two largest n need a second pass of the capped grid, the last one with a tail."""
    H = _H()
    src, _, _ = R.cast_inputs(n)
    sd, dst = _dev32(src), _out16(n)
    H.call('asr_cast_bf16', H.ptr(sd), H.ptr(dst), n, H.stream_ptr())
    torch.cuda.synchronize()
    got, want = _back16(dst, n), R.bf16_bits(src)
    nan = np.isnan(src)
    sub = (np.abs(src) < 2.0 ** -126) & (src != 0)
    print('EXACT cast_bf16 n %d: wrong %d of %d, of them subnormal inputs %d of %d'
          % (n, int((got != want)[~nan].sum()), n, int((got != want)[sub].sum()), int(sub.sum())))
    assert np.isnan(R.bf16_value(got[nan])).all()
    assert np.array_equal(got[~nan & ~sub], want[~nan & ~sub])
    assert np.array_equal(got[sub], want[sub]), 'float32 subnormals must round to nearest-even, not flush (include/asr_hip.h)'


@gpu
@pytest.mark.parametrize('accum', [0, 1])
@pytest.mark.parametrize('n', R.CAST_N)
def test_cast_f32(n, accum):
    H = _H()
    _, src16, init = R.cast_inputs(n)
    sd, dst = _dev16(src16), _out32(n, init if accum else None)
    H.call('asr_cast_f32', H.ptr(sd), H.ptr(dst), n, accum, H.stream_ptr())
    torch.cuda.synchronize()
    got, val = _back32(dst, n), R.bf16_value(src16)
    with np.errstate(invalid='ignore'):
        want = init + val if accum else val
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all() and (n < 16 or int(nan.sum()) >= 1)
    assert _same32(got[~nan], want[~nan]), 'asr_cast_f32 n %d accum %d: %d wrong' % (n, accum, int((got.view(np.uint32) != want.view(np.uint32))[~nan].sum()))


# ---------------------------------------------------------------------------------------------------------------------
# the mask
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('seed', R.SEEDS)
@pytest.mark.parametrize('n', [1, 5, 1003, R.GRID_CAP + 259])
def test_dropout_mask_is_philox(n, seed):
    H = _H()
    for p in R.DROP_P:
        m = _out32(n)
        H.call('asr_dropout_mask', H.ptr(m), n, float(p), seed, H.stream_ptr())
        torch.cuda.synchronize()
        got = _back32(m, n)
        assert _same32(got, R.keep_mask(n, p, seed).astype(F32)), 'mask n %d p %g seed %#x' % (n, p, seed)
        if p == 0.0:
            assert (got == 1).all()


# ---------------------------------------------------------------------------------------------------------------------
# dropout + down-sampling
# ---------------------------------------------------------------------------------------------------------------------
def _poison_unselected(y, T2, rate, style):
    yn = y.copy()
    yn[:, ~R.selected_rows(y.shape[1], T2, rate, style)] = np.nan
    return yn


def _drop32(B, T, D, T2, rate, style, p, seed, y, dz, lead):
    """One forward and one backward of the fp32 kernels, every buffer `lead` floats off its 16-byte aligned base."""
    H = _H()
    st = H.stream_ptr()
    nz = dz.size
    yd = _dev32(np.concatenate([np.full(lead, np.nan, dtype=F32), _poison_unselected(y, T2, rate, style).reshape(-1)]))
    dzd = _dev32(np.concatenate([np.full(lead, np.nan, dtype=F32), dz.reshape(-1)]))
    z, dy = _out32(nz, None, lead), _out32(y.size, None, lead)
    H.call('asr_dropout_downsample_fwd', _at(yd, 4 * lead), _at(z, 4 * lead), B, T, D, T2, rate, style, float(p), seed, st)
    H.call('asr_dropout_downsample_bwd', _at(dzd, 4 * lead), _at(dy, 4 * lead), B, T, D, T2, rate, style, float(p), seed, st)
    torch.cuda.synchronize()
    return _back32(z, nz, lead), _back32(dy, y.size, lead)


def _check_drop32(B, T, D, rate, style, T2, p, seed, leads, tag=0):
    name = 'dropout B%d T%d D%d rate%d style%d T2 %d p %g seed %#x' % (B, T, D, rate, style, T2, p, seed)
    y, dz = R.drop_inputs(B, T, D, T2, rate, style, tag, rounded=False)
    mask, sc = R.keep_mask(B * T * D, p, seed).reshape(B, T, D), R.drop_scale(p)
    want_z = R.downsample_ref(_poison_unselected(y, T2, rate, style), mask, sc, rate, style, T2)
    want_dy = R.downsample_bwd_ref(dz, mask, sc, rate, style, T)
    for lead in leads:
        got_z, got_dy = _drop32(B, T, D, T2, rate, style, p, seed, y, dz, lead)
        assert _same32(got_z, want_z), name + ' lead %d: forward' % lead
        assert _same32(got_dy, want_dy), name + ' lead %d: backward' % lead


@gpu
@pytest.mark.parametrize('B,T,D', R.DROP_SHAPES32)
def test_dropout_downsample_fp32(B, T, D):
    """D = 5 takes the scalar kernel, D = 4, 8, 24 the vec4 kernel on aligned buffers and the scalar kernel on buffers that
    start one float later; the two must agree with the reference, hence with each other, bit for bit."""
    leads = (0, 1) if D in (4, 8) else (0,)
    for (rate, style, T2) in R.drop_variants(T):
        for p in R.DROP_P:
            for seed in R.SEEDS:
                _check_drop32(B, T, D, rate, style, T2, p, seed, leads)


@gpu
@pytest.mark.parametrize('case', [R.DROP_BIG_VEC4, R.DROP_BIG_SCALAR], ids=['vec4', 'scalar'])
def test_dropout_downsample_fp32_grid_stride(case):
    B, T, D, rate, style = case
    _check_drop32(B, T, D, rate, style, R.out_frames(T, rate, style), 0.3, R.SEEDS[1], (0,), tag=1)


def _layout16(T, D, layout):
    """(y_off, y_bstride, elements in front of row 0 of a batch entry that belong to nobody) of the two addressings."""
    if layout == 'padded':
        return D, (T + 2) * D
    return T * D + 8, T * D + 16


def _check_drop16(B, T, D, rate, style, T2, p, seed, layout, tag=0):
    H = _H()
    st = H.stream_ptr()
    name = 'dropout16 B%d T%d D%d rate%d style%d T2 %d p %g seed %#x %s' % (B, T, D, rate, style, T2, p, seed, layout)
    y, dz = R.drop_inputs(B, T, D, T2, rate, style, tag)
    mask, sc = R.keep_mask(B * T * D, p, seed).reshape(B, T, D), R.drop_scale(p)
    yn = _poison_unselected(y, T2, rate, style)
    want_z = R.bf16_bits(R.downsample_ref(yn, mask, sc, rate, style, T2))
    want_dy = R.bf16_bits(R.downsample_bwd_ref(dz, mask, sc, rate, style, T))
    y_off, y_bs = _layout16(T, D, layout)
    ybuf = np.full(y_off + B * y_bs, NAN16, dtype=np.uint16)                       # everything outside the addressed rows is NaN
    yb = R.bf16_bits(yn)
    for b in range(B):
        ybuf[y_off + b * y_bs:y_off + b * y_bs + T * D] = yb[b].reshape(-1)
    yd, dzd = _dev16(ybuf), _dev16(R.bf16_bits(dz))
    z, dy = _out16(dz.size), _out16(y.size)
    H.call('asr_dropout_downsample16_fwd', H.ptr(yd), y_bs, y_off, H.ptr(z), B, T, D, T2, rate, style, float(p), seed, st)
    H.call('asr_dropout_downsample16_bwd', H.ptr(dzd), H.ptr(dy), B, T, D, T2, rate, style, float(p), seed, st)
    torch.cuda.synchronize()
    assert np.array_equal(_back16(z, dz.size), want_z.reshape(-1)), name + ': forward'
    assert np.array_equal(_back16(dy, y.size), want_dy.reshape(-1)), name + ': backward'


@gpu
@pytest.mark.parametrize('layout', ['padded', 'slice'])
@pytest.mark.parametrize('B,T,D', R.DROP_SHAPES16)
def test_dropout_downsample16(B, T, D, layout):
    """y time-padded (y_off = D, y_bstride = (T+2) D: the y16 of the recurrence) and as a slice of a wider buffer (both beyond
    T D); pad rows, the gaps between batch entries and the rows the map does not select hold NaN."""
    for (rate, style, T2) in R.drop_variants(T):
        for p in R.DROP_P:
            for seed in R.SEEDS:
                _check_drop16(B, T, D, rate, style, T2, p, seed, layout)


@gpu
def test_dropout_downsample16_grid_stride():
    B, T, D, rate, style = R.DROP_BIG_16
    _check_drop16(B, T, D, rate, style, R.out_frames(T, rate, style), 0.3, R.SEEDS[1], 'padded', tag=1)


@gpu
@pytest.mark.parametrize('B,T,D', [(1, 1, 8), (3, 5, 24), (3, 11, 8), (1, 11, 320)])
def test_dropout16_keeps_what_fp32_keeps(B, T, D):
    """The bf16 form draws two Philox blocks per thread, the fp32 forms one block (vec4) or one word (scalar): on an input of
    ones the three must keep exactly the same elements for the same (B, T, D, p, seed)."""
    H = _H()
    st = H.stream_ptr()
    n = B * T * D
    one32, one16 = _dev32(np.ones(n, dtype=F32)), _dev16(np.full(n, 0x3f80, dtype=np.uint16))
    for p in (0.3, 0.5):
        for seed in R.SEEDS:
            z32, z32s, z16 = _out32(n), _out32(n, None, 1), _out16(n)
            lead1 = _dev32(np.ones(n + 1, dtype=F32))
            H.call('asr_dropout_downsample_fwd', H.ptr(one32), H.ptr(z32), B, T, D, T, 1, 0, p, seed, st)
            H.call('asr_dropout_downsample_fwd', _at(lead1, 4), _at(z32s, 4), B, T, D, T, 1, 0, p, seed, st)
            H.call('asr_dropout_downsample16_fwd', H.ptr(one16), T * D, 0, H.ptr(z16), B, T, D, T, 1, 0, p, seed, st)
            torch.cuda.synchronize()
            k32, k32s, k16 = _back32(z32, n) != 0, _back32(z32s, n, 1) != 0, R.bf16_value(_back16(z16, n)) != 0
            assert np.array_equal(k32, R.keep_mask(n, p, seed))
            assert np.array_equal(k16, k32) and np.array_equal(k32s, k32)


# ---------------------------------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('case', R.PACK_CASES, ids=lambda c: 'H%s_ND%s_Din%s_D%s' % c)
def test_rnn_pack_weights(case):
    """32 x 32 transpose tiles through LDS: Din and G on and off multiples of 32, one tile, with and without the projection weight,
    and 2000 tiles against 1024 workgroups (the job-stride loop with its barriers)."""
    H = _H()
    Hd, ND, Din, D = case
    c = R.pack_inputs(case)
    want = R.pack_ref(c['w_ih'], c['b_ih'], c['b_hh'], c['pj'], Hd, ND)
    G = ND * 4 * Hd
    wd, bi, bh = _dev32(c['w_ih']), _dev32(c['b_ih']), _dev32(c['b_hh'])
    w16, wT16, bias = _out16(G * Din), _out16(G * Din), _out32(G)
    if D is None:
        pjd = pj16 = pjT16 = None
    else:
        pjd, pj16, pjT16 = _dev32(c['pj']), _out16(D * D), _out16(D * D)
    H.call('asr_rnn_pack_weights', H.ptr(wd), H.ptr(bi), H.ptr(bh), H.ptr(pjd), H.ptr(w16), H.ptr(wT16), H.ptr(bias), H.ptr(pj16), H.ptr(pjT16),
           Hd, ND, Din, 0 if D is None else D, H.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_back16(w16, G * Din), want['wih16'].reshape(-1)), 'w_ih16'
    assert np.array_equal(_back16(wT16, G * Din), want['wihT16'].reshape(-1)), 'w_ihT16'
    assert _same32(_back32(bias, G), want['bias']), 'bias'
    if D is not None:
        assert np.array_equal(_back16(pj16, D * D), want['pj16'].reshape(-1)), 'pj16'
        assert np.array_equal(_back16(pjT16, D * D), want['pjT16'].reshape(-1)), 'pjT16'


# ---------------------------------------------------------------------------------------------------------------------
# activation backward
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('act', [ACT_TANH, ACT_RELU], ids=['tanh', 'relu'])
@pytest.mark.parametrize('n', R.ACT_N)
def test_act_bwd16(n, act):
    """ReLU is what the VGG stack calls it with: o holds +0, -0, the smallest positive bf16 and negatives."""
    H = _H()
    gr, o = R.act_inputs(n, act)
    gd, od, dpre = _dev16(R.bf16_bits(gr)), _dev16(R.bf16_bits(o)), _out16(n)
    H.call('asr_act_bwd16', H.ptr(gd), H.ptr(od), H.ptr(dpre), n, act, H.stream_ptr())
    torch.cuda.synchronize()
    got, want = _back16(dpre, n), R.act_bwd16_ref(gr, o, act)
    assert np.array_equal(got, want), 'act_bwd16 n %d act %d: %d wrong' % (n, act, int((got != want).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------------------
def _colsum_case(M, N, lda, perms, out2_modes):
    H = _H()
    st = H.stream_ptr()
    rpb = R.rows_per_block(M, N)
    for recipe in ('integer', 'random'):
        A, o1, o2 = R.colsum_inputs(M, N, lda, recipe)
        a64 = A[:, :N].double()
        col, absum = a64.sum(0).numpy(), a64.abs().sum(0).numpy()
        if recipe == 'integer':
            assert float(absum.max()) + 64 < 2 ** 24, 'the integer recipe must stay exact in fp32'
        Ad = A.to(torch.bfloat16).cuda()
        runs, worst = 0, (-1.0, 0.0, '')
        for perm_h in perms:
            dst = R.colsum_perm(N, perm_h)
            for with2 in out2_modes:
                name = 'colsum16 M%d N%d lda%d perm_h%d %s %s rows_per_block %d' % (M, N, lda, perm_h, 'out2' if with2 else 'NULL', recipe, rpb)
                b1, b2 = _out32(N, o1.numpy()), (_out32(N, o2.numpy()) if with2 else None)
                H.call('asr_colsum16', H.ptr(Ad), lda, M, N, H.ptr(b1), H.ptr(b2), perm_h, st)
                torch.cuda.synchronize()
                for what, buf, o in (('out', b1, o1), ('out2', b2, o2)):
                    if buf is None:
                        continue
                    got = _back32(buf, N)
                    want = o.double().numpy().copy()
                    terms = o.double().abs().numpy().copy()
                    want[dst] += col
                    terms[dst] += absum
                    assert not np.isnan(got).any(), (name, what)
                    err = np.abs(got.astype(np.float64) - want)
                    bound = (M + 1) * U24 * terms
                    runs += 1
                    frac = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))          # a column of zeros has bound 0
                    worst = max(worst, (float(frac.max()), float(err.max()), 'perm_h%d %s %s' % (perm_h, 'out2' if with2 else 'NULL', what)))
                    if recipe == 'integer':
                        assert _same32(got, want.astype(F32)), (name, what, float(err.max()))
                    else:
                        assert (err <= bound).all(), (name, what, float(err.max()), float(bound.min()))
        print('SUM   colsum16 M%d N%d lda%d %-7s rows_per_block %3d: %2d outputs judged, worst err / bound %.2e (err %.3e) at %s'
              % (M, N, lda, recipe, rpb, runs, worst[0], worst[1], worst[2]))


@gpu
@pytest.mark.parametrize('N', R.COLSUM_N)
@pytest.mark.parametrize('M', R.COLSUM_M)
def test_colsum16(M, N):
    """Eight row groups of eight columns per thread, 16 rows per unrolled trip and an 8-row remainder loop (M below 8, an odd
    number of row groups), N below, at and above one 256-column block, lda = N and N + 8 (the columns past N hold NaN),
    perm_h = 0 and N / 8, out2 given and NULL."""
    for lda in (N, N + 8):
        _colsum_case(M, N, lda, (0, N // 8), (True, False))


@gpu
@pytest.mark.parametrize('M,N', R.COLSUM_BIG)
def test_colsum16_row_blocks(M, N):
    """rows_per_block 64 and 128 of the host rule (the table above stays at 32), ten column blocks."""
    assert R.rows_per_block(M, N) in (64, 128)
    _colsum_case(M, N, N, (N // 8,), (True,))


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def _refused(name, code, outs, *args):
    H = _H()
    rc = _rc(name, *args)
    torch.cuda.synchronize()
    assert rc == code, (name, rc, code, args)
    last = H.lib().asr_last_error().decode()
    assert last.startswith(name + ':'), (name, last)
    for o in outs:
        assert (_untouched16(o) if o.dtype == torch.int16 else _untouched32(o)), name + ' wrote an output although it refused'


@gpu
def test_refusals_leave_the_outputs_untouched():
    """Each call returns its documented code, writes nothing and leaves asr_last_error naming the entry point."""
    H = _H()
    st = H.stream_ptr()
    n = 64
    s32, s16 = _dev32(np.ones(n + 8, dtype=F32)), _dev16(np.full(n + 8, 0x3f80, dtype=np.uint16))
    o16, o32 = _out16(n + 8), _out32(n + 8)
    # casts: misaligned pointers, n = 0
    _refused('asr_cast_bf16', E_ARG, [o16], _at(s32, 4), _at(o16), n, st)
    _refused('asr_cast_bf16', E_ARG, [o16], _at(s32), _at(o16, 2), n, st)
    _refused('asr_cast_bf16', E_ARG, [o16], _at(s32), _at(o16), 0, st)
    _refused('asr_cast_f32', E_ARG, [o32], _at(s16, 2), _at(o32), n, 0, st)
    _refused('asr_cast_f32', E_ARG, [o32], _at(s16), _at(o32, 4), n, 0, st)
    # activation backward: n % 8, a bad act
    _refused('asr_act_bwd16', E_ARG, [o16], _at(s16), _at(s16), _at(o16), 12, ACT_TANH, st)
    for act in (0, 3):
        _refused('asr_act_bwd16', E_ARG, [o16], _at(s16), _at(s16), _at(o16), 16, act, st)
    # column sums
    c1, c2 = _out32(16), _out32(16)
    _refused('asr_colsum16', E_ARG, [c1, c2], _at(s16), 8, 2, 16, _at(c1), _at(c2), 0, st)                    # lda < N
    _refused('asr_colsum16', E_UNSUPPORTED, [c1, c2], _at(s16), 16, 2, 12, _at(c1), _at(c2), 0, st)           # N % 8
    _refused('asr_colsum16', E_UNSUPPORTED, [c1, c2], _at(s16), 20, 2, 16, _at(c1), _at(c2), 0, st)           # lda % 8
    _refused('asr_colsum16', E_UNSUPPORTED, [c1, c2], _at(s16, 2), 16, 2, 16, _at(c1), _at(c2), 0, st)        # misaligned A
    _refused('asr_colsum16', E_ARG, [c1, c2], _at(s16), 16, 2, 16, _at(c1), _at(c2), 3, st)                   # 12 does not divide 16
    # pack: the projection weight without its copies
    G, Din, D = 8, 4, 4
    w16, wT16, bias, pj16 = _out16(G * Din), _out16(G * Din), _out32(G), _out16(D * D)
    for (a, b) in ((None, _at(pj16)), (_at(pj16), None)):
        _refused('asr_rnn_pack_weights', E_ARG, [w16, wT16, bias, pj16], _at(s32), _at(s32), _at(s32), _at(s32), _at(w16), _at(wT16), _at(bias), a, b,
                 2, 1, Din, D, st)
    _refused('asr_rnn_pack_weights', E_ARG, [w16, wT16, bias], _at(s32), _at(s32), _at(s32), None, _at(w16), _at(wT16), _at(bias), None, None,
             2, 3, Din, 0, st)                                                                                # ND = 3
    # dropout: the four down-sampling entry points share p, style and T2; the bf16 ones add their alignment rules
    B, T, D = 1, 4, 8

    def ds32(which, T2=2, rate=2, style=0, p=0.3, code=E_ARG):
        out = _out32(B * T * D)
        _refused('asr_dropout_downsample_' + which, code, [out], _at(s32), _at(out), B, T, D, T2, rate, style, p, 7, st)

    def ds16(which, T2=2, rate=2, style=0, p=0.3, code=E_ARG, d=D, y_off=0, y_bs=T * D, src_off=0, dst_off=0):
        out = _out16(B * T * D + 8)
        if which == 'fwd':
            _refused('asr_dropout_downsample16_fwd', code, [out], _at(s16, src_off), y_bs, y_off, _at(out, dst_off), B, T, d, T2, rate, style, p, 7, st)
        else:
            _refused('asr_dropout_downsample16_bwd', code, [out], _at(s16, src_off), _at(out, dst_off), B, T, d, T2, rate, style, p, 7, st)

    for which in ('fwd', 'bwd'):
        for ds in (ds32, ds16):
            for p in (1.0, 1.5, -0.1, float('nan')):
                ds(which, p=p)
            for style in (2, -1):
                ds(which, style=style)
            ds(which, T2=3, rate=2, style=0)                       # (T2 - 1) rate = 4 >= T
            ds(which, T2=3, rate=2, style=1)                       # T2 rate = 6 > T
            ds(which, T2=2, rate=3, style=1)
            ds(which, T2=5, rate=1, style=0)
            ds(which, T2=0)
        ds16(which, code=E_UNSUPPORTED, d=4)                       # D % 8
        ds16(which, code=E_UNSUPPORTED, src_off=2)
        ds16(which, code=E_UNSUPPORTED, dst_off=2)
    ds16('fwd', code=E_UNSUPPORTED, y_off=4)
    ds16('fwd', code=E_UNSUPPORTED, y_bs=T * D + 4)
    m = _out32(n)
    for p in (1.0, -0.5, float('nan')):
        _refused('asr_dropout_mask', E_ARG, [m], _at(m), n, p, 7, st)
    # the legal neighbours of the refused T2 go through
    for (T2, rate, style) in ((2, 2, 0), (2, 2, 1), (1, 3, 1), (4, 1, 0)):
        z = _out32(B * T * D)
        assert _rc('asr_dropout_downsample_fwd', _at(s32), _at(z), B, T, D, T2, rate, style, 0.3, 7, st) == 0
    torch.cuda.synchronize()
