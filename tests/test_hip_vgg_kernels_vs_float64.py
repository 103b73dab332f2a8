"""The fp32 support kernels of the VGG front-ends (csrc/vgg.hip: asr_permute_last2, asr_conv_weight_permute, asr_maxpool2x2_fwd /
_bwd, asr_ln_freq_fwd / _bwd), each called through the C ABI and held to the float64 restatements of
tests/test_vgg16_kernels_reference.py, which also owns the case tables and the input recipes.  Those restatements speak of
bordered images; the fp32 kernels work on unbordered channel-last images (B, T, F, C), so inputs go through interior() and the
expected outputs too.

Conditions on every case: fully written outputs start as NaN (index bytes: 0xAB), accumulated outputs (mode 2 of the weight permute,
dw / db of LayerNorm) start from random values and must equal init + contribution, every output buffer carries a 64-element
sentinel tail.

BIT FOR BIT: asr_permute_last2 (one case with more elements than the grid capped at 16384 x 256 threads); asr_conv_weight_permute
modes 0 and 1 against the unrounded packing rule and mode 2 as one float32 add per element onto random start values; pooling
values AND index bytes (ceil and floor sizes, post-ReLU images that are mostly ties, all-negative images, tied maxima from every
window position on, -inf entries and whole -inf windows), and the pooling backward, which writes all of dx.  Pooling inputs are
finite or -inf; NaN is out of scope.

LayerNorm over frequency follows tests/test_hip_glue_kernels_vs_float64.py: each case measures e32 = max |the same formula in
torch float32 on the CPU - float64| on ITS inputs and bounds the kernel by K_LN * e32 + 4 * 2^-23 * scale, scale = max(1, max
|reference|); every run prints a RATIO line before it asserts.  An element whose float64 pre-activation lies within 1e-5 * scale
of zero may gate either way: it is left out (at most 0.1 % of a case, a condition asserted on the CPU by the reference module), and
what its gate can change in dx of its row and in dw / db of its f is added to their bounds.  The backward reads the float64
statistics rounded to fp32, so it does not depend on the forward.

K_LN is the smallest power of two that clears the worst measured ratio by 2x over the runs whose e32 exceeds one ulp of scale,
capped at 4.  Measured on the MI355X (worst err_kernel / e32 per output over the 7 cases x relu 0 / 1 of test_ln_freq_fwd_bwd and
the two forward-only runs of test_ln_freq_fwd_grid_stride; excluded share = ambiguous gates of the relu = 1 run):
  output   runs  above   worst ratio at                       | incl. runs below one ulp
  y          16     14    1.56  B1 T2 F128 C8 relu1            |  1.56
  mean       16      4    1.97  B2 T4 F40 C64                  |  2.06  B1 T2 F128 C8
  rstd       16      2    0.74  B8 T1025 F2 C512               |  2.39  B1 T2 F128 C8
  dx         14      7    1.76  B8 T127 F2 C512 relu1          |  1.76                      (was infinite at B1 T1 F1 C8, see below)
  dw         14     11    1.47  B2 T4 F40 C64 relu0            |  1.47                      (was 2.91 at 527352 columns, see below)
  db         14      4    0.97  B8 T129 F8 C511 relu0          |  1.00  B3 T5 F20 C128 relu1 (was 3.88 at 527352 columns, see below)
  excluded share (relu = 1): B1 T1 F1 C8 0 of 8; B2 T3 F5 C6 0 of 180; B2 T4 F40 C64 1 of 20480 (0.0049 %); B1 T2 F128 C8 0 of 2048;
                             B3 T5 F20 C128 1 of 38400 (0.0026 %); B8 T127 F2 C512 1 of 1040384 (0.0001 %); B8 T129 F8 C511 320 of
                             4218816 (0.0076 %); B8 T1025 F2 C512 0 of 8396800
"above" counts the runs whose e32 exceeds one ulp of scale.  dw / db come out of atomics, so their figures move from run to run
(dw between 0.6 and 1.5 over four runs).  The kernel sums the F values of a row one after the other where torch sums pairwise, which
is the 1.97 on the mean at F = 40; 2 x 1.97 <= 4  ->  K_LN = 4.

Grid stride.  Every kernel of csrc/vgg.hip runs past its capped grid in some case: asr_permute_last2 at (5, 1024, 820),
asr_conv_weight_permute at (1024, 512), both pooling kernels in test_maxpool2x2_grid_stride, asr_ln_freq_fwd in
test_ln_freq_fwd_grid_stride (forward only: 4 198 400 columns), asr_ln_freq_bwd at B8 T129 F8 C511 (527352 columns against 512 x 1024
thread slots, the last workgroup partly out of range).  The common LN_CASES alone do not: their largest has 520192 columns.

Two findings of this module, fixed in csrc/vgg.hip.
  fused product    the one asr_ln_freq16_bwd had.  ln_f_bwd_kernel summed s1 = sum_f round(g w) in its first loop and evaluated
                   rstd (g w - s1 / F - xh s2) in the second, where the compiler fused g w into the subtraction: the unrounded
                   product minus the rounded one.  At F = 1 the gradient is exactly zero (torch float32 gives 0, so e32 = 0), rstd =
                   1 / sqrt(eps) = 316, and the kernel returned dx = 1.855e-05 (B1 T1 F1 C8 relu0: err 1.855e-05 against a bound
                   of 4.8e-07).  The product is now rounded on its own in both loops (mul_rounded): err 0 on that case.
  dw / db chain    one global atomic per workgroup and f: 2060 workgroups of 256 threads made a chain of 2060 fp32 roundings at the
                   magnitude of the finished sum, a random walk of about 4e-4 on sums near 500.  On 527352 columns with F = 2 that
                   gave dw 2.91 and db 3.88 times torch's float32 error (err 2.878e-04, e32 7.413e-05, bound 5.3e-04), which K = 4
                   does not clear by 2x and which a different order of the atomics can push over the bound.  The launch is now at
                   most 512 workgroups of 1024 threads: the same thread slots, a quarter of the chain, and faster (174 vs 190 us at
                   rows 16000 F 40 C 64).  The stride case has F = 8 because with two outputs e32 itself - the maximum of torch's
                   error over the F sums, which varied 16-fold between relu 0 and 1 - is a lottery.
The backward of the pooling also lacked the size check of the forward; it refuses what the forward refuses now.
"""
import math

import pytest
import torch

import test_vgg16_kernels_reference as R
from test_vgg16_kernels_reference import F32, F64, border, interior

gpu = pytest.mark.gpu

ULP32 = 2.0 ** -23
FLOOR = 4 * ULP32
K_LN = 4
TAIL = 64
SENT = -776.0
E_ARG, E_UNSUPPORTED = -1, -3


def _H():
    from src import hipabi as H
    return H


def _rc(name, *args):
    return getattr(_H().lib(), name)(*args)


def _out(shape, init=None, dtype=F32):
    n = math.prod(shape)
    if dtype == torch.uint8:
        t = torch.full((n + TAIL,), 0xCD, dtype=torch.uint8)
        t[:n] = 0xAB
        return t.cuda()
    t = torch.full((n + TAIL,), SENT, dtype=F32)
    t[:n] = float('nan') if init is None else init.reshape(-1).to(F32)
    return t.cuda()


def _back(buf, shape):
    """The output as it is (float32 or uint8), after checking the sentinel tail; a NaN left anywhere fails."""
    n = math.prod(shape)
    c = buf.cpu()
    if c.dtype == torch.uint8:
        assert bool((c[n:] == 0xCD).all()), 'the sentinel tail behind the output was overwritten'
        return c[:n].view(shape)
    assert bool((c[n:] == SENT).all()), 'the sentinel tail behind the output was overwritten'
    assert not bool(torch.isnan(c[:n]).any()), 'NaN left in an output the kernel must write'
    return c[:n].view(shape)


def _same_bits(got, want):
    """float32 tensors, bit for bit (tells -0 from +0)."""
    return torch.equal(got.contiguous().view(torch.int32), want.to(F32).contiguous().view(torch.int32))


def _untouched(buf):
    c = buf.cpu()
    if c.dtype == torch.uint8:
        return bool((c[:-TAIL] == 0xAB).all()) and bool((c[-TAIL:] == 0xCD).all())
    return bool(torch.isnan(c[:-TAIL]).all()) and bool((c[-TAIL:] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------
# layout changes
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('rows,A,Bd', [(1, 1, 1), (7, 3, 5), (3, 1, 9), (2, 64, 40), (5, 1024, 820)])
def test_permute_last2(rows, A, Bd):
    """out[r, b, a] = in[r, a, b]; the last case has 4 198 400 elements against 16384 x 256 = 4 194 304 threads."""
    H = _H()
    assert (rows, A, Bd) != (5, 1024, 820) or rows * A * Bd > 16384 * 256
    x = torch.randn(rows, A, Bd, generator=R.gen(4700 + rows))
    x.view(-1)[0] = -0.0
    xd, out = x.cuda(), _out((rows, Bd, A))
    H.call('asr_permute_last2', H.ptr(xd), H.ptr(out), rows, A, Bd, H.stream_ptr())
    torch.cuda.synchronize()
    assert _same_bits(_back(out, (rows, Bd, A)), x.transpose(1, 2))


@gpu
@pytest.mark.parametrize('Co,Ci', [(1, 1), (3, 2), (64, 1), (64, 64), (128, 64), (1024, 512)])
def test_conv_weight_permute(Co, Ci):
    """Modes 0 and 1 move values (no rounding: the fp32 convolution reads them as they are), mode 2 adds the packed gradient back
    onto a (Co,Ci,3,3) tensor that already holds something.  The last case has 4 718 592 elements against 16384 x 256 threads."""
    H = _H()
    assert (Co, Ci) != (1024, 512) or Co * Ci * 9 > 16384 * 256
    g = R.gen(4800 + Co + Ci)
    w = torch.randn(Co, Ci, 3, 3, generator=g)
    wd = w.cuda()
    for mode in (0, 1):
        want = R.pack_unrounded(w, mode)
        out = _out(tuple(want.shape))
        H.call('asr_conv_weight_permute', H.ptr(wd), H.ptr(out), Co, Ci, mode, H.stream_ptr())
        torch.cuda.synchronize()
        assert _same_bits(_back(out, tuple(want.shape)), want), 'mode %d' % mode
    src, init = torch.randn(Co, 9 * Ci, generator=g), torch.randn(Co, Ci, 3, 3, generator=g)
    sd, out = src.cuda(), _out((Co, Ci, 3, 3), init)
    H.call('asr_conv_weight_permute', H.ptr(sd), H.ptr(out), Co, Ci, 2, H.stream_ptr())
    torch.cuda.synchronize()
    assert _same_bits(_back(out, (Co, Ci, 3, 3)), R.fold_ref(src, init)), 'mode 2'


# ---------------------------------------------------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------------------------------------------------
def _pool_check(name, c, B, T, Fq, C, modes=(True, False)):
    H = _H()
    x = interior(c['x']).to(F32).contiguous()
    xd = x.cuda()
    ran = 0
    for ceil in modes:
        T2, F2 = R.pool_sizes(T, Fq, ceil)
        if T2 == 0 or F2 == 0:
            continue
        ran += 1
        tag = name + (' ceil' if ceil else ' floor')
        y, idx = _out((B, T2, F2, C)), _out((B, T2, F2, C), dtype=torch.uint8)
        H.call('asr_maxpool2x2_fwd', H.ptr(xd), H.ptr(y), H.ptr(idx), B, T, Fq, C, T2, F2, H.stream_ptr())
        torch.cuda.synchronize()
        y_ref, idx_ref = R.pool_ref(c['x'], T2, F2)
        got_y, got_idx = _back(y, (B, T2, F2, C)), _back(idx, (B, T2, F2, C))
        want_idx = interior(idx_ref).to(torch.uint8)
        print('EXACT %-44s values wrong %d, index bytes wrong %d of %d'
              % (tag, int((got_y.double() != interior(y_ref)).sum()), int((got_idx != want_idx).sum()), got_y.numel()))
        assert _same_bits(got_y, interior(y_ref)), tag + ': values'
        assert torch.equal(got_idx, want_idx), tag + ': index bytes'
        g = c['g'][:, :T2, :F2].to(F32).contiguous()
        gd, idx_d = g.cuda(), want_idx.contiguous().cuda()          # the reference's bytes: independent of the forward
        dx = _out((B, T, Fq, C))
        H.call('asr_maxpool2x2_bwd', H.ptr(gd), H.ptr(idx_d), H.ptr(dx), B, T, Fq, C, T2, F2, H.stream_ptr())
        torch.cuda.synchronize()
        got_dx = _back(dx, (B, T, Fq, C))
        assert _same_bits(got_dx, interior(R.pool_bwd_ref(border(g.double()), idx_ref, T, Fq))), tag + ': backward'
        assert bool((got_dx[:, 2 * T2:] == 0).all()) and bool((got_dx[:, :, 2 * F2:] == 0).all())
    return ran


@gpu
@pytest.mark.parametrize('kind', R.POOL_KINDS)
@pytest.mark.parametrize('case', R.POOL_CASES, ids=lambda c: 'B%d_T%d_F%d_C%d' % c)
def test_maxpool2x2(case, kind):
    """Ceil and floor output sizes (floor is left out where it gives no output); scan order (0,0),(0,1),(1,0),(1,1), strictly
    greater wins; in floor mode the rows and columns no window covers get zero."""
    B, T, Fq, C = case
    assert _pool_check('pool B%d T%d F%d C%d %s' % (B, T, Fq, C, kind), R.pool_inputs(case, kind), B, T, Fq, C) >= 1


@gpu
def test_maxpool2x2_grid_stride():
    """4 259 840 outputs and 17 039 360 inputs against 16384 x 256 threads: the forward takes a second pass, the backward five.
    Even sizes, so the ceil and the floor output sizes are the same and one of them runs."""
    B, T, Fq, C = R.POOL_CASE_STRIDE
    assert R.pool_sizes(T, Fq, True) == R.pool_sizes(T, Fq, False)
    assert _pool_check('pool B%d T%d F%d C%d post_relu' % (B, T, Fq, C), R.pool_inputs(R.POOL_CASE_STRIDE, 'post_relu'), B, T, Fq, C, (True,)) == 1


@gpu
@pytest.mark.parametrize('kind', R.POOL_EXTRA_KINDS)
def test_maxpool2x2_ties_and_neg_inf(kind):
    B, T, Fq, C = R.POOL_EXTRA_CASE
    assert _pool_check('pool B%d T%d F%d C%d %s' % (B, T, Fq, C, kind), R.pool_extra_inputs(kind), B, T, Fq, C) == 2


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm over frequency
# ---------------------------------------------------------------------------------------------------------------------
_LN_REF = {}


def _ln_refs(case, relu):
    if (case, relu) not in _LN_REF:
        c = R.ln_inputs(case)
        _LN_REF[(case, relu)] = (c, R.ln_ref(c['x'], c['w'], c['b'], c['dy'], relu, F64), R.ln_ref(c['x'], c['w'], c['b'], c['dy'], relu, F32))
    return _LN_REF[(case, relu)]


def _judge_ln(name, what, got, ref64, ref32, keep=None, slack=None):
    keep = torch.ones_like(ref64, dtype=torch.bool) if keep is None else keep
    scale = max(1.0, float(ref64.abs().max()))
    e32 = float((ref32.double() - ref64)[keep].abs().max())
    excess = (got.double() - ref64).abs() - (0.0 if slack is None else slack)
    err = max(0.0, float(excess[keep].max()))
    print('RATIO %-36s %-6s err %.3e e32 %.3e ratio %7.2f scale %.3g%s'
          % (name, what, err, e32, err / max(e32, 1e-300), scale, '' if e32 > ULP32 * scale else '  (e32 below one ulp of scale)'))
    assert err <= K_LN * e32 + FLOOR * scale, (name, what, err, e32, scale)


@gpu
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('case', R.LN_CASES + [R.LN_CASE_BWD_STRIDE], ids=lambda c: 'B%d_T%d_F%d_C%d' % c)
def test_ln_freq_fwd_bwd(case, relu):
    """One thread per (b, t, c) walking f.  F = 1 (constant rows), F = 128 (the LDS limit of the backward), B T C = 520192 (508
    workgroups of 1024: one pass of either kernel, just below the backward's 512) and B T C = 527352: a second pass of the
    backward's loop by 3 workgroups - wave_sum with lanes masked by `ok` in the last of them, the LDS accumulators carried from
    pass to pass.  The forward's cap of 16384 workgroups is crossed by test_ln_freq_fwd_grid_stride.  dw / db are accumulated
    onto random values."""
    H = _H()
    B, T, Fq, C = case
    name = 'ln B%d T%d F%d C%d relu%d' % (B, T, Fq, C, relu)
    c, r64, r32 = _ln_refs(case, relu)
    amb = R.ln_ambiguous(r64['pre64']) if relu else torch.zeros(B, T, Fq, C, dtype=torch.bool)
    assert int(amb.sum()) <= R.GATE_CAP * amb.numel()
    print('GATES %-36s excluded %d of %d (%.4f %%)' % (name, int(amb.sum()), amb.numel(), 100.0 * int(amb.sum()) / amb.numel()))
    keep = ~amb
    x = interior(c['x']).contiguous()
    xd, wd, bd, dyd = x.cuda(), c['w'].cuda(), c['b'].cuda(), interior(c['dy']).contiguous().cuda()
    rows = B * T
    y, stats = _out((B, T, Fq, C)), _out((B, T, C, 2))
    H.call('asr_ln_freq_fwd', H.ptr(xd), H.ptr(wd), H.ptr(bd), H.ptr(y), H.ptr(stats), rows, Fq, C, R.LN_EPS, relu, H.stream_ptr())
    std = torch.stack([r64['mean'], r64['rstd']], -1).to(F32).contiguous().cuda()          # the float64 statistics rounded to fp32
    dx, dw, db = _out((B, T, Fq, C)), _out((Fq,), c['dw0']), _out((Fq,), c['db0'])
    H.call('asr_ln_freq_bwd', H.ptr(dyd), H.ptr(xd), H.ptr(wd), H.ptr(bd), H.ptr(std), H.ptr(dx), H.ptr(dw), H.ptr(db), rows, Fq, C, relu,
           H.stream_ptr())
    torch.cuda.synchronize()
    got_st = _back(stats, (B, T, C, 2))
    _judge_ln(name, 'y', _back(y, (B, T, Fq, C)), interior(r64['y']), interior(r32['y']), keep)
    _judge_ln(name, 'mean', got_st[..., 0], r64['mean'], r32['mean'])
    _judge_ln(name, 'rstd', got_st[..., 1], r64['rstd'], r32['rstd'])
    # what the gate of an ambiguous element i can change: g_i in db[f_i], g_i xh_i in dw[f_i], and through the two row sums
    # rstd (|g_i w_i| + |xh_j| |g_i w_i xh_i|) / F in dx of every j of its row
    x64, g64 = x.double(), interior(c['dy']).double()
    w64 = c['w'].double().view(1, 1, Fq, 1)
    mean, rstd = r64['mean'].unsqueeze(2), r64['rstd'].unsqueeze(2)
    xh = (x64 - mean) * rstd
    a = amb.double()
    s_dx = rstd * ((a * (g64 * w64).abs()).sum(2, keepdim=True) + xh.abs() * (a * (g64 * w64 * xh).abs()).sum(2, keepdim=True)) / Fq
    _judge_ln(name, 'dx', _back(dx, (B, T, Fq, C)), interior(r64['dx']), interior(r32['dx']), keep, s_dx)
    _judge_ln(name, 'dw', _back(dw, (Fq,)), c['dw0'].double() + r64['dw'], c['dw0'] + r32['dw'], None, (a * (g64 * xh).abs()).sum((0, 1, 3)))
    _judge_ln(name, 'db', _back(db, (Fq,)), c['db0'].double() + r64['db'], c['db0'] + r32['db'], None, (a * g64.abs()).sum((0, 1, 3)))


@gpu
@pytest.mark.parametrize('relu', [0, 1])
def test_ln_freq_fwd_grid_stride(relu):
    """B T C = 4 198 400 threads' worth against the forward's 16384 x 256: the forward alone (y, mean, rstd; the backward's own
    stride loop runs in test_ln_freq_fwd_bwd), judged by the same rule."""
    H = _H()
    case = R.LN_CASE_FWD_STRIDE
    B, T, Fq, C = case
    name = 'ln fwd B%d T%d F%d C%d relu%d' % (B, T, Fq, C, relu)
    c = R.ln_inputs(case)
    x = interior(c['x']).contiguous()
    pre64, mean64, rstd64 = R.ln_pre(x.double(), c['w'].double(), c['b'].double())
    pre32, mean32, rstd32 = R.ln_pre(x, c['w'], c['b'])
    amb = R.ln_ambiguous(pre64) if relu else torch.zeros(B, T, Fq, C, dtype=torch.bool)
    assert int(amb.sum()) <= R.GATE_CAP * amb.numel()
    print('GATES %-36s excluded %d of %d (%.4f %%)' % (name, int(amb.sum()), amb.numel(), 100.0 * int(amb.sum()) / amb.numel()))
    gate = (pre64 > 0) if relu else torch.ones_like(pre64, dtype=torch.bool)
    xd, wd, bd = x.cuda(), c['w'].cuda(), c['b'].cuda()
    y, stats = _out((B, T, Fq, C)), _out((B, T, C, 2))
    H.call('asr_ln_freq_fwd', H.ptr(xd), H.ptr(wd), H.ptr(bd), H.ptr(y), H.ptr(stats), B * T, Fq, C, R.LN_EPS, relu, H.stream_ptr())
    torch.cuda.synchronize()
    got_st = _back(stats, (B, T, C, 2))
    _judge_ln(name, 'y', _back(y, (B, T, Fq, C)), pre64 * gate, pre32 * gate, ~amb)
    _judge_ln(name, 'mean', got_st[..., 0], mean64, mean32)
    _judge_ln(name, 'rstd', got_st[..., 1], rstd64, rstd32)


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_leave_the_outputs_untouched():
    """Pooling outputs larger than ceil(T/2) x ceil(F/2) are refused by the forward and by the backward, F = 129 by the LayerNorm
    backward; each returns its documented code, writes nothing and leaves asr_last_error naming the entry point."""
    H = _H()
    st = H.stream_ptr()
    B, T, Fq, C = 1, 5, 7, 8
    x = torch.zeros(B * T * Fq * C + 64).cuda()
    idx_in = torch.zeros(B * 4 * 5 * C, dtype=torch.uint8).cuda()
    for (T2, F2) in ((4, 4), (3, 5), (0, 4), (3, 0)):
        y, idx, dx = _out((B, 4, 5, C)), _out((B, 4, 5, C), dtype=torch.uint8), _out((B, T, Fq, C))
        for name, outs, args in (('asr_maxpool2x2_fwd', [y, idx], (H.ptr(x), H.ptr(y), H.ptr(idx))),
                                 ('asr_maxpool2x2_bwd', [dx], (H.ptr(x), H.ptr(idx_in), H.ptr(dx)))):
            rc = _rc(name, *args, B, T, Fq, C, T2, F2, st)
            torch.cuda.synchronize()
            assert rc == E_ARG, (name, T2, F2, rc)
            assert H.lib().asr_last_error().decode().startswith(name + ':')
            assert all(_untouched(o) for o in outs), name + ' wrote an output although it refused'
    for (T2, F2) in ((3, 4), (2, 3), (1, 1)):                        # ceil, floor and smaller sizes go through
        y, idx, dx = _out((B, T2, F2, C)), _out((B, T2, F2, C), dtype=torch.uint8), _out((B, T, Fq, C))
        H.call('asr_maxpool2x2_fwd', H.ptr(x), H.ptr(y), H.ptr(idx), B, T, Fq, C, T2, F2, st)
        H.call('asr_maxpool2x2_bwd', H.ptr(x), H.ptr(idx_in), H.ptr(dx), B, T, Fq, C, T2, F2, st)
        torch.cuda.synchronize()
        assert bool((_back(dx, (B, T, Fq, C)) == 0).all())
    Fq, C = 129, 8
    z = torch.zeros(2 * Fq * C + 64).cuda()
    dx, dw, db = _out((2, Fq, C)), _out((Fq,)), _out((Fq,))
    rc = _rc('asr_ln_freq_bwd', H.ptr(z), H.ptr(z), H.ptr(z), H.ptr(z), H.ptr(z), H.ptr(dx), H.ptr(dw), H.ptr(db), 2, Fq, C, 0, st)
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED and H.lib().asr_last_error().decode().startswith('asr_ln_freq_bwd:')
    assert _untouched(dx) and _untouched(dw) and _untouched(db)
    assert _rc('asr_permute_last2', H.ptr(z), H.ptr(dx), 0, 3, 5, st) == E_ARG and _untouched(dx)
    assert _rc('asr_conv_weight_permute', H.ptr(z), H.ptr(dx), 2, 2, 3, st) == E_ARG and _untouched(dx)
