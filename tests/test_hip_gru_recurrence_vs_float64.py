"""The GRU recurrence behind the RNN-LM (csrc/gru_rec.hip), launched through the C ABI (asr_gru_rec_fwd / asr_gru_rec_bwd) at
ASR_F32 and ASR_BF16 and held per element to the step-forced float64 reference of tests/test_gru_recurrence_reference.py, which
owns the case table, the input recipe, the bounds and their measurement:
    |got - ref| <= 4 x (deviation of the fp32 stand-in) x max(1, |ref|)
    fp32: forward 3.55e-06 backward 3.38e-06     bf16: forward 1.53e-06 backward 1.26e-06
on every element of y, saved, dgi, dgh and dh0.

Conditions on every case: gi, W_hh, b_hh, h0, y, saved, dy, dgi, dgh and dh0 are views into larger allocations with (at least)
one batch row of guard on each side, the workspace has 4 KiB of guard behind asr_gru_rec_workspace_bytes(B, H); all guards hold
a bit pattern and must be bit-identical after each call.  Outputs start as NaN and so does the workspace (the kernel must write
the transposed W_hh and the carry before it reads them).  The inputs of both calls (gi, W_hh, b_hh, h0, and y, saved, dy for
the backward) must be bit-identical afterwards.  A second run of the case must repeat every output bit for bit, saved = NULL
(inference) must give the same y, and dh0 = NULL against a requested dh0 must leave dgi and dgh unchanged.
Variants: `sat` (everything finite; r, z, n exactly 0 / 1 / -1 wherever the float64 value rounds to that in fp32), `zero_dy`
(all gradients exactly 0), `zero_w` (saved[..., 3H:] exactly 0).
test_unaligned_rows_equal_aligned: W_hh, h0, y (and dgh in the backward) moved 4 bytes off their 16-byte alignment force
vec = 0 at H % 4 == 0 (load8_slow in place of load8_raw + cvt8; what a view into a flat parameter buffer gives).  The k-steps,
the conversions and the MFMA order are the same, so every output must equal the aligned run's bit for bit.
test_refusals: every call the entry points refuse returns its code, names the entry point in asr_last_error and leaves
sentinel-filled outputs and workspace untouched.
test_layer_fn_accumulates: GRULayerFn.backward (src/lm.py) ADDS its parameter gradients to what the flat gradient views hold.

Measured on the MI355X, worst error / bound per entry point, precision and tensor over all cases (every case prints its own):
    asr_gru_rec_fwd  fp32   y 0.062  saved 0.207          asr_gru_rec_bwd  fp32   dgi 0.083  dgh 0.064  dh0 0.192
    asr_gru_rec_fwd  bf16   y 0.088  saved 0.172          asr_gru_rec_bwd  bf16   dgi 0.180  dgh 0.184  dh0 0.197
The kernel sits at or below the fp32 stand-in's own figures (0.25 of the bound): no defect was found in csrc/gru_rec.hip or in
dot_rows_cat / load8_raw / cvt8 / load8_slow of csrc/common.h.  Every guard, every input, every bit-for-bit comparison and every
refusal held.  Branches of dot_rows this file runs for the first time through this kernel: the bf16 vector path with a ragged
last k-step at K = H and K = 3H (H = 20, 36, 100, 344, 516, 1028); the second pass of the unrolled k-loop one k-step past its
boundary (bf16 K = 1028 forward and K = 1032 backward, fp32 K = 516 forward); vec = 0 at H % 4 == 0 (rows off their 16-byte
alignment); batch tiles of 15, 16 and 17 rows.
test_layer_fn_accumulates found the one defect of this work, outside the recurrence: asr_colsum added the bias gradients of a
small batch as three atomically ordered partial sums (fixed in csrc/elementwise.hip, see the test's docstring).
"""
import ctypes
import functools

import pytest
import torch

import test_gru_recurrence_reference as R
from test_gru_recurrence_reference import F32, F64
from test_hip_lstm_recurrence_vs_float64 import PATTERN, WS_GUARD, Guarded

gpu = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = -1, -3
NAN = float('nan')
WORST = {}                                     # (entry point, precision, tensor) -> worst error / bound so far, printed by every case


class Shifted(Guarded):
    """Guarded, the view moved `shift` bytes further into the allocation (4: off the 16-byte alignment); both guards keep their size"""

    def __init__(self, shape, dtype, fill=None, shift=0):
        Guarded.__init__(self, shape, dtype)
        if shift:
            self.raw = torch.full((self.g + shift + self.nbytes + self.g,), PATTERN, dtype=torch.uint8, device='cuda')
            self.g += shift
            self.data = self.raw[self.g:self.g + self.nbytes].view(dtype).view(shape)
        if fill is not None:
            self.data.fill_(fill)


class Work:
    """nbytes (as the query reports) of 0xFF bytes, NaN as floats, and WS_GUARD bytes of PATTERN behind them"""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.t = torch.full((self.n + WS_GUARD,), 0xFF, dtype=torch.uint8, device='cuda')
        self.t[self.n:] = PATTERN
        assert self.t.data_ptr() % 16 == 0

    def guard_ok(self):
        return bool((self.t[self.n:] == PATTERN).all())


class Run:
    """One case on the device at one precision: forward, then backward; the stored outputs as float64 tensors in .st and their
    bits in .bits.  shift: bytes by which W_hh, h0, y and dgh are moved off their alignment."""

    INPUTS_FWD = ('gi', 'whh', 'bhh', 'h0')
    INPUTS_BWD = ('gi', 'whh', 'bhh', 'h0', 'y', 'saved', 'dy')

    def __init__(self, Hh, case, prec, shift=0, with_saved=True, want_dh0=None):
        self.Hh, self.lib, self.case, self.prec = Hh, Hh.lib(), case, prec
        self.inp = inp = R.make_inputs(case)
        B, T, Hd = case.B, case.T, case.H
        want_dh0 = case.dh0 if want_dh0 is None else want_dh0
        self.buf = {'gi': Guarded((B, T, 3 * Hd), F32).put(inp.gi),
                    'whh': Shifted((3 * Hd, Hd), F32, shift=shift).put(inp.whh),
                    'bhh': Guarded((3 * Hd,), F32).put(inp.bhh),
                    'h0': None if inp.h0 is None else Shifted((B, Hd), F32, shift=shift).put(inp.h0),
                    'y': Shifted((B, T, Hd), F32, NAN, shift=shift),
                    'saved': Guarded((B, T, 4 * Hd), F32, NAN) if with_saved else None,
                    'dy': Guarded((B, T, Hd), F32).put(inp.dy),
                    'dgi': Guarded((B, T, 3 * Hd), F32, NAN),
                    'dgh': Shifted((B, T, 3 * Hd), F32, NAN, shift=shift),
                    'dh0': Guarded((B, Hd), F32, NAN) if want_dh0 else None}
        self.ws = Work(self.lib.asr_gru_rec_workspace_bytes(B, Hd))
        assert self.ws.n == 4 * ((3 * Hd * Hd + 63) // 64 * 64 + B * Hd)
        self.st, self.bits = {}, {}

    def p(self, name):
        b = self.buf[name]
        return None if b is None else self.Hh.ptr(b.data)

    def _snapshot(self, names):
        return {k: self.buf[k].bits() for k in names if self.buf[k] is not None}

    def _check(self, when, before):
        torch.cuda.synchronize()
        for k, b in self.buf.items():
            assert b is None or b.guards_ok(), 'guard rows around %s overwritten by the %s call' % (k, when)
        assert self.ws.guard_ok(), 'guard behind the workspace overwritten by the %s call' % when
        for k, bits in before.items():
            assert torch.equal(self.buf[k].bits(), bits), 'the %s call wrote its input %s' % (when, k)

    def _take(self, names):
        for k in names:
            b = self.buf[k]
            self.st[k] = None if b is None else b.data.cpu().to(F64)
            self.bits[k] = None if b is None else b.bits()

    def forward(self):
        c = self.case
        before = self._snapshot(self.INPUTS_FWD)
        self.Hh.call('asr_gru_rec_fwd', self.p('gi'), self.p('whh'), self.p('bhh'), self.p('h0'), c.B, c.T, c.H, self.prec, self.p('y'),
                     self.p('saved'), self.Hh.stream_ptr())
        self._check('forward', before)
        for k in ('dgi', 'dgh', 'dh0'):
            assert self.buf[k] is None or bool(torch.isnan(self.buf[k].data).all()), 'the forward call wrote %s' % k
        self._take(('y', 'saved'))
        return self

    def backward(self):
        c = self.case
        before = self._snapshot(self.INPUTS_BWD)
        self.Hh.call('asr_gru_rec_bwd', self.p('dy'), self.p('y'), self.p('saved'), self.p('h0'), self.p('whh'), c.B, c.T, c.H, self.prec,
                     self.p('dgi'), self.p('dgh'), self.p('dh0'), self.Hh.ptr(self.ws.t), self.ws.n, self.Hh.stream_ptr())
        self._check('backward', before)
        self._take(('dgi', 'dgh', 'dh0'))
        return self


def _same(a, b, names, what):
    for k in names:
        if a.bits[k] is not None and b.bits[k] is not None:
            assert torch.equal(a.bits[k], b.bits[k]), '%s: %s differs' % (what, k)


def _record(prec, rs):
    for k, (v, _) in rs.items():
        key = ('asr_gru_rec_fwd' if k in R.FWD_OUT else 'asr_gru_rec_bwd', R.PREC_NAME[prec], k)
        WORST[key] = max(WORST.get(key, 0.0), v)
    print('worst error / bound so far: ' + '  '.join('%s %s %s %.3f' % (k + (v,)) for k, v in sorted(WORST.items())))


@gpu
@pytest.mark.parametrize('prec', R.PRECS, ids=lambda p: R.PREC_NAME[p])
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_every_case_vs_forced_float64(case, prec):
    from src import hipabi as Hh
    run = Run(Hh, case, prec).forward().backward()
    st, Hd = run.st, case.H
    _record(prec, R.assert_forced(prec, run.inp, st, R.case_id(case)))
    if case.variant == 'sat':
        assert all(bool(torch.isfinite(v).all()) for v in st.values() if v is not None)
        ref = R.forced_forward(prec, run.inp, st['y'])[1][..., :3 * Hd].to(F32)
        exact = (ref == 0) | (ref.abs() == 1)
        assert bool(exact[..., :4].any()) and bool(exact[..., 2 * Hd:2 * Hd + 4].all())
        assert torch.equal(st['saved'][..., :3 * Hd].to(F32)[exact], ref[exact]), 'a saturated gate is not exactly 0 / 1 / -1'
    elif case.variant == 'zero_dy':
        assert all(not bool(st[k].any()) for k in ('dgi', 'dgh', 'dh0') if st[k] is not None), 'zero dy must give gradients that are exactly 0'
    elif case.variant == 'zero_w':
        assert not bool(st['saved'][..., 3 * Hd:].any()), 'gh_n is not exactly 0 with W_hh = 0 and b_hh = 0'
    # determinism: a second run; inference (saved = NULL); dh0 requested against dh0 = NULL
    again = Run(Hh, case, prec, want_dh0=not case.dh0).forward().backward()
    _same(run, again, ('y', 'saved', 'dgi', 'dgh'), 'second run, dh0 %s' % ('NULL' if case.dh0 else 'requested'))
    inf = Run(Hh, case, prec, with_saved=False).forward()
    _same(run, inf, ('y',), 'saved = NULL')
    if case.dh0:
        third = Run(Hh, case, prec).forward().backward()
        _same(run, third, ('y', 'saved', 'dgi', 'dgh', 'dh0'), 'second run')


@gpu
@pytest.mark.parametrize('prec', R.PRECS, ids=lambda p: R.PREC_NAME[p])
@pytest.mark.parametrize('Hd', R.ALIGN_H)
def test_unaligned_rows_equal_aligned(Hd, prec):
    from src import hipabi as Hh
    case = next(c for c in R.CASES if c.H == Hd and c.h0 and c.dh0 and c.variant == 'plain' and c.T >= 2)
    a = Run(Hh, case, prec).forward().backward()
    b = Run(Hh, case, prec, shift=4)
    for k in ('whh', 'h0', 'y', 'dgh'):
        assert b.buf[k].data.data_ptr() % 16 == 4 and a.buf[k].data.data_ptr() % 16 == 0
    b.forward().backward()
    _record(prec, R.assert_forced(prec, b.inp, b.st, R.case_id(case) + ' unaligned'))
    _same(a, b, ('y', 'saved', 'dgi', 'dgh', 'dh0'), 'rows 4 bytes off their alignment')


# ---- refusals ------------------------------------------------------------------------------------------------------------
SENTINEL = 777.0


class _Refusal:
    """buffers of one small shape (sized for it: a refusal that failed would launch inside them), outputs and workspace
    sentinel-filled"""

    def __init__(self, Hh, B, T, Hd):
        self.Hh, self.lib, self.B, self.T, self.H = Hh, Hh.lib(), B, T, Hd
        z = lambda *s: torch.zeros(s, device='cuda')
        o = lambda *s: torch.full(s, SENTINEL, device='cuda')
        self.inp = {'gi': z(B, T, 3 * Hd), 'whh': z(3 * Hd, Hd), 'bhh': z(3 * Hd), 'h0': z(B, Hd), 'dy': z(B, T, Hd)}
        self.out = {'y': o(B, T, Hd), 'saved': o(B, T, 4 * Hd), 'dgi': o(B, T, 3 * Hd), 'dgh': o(B, T, 3 * Hd), 'dh0': o(B, Hd)}
        self.n = int(self.lib.asr_gru_rec_workspace_bytes(B, Hd))
        assert self.n > 0
        self.ws = torch.full((self.n // 4 + 64,), SENTINEL, device='cuda')

    def args(self, entry, **over):
        t = dict(self.inp, **self.out)
        a = {k: self.Hh.ptr(v) for k, v in t.items()}
        a.update(B=self.B, T=self.T, H=self.H, prec=R.FP32, ws=self.Hh.ptr(self.ws), nbytes=self.n, st=self.Hh.stream_ptr())
        a.update(over)
        if entry == 'asr_gru_rec_fwd':
            return [a[k] for k in ('gi', 'whh', 'bhh', 'h0', 'B', 'T', 'H', 'prec', 'y', 'saved', 'st')]
        return [a[k] for k in ('dy', 'y', 'saved', 'h0', 'whh', 'B', 'T', 'H', 'prec', 'dgi', 'dgh', 'dh0', 'ws', 'nbytes', 'st')]

    def refused(self, entry, code, what, **over):
        rc = getattr(self.lib, entry)(*self.args(entry, **over))
        msg = self.lib.asr_last_error().decode()
        torch.cuda.synchronize()
        assert rc == code, '%s, %s: returned %d, not %d (%s)' % (entry, what, rc, code, msg)
        assert entry in msg, '%s, %s: asr_last_error does not name the entry point: %r' % (entry, what, msg)
        for k, v in list(self.out.items()) + [('workspace', self.ws)]:
            assert bool((v == SENTINEL).all()), '%s, %s: the refused call wrote %s' % (entry, what, k)


@gpu
def test_refusals():
    from src import hipabi as Hh
    lib = Hh.lib()
    assert lib.asr_gru_rec_workspace_bytes(0, 8) == 0
    assert lib.asr_gru_rec_workspace_bytes(8, 0) == 0
    FWD, BWD = 'asr_gru_rec_fwd', 'asr_gru_rec_bwd'
    r = _Refusal(Hh, 3, 1, 8)
    for entry, required in ((FWD, ('gi', 'whh', 'bhh', 'y')), (BWD, ('dy', 'y', 'saved', 'whh', 'dgi', 'dgh', 'ws'))):
        for k in required:
            r.refused(entry, E_ARG, '%s = NULL' % k, **{k: None})
        r.refused(entry, E_ARG, 'prec = 7', prec=7)
        for k in ('B', 'T', 'H'):
            r.refused(entry, E_ARG, '%s = 0' % k, **{k: 0})
            r.refused(entry, E_ARG, '%s = -1' % k, **{k: -1})
    r.refused(FWD, E_ARG, 'h0 == y', h0=Hh.ptr(r.out['y']))                   # T = 1: y is (B,1,H), as large as h0
    r.refused(BWD, E_ARG, 'workspace one byte short', nbytes=r.n - 1)
    r.refused(BWD, E_ARG, 'workspace 4 bytes off its alignment', ws=ctypes.c_void_p(r.ws.data_ptr() + 4))
    big = _Refusal(Hh, 1, 1, 2049)
    big.refused(FWD, E_UNSUPPORTED, 'H = 2049')
    big.refused(BWD, E_UNSUPPORTED, 'H = 2049')
    # and the same buffers are accepted as they stand
    Hh.check(getattr(lib, FWD)(*r.args(FWD)), FWD)
    Hh.check(getattr(lib, BWD)(*r.args(BWD)), BWD)
    torch.cuda.synchronize()
    assert all(not bool((v == SENTINEL).any()) for v in r.out.values())


# ---- GRULayerFn ------------------------------------------------------------------------------------------------------------
LAYER_GRADS = ('w_ih', 'w_hh', 'b_ih', 'b_hh')


@functools.lru_cache(maxsize=None)
def _layer_runs(prec):
    """H = 20, B = 17, T = 5, Din = 24: GRULayerFn forward + backward into zero-filled and into pattern-filled gradient views
    -> (pattern, gradients of the zero-filled run, gradients of the pattern-filled run)"""
    from src.lm import GRULayerFn
    Hd, B, T, Din = 20, 17, 5, 24
    g = torch.Generator().manual_seed(20175)
    k = 1.0 / Hd ** 0.5
    u = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) * k).cuda()

    class Layer(object):
        pass
    layer = Layer()
    layer.dim = Hd
    for n, shape in zip(LAYER_GRADS, ((3 * Hd, Din), (3 * Hd, Hd), (3 * Hd,), (3 * Hd,))):
        setattr(layer, n, u(*shape))
    x = torch.randn(B, T, Din, generator=g).cuda()
    dy = torch.randn(B, T, Hd, generator=g).cuda()
    pattern = {n: (torch.randn(getattr(layer, n).shape, generator=g) * 3 + 0.5).cuda() for n in LAYER_GRADS}
    assert all(bool((p != 0).all()) for p in pattern.values())

    def backward(start):
        for n in LAYER_GRADS:
            setattr(layer, 'g_' + n, start[n].clone())
        anchor = torch.zeros(1, device='cuda', requires_grad=True)
        xf = x.clone().requires_grad_(True)
        y = GRULayerFn.apply(anchor, xf, layer, prec)
        y.backward(dy)
        torch.cuda.synchronize()
        return {n: getattr(layer, 'g_' + n).clone() for n in LAYER_GRADS}, y.detach().clone(), xf.grad.clone()

    zero, y0, dx0 = backward({n: torch.zeros_like(p) for n, p in pattern.items()})
    acc, y1, dx1 = backward(pattern)
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    return pattern, zero, acc


@gpu
@pytest.mark.parametrize('prec', R.PRECS, ids=lambda p: R.PREC_NAME[p])
@pytest.mark.parametrize('name', LAYER_GRADS)
def test_layer_fn_accumulates(name, prec):
    """One backward into a pattern-filled g_w_ih, g_w_hh, g_b_ih, g_b_hh adds exactly what a zero-filled run produces:
    fl(pattern + g) against the device's one addition, 1 ulp of the sum.

    DEFECT FOUND HERE AND FIXED (csrc/elementwise.hip, asr_colsum2's host rule).  The weight gradients are one asr_gemm with
    accum = 1 and one slice: the accumulator is added to the pattern once.  The bias gradients are asr_colsum, which split the
    85 rows of this batch into cdiv(85, 32) = 3 row blocks and added each block's partial sum to the output with its own
    atomicAdd, in whatever order the blocks arrived: ((p + a) + b) + c against (a + b) + c, three roundings against two, and a
    bias gradient that differed between two runs of the same step.  Measured before the fix: g_w_ih 0.5, g_w_hh 0.5, g_b_ih 2.0,
    g_b_hh 1.5 to 3.0 ulp of the sum (varying from run to run).  asr_colsum now takes a matrix of up to 128 rows as one row block
    (the same two trips of its unrolled loop that a 128-row block of a larger matrix runs): a fixed order and one addition.
    Above 128 rows the partial sums of the row blocks are still added atomically, as the slices of the weight-gradient
    contraction are above 1024 rows.  Measured after the fix, both precisions: all four tensors 0.5 ulp."""
    pattern, zero, acc = _layer_runs(prec)
    assert bool((zero[name] != 0).any())
    want = pattern[name].double() + zero[name].double()
    ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp(min=2.0 ** -126))) - 23)
    worst = float(((acc[name].double() - want).abs() / ulp).max())
    print('g_%s %s: worst |got - (pattern + g)| = %.3f ulp of the sum' % (name, R.PREC_NAME[prec], worst))
    assert worst <= 1.0, 'g_%s is not pattern + gradient: off by %.3g ulp of the sum' % (name, worst)
