"""Every kernel of the encoder LSTM recurrence (csrc/lstm.hip per step, lstm_persist.hip, lstm_persist2.hip, lstm_persist3.hip),
launched through the C ABI (asr_lstm_fwd / asr_lstm_bwd under asr_lstm_set_persistent(0 | 1 | 2), asr_lstm16_fwd / asr_lstm16_bwd)
and held per element to the step-forced float64 reference of tests/test_lstm_recurrence_reference.py, which owns the case tables
(shape -> template instantiation), the input recipe, the bounds and their derivation:
    fp32-stored |got - ref| <= 2e-5 max(1, |ref|);  bf16-stored: + 2^-8 |ref|
on the activated gates saved for BPTT, the cell states, y, and the pre-activation gradients the backward writes over the gates.

Conditions on every case: gates, y, c and dy are views into larger allocations with (at least) one batch row of guard on each
side, the workspace has 4 KiB of guard behind the size the query reports; all guards hold a bit pattern and must be bit-identical
after the forward and after the backward call.  y and c start as NaN (the forward must write all of them), the workspace of the
fp32-storage entry points starts poisoned (what each call leaves of the poison tells a persistent launch from the per-step path,
which must be the one the case table names; asr_lstm_plan tells the second generation from the first), the abort word of the
launch's status block must be 0, W_hh, dy and c must be untouched by the backward.  The third generation's y must have bit 14 of every bf16 clear and zero time pads.
Variants: `sat` (pre-activations of units 0..3 shifted by +30, -30, +95, -95: everything finite, |h| <= 1, the +-95 units exactly
1 / 0 / -1 although __expf overflows), `zero_in` (all-zero pre-activations), `zero_dy` (all gradients exactly 0).
test_epochs_on_one_workspace: 70 consecutive launch epochs of the third generation on one workspace per pass (the exchange
region rotates and the tag space repeats with period 32), every output bit-identical to epoch 1's - every sum of these kernels
has a fixed order.  Workspaces come from the hand-off pool of src/hipabi.py (never back to the allocator, see there).

Measured on the MI355X, worst error / bound per entry point over all 248 cases (every case prints its own four figures):
    asr_lstm16_* (third generation)   gates 0.986  c 0.014  y 0.986  dgates 0.990   <- the bf16 rounding itself, see the reference
    asr_lstm_* mode 1, bf16 (second)  gates 0.012  c 0.012  y 0.012  dgates 0.017      module: 2^-8 |ref| is reached by a correctly
    asr_lstm_* mode 2, fp32 (first)   gates 0.028  c 0.024  y 0.010  dgates 0.012      rounded store just above a power of two
    asr_lstm_* mode 2, bf16 (first)   gates 0.013  c 0.012  y 0.012  dgates 0.014
    asr_lstm_* mode 0, fp32 (steps)   gates 0.024  c 0.019  y 0.012  dgates 0.012
    asr_lstm_* mode 0, bf16 (steps)   gates 0.008  c 0.008  y 0.006  dgates 0.009
These are the figures of the torch fp32 stand-in of the reference module to within a factor of two: no kernel defect was found,
and every instantiation of the dispatch tables that a shape can reach computes what the float64 step says.  `zero_in` gave y and c
of exactly 0 on every entry point (printed, not asserted: it rests on rcp(2) being exactly 0.5)."""
import pytest
import torch

import test_lstm_recurrence_reference as R
from test_lstm_recurrence_reference import BF, F32, F64

gpu = pytest.mark.gpu

PATTERN = 0xA5
WS_GUARD = 4096


class Guarded:
    """`shape` of `dtype` inside a larger device allocation filled with PATTERN bytes; .data is the view the kernel gets."""

    def __init__(self, shape, dtype, fill=None):
        es = torch.empty((), dtype=dtype).element_size()
        n = 1
        for v in shape:
            n *= v
        row = n // shape[0] * es
        self.g = (row + 255) // 256 * 256                    # >= one batch row, keeps the view 256-byte aligned
        self.nbytes = n * es
        self.raw = torch.full((self.g + self.nbytes + self.g,), PATTERN, dtype=torch.uint8, device='cuda')
        self.data = self.raw[self.g:self.g + self.nbytes].view(dtype).view(shape)
        if fill is not None:
            self.data.fill_(fill)

    def put(self, x64):
        """upload float64 values that are exactly representable in the buffer's dtype"""
        v = x64.to(F32).to(self.data.dtype)
        assert torch.equal(v.to(F64), x64), 'input is not representable'
        self.data.copy_(v.contiguous().view(self.data.shape))
        return self

    def guards_ok(self):
        return bool((self.raw[:self.g] == PATTERN).all()) and bool((self.raw[self.g + self.nbytes:] == PATTERN).all())

    def bits(self):
        return self.raw[self.g:self.g + self.nbytes].clone()


class Workspace:
    """nbytes (as the query reports) + WS_GUARD from the hand-off pool; the guard holds PATTERN."""

    def __init__(self, Hh, nbytes, poison=None):
        self.Hh, self.n = Hh, int(nbytes)
        self.t = Hh.handoff_acquire(self.n + WS_GUARD, torch.device('cuda', torch.cuda.current_device()))
        if poison is not None:
            self.t[:self.n] = poison
        self.t[self.n:self.n + WS_GUARD] = PATTERN

    def guard_ok(self):
        return bool((self.t[self.n:self.n + WS_GUARD] == PATTERN).all())

    def word(self, off=0):
        return int(self.t[off:off + 4].view(torch.int32).item())

    def release(self):
        self.t[self.n:self.n + WS_GUARD] = 0
        self.Hh.handoff_release(self.t)


def _canon16(g16):
    """device bf16 gate-minor (B,T,ND,H,4) -> float64 canonical (B,T,ND,4,H)"""
    return g16.float().cpu().to(F64).permute(0, 1, 2, 4, 3).contiguous()


class Run:
    """One case on the device: buffers, the two calls, the stored outputs as float64 canonical tensors."""

    def __init__(self, Hh, case, inp):
        self.Hh, self.lib, self.case, self.inp = Hh, Hh.lib(), case, inp
        c = case
        B, T, H, ND = c.B, c.T, c.H, c.ND
        self.st = Hh.stream_ptr()
        self.whh = inp.whh.to(F32).reshape(ND, 4 * H, H).contiguous().cuda()
        self.whh_bits = self.whh.clone()
        self.bias2 = None if inp.bias2 is None else inp.bias2.to(F32).reshape(ND, 4 * H).contiguous().cuda()
        if c.api == 'lstm16':
            assert R.gen3(B, H, ND, False) is not None
            self.gates = Guarded((B, T, ND, H, 4), BF)
            self.y = Guarded((B, T + 2, ND * H), BF, float('nan'))
            self.dy = Guarded((B, T, ND * H), BF).put(inp.dy)
            nf, nb = (int(self.lib.asr_lstm16_workspace_bytes(B, H, ND, k)) for k in (0, 1))
            assert nf > 0 and nb > 0, 'shape must have a bf16-storage plan'
            self.wsf, self.wsb = Workspace(Hh, nf), Workspace(Hh, nb)
        else:
            self.gates = Guarded((B, T, ND, 4 * H), F32)
            self.y = Guarded((B, T, ND * H), F32, float('nan'))
            self.dy = Guarded((B, T, ND * H), F32).put(inp.dy)
            n = int(self.lib.asr_lstm_workspace_bytes(B, H, ND))
            self.wsf = self.wsb = Workspace(Hh, n, poison=0x5A)
            assert (self.lib.asr_lstm_plan(B, T, H, ND, c.prec) == 2) == R.route(c.api, c.mode, c.prec, B, H, ND, False).startswith('fwd2')
        self.c = Guarded((B, T, ND, H), F32, float('nan'))
        self.load_gates()

    def load_gates(self):
        gi = self.inp.gates_in
        self.gates.put(gi.permute(0, 1, 2, 4, 3) if self.case.api == 'lstm16' else gi)

    def _guards(self, when):
        for name in ('gates', 'y', 'c', 'dy'):
            assert getattr(self, name).guards_ok(), 'guard rows around %s overwritten by the %s call' % (name, when)
        assert self.wsf.guard_ok() and self.wsb.guard_ok(), 'guard behind the workspace overwritten by the %s call' % when
        assert torch.equal(self.whh, self.whh_bits), 'W_hh written by the %s call' % when

    def forward(self, epoch=1):
        c, Hh = self.case, self.Hh
        if c.api == 'lstm16':
            Hh.call('asr_lstm16_fwd', Hh.ptr(self.gates.data), Hh.ptr(self.whh), Hh.ptr(self.y.data), Hh.ptr(self.c.data), c.B, c.T, c.H, c.ND,
                    Hh.ptr(self.wsf.t), self.wsf.n, epoch, 0, self.st)
            word = self.wsf.word((epoch & 1) * 1024)
        else:
            Hh.call('asr_lstm_fwd', Hh.ptr(self.gates.data), Hh.ptr(self.whh), Hh.ptr(self.bias2), Hh.ptr(self.y.data), Hh.ptr(self.c.data),
                    c.B, c.T, c.H, c.ND, c.prec, Hh.ptr(self.wsf.t), self.wsf.n, self.st)
            word = self.wsf.word(0)
            # a persistent launcher clears its pass's bytes of the poisoned workspace, the per-step path the abort word alone
            per_step = self.wsf.word(4) == 0x5A5A5A5A
            assert per_step == R.route(c.api, c.mode, c.prec, c.B, c.H, c.ND, False).startswith('fwd0'), 'not the kernel the case table names'
        assert word == 0, 'abort word 0x%x after the forward call' % (word & 0xffffffff)

    def backward(self, epoch=1):
        c, Hh = self.case, self.Hh
        if c.api == 'lstm16':
            Hh.call('asr_lstm16_bwd', Hh.ptr(self.gates.data), Hh.ptr(self.whh), Hh.ptr(self.dy.data), Hh.ptr(self.c.data), c.B, c.T, c.H, c.ND,
                    Hh.ptr(self.wsb.t), self.wsb.n, epoch, 0, self.st)
            word = self.wsb.word((epoch & 1) * 1024)
        else:
            Hh.call('asr_lstm_bwd', Hh.ptr(self.gates.data), Hh.ptr(self.whh), Hh.ptr(self.dy.data), Hh.ptr(self.c.data),
                    c.B, c.T, c.H, c.ND, c.prec, Hh.ptr(self.wsb.t), self.wsb.n, self.st)
            word = self.wsb.word(0)
            # the per-step path keeps the transposed W_hh behind the status block, a persistent one its (cleared) granules
            per_step = float(self.wsb.t[256:260].view(F32).item()) == float(self.whh[0, 0, 0])
            assert per_step == R.route(c.api, c.mode, c.prec, c.B, c.H, c.ND, True).startswith('bwd0'), 'not the kernel the case table names'
        assert word == 0, 'abort word 0x%x after the backward call' % (word & 0xffffffff)

    def stored_gates(self):
        c = self.case
        if c.api == 'lstm16':
            return _canon16(self.gates.data)
        return self.gates.data.cpu().to(F64).view(c.B, c.T, c.ND, 4, c.H)

    def stored_y(self):
        c = self.case
        y = self.y.data[:, 1:c.T + 1] if c.api == 'lstm16' else self.y.data
        return y.float().cpu().to(F64).reshape(c.B, c.T, c.ND, c.H)

    def release(self):
        self.wsf.release()
        if self.wsb is not self.wsf:
            self.wsb.release()


def _mode(lib, case):
    return lib.asr_lstm_set_persistent(case.mode if case.api == 'lstm' else 1)


def _run(case):
    from src import hipabi as Hh
    lib = Hh.lib()
    scheme = R.case_scheme(case)
    inp = R.make_inputs(case.B, case.T, case.H, case.ND, scheme.store16, case.api == 'lstm', case.variant)
    old = _mode(lib, case)
    run = None
    try:
        run = Run(Hh, case, inp)
        run.forward()
        run._guards('forward')
        st = {'act': run.stored_gates(), 'c': run.c.data.cpu().to(F64), 'y': run.stored_y()}
        if case.api == 'lstm16':
            yb = run.y.data.view(torch.int16)
            assert not bool((yb & 0x4000).any()), 'bit 14 set in a stored bf16 h'
            assert not bool(yb[:, 0].any()) and not bool(yb[:, case.T + 1].any()), 'time pads of y are not zero'
        c_bits, dy_bits = run.c.bits(), run.dy.bits()
        run.backward()
        run._guards('backward')
        assert torch.equal(run.c.bits(), c_bits) and torch.equal(run.dy.bits(), dy_bits), 'the backward call wrote c or dy'
        st['dg'] = run.stored_gates()
    finally:
        lib.asr_lstm_set_persistent(old)
        if run is not None:
            run.release()
    R.assert_forced(scheme, inp, st, R.case_id(case) + ' ' + ' / '.join(R.case_routes(case)))
    if case.variant == 'sat':
        assert all(bool(torch.isfinite(v).all()) for v in st.values())
        assert float(st['y'].abs().max()) <= 1.0
        up, dn = st['act'][..., 2], st['act'][..., 3]                    # units shifted by +95 and -95, all four gates
        assert bool((up == 1.0).all()), 'a +95 pre-activation did not saturate to exactly 1'
        assert bool((dn[..., [0, 1, 3]] == 0.0).all()) and bool((dn[..., 2] == -1.0).all()), 'a -95 pre-activation did not saturate to exactly 0 / -1'
    elif case.variant == 'zero_in':
        print('zero_in: max |y| %.3e max |c| %.3e' % (float(st['y'].abs().max()), float(st['c'].abs().max())))
    elif case.variant == 'zero_dy':
        assert bool((st['dg'] == 0).all()), 'zero dy must give gradients that are exactly 0'


@gpu
@pytest.mark.parametrize('case', R.INST_CASES, ids=R.case_id)
def test_every_instantiation_vs_forced_float64(case):
    _run(case)


@gpu
@pytest.mark.parametrize('case', R.EDGE_CASES, ids=R.case_id)
def test_edges_vs_forced_float64(case):
    _run(case)


@gpu
def test_epochs_on_one_workspace():
    """Third generation, B=3 T=5 H=32 ND=2, one fresh zeroed workspace per pass (as src/functions.py keeps them), forward and
    backward at launch epochs 1..70: bit-identical outputs at every epoch, abort word of that epoch's status block 0; epoch 1 is
    held to the forced reference."""
    from src import hipabi as Hh
    lib = Hh.lib()
    case = R.EPOCH_CASE
    inp = R.make_inputs(case.B, case.T, case.H, case.ND, True, False)
    old = _mode(lib, case)
    run = None
    try:
        run = Run(Hh, case, inp)
        first, st = None, None
        for epoch in range(1, R.EPOCHS + 1):
            run.load_gates()
            run.y.data.fill_(float('nan'))
            run.c.data.fill_(float('nan'))
            run.forward(epoch)
            got = [run.y.bits(), run.c.bits(), run.gates.bits()]
            if epoch == 1:
                st = {'act': run.stored_gates(), 'c': run.c.data.cpu().to(F64), 'y': run.stored_y()}
            run.backward(epoch)
            got.append(run.gates.bits())
            if epoch == 1:
                first = got
                st['dg'] = run.stored_gates()
                continue
            same = [torch.equal(a, b) for a, b in zip(got, first)]
            assert all(same), 'epoch %d differs from epoch 1 in (y, c, activated gates, gradients): %s' % (epoch, same)
        run._guards('epoch')
    finally:
        lib.asr_lstm_set_persistent(old)
        if run is not None:
            run.release()
    R.assert_forced(R.S_B16, inp, st, 'epoch 1')
