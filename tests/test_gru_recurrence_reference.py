"""Step-forced float64 reference of the GRU recurrence behind the RNN-LM (csrc/gru_rec.hip: asr_gru_rec_fwd / asr_gru_rec_bwd),
the case table of tests/test_hip_gru_recurrence_vs_float64.py, the input recipe, the bounds and the CPU checks of all four.
Nothing of the code under test is imported here.

THE STEP.  gi (B,T,3H) = x W_ih^T + b_ih in the gate order r | z | n, W_hh (3H,H), b_hh (3H), h0 (B,H) or none (zeros):
    gh = h_prev W_hh^T + b_hh;  r = s(gi_r + gh_r);  z = s(gi_z + gh_z);  n = tanh(gi_n + r gh_n);  h = (1 - z) n + z h_prev
    saved = r | z | n | gh_n  (B,T,4H)
Backward, as gru_rec_bwd_step walks it (t = T-1 .. 0, then t = -1 for dh0):
    dh_t = dy_t + carry + dgh_{t+1} W_hh     (no carry and no recurrent term at t = T-1)
    dpn = dh (1 - z)(1 - n^2);  dpz = dh (h_prev - n) z (1 - z);  dpr = dpn gh_n r (1 - r)
    dgi = (dpr, dpz, dpn);  dgh = (dpr, dpz, dpn r);  carry = dh z;  dh0 = carry + dgh_0 W_hh

THE FORCED REFERENCE.  A whole sequence against float64 needs a loose bound, because rounding differences compound over time.
Here step t is computed in float64 from what THE KERNEL ITSELF stored for the neighbouring step, so only one step's arithmetic
is compared: the forward takes the device's own y[:, t-1] (h0 at t = 0), the backward the device's own y, saved and dgh[:, t+1].
The carry dh z lives only in the kernel's workspace and is never an output, so the reference follows ITS OWN float64 chain for
it, from its own forced dh.  An error in the device's carry is one fp32 rounding per step, multiplied by z < 1 at every step
after: it grows as fp32 round-off does and not as a rounding difference that compounds.
prec = BF16: the kernel rounds both operands of each contraction to bf16, round to nearest even (cvt8 / load8_slow of
csrc/common.h): h_prev and W_hh in the forward, dgh_{t+1} and W_hh in the backward.  The reference rounds the same operands
(the device's stored fp32 values) and then sums exactly in float64.  b_hh, the h_prev of the blend z h_prev and of dpz, the
saved gates and dy stay fp32.  What remains is fp32 accumulation and the device's exp / tanh, so the bf16 bound has the form of
the fp32 one.

BOUNDS: measured, not chosen, applied per element: |got - ref| <= bound * max(1, |ref|), never a per-tensor maximum.
emulate(dtype = fp32) is the stand-in for a correct fp32 kernel: the same step in torch fp32 (torch.sigmoid / torch.tanh) with
the same operand rounding, each contraction summed by ONE fp32 accumulator over the MFMA's k-steps in turn (_dot; a BLAS sgemm
with its dozens of partial sums is no model of a kernel: at K = 6144 it is closer to float64 than a correct kernel can be, and
the bound would test the sum order).  Fed through the forced check as if it were the kernel, its largest deviation in units
of max(1, |ref|) over every case of the table is recorded below per precision, for the forward outputs (y, saved) and for the
backward outputs (dgi, dgh, dh0); test_recorded_stand_in_figures recomputes the four and prints recorded against measured.
The kernel gets FACTOR = 4 times the recorded figure (the project's usual factor: the sum order across the four waves and
inside the MFMA differs from the stand-in's, and so do the device's expf / tanhf).
    recorded  fp32: forward 8.87e-07 backward 8.44e-07     bf16: forward 3.82e-07 backward 3.16e-07
    bound     fp32: forward 3.55e-06 backward 3.38e-06     bf16: forward 1.53e-06 backward 1.26e-06
All four maxima are taken at H = 2048, B = 17 (gh_n of saved, dh0), and all four bounds are below the 2e-5 max(1, |ref|) the
encoder LSTM's recurrence is held to.  The bf16 figures are the smaller ones: a k-step of 32 products is summed at once and
the accumulator takes 64 (192) additions at H = 2048 where the fp32 one takes 512 (1536).

MUTATIONS (test_mutations_are_caught): each is applied to the float64 chain (emulate(dtype = float64, mut = ...), with the
precision's operand rounding, which alone stays below 1e-6 of the bound) and must exceed the kernel's bound on the named case.
The table is MUTATIONS below: b_hh dropped; r applied to gi_n + gh_n; the last 4 elements of K dropped where K % 32 != 0; the
last whole k-step (32 elements bf16, 4 fp32) dropped; k-steps 32 and above dropped on the bf16 path; the carry omitted; dgh_n
without the factor r; h_prev taken from t - 2; dh0 without the carry; batch row 16 reading row 0.  This replaces the argument
that a wrong row moves things by O(1).

CASE TABLE (CASES; test_case_table_covers_the_edges holds it to this list).  T <= 5 everywhere: the kernel launches per step.
    H 1, 3           fewer elements than one k-step, scalar loads
    H 15, 16, 17     the 16-unit column tile and its neighbours
    H 20, 36, 100    H % 4 == 0 and H % 32 != 0: vector loads with a ragged last k-step (load8_raw's clamped kend - 4 loads,
                     cvt8's selects); K = 3H of the backward is 60, 108, 300
    H 37             scalar loads, ragged
    H 344            backward K = 1032: 33 bf16 k-steps, the second pass of the unrolled loop runs with one live wave, tail 8
    H 516            fp32: 129 k-steps of 4, the second pass runs after 128 k-steps
    H 1028           forward bf16: 33 k-steps with a tail of 4
    H 2048           the maximum
    B 1, 15, 16, 17, 33 (2048 and 1028 with B in {1, 17} and T = 2 only);  T 1, 2, 5 (T = 1: no recurrent term in the backward,
    T = 2: exactly one);  h0 given and none;  dh0 requested and not.
    Variants: `sat` (gi of units 0..3, all three gates, shifted by +30, -30, +95, -95: everything finite, gates exactly 0 / 1 / -1
    where the float64 value rounds to that in fp32), `zero_dy` (every gradient exactly 0), `zero_w` (W_hh = 0 and b_hh = 0: gh and
    so saved[..., 3H:] exactly 0).
"""
import collections
import functools
import math

import pytest
import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
FP32, BF16 = 0, 1                      # `prec` of the C ABI
PRECS = (FP32, BF16)
PREC_NAME = {FP32: 'fp32', BF16: 'bf16'}
FWD_OUT, BWD_OUT = ('y', 'saved'), ('dgi', 'dgh', 'dh0')

# largest deviation of the fp32 stand-in from the forced float64 reference in units of max(1, |ref|), over every case of CASES
# (stand_in_deviation; fp32 products and activations differ in the last bit between hosts, so test_recorded_stand_in_figures prints
# the measured value beside the recorded one)
STAND_IN_DEV = {(FP32, 'fwd'): 8.87e-07, (FP32, 'bwd'): 8.44e-07, (BF16, 'fwd'): 3.82e-07, (BF16, 'bwd'): 3.16e-07}
FACTOR = 4


def bound(prec, name):
    """the kernel's bound on output `name`, in units of max(1, |ref|)"""
    return FACTOR * STAND_IN_DEV[(prec, 'fwd' if name in FWD_OUT else 'bwd')]


def rbf(x):
    """(__bf16)x of fp32 values held in any float dtype: round to nearest even, returned in the dtype of x."""
    return x.to(F32).to(BF).to(x.dtype)


def _op(x, prec):
    return rbf(x) if prec == BF16 else x


# ---------------------------------------------------------------------------------------------------------------------
# one step, any leading dims: the ONLY arithmetic of the reference (forced and unforced use the same functions)
# ---------------------------------------------------------------------------------------------------------------------
def cell_fwd(gi, gh, h_prev, mut=None):
    """gi, gh (..., 3H), h_prev (..., H) -> h (..., H), saved (..., 4H)"""
    Hd = h_prev.shape[-1]
    r = torch.sigmoid(gi[..., :Hd] + gh[..., :Hd])
    z = torch.sigmoid(gi[..., Hd:2 * Hd] + gh[..., Hd:2 * Hd])
    ghn = gh[..., 2 * Hd:]
    n = torch.tanh(r * (gi[..., 2 * Hd:] + ghn) if mut == 'r_all' else gi[..., 2 * Hd:] + r * ghn)
    return (1 - z) * n + z * h_prev, torch.cat([r, z, n, ghn], -1)


def cell_bwd(dh, saved, h_prev, mut=None):
    """dh (..., H) -> dgi, dgh (..., 3H) and the carry dh z for the step before"""
    Hd = dh.shape[-1]
    r, z, n, ghn = (saved[..., k * Hd:(k + 1) * Hd] for k in range(4))
    dpn = dh * (1 - z) * (1 - n * n)
    dpz = dh * (h_prev - n) * z * (1 - z)
    dpr = dpn * ghn * r * (1 - r)
    return torch.cat([dpr, dpz, dpn], -1), torch.cat([dpr, dpz, dpn if mut == 'dghn_no_r' else dpn * r], -1), dh * z


def _keep(K, prec, mut):
    """the k a mutated contraction still sums (None: all of them)"""
    keep = torch.ones(K, dtype=torch.bool)
    if mut == 'tail4' and K % 32 != 0:
        keep[max(K - 4, 0):] = False
    elif mut == 'last_kstep':
        ks = 32 if prec == BF16 else 4
        keep[(K - 1) // ks * ks:] = False
    elif mut == 'ks32' and prec == BF16:
        keep[32 * 32:] = False
    else:
        return None
    return keep


def _rows(a, mut):
    if mut == 'row16' and a.shape[0] > 16:
        a = a.clone()
        a[16] = a[0]
    return a


def _dot(a, Wt, prec):
    """a (..., K) . Wt (K, N).  float64: the exact sum, as far as this module is concerned.  fp32 (the stand-in): ONE fp32
    accumulator that takes the k-steps of the MFMA (4 elements fp32, 32 bf16) one after the other, the order of a plain
    one-wave kernel.  A BLAS sgemm keeps dozens of partial sums per output and is closer to float64 at K = 6144 than any
    kernel with one accumulator per wave can be; the stand-in is to stand for a correct KERNEL."""
    if a.dtype != F32:
        return a @ Wt
    ks = 32 if prec == BF16 else 4
    Wt = Wt.contiguous()
    acc = torch.zeros(a.shape[:-1] + (Wt.shape[1],), dtype=F32)
    for k in range(0, Wt.shape[0], ks):
        acc = acc + a[..., k:k + ks] @ Wt[k:k + ks]
    return acc


def rec_fwd(h_op, W, prec, mut=None):
    """h_op (B, ..., H), W (3H, H), both already rounded for `prec` -> h W^T (B, ..., 3H)"""
    keep = _keep(W.shape[1], prec, mut)
    if keep is not None:
        W = W * keep.to(W.dtype)
    return _dot(_rows(h_op, mut), W.t(), prec)


def rec_bwd(dgh_op, W, prec, mut=None):
    """dgh_op (B, ..., 3H), W (3H, H) -> dgh W (B, ..., H); the reduction runs over K = 3H"""
    keep = _keep(W.shape[0], prec, mut)
    if keep is not None:
        W = W * keep.to(W.dtype)[:, None]
    return _dot(_rows(dgh_op, mut), W, prec)


# ---------------------------------------------------------------------------------------------------------------------
# inputs and cases
# ---------------------------------------------------------------------------------------------------------------------
Inputs = collections.namedtuple('Inputs', 'gi whh bhh h0 dy')          # float64 tensors holding fp32 values; h0 may be None
Case = collections.namedtuple('Case', 'H B T h0 dh0 variant')
SAT_SHIFT = (30.0, -30.0, 95.0, -95.0)          # added to all three gates of units 0, 1, 2, 3 (variant 'sat')
VARIANTS = ('plain', 'sat', 'zero_dy', 'zero_w')


def _c(H, B, T, h0=True, dh0=True, variant='plain'):
    return Case(H, B, T, h0, dh0, variant)


CASES = (
    _c(1, 1, 1, False, False), _c(1, 17, 2), _c(3, 15, 5), _c(3, 1, 1, False, False),
    _c(15, 16, 2), _c(15, 33, 5, False, False), _c(16, 1, 1), _c(16, 17, 5, False, False), _c(16, 33, 2), _c(17, 15, 5, True, False),
    _c(17, 16, 1, False, True),
    _c(20, 17, 5), _c(20, 1, 2, False, False), _c(36, 16, 5), _c(36, 15, 2, False, True), _c(100, 33, 5), _c(100, 15, 1, False, False),
    _c(100, 17, 2, True, False),
    _c(37, 17, 5), _c(37, 33, 2, False, False),
    _c(344, 17, 2), _c(344, 1, 5, False, False), _c(344, 16, 5),
    _c(516, 17, 2), _c(516, 15, 5, False, False),
    _c(1028, 17, 2), _c(1028, 1, 2, False, False),
    _c(2048, 17, 2), _c(2048, 1, 2, False, False),
    _c(20, 17, 5, True, True, 'sat'), _c(344, 16, 2, False, True, 'sat'),
    _c(36, 17, 5, True, True, 'zero_dy'), _c(16, 15, 2, False, False, 'zero_dy'),
    _c(100, 17, 2, True, True, 'zero_w'), _c(37, 16, 5, False, False, 'zero_w'),
)
ALIGN_H = (16, 100, 344)               # forced vec = 0 at H % 4 == 0: the cases of these H with h0 and dh0


def case_id(c):
    return 'H%d-B%d-T%d-%s-%s%s' % (c.H, c.B, c.T, 'h0' if c.h0 else 'noh0', 'dh0' if c.dh0 else 'nodh0', '' if c.variant == 'plain' else '-' + c.variant)


def case_named(cid):
    return next(c for c in CASES if case_id(c) == cid)


@functools.lru_cache(maxsize=None)
def make_inputs(case):
    """Seeded, generated in float64 and made exactly representable in fp32: gi = 0.7 randn, W_hh and b_hh ~ U(-1/sqrt(H), 1/sqrt(H))
    (nn.GRU's initialisation), |h0| <= 0.8 uniform, dy = randn.  The result is shared: never written."""
    Hd, B, T = case.H, case.B, case.T
    g = torch.Generator().manual_seed(1000003 * B + 10007 * T + 101 * Hd + VARIANTS.index(case.variant))
    k = 1.0 / Hd ** 0.5
    gi = torch.randn(B, T, 3 * Hd, generator=g, dtype=F64) * 0.7
    whh = (torch.rand(3 * Hd, Hd, generator=g, dtype=F64) * 2 - 1) * k
    bhh = (torch.rand(3 * Hd, generator=g, dtype=F64) * 2 - 1) * k
    h0 = (torch.rand(B, Hd, generator=g, dtype=F64) * 2 - 1) * 0.8
    dy = torch.randn(B, T, Hd, generator=g, dtype=F64)
    if case.variant == 'sat':
        for u, s in enumerate(SAT_SHIFT):
            gi[..., u::Hd] += s
    elif case.variant == 'zero_dy':
        dy = torch.zeros_like(dy)
    elif case.variant == 'zero_w':
        whh, bhh = torch.zeros_like(whh), torch.zeros_like(bhh)
    f = lambda t: t.to(F32).to(F64)
    return Inputs(f(gi), f(whh), f(bhh), f(h0) if case.h0 else None, f(dy))


def _h_prev(inp, y):
    """(B,T,H): h0 (zeros if none) followed by y[:, :-1]"""
    B, T, Hd = y.shape
    first = y.new_zeros(B, 1, Hd) if inp.h0 is None else inp.h0.to(y.dtype)[:, None]
    return torch.cat([first, y[:, :-1]], 1)


# ---------------------------------------------------------------------------------------------------------------------
# forced reference
# ---------------------------------------------------------------------------------------------------------------------
def forced_forward(prec, inp, k_y):
    """float64 y and saved of EVERY step, each from the kernel's stored y of the step before."""
    hp = _h_prev(inp, k_y)
    gh = rec_fwd(_op(hp, prec), _op(inp.whh, prec), prec) + inp.bhh
    return cell_fwd(inp.gi, gh, hp)


def forced_backward(prec, inp, k_y, k_saved, k_dgh, want_dh0):
    """float64 dgi, dgh of every step and dh0: the recurrent term from the kernel's stored dgh of the step after, coefficients
    from the stored y and saved of the forward call, the carry in float64 from this function's own dh."""
    B, T, Hd = k_y.shape
    hp = _h_prev(inp, k_y)
    rec = rec_bwd(_op(k_dgh, prec), _op(inp.whh, prec), prec)                  # rec[:, t] is the recurrent term of dh_{t-1}
    dgi, dgh = torch.empty_like(k_dgh), torch.empty_like(k_dgh)
    carry = torch.zeros(B, Hd, dtype=F64)
    for t in range(T - 1, -1, -1):
        dh = inp.dy[:, t] + (carry + rec[:, t + 1] if t < T - 1 else 0)
        dgi[:, t], dgh[:, t], carry = cell_bwd(dh, k_saved[:, t], hp[:, t])
    return dgi, dgh, (carry + rec[:, 0]) if want_dh0 else None


def units(got, ref):
    """worst |got - ref| / max(1, |ref|) and where; NaN / inf in `got` counts as infinite."""
    r = (got - ref).abs() / ref.abs().clamp(min=1.0)
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float('inf')))
    k = int(r.argmax())
    return float(r.reshape(-1)[k]), tuple(int(v) for v in torch.unravel_index(torch.tensor(k), r.shape))


def forced_errors(prec, inp, st):
    """st: the kernel's stored outputs as float64 tensors: y, saved, and after the backward call dgi, dgh, dh0 (None if not
    requested).  -> {name: (worst error in units of max(1, |ref|), index)}"""
    ry, rs = forced_forward(prec, inp, st['y'])
    out = {'y': units(st['y'], ry)}
    if st.get('saved') is not None:
        out['saved'] = units(st['saved'], rs)
    if st.get('dgh') is not None:
        want = st.get('dh0') is not None
        rdgi, rdgh, rdh0 = forced_backward(prec, inp, st['y'], st['saved'], st['dgh'], want)
        out['dgi'], out['dgh'] = units(st['dgi'], rdgi), units(st['dgh'], rdgh)
        if want:
            out['dh0'] = units(st['dh0'], rdh0)
    return out


def assert_forced(prec, inp, st, what=''):
    es = forced_errors(prec, inp, st)
    rs = {k: (v[0] / bound(prec, k), v[1]) for k, v in es.items()}
    print('forced %s %s (error / bound): %s' % (PREC_NAME[prec], what, '  '.join('%s %.3f @%s' % (k, v[0], v[1]) for k, v in rs.items())))
    bad = {k: v for k, v in rs.items() if not v[0] <= 1.0}
    assert not bad, 'outside the forced float64 bound (error / bound, index) %s %s: %s' % (PREC_NAME[prec], what, bad)
    return rs


# ---------------------------------------------------------------------------------------------------------------------
# the chain unrolled over T, its own values handed on: float64 (parity, mutations) or fp32 (the stand-in)
# ---------------------------------------------------------------------------------------------------------------------
def emulate(prec, inp, dtype=F32, want_dh0=True, mut=None):
    """-> {y, saved, dgi, dgh, dh0} as float64 tensors, computed in `dtype` with the operand rounding of `prec`."""
    gi, whh, bhh, dy = (t.to(dtype) for t in (inp.gi, inp.whh, inp.bhh, inp.dy))
    B, T, G = gi.shape
    Hd = G // 3
    W = _op(whh, prec)
    if mut == 'no_bhh':
        bhh = torch.zeros_like(bhh)
    hs = [torch.zeros(B, Hd, dtype=dtype) if inp.h0 is None else inp.h0.to(dtype)]
    saved = []
    for t in range(T):
        hp = hs[max(t - 1, 0)] if mut == 'stale_h' else hs[t]
        gh = rec_fwd(_op(hp, prec), W, prec, mut) + bhh
        h, sv = cell_fwd(gi[:, t], gh, hp, mut)
        hs.append(h)
        saved.append(sv)
    dgi, dgh = [None] * T, [None] * T
    carry = torch.zeros(B, Hd, dtype=dtype)
    for t in range(T - 1, -1, -1):
        dh = dy[:, t]
        if t < T - 1:
            dh = dh + rec_bwd(_op(dgh[t + 1], prec), W, prec, mut) + (0 if mut == 'no_carry' else carry)
        dgi[t], dgh[t], carry = cell_bwd(dh, saved[t], hs[t], mut)          # the backward's h_prev is y[t-1] as stored
    dh0 = None
    if want_dh0:
        dh0 = rec_bwd(_op(dgh[0], prec), W, prec, mut) + (0 if mut == 'dh0_no_carry' else carry)
    out = {'y': torch.stack(hs[1:], 1), 'saved': torch.stack(saved, 1), 'dgi': torch.stack(dgi, 1), 'dgh': torch.stack(dgh, 1), 'dh0': dh0}
    return {k: None if v is None else v.to(F64) for k, v in out.items()}


def stand_in_deviation(cases=CASES):
    """{(prec, 'fwd' | 'bwd'): (largest deviation of the fp32 stand-in in units of max(1, |ref|), case id, tensor)}"""
    worst = {}
    for c in cases:
        inp = make_inputs(c)
        for prec in PRECS:
            for k, (e, _) in forced_errors(prec, inp, emulate(prec, inp, F32, c.dh0)).items():
                key = (prec, 'fwd' if k in FWD_OUT else 'bwd')
                if e >= worst.get(key, (-1.0,))[0]:
                    worst[key] = (e, case_id(c), k)
    return worst


# name, precision, the case that must catch it
MUTATIONS = (
    ('no_bhh', BF16, 'H2048-B17-T2-h0-dh0'),             # b_hh dropped (|b_hh| <= 0.022 at H = 2048)
    ('r_all', FP32, 'H16-B1-T1-h0-dh0'),                 # n = tanh(r (gi_n + gh_n))
    ('tail4', BF16, 'H1028-B17-T2-h0-dh0'),              # last 4 elements of K: the whole ragged k-step of the forward
    ('tail4', FP32, 'H20-B17-T5-h0-dh0'),                # ... and of K = 20 forward, K = 60 backward
    ('last_kstep', BF16, 'H344-B17-T2-h0-dh0'),          # backward K = 1032: k-step 32 of 33 holds the last 8 elements
    ('last_kstep', FP32, 'H516-B17-T2-h0-dh0'),          # fp32 k-step 128 of 129: the second pass of the unrolled loop
    ('ks32', BF16, 'H1028-B1-T2-noh0-nodh0'),            # k-steps 32 and above of the bf16 path, forward K = 1028 (and backward)
    ('ks32', BF16, 'H344-B1-T5-noh0-nodh0'),             # ... backward K = 1032 alone (the forward has 11 k-steps)
    ('no_carry', FP32, 'H20-B1-T2-noh0-nodh0'),          # dh_t without dh_{t+1} z_{t+1}
    ('dghn_no_r', BF16, 'H3-B15-T5-h0-dh0'),             # dgh_n = dpn
    ('stale_h', FP32, 'H36-B16-T5-h0-dh0'),              # h_prev from t - 2
    ('dh0_no_carry', BF16, 'H36-B15-T2-noh0-dh0'),       # dh0 = dgh_0 W_hh alone
    ('row16', BF16, 'H15-B33-T5-noh0-nodh0'),            # batch row 16 (first row of the second tile) contracts row 0's operand
    ('row16', FP32, 'H2048-B17-T2-h0-dh0'),
)


# ---------------------------------------------------------------------------------------------------------------------
# CPU checks
# ---------------------------------------------------------------------------------------------------------------------
def _autograd_unrolled(gi, whh, bhh, h0, dy):
    """float64 autograd through nn.GRU's cell unrolled by hand with gh retained, as tests/test_hip_gru_rec.py forms it."""
    B, T, G = gi.shape
    Hd = G // 3
    gi = gi.clone().requires_grad_(True)
    h = (torch.zeros(B, Hd, dtype=F64) if h0 is None else h0.clone()).requires_grad_(True)
    h_init, ys, ghs = h, [], []
    for t in range(T):
        gh = h @ whh.t() + bhh
        gh.retain_grad()
        ghs.append(gh)
        r = torch.sigmoid(gi[:, t, :Hd] + gh[:, :Hd])
        z = torch.sigmoid(gi[:, t, Hd:2 * Hd] + gh[:, Hd:2 * Hd])
        n = torch.tanh(gi[:, t, 2 * Hd:] + r * gh[:, 2 * Hd:])
        h = (1 - z) * n + z * h
        ys.append(h)
    y = torch.stack(ys, 1)
    (y * dy).sum().backward()
    return y.detach(), gi.grad, torch.stack([g_.grad for g_ in ghs], 1), h_init.grad


@pytest.mark.parametrize('Hd,B,T,given', [(20, 3, 5, True), (37, 4, 5, False), (16, 17, 2, True), (1, 2, 1, False), (3, 1, 4, True)])
def test_unforced_float64_equals_nn_gru_and_autograd(Hd, B, T, given):
    """the unrolled float64 chain, no forcing and no rounding, against torch.nn.GRU(batch_first=True).double() and autograd"""
    torch.manual_seed(Hd * 100 + B * 10 + T)
    Din = 6
    gru = torch.nn.GRU(Din, Hd, batch_first=True).double()
    x = torch.randn(B, T, Din, dtype=F64, requires_grad=True)
    h0 = ((torch.rand(B, Hd, dtype=F64) * 2 - 1) * 0.8).requires_grad_(True) if given else None
    dy = torch.randn(B, T, Hd, dtype=F64)
    y_ref, _ = gru(x) if h0 is None else gru(x, h0[None])
    (y_ref * dy).sum().backward()
    w_ih, w_hh, b_ih, b_hh = (p.detach() for p in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0))
    xd = x.detach()
    inp = Inputs(xd @ w_ih.t() + b_ih, w_hh, b_hh, None if h0 is None else h0.detach(), dy)
    st = emulate(FP32, inp, F64, want_dh0=True)
    tol = 1e-12
    assert float((st['y'] - y_ref.detach()).abs().max()) < tol
    # through the retained gh, element by element
    ya, dgi_a, dgh_a, dh0_a = _autograd_unrolled(inp.gi, w_hh, b_hh, inp.h0, dy)
    for name, a in (('y', ya), ('dgi', dgi_a), ('dgh', dgh_a), ('dh0', dh0_a)):
        assert float((st[name] - a).abs().max()) < tol, name
    # and nn.GRU's own autograd through the contractions that follow the recurrence
    dgi, dgh = st['dgi'].reshape(B * T, -1), st['dgh'].reshape(B * T, -1)
    hp = _h_prev(inp, st['y']).reshape(B * T, Hd)
    for name, got, ref in (('dx', (dgi @ w_ih).view(B, T, Din), x.grad), ('dW_ih', dgi.t() @ xd.reshape(B * T, Din), gru.weight_ih_l0.grad),
                           ('dW_hh', dgh.t() @ hp, gru.weight_hh_l0.grad), ('db_ih', dgi.sum(0), gru.bias_ih_l0.grad),
                           ('db_hh', dgh.sum(0), gru.bias_hh_l0.grad)):
        assert float((got - ref).abs().max()) < tol * max(1.0, float(ref.abs().max())), name
    if given:
        assert float((st['dh0'] - h0.grad).abs().max()) < tol
    # forced on its own outputs, unrounded, the forced functions are the same map
    assert max(v[0] for v in forced_errors(FP32, inp, st).values()) < tol


def test_hand_case_h1_t1():
    """H = 1, T = 1, B = 1 by hand: gi = (0.5, -0.25, 0.75), W_hh = (0.5, -1, 0.25), b_hh = (0.125, 0.25, -0.5), h0 = 0.5, dy = 2.
    gh = (0.375, -0.25, -0.375); r = s(0.875), z = s(-0.5), n = tanh(0.75 - 0.375 r), h = (1 - z) n + z / 2."""
    s = lambda v: 1.0 / (1.0 + math.exp(-v))
    r, z = s(0.875), s(-0.5)
    n = math.tanh(0.75 - 0.375 * r)
    h = (1 - z) * n + z * 0.5
    assert abs(r - 0.7057850278370112) < 1e-15 and abs(z - 0.3775406687981454) < 1e-15
    dpn = 2.0 * (1 - z) * (1 - n * n)
    dpz = 2.0 * (0.5 - n) * z * (1 - z)
    dpr = dpn * -0.375 * r * (1 - r)
    dh0 = 2.0 * z + dpr * 0.5 + dpz * -1.0 + dpn * r * 0.25
    t = lambda *v: torch.tensor(v, dtype=F64)
    inp = Inputs(t(0.5, -0.25, 0.75).view(1, 1, 3), t(0.5, -1.0, 0.25).view(3, 1), t(0.125, 0.25, -0.5), t(0.5).view(1, 1), t(2.0).view(1, 1, 1))
    st = emulate(FP32, inp, F64)
    for name, want in (('y', [h]), ('saved', [r, z, n, -0.375]), ('dgi', [dpr, dpz, dpn]), ('dgh', [dpr, dpz, dpn * r]), ('dh0', [dh0])):
        assert float((st[name].reshape(-1) - t(*want)).abs().max()) < 1e-15, name
    # the forced reference reproduces it from these outputs
    assert max(v[0] for v in forced_errors(FP32, inp, st).values()) < 1e-15


def test_case_table_covers_the_edges():
    assert len({case_id(c) for c in CASES}) == len(CASES)
    assert {c.H for c in CASES} == {1, 3, 15, 16, 17, 20, 36, 100, 37, 344, 516, 1028, 2048}
    assert {c.B for c in CASES} == {1, 15, 16, 17, 33}
    assert {c.T for c in CASES} == {1, 2, 5}
    assert {c.variant for c in CASES} == set(VARIANTS)
    for c in CASES:
        if c.H in (1028, 2048):
            assert c.B in (1, 17) and c.T == 2, c
    by_h = lambda Hd: [c for c in CASES if c.H == Hd]
    for Hd in {c.H for c in CASES}:
        assert len({c.B for c in by_h(Hd)}) >= 2, Hd                               # one tile and more, or a full and a partial one
        assert any(c.T >= 2 for c in by_h(Hd)), Hd                                  # the backward's contraction runs
        assert {c.h0 for c in by_h(Hd)} == {True, False}, Hd
    for Hd in (20, 36, 100):
        assert Hd % 4 == 0 and Hd % 32 != 0 and (3 * Hd) % 32 != 0
    assert (3 * 344 + 31) // 32 == 33 and 3 * 344 - 32 * 32 == 8                   # one k-step into the second pass, tail 8
    assert (516 + 3) // 4 == 129                                                    # fp32: one k-step past 4 waves x 32
    assert (1028 + 31) // 32 == 33 and 1028 - 32 * 32 == 4
    # every combination of h0 and dh0, T = 1 and T = 2 with a requested dh0, rows on both sides of the 16-row tile
    assert {(c.h0, c.dh0) for c in CASES} == {(a, b) for a in (True, False) for b in (True, False)}
    assert any(c.T == 1 and c.dh0 for c in CASES) and any(c.T == 2 and c.dh0 for c in CASES)
    for Hd in ALIGN_H:
        assert Hd % 4 == 0 and any(c.h0 and c.dh0 and c.variant == 'plain' and c.T >= 2 for c in by_h(Hd)), Hd
    for v in ('sat', 'zero_dy', 'zero_w'):
        assert any(c.variant == v and c.B > 16 for c in CASES) or v == 'sat'
    assert all(c.H >= 4 for c in CASES if c.variant == 'sat')
    assert all(case_id(c) in {case_id(k) for k in CASES} for c in (case_named(m[2]) for m in MUTATIONS))


def test_float64_chain_with_operand_rounding_sits_on_the_reference():
    """the float64 chain with the precision's operand rounding, forced on itself: what the mutations are planted into is clean"""
    for cid in sorted({m[2] for m in MUTATIONS}):
        c = case_named(cid)
        inp = make_inputs(c)
        for prec in PRECS:
            es = forced_errors(prec, inp, emulate(prec, inp, F64, c.dh0))
            assert max(v[0] / bound(prec, k) for k, v in es.items()) < 1e-6, (cid, prec, es)


@pytest.mark.parametrize('mut,prec,cid', MUTATIONS, ids=['%s-%s-%s' % (m, PREC_NAME[p], c) for m, p, c in MUTATIONS])
def test_mutations_are_caught(mut, prec, cid):
    c = case_named(cid)
    inp = make_inputs(c)
    es = forced_errors(prec, inp, emulate(prec, inp, F64, c.dh0, mut))
    rs = {k: v[0] / bound(prec, k) for k, v in es.items()}
    print('mutation %-12s %s %s: error / bound %s' % (mut, PREC_NAME[prec], cid, '  '.join('%s %.3g' % kv for kv in rs.items())))
    assert max(rs.values()) > 1.0, 'mutation %s is not caught on %s' % (mut, cid)


def test_recorded_stand_in_figures():
    """recomputes STAND_IN_DEV; the stand-in itself is held to what the kernel is held to"""
    worst = stand_in_deviation()
    assert set(worst) == set(STAND_IN_DEV)
    for key in sorted(worst):
        e, cid, k = worst[key]
        print('%s %s: fp32 stand-in deviates by %.3g max(1, |ref|) (%s of %s), recorded %.3g, kernel bound %.3g' % (
            PREC_NAME[key[0]], key[1], e, k, cid, STAND_IN_DEV[key], FACTOR * STAND_IN_DEV[key]))
    for key, (e, cid, k) in worst.items():
        assert e <= FACTOR * STAND_IN_DEV[key], (key, e, cid, k)
        assert FACTOR * STAND_IN_DEV[key] <= 2e-5                                # at or below the LSTM recurrence's bound


def test_variants_do_what_they_say():
    """sat: the float64 gates round to exactly 0 / 1 / -1 in fp32 where the test says the kernel must; zero_dy and zero_w"""
    for c in CASES:
        if c.variant == 'plain':
            continue
        inp = make_inputs(c)
        st = emulate(FP32, inp, F64, c.dh0)
        Hd = c.H
        if c.variant == 'sat':
            r, z, n = (st['saved'][..., k * Hd:(k + 1) * Hd].to(F32) for k in range(3))
            assert bool((r[..., 0] == 1).all()) and bool((z[..., 2] == 1).all()) and bool((n[..., 0] == 1).all())
            assert bool((n[..., 3] == -1).all()) and bool((n[..., 1] == -1).all())
            assert all(bool(torch.isfinite(v).all()) for v in st.values() if v is not None)
        elif c.variant == 'zero_dy':
            assert all(not bool(st[k].any()) for k in ('dgi', 'dgh'))
        else:
            assert not bool(st['saved'][..., 3 * Hd:].any())


if __name__ == '__main__':
    for key, v in sorted(stand_in_deviation().items()):
        print(PREC_NAME[key[0]], key[1], '%.3e' % v[0], v[1], v[2])
