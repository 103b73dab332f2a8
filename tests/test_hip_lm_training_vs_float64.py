"""RNN-LM training on the device (src/lm.py::RNNLM.forward, EmbeddingFn / DropoutFn / RNNLayerFn / GRULayerFn / LinearFn, the loss,
their backward) and asr_adam_step, held to the float64 restatements of tests/test_lm_training_reference.py, which owns the case
table (module x recurrence route x layers x tying x dropout x precision x B, T, V), the inputs and the derivations.

TRAINING PASS (test_training_pass_vs_float64, one test per case): lm.train(), forward, CrossEntropyLoss(ignore_index=0), backward,
as the Solver does; the seed of the call is read from the model, the masks are rebuilt from it with lm_masks and the logits at
the valid positions, the loss and every parameter gradient (relative norm) are compared with lm_train_ref.  Ceilings, the
project's own (tests/test_lm_gru.py): fp32 1e-4 / 1e-4, bf16 3e-2 / 4e-2.  Every LSTM case asserts through asr_lstm_plan that the
recurrence takes the generation its table entry names.  A tied case asserts that each of the two writers of emb.weight.grad
(asr_embedding_bwd, the output projection's weight-gradient GEMM) holds at least 10 % of its norm; a case with p > 0 asserts that
the pass WITHOUT dropout misses the device by more than ten times the ceiling.
Measured on the MI355X, worst error / ceiling over the 24 cases and the wiring tests (every test prints its own):
    fp32   logits 0.009   loss 0.001   gradients 0.012
    bf16   logits 0.21    loss 0.074   gradients 0.21
No case needed a witness measurement: the four-layer, p = 0.5 (scale 2), H = 516 cases stay under the ceilings as well.

DROPOUT WIRING: eval() on a p = 0.5 model is the pass without masks; two consecutive training calls use seeds 7919 apart, give
different logits and each matches the reference of its own seed; p = 0 in train() matches with no masks (the p = 0 cases above).

GRADIENT ACCUMULATION (test_gradients_accumulate): flat_grad is filled with 0.5 before the backward and every parameter must read
0.5 + gradient - asr_embedding_bwd, asr_colsum / asr_colsum2, the split weight-gradient GEMMs and the tied double write all add,
the convention hipabi.linear_bwd writes down.  No writer overwrites.

ADAM (test_adam_vs_float64 and the tests behind it): asr_adam_step through hipabi.call against adam_ref at the float values the C
ABI carries, bound adam_tol = K 2^-24 (|ref| + max |ref|) with K = 32 roundings per step x 3 steps = 96 (the count is in
adam_tol's docstring).  Measured worst error / bound over the 192 cases: param 0.015, exp_avg 0.011, exp_avg_sq 0.017,
max_exp_avg_sq 0.017.  Step modes (device counter, host step, bit equality of the two), the three refusals (NaN norm, inf
norm, status word: nothing moves, the counter included, and the next update is the one of a run that skipped the step) and the
HipAdam checkpoint round trip follow.
"""
import collections
import copy
import math

import numpy as np
import pytest
import torch

import test_lm_training_reference as L
from test_lm_training_reference import BF16, CASES, SEED0, SEED_STRIDE, case_id

gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# the training pass
# ---------------------------------------------------------------------------------------------------------------------
def _lm(c):
    from src import hipabi as H
    from src.lm import RNNLM
    sd, _, _ = L.case_inputs(c)
    lm = RNNLM(c.V, c.tying, c.H, c.module, c.H, c.layers, c.p)
    lm.load_state_dict({k: v.float() for k, v in sd.items()})
    lm = lm.cuda()
    lm.prec = H.BF16 if c.prec == BF16 else H.F32
    lm.flatten()
    return lm


Pass = collections.namedtuple('Pass', 'logits loss grads seed')


def _train_pass(lm, c, fill=0.0):
    """One step's forward and backward as bin/train_lm.py::Solver runs them; `fill`: what flat_grad holds before the backward."""
    from src.util import CrossEntropyLoss
    _, x, y = L.case_inputs(c)
    lm.train()
    lm.flat_grad.fill_(fill)
    out, _ = lm(x.cuda(), (y != 0).sum(1).cuda())
    loss = CrossEntropyLoss(ignore_index=0)(out.view(-1, c.V), y.cuda().reshape(-1))
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu().double() for n, p in lm.named_parameters()}
    return Pass(out.detach().cpu().double(), float(loss.detach()), grads, lm._seed)


def _figures(got, ref, y):
    return L.logits_error(got.logits, ref.logits, y), L.loss_error(got.loss, ref.loss), L.grad_errors(got.grads, ref.grads)


def _assert_matches(c, got, ref, what):
    _, _, y = L.case_inputs(c)
    tol, gtol = L.tolerances(c)
    e_log, e_loss, e_grad = _figures(got, ref, y)
    worst = max(e_grad, key=e_grad.get)
    print('%s %s: error / ceiling  logits %.3f  loss %.3f  gradients %.3f (%s)' % (case_id(c), what, e_log / tol, e_loss / tol, e_grad[worst] / gtol, worst))
    assert e_log < tol, (case_id(c), what, 'logits', e_log)
    assert e_loss < tol, (case_id(c), what, 'loss', e_loss)
    for n, e in e_grad.items():
        assert e < gtol, (case_id(c), what, n, e)


class _lstm_mode:
    """the recurrence plans under asr_lstm_set_persistent(LSTM_MODE), the library's default, for the duration of a test"""

    def __enter__(self):
        from src import hipabi as H
        self.lib = H.lib()
        self.old = self.lib.asr_lstm_set_persistent(L.LSTM_MODE)
        return self.lib

    def __exit__(self, *exc):
        self.lib.asr_lstm_set_persistent(self.old)


@gpu
@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_training_pass_vs_float64(c):
    _, _, y = L.case_inputs(c)
    tol, gtol = L.tolerances(c)
    with _lstm_mode() as lib:
        if c.module == 'LSTM':
            assert (lib.asr_lstm_plan(c.B, c.T, c.H, 1, c.prec) == 2) == c.fwd.startswith('fwd2'), 'not the route the case table names'
        got = _train_pass(_lm(c), c)
    assert got.seed == SEED0
    ref = L.case_ref(c, got.seed if c.p > 0 else None)
    _assert_matches(c, got, ref, 'train')
    if c.tying:
        total = float(ref.grads['emb.weight'].norm())
        assert min(float(ref.emb_lookup.norm()), float(ref.emb_projection.norm())) >= 0.1 * total
    if c.p > 0:
        e_log, _, e_grad = _figures(got, L.case_ref(c, None), y)
        assert e_log > 10 * tol and max(e_grad.values()) > 10 * gtol, (e_log, e_grad)


def _first(module, **want):
    return next(c for c in CASES if c.module == module and all(getattr(c, k) == v for k, v in want.items()))


WIRING = [_first(m, p=0.5, prec=prec, layers=2) for prec in (L.FP32, BF16) for m in ('LSTM', 'GRU')]


@gpu
@pytest.mark.parametrize('c', WIRING, ids=case_id)
def test_eval_has_no_dropout(c):
    _, x, y = L.case_inputs(c)
    tol, _ = L.tolerances(c)
    lm = _lm(c)
    lm.eval()
    with _lstm_mode(), torch.no_grad():
        out, _ = lm(x.cuda(), None)
    torch.cuda.synchronize()
    e = L.logits_error(out.cpu().double(), L.case_ref(c, None).logits, y)
    print('%s eval: logits error / ceiling %.3f' % (case_id(c), e / tol))
    assert e < tol


@gpu
@pytest.mark.parametrize('c', WIRING, ids=case_id)
def test_consecutive_calls_draw_new_masks(c):
    _, _, y = L.case_inputs(c)
    tol, _ = L.tolerances(c)
    lm = _lm(c)
    with _lstm_mode():
        a = _train_pass(lm, c)
        b = _train_pass(lm, c)
    assert a.seed == SEED0 and b.seed == a.seed + SEED_STRIDE
    assert L.logits_error(b.logits, a.logits, y) > 10 * tol
    _assert_matches(c, a, L.case_ref(c, a.seed), 'first call')
    _assert_matches(c, b, L.case_ref(c, b.seed), 'second call')


ACCUM = [_first('LSTM', tying=True, prec=L.FP32, p=0.5), _first('LSTM', tying=False, prec=L.FP32, p=0.5),
         _first('GRU', tying=True, prec=L.FP32, p=0.5, layers=2), _first('GRU', tying=False, prec=L.FP32, p=0.5)]
FILL = 0.5


@gpu
@pytest.mark.parametrize('c', ACCUM, ids=case_id)
def test_gradients_accumulate(c):
    """Every parameter reads FILL + gradient.  The bound is the case's gradient ceiling plus the fp32 roundings of the sums
    FILL + g themselves: one addition rounds by at most 2^-24 (FILL + max |g|) per element, and a writer that adds in parts
    (reduction slices, atomics, the tied double write) by that much per part - four parts are allowed for."""
    _, gtol = L.tolerances(c)
    with _lstm_mode():
        got = _train_pass(_lm(c), c, fill=FILL)
    ref = L.case_ref(c, got.seed)
    for n, g in got.grads.items():
        r = ref.grads[n]
        half_ulp = 2.0 ** -24 * (FILL + float(r.abs().max()))
        e = float((g - FILL - r).norm())
        bound = gtol * float(r.norm()) + 4 * half_ulp * math.sqrt(r.numel())
        print('%s %s: |got - %.1f - ref| %.3g bound %.3g (|ref| %.3g)' % (case_id(c), n, FILL, e, bound, float(r.norm())))
        assert e <= bound, (case_id(c), n, e, bound)
        assert float((g - FILL).norm()) > 0.5 * float(r.norm()) or float(r.norm()) == 0          # FILL alone (the gradient lost) is not within it; dW_hh at T = 1 is 0


# ---------------------------------------------------------------------------------------------------------------------
# asr_adam_step
# ---------------------------------------------------------------------------------------------------------------------
LR, B1, B2, EPS = (L.abi_float(v) for v in (0.05, 0.9, 0.999, 1e-3))          # eps large enough that dropping it is seen
ADAM_N = [1, 3, 255, 257, 100003, 2048 * 256 + 77]
NAMES = ('param', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')


class _Dev:
    """the device side of one Adam run: state tensors, the step counter, a status word of the test's own"""

    def __init__(self, p0, amsgrad, counter=True):
        n = p0.numel()
        self.n = n
        self.p = p0.clone().cuda()
        self.m, self.v = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
        self.vmax = torch.zeros(n, device='cuda') if amsgrad else None
        self.count = torch.zeros(1, dtype=torch.int64, device='cuda') if counter else None
        self.nsq = torch.zeros(1, dtype=torch.float64, device='cuda')
        self.status = torch.zeros(1, dtype=torch.int32, device='cuda')

    def load(self, st, count=None):
        for t, a in ((self.p, st.p), (self.m, st.m), (self.v, st.v), (self.vmax, st.vmax)):
            if t is not None:
                t.copy_(torch.from_numpy(a).float())
        if count is not None:
            self.count.fill_(count)

    def step(self, gr, wd, clip, gmul, use_norm=True, host_step=0, nsq=None):
        from src import hipabi as H
        gd = gr.cuda()
        if nsq is None:
            H.call('asr_sumsq', H.ptr(gd), self.n, H.ptr(self.nsq), H.stream_ptr())
        else:
            self.nsq.fill_(nsq)
        H.call('asr_adam_step', H.ptr(self.p), H.ptr(gd), H.ptr(self.m), H.ptr(self.v), H.ptr(self.vmax), self.n, LR, B1, B2, EPS, wd, host_step,
               clip, H.ptr(self.nsq) if use_norm else None, gmul, H.ptr(self.status), H.ptr(self.count), H.stream_ptr())
        torch.cuda.synchronize()

    def tensors(self):
        return [t for t in (self.p, self.m, self.v, self.vmax) if t is not None]

    def bits(self):
        return [t.clone() for t in self.tensors()] + ([] if self.count is None else [self.count.clone()])

    def ratios(self, st):
        """error / adam_tol per state tensor"""
        out = {}
        for name, t, want in zip(NAMES, (self.p, self.m, self.v, self.vmax), (st.p, st.m, st.v, st.vmax)):
            if t is not None:
                err = np.abs(t.cpu().double().numpy() - want)
                out[name] = float((err / L.adam_tol(want)).max())
        return out


def _ref_step(st, n, k, wd, clip, gmul, use_norm=True, **kw):
    """adam_ref on gradient k of adam_inputs(n)"""
    g64 = L.adam_inputs(n)[1][k].double().numpy()
    return L.adam_ref(st, g64, LR, B1, B2, EPS, L.abi_float(wd), clip, L.adam_normsq(n, k) if use_norm else None, gmul, **kw)


def _clip(n, gmul, mode):
    norm0 = math.sqrt(L.adam_normsq(n, 0)) * gmul                                 # the smallest of the steps' norms
    return {'active': 0.5 * norm0, 'inactive': 12.0 * norm0, 'zero': 0.0, 'null': 5.0}[mode]


@gpu
@pytest.mark.parametrize('n', ADAM_N)
@pytest.mark.parametrize('gmul', [1.0, 0.25])
@pytest.mark.parametrize('amsgrad', [False, True])
@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('clipmode', ['active', 'inactive', 'zero', 'null'])
def test_adam_vs_float64(clipmode, wd, amsgrad, gmul, n):
    p0, grads = L.adam_inputs(n)
    clip = L.abi_float(_clip(n, gmul, clipmode))
    dev = _Dev(p0, amsgrad)
    st = L.adam_init(p0.double().numpy(), amsgrad)
    assert int(dev.count) == 0
    for step in range(L.ADAM_STEPS):
        dev.step(grads[step], wd, clip, gmul, use_norm=clipmode != 'null')
        nrm = math.sqrt(L.adam_normsq(n, step)) * gmul
        if clipmode == 'active':
            assert clip < nrm
        if clipmode == 'inactive':
            assert clip > nrm + 1e-6
        st = _ref_step(st, n, step, wd, clip, gmul, use_norm=clipmode != 'null')
        assert int(dev.count) == step + 1 == st.applied                         # the device counter: k after k applied updates
    r = dev.ratios(st)
    print('adam n=%d %s wd=%g amsgrad=%d gmul=%g: error / bound %s' % (n, clipmode, wd, amsgrad, gmul, {k: '%.3f' % v for k, v in r.items()}))
    assert max(r.values()) <= 1.0, r
    assert set(r) == set(NAMES if amsgrad else NAMES[:3])
    assert float(np.abs(st.p - p0.double().numpy()).min()) > 0                  # every parameter moved: the comparison is not vacuous
    if (n + 255) // 256 > 2048:
        assert n == ADAM_N[-1]                                                   # the one size past the grid cap: the grid-stride loop ran


@gpu
@pytest.mark.parametrize('step', [1, 1000, 100000])
@pytest.mark.parametrize('amsgrad', [False, True])
def test_adam_host_step_and_counter_agree(step, amsgrad):
    """step_counter = NULL takes `step` from the host; a device counter that reads step - 1 gives the same bits."""
    n, wd, gmul = 100003, 0.01, 1.0
    p0, grads = L.adam_inputs(n)
    clip = L.abi_float(_clip(n, gmul, 'active'))
    st0 = _ref_step(L.adam_init(p0.double().numpy(), amsgrad), n, 0, wd, clip, gmul)          # a state with non-zero moments
    st0 = st0._replace(p=st0.p.astype(np.float32).astype(np.float64), m=st0.m.astype(np.float32).astype(np.float64),
                       v=st0.v.astype(np.float32).astype(np.float64), vmax=None if st0.vmax is None else st0.vmax.astype(np.float32).astype(np.float64))
    host, cnt = _Dev(p0, amsgrad, counter=False), _Dev(p0, amsgrad)
    host.load(st0)
    cnt.load(st0, count=step - 1)
    host.step(grads[1], wd, clip, gmul, host_step=step)
    cnt.step(grads[1], wd, clip, gmul)
    assert int(cnt.count) == step
    for a, b in zip(host.tensors(), cnt.tensors()):
        assert torch.equal(a, b)
    want = _ref_step(st0, n, 1, wd, clip, gmul, step=step)
    r = host.ratios(want)
    print('adam host step %d amsgrad=%d: error / bound %s' % (step, amsgrad, {k: '%.3f' % v for k, v in r.items()}))
    assert max(v for v in r.values()) * L.ADAM_STEPS <= 1.0, r                   # ONE step: a third of the three-step bound
    if step > 1:
        other = _ref_step(st0, n, 1, wd, clip, gmul, step=1)
        assert float(np.abs(other.p - want.p).max()) > 100 * float(L.adam_tol(want.p).max())          # the step number matters


@gpu
@pytest.mark.parametrize('kind', ['nan', 'inf', 'status'])
@pytest.mark.parametrize('amsgrad', [False, True])
def test_adam_refusals_leave_everything_untouched(kind, amsgrad):
    n, wd, gmul = 100003, 0.01, 0.25
    p0, grads = L.adam_inputs(n)
    clip = L.abi_float(_clip(n, gmul, 'active'))
    dev = _Dev(p0, amsgrad)
    st = L.adam_init(p0.double().numpy(), amsgrad)
    dev.step(grads[0], wd, clip, gmul)
    st = after_one = _ref_step(st, n, 0, wd, clip, gmul)
    before = dev.bits()
    assert int(dev.count) == 1
    if kind == 'status':
        dev.status.fill_(2)                                                      # the test's own word, as asr_status_collect would leave it
        dev.step(grads[1], wd, clip, gmul)
        refused = _ref_step(st, n, 1, wd, clip, gmul, status=2)
        dev.status.zero_()
    else:
        bad = float(kind)
        dev.step(grads[1], wd, clip, gmul, nsq=bad)
        refused = L.adam_ref(st, L.adam_inputs(n)[1][1].double().numpy(), LR, B1, B2, EPS, L.abi_float(wd), clip, bad, gmul)
    assert refused is st
    for a, b in zip(before, dev.bits()):
        assert torch.equal(a, b), 'a refused update wrote state'
    assert int(dev.count) == 1
    # the next accepted update is update 2 of a run that never saw the refused gradient
    dev.step(grads[2], wd, clip, gmul)
    st = _ref_step(st, n, 2, wd, clip, gmul)
    assert int(dev.count) == 2 == st.applied
    r = dev.ratios(st)
    print('adam after a refused update (%s, amsgrad=%d): error / bound %s' % (kind, amsgrad, {k: '%.3f' % v for k, v in r.items()}))
    assert max(r.values()) <= 1.0, r
    # had the refused call advanced the counter, the bias corrections of update 3 would have been used: far outside the bound
    counted = _ref_step(after_one._replace(applied=2), n, 2, wd, clip, gmul)
    assert float(np.abs(counted.p - st.p).max()) > 100 * float(L.adam_tol(st.p).max())


@gpu
@pytest.mark.parametrize('amsgrad', [False, True])
def test_hip_adam_resumes_from_its_state_dict(amsgrad):
    """three steps, state_dict() -> a new HipAdam -> load_state_dict(), two more steps == five uninterrupted steps, bit for bit"""
    from src.optim import HipAdam
    c = _first('GRU', H=30, layers=2)
    g = torch.Generator().manual_seed(8)

    def run(resume_at):
        lm = _lm(c)
        mk = lambda: HipAdam(lm.parameters(), lr=1e-2, eps=1e-8, weight_decay=0.01, amsgrad=amsgrad)
        opt = mk()
        for it in range(5):
            if it == resume_at:
                sd = copy.deepcopy(opt.state_dict())
                assert float(sd['state'][0]['step']) == it
                opt = mk()
                assert int(opt.steps_dev) == 0
                opt.load_state_dict(sd)
                assert int(opt.steps_dev) == it
            lm.flat_grad.copy_(grads[it])
            opt.grad_norm()
            opt.step(clip=0.5, use_norm=True)
        torch.cuda.synchronize()
        return lm, opt

    # gradients on the parameters only: the alignment gaps of the flat buffer hold zeros in training, and no state is kept for them
    probe = _lm(c)
    for p in probe.parameters():
        p.grad.fill_(1.0)
    inside = probe.flat_grad.clone()
    assert 0 < int(inside.sum()) == sum(p.numel() for p in probe.parameters()) <= inside.numel()
    grads = [(torch.randn(inside.numel(), generator=g) * 0.1).cuda() * inside for _ in range(5)]
    lm_a, opt_a = run(None)
    lm_b, opt_b = run(3)
    assert int(opt_a.steps_dev) == 5 and int(opt_b.steps_dev) == 5
    assert torch.equal(lm_a.flat_param, lm_b.flat_param)
    assert torch.equal(opt_a.exp_avg, opt_b.exp_avg) and torch.equal(opt_a.exp_avg_sq, opt_b.exp_avg_sq)
    if amsgrad:
        assert torch.equal(opt_a.max_exp_avg_sq, opt_b.max_exp_avg_sq)
    lm_0 = _lm(c)
    assert not torch.equal(lm_a.flat_param, lm_0.flat_param)
