"""The beam-search bookkeeping kernels of csrc/beam_step.hip, csrc/ctc_prefix.hip and csrc/decode.hip, each on its own,
against the float64 restatement of
tests/test_beam_step_reference.py: asr_beam_step, asr_beam_candidates, asr_ctc_prefix_{init,score}[_batched], asr_lstm_cell,
asr_gather_rows and asr_sample_tokens, driven through src.hipabi on hand-built buffers - no model anywhere.

Every output buffer lies between two guard rows of a canary value; the columns of seq / score / fin_seq / fin_score past
what a step may write, the rows of the finals past fin_n and every column of the token table but the one written hold the
canary too, and all of that is checked after every launch.  (A final that is inserted before longer ones leaves their
tokens behind its own length, and the shifting copies move whole rows: so the columns checked in the finals are those past
the longest final the utterance has held so far, and the last column, which no final can reach.)

Integer outputs - alive, len, seq, last_token, parent, ctc_index, the token-table column, done, fin_n, fin_len, fin_seq, the
candidates, the sampled tokens, the gathered rows - must equal the restatement's EXACTLY: the seeded cases hold every
decision apart by more than GAP = 1e-3 (test_beam_step_reference.py::test_committed_seeds_hold_the_conditions), the tie
cases are exact in fp32.

Float outputs: the deviation is |got - float64| / max(1, |float64|); relative, because fused scores reach 1e7 and the
prefix scorer's log zero is -1e8.  The constants are the largest deviation of the restatement's fp32 TRANSCRIPTION from
its float64 result over all committed cases, measured on the CPU (test_fp32_transcription_within_the_recorded_deviation
re-measures them); the kernel is allowed 4 x that, for its different summation order and the device's exp / log1p:

  group                                      fp32 transcription     kernel on the MI355X (largest over the group's cases)
  step: sum, score, ctcp, fin_avg, fin_score STEP_DEV = 1.26e-7     1.26e-7 (v31_b5_ctc; 1.25e-7 v300_b16_att_finals_full; the tie cases 1.2e-8)
  prefix scorer: psi, r                      CTC_DEV  = 3.32e-7     3.29e-7 (batched, Tmax 37, V 300; single 2.86e-7); 1.25e-7 from the fp32 transcription
  lstm cell: h, c                            LSTM_DEV = 2.14e-7     2.14e-7 ((3,1024), saturating gates)
"""
import ctypes

import numpy as np
import pytest
import torch

import test_beam_step_reference as R
from test_beam_step_reference import CASES

STEP_DEV = 1.2553315911274563e-07        # v300_b16_ctc_lm and its like: a fused score
CTC_DEV = 3.3153993365392874e-07
LSTM_DEV = 2.1364743049564615e-07
TOL_FACTOR = 4
E_ARG, E_UNSUPPORTED = -1, -3
CAN_I, CAN_F = -77, 7.5            # canaries


def rel_dev(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


# ---- guarded device buffers ---------------------------------------------------------------------------------------------
class Guarded(object):
    """A device buffer of `shape` between two guard rows of the canary."""

    def __init__(self, shape, dtype, content=None):
        self.fill = CAN_F if dtype.is_floating_point else CAN_I
        self.full = torch.full((shape[0] + 2,) + tuple(shape[1:]), self.fill, dtype=dtype, device='cuda')
        self.t = self.full[1:-1]
        if content is not None:
            self.t.copy_(torch.as_tensor(np.asarray(content)).to(dtype))

    def ptr(self):
        from src import hipabi as H
        return H.ptr(self.t)

    def host(self):
        """-> numpy content; asserts the guard rows."""
        full = self.full.cpu().numpy()
        assert (full[0] == self.fill).all() and (full[-1] == self.fill).all(), 'guard row overwritten'
        return full[1:-1]


# ---- asr_beam_step -------------------------------------------------------------------------------------------------------
_REF = {}


def reference(name):
    """float64 drive of a case, computed once and shared: [state after step t]."""
    if name not in _REF:
        _REF[name] = R.run_case(name)[0]
    return _REF[name]


def state_bufs(R_, Lmax):
    i32, f32 = torch.int32, torch.float32
    return {'alive': Guarded((R_,), i32), 'sum': Guarded((R_,), f32), 'ctcp': Guarded((R_,), f32), 'len': Guarded((R_,), i32),
            'seq': Guarded((R_, Lmax), i32), 'sc': Guarded((R_, Lmax), f32)}


def launch_step(tab, st_in, st_out, aux, name, t, **override):
    from src import hipabi as H
    c = CASES[name]
    U, R_, Lmax, tok_ld = R.case_dims(name)
    p = R.case_params(name, t)
    a = H.BeamStep()
    dev = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to('cuda', torch.int32 if k == 'cand' else torch.float32))
           for k, v in tab.items()}
    ptrs = {'att_logp': dev['att'], 'lm_logp': dev['lm'], 'psi': dev['psi'], 'candidates': dev['cand'],
            'alive_in': st_in['alive'].t, 'sum_in': st_in['sum'].t, 'ctcp_in': st_in['ctcp'].t, 'len_in': st_in['len'].t,
            'seq_in': st_in['seq'].t, 'score_in': st_in['sc'].t, 'alive_out': st_out['alive'].t, 'sum_out': st_out['sum'].t,
            'ctcp_out': st_out['ctcp'].t, 'len_out': st_out['len'].t, 'seq_out': st_out['seq'].t, 'score_out': st_out['sc'].t,
            'last_token': aux['last_tok'].t, 'parent': aux['parent'].t, 'ctc_index': aux['ctcidx'].t, 'tokens': aux['tokens'].t,
            'min_len': aux['min_len'], 'max_len': aux['max_len'], 'done': aux['done'].t, 'fin_n': aux['fin_n'].t,
            'fin_len': aux['fin_len'].t, 'fin_avg': aux['fin_avg'].t, 'fin_seq': aux['fin_seq'].t, 'fin_score': aux['fin_sc'].t}
    for k, v in ptrs.items():
        setattr(a, k, None if v is None else v.data_ptr())
    a.tokens_ld = tok_ld
    a.U, a.beam, a.V, a.C, a.Lmax, a.t = U, c['beam'], c['V'], c['C'], Lmax, t
    a.ctc_weight, a.lm_weight, a.eos_threshold = float(p['ctc_w']), float(p['lm_w']), float(p['eos_thr'])
    for k, v in override.items():
        setattr(a, k, v)
    rc = H.lib().asr_beam_step(ctypes.byref(a), H.stream_ptr())
    torch.cuda.synchronize()
    return rc


def new_aux(name):
    c = CASES[name]
    U, R_, Lmax, tok_ld = R.case_dims(name)
    i32, f32, i64, beam = torch.int32, torch.float32, torch.int64, c['beam']
    s0 = R.case_state0(name)
    aux = {'tokens': Guarded((R_, tok_ld), i64), 'done': Guarded((U,), i32, s0['done']),
           'fin_n': Guarded((U,), i32, [len(f) for f in s0['finals']]), 'fin_len': Guarded((U, beam), i32),
           'fin_avg': Guarded((U, beam), f32), 'fin_seq': Guarded((U, beam, Lmax + 1), i32), 'fin_sc': Guarded((U, beam, Lmax + 1), f32),
           'min_len': torch.tensor(c['min_len'], dtype=i32, device='cuda'), 'max_len': torch.tensor(c['max_len'], dtype=i32, device='cuda')}
    for u, fin in enumerate(s0['finals']):
        for i, (avg, seq, score) in enumerate(fin):
            aux['fin_len'].t[u, i], aux['fin_avg'].t[u, i] = len(seq), float(avg)
            aux['fin_seq'].t[u, i, :len(seq)] = torch.tensor(seq, dtype=i32)
            aux['fin_sc'].t[u, i, :len(seq)] = torch.tensor([float(s) for s in score], dtype=f32)
    return aux


def fresh_step_outputs(aux, R_):
    aux['last_tok'], aux['parent'], aux['ctcidx'] = Guarded((R_,), torch.int32), Guarded((R_,), torch.int64), Guarded((R_,), torch.int64)


def read_step(st_out, aux):
    got = {k: v.host() for k, v in st_out.items()}
    got.update({k: aux[k].host() for k in ('last_tok', 'parent', 'ctcidx', 'tokens', 'done', 'fin_n', 'fin_len', 'fin_avg', 'fin_seq', 'fin_sc')})
    return got


def compare_step(got, ref, tok_model, fin_hi, beam):
    """One step's buffers against the restatement's state; updates the token-table model and the longest final so far
    (fin_hi, per utterance); returns the largest float deviation."""
    dev = 0.0
    R_ = len(ref['alive'])
    assert got['alive'].tolist() == ref['alive'].tolist()
    assert got['len'].tolist() == ref['len'].tolist()
    assert got['last_tok'].tolist() == ref['last_token'].tolist()
    assert got['parent'].tolist() == ref['parent'].tolist()
    assert got['ctcidx'].tolist() == ref['ctc_index'].tolist()
    assert got['done'].tolist() == ref['done'].tolist()
    for r in range(R_):
        n = int(ref['len'][r])
        assert got['seq'][r, :n].tolist() == ref['seq'][r], r
        assert (got['seq'][r, n:] == CAN_I).all() and (got['sc'][r, n:] == CAN_F).all(), 'row %d written past its length' % r
        dev = max(dev, rel_dev(got['sc'][r, :n], ref['score'][r]))
    dev = max(dev, rel_dev(got['sum'], ref['sum']), rel_dev(got['ctcp'], ref['ctcp']))
    tok_model[:, ref['tok_col']] = ref['tok_val']
    assert (got['tokens'] == tok_model).all(), 'token table: a wrong value, or a column other than %d touched' % ref['tok_col']
    for u, fin in enumerate(ref['finals']):
        assert int(got['fin_n'][u]) == len(fin), (u, int(got['fin_n'][u]), len(fin))
        fin_hi[u] = max([fin_hi[u]] + [len(f[1]) for f in fin])
        for i, (avg, seq, score) in enumerate(fin):
            assert int(got['fin_len'][u, i]) == len(seq), (u, i)
            assert got['fin_seq'][u, i, :len(seq)].tolist() == seq, (u, i, got['fin_seq'][u, i].tolist(), seq)
            dev = max(dev, rel_dev(got['fin_avg'][u, i], avg), rel_dev(got['fin_sc'][u, i, :len(seq)], score))
        n = len(fin)
        assert (got['fin_len'][u, n:] == CAN_I).all() and (got['fin_avg'][u, n:] == CAN_F).all()
        assert (got['fin_seq'][u, n:] == CAN_I).all() and (got['fin_sc'][u, n:] == CAN_F).all(), 'finals past fin_n touched'
        assert (got['fin_seq'][u, :, fin_hi[u]:] == CAN_I).all() and (got['fin_sc'][u, :, fin_hi[u]:] == CAN_F).all(), 'finals written past their length'
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_beam_step_drive_equals_float64_restatement(name):
    """Multi-step drive: the kernel's own state is fed back, every step is compared; one call more than the longest
    utterance needs, so that a step on done utterances alone is part of every case."""
    c = CASES[name]
    U, R_, Lmax, tok_ld = R.case_dims(name)
    ref = reference(name)
    s0 = R.case_state0(name)
    st_in = state_bufs(R_, Lmax)
    for k, key in (('alive', 'alive'), ('sum', 'sum'), ('ctcp', 'ctcp'), ('len', 'len')):
        st_in[k].t.copy_(torch.as_tensor(s0[key]).to(st_in[k].t.dtype))
    aux = new_aux(name)
    tok_model = np.full((R_, tok_ld), CAN_I, dtype=np.int64)
    fin_hi = [max([0] + [len(f[1]) for f in fin]) for fin in s0['finals']]
    dev = 0.0
    for t in range(len(ref)):
        st_out = state_bufs(R_, Lmax)
        fresh_step_outputs(aux, R_)
        assert launch_step(R.case_tables(name, t), st_in, st_out, aux, name, t) == 0
        for b in st_in.values():
            b.host()                                    # inputs: guards intact
        dev = max(dev, compare_step(read_step(st_out, aux), ref[t], tok_model, fin_hi, c['beam']))
        st_in = st_out
    assert all(ref[-1]['done'])
    print('%s: largest float deviation %.3g (fp32 transcription %.3g, allowed %.3g)' % (name, dev, STEP_DEV, TOL_FACTOR * STEP_DEV))
    assert dev <= TOL_FACTOR * STEP_DEV


def step_fp32_dev():
    """largest deviation of the fp32 transcription of the drive from float64 over the committed cases."""
    dev = 0.0
    for name in CASES:
        for a, b in zip(R.run_case(name)[0], R.run_case(name, np.float32)[0]):
            assert a['seq'] == b['seq']
            dev = max(dev, rel_dev(b['sum'], a['sum']), rel_dev(b['ctcp'], a['ctcp']))
            for x, y in zip(a['score'], b['score']):
                dev = max(dev, rel_dev(y, x))
            for fa, fb in zip(a['finals'], b['finals']):
                for (avg, _, sc), (avg2, _, sc2) in zip(fa, fb):
                    dev = max(dev, rel_dev(avg2, avg), rel_dev(sc2, sc))
    return dev


def _refusal_setup(name='v31_b5_ctc'):
    U, R_, Lmax, tok_ld = R.case_dims(name)
    st_in, st_out, aux = state_bufs(R_, Lmax), state_bufs(R_, Lmax), new_aux(name)
    fresh_step_outputs(aux, R_)
    return st_in, st_out, aux


@pytest.mark.gpu
@pytest.mark.parametrize('what', ['beam17', 'v2049', 'psi_without_candidates', 'null_att', 'null_fin_seq', 'null_ctcp_out'])
def test_beam_step_refuses_before_any_launch(what):
    name = 'v31_b5_ctc'
    st_in, st_out, aux = _refusal_setup(name)
    tab = R.case_tables(name, 0)
    over = {'beam17': {'beam': 17}, 'v2049': {'V': 2049}, 'psi_without_candidates': {'candidates': None}, 'null_att': {'att_logp': None},
            'null_fin_seq': {'fin_seq': None}, 'null_ctcp_out': {'ctcp_out': None}}[what]
    assert launch_step(tab, st_in, st_out, aux, name, 0, **over) == E_ARG
    for b in list(st_out.values()) + [aux[k] for k in ('last_tok', 'parent', 'ctcidx', 'tokens', 'fin_len', 'fin_avg', 'fin_seq', 'fin_sc')]:
        assert (b.host() == b.fill).all()                # nothing was launched


# ---- asr_beam_candidates -------------------------------------------------------------------------------------------------
def candidate_rows(rows, V, seed):
    rng = np.random.RandomState(seed)
    x = rng.randn(rows, V).astype(np.float32)
    x[0, rng.rand(V) < 0.5] = R.NEG_INF                                 # -inf entries
    if rows > 2:
        x[1] = R.NEG_INF
        x[1, rng.choice(V, size=min(2, V), replace=False)] = [-1.0, -2.0][:min(2, V)]       # fewer than C above -inf: token 0 fills
        x[2] = -rng.randint(1, 4, size=V) / 2.0                          # ties, in one lane and across lanes
        x[3, :] = -1.0
        x[3, V // 2:] = -0.5
    return x


@pytest.mark.gpu
@pytest.mark.parametrize('V', [3, 31, 64, 65, 129, 300, 2047, 2048])
def test_beam_candidates_equal_the_restatement(V):
    from src import hipabi as H
    for rows in (1, 48):
        x = candidate_rows(rows, V, V + rows)
        xd = torch.from_numpy(x).cuda()
        for C in sorted(set(c for c in (1, 12, 24, V) if c <= V)):
            out = Guarded((rows, C), torch.int32)
            H.call('asr_beam_candidates', H.ptr(xd), out.ptr(), rows, V, C, H.stream_ptr())
            torch.cuda.synchronize()
            want = R.beam_candidates(x, C)
            got = out.host()
            assert (got == want).all(), (rows, C, np.argwhere(got != want)[:4].tolist())


@pytest.mark.gpu
def test_beam_candidates_refusals():
    from src import hipabi as H
    x = torch.zeros(2, 2049, device='cuda')
    out = Guarded((2, 8), torch.int32)
    assert H.lib().asr_beam_candidates(H.ptr(x), out.ptr(), 2, 2049, 8, H.stream_ptr()) == E_UNSUPPORTED
    assert H.lib().asr_beam_candidates(H.ptr(x), out.ptr(), 2, 5, 6, H.stream_ptr()) == E_ARG
    assert H.lib().asr_beam_candidates(None, out.ptr(), 2, 5, 5, H.stream_ptr()) == E_ARG
    torch.cuda.synchronize()
    assert (out.host() == CAN_I).all()


# ---- CTC prefix scorer ---------------------------------------------------------------------------------------------------
# single utterance: (T, V, N, C); N*C covers 1, 63, 64, 65 and 16*24
CTC_SINGLE = [(1, 5, 1, 1), (2, 31, 7, 9), (37, 300, 8, 8), (37, 31, 5, 13), (37, 300, 16, 24), (2, 5, 8, 8), (1, 31, 5, 13)]
# batched, U = 3 with tlen = (1, Tmax, Tmax // 2): (Tmax, V, rows_per_utt, C)
CTC_BATCHED = [(37, 31, 1, 21), (37, 300, 4, 32), (2, 5, 4, 5), (37, 31, 4, 16)]


def ctc_rows(seed, T_of_row, V, N, C, x_of_row):
    """prefix length cycling over 0, 1, T-1, T; candidates holding the last token, <eos>, the blank and a duplicate; the
    previous state is the initial one for the empty prefix and arbitrary log-values (log zero before plen - 1) else."""
    rng = np.random.RandomState(seed)
    plen = np.array([[0, 1, max(T_of_row[n] - 1, 0), T_of_row[n]][n % 4] for n in range(N)], dtype=np.int32)
    last = np.where(plen > 0, rng.randint(2, V, size=N), 0).astype(np.int32)
    cand = rng.randint(0, V, size=(N, C)).astype(np.int32)
    Tmax = max(T_of_row)
    r_prev = np.full((N, Tmax, 2), R.DO.LOGZERO_CTC, dtype=np.float32)
    for n in range(N):
        for j, tok in enumerate((last[n], 1, 0)):
            if j < C:
                cand[n, (n + j) % C] = tok
        if C >= 5:
            cand[n, (n + 3) % C] = cand[n, (n + 4) % C]
        T = T_of_row[n]
        if plen[n] == 0:
            r_prev[n, :T] = R.ctc_prefix_init(x_of_row(n)[:T], np.float32)
        else:
            r_prev[n, max(plen[n] - 1, 0):T] = -10.0 * rng.rand(T - max(plen[n] - 1, 0), 2)
    return plen, last, cand, r_prev


def ctc_single_case(T, V, N, C, dtype):
    x = R.log_softmax32(3.0 * np.random.RandomState(T * 1000 + V).randn(T, V))
    plen, last, cand, r_prev = ctc_rows(T + V + N, [T] * N, V, N, C, lambda n: x)
    psi = np.zeros((N, C), dtype=dtype)
    r = np.zeros((N, C, T, 2), dtype=dtype)
    for n in range(N):
        psi[n], r[n] = R.ctc_prefix_cheap(x, plen[n], last[n], r_prev[n], cand[n], dtype)
    return (x, plen, last, cand, r_prev), psi, r


def ctc_batched_case(Tmax, V, rpu, C, dtype):
    U, N = 3, 3 * rpu
    tlen = np.array([1, Tmax, max(Tmax // 2, 1)], dtype=np.int32)
    x = R.log_softmax32(3.0 * np.random.RandomState(Tmax * 1000 + V + rpu).randn(U, Tmax, V))
    plen, last, cand, r_prev = ctc_rows(Tmax + V + rpu, [int(tlen[n // rpu]) for n in range(N)], V, N, C, lambda n: x[n // rpu])
    psi, r = R.ctc_prefix_score_batched(x, tlen, r_prev, cand, plen, last, rpu, dtype)
    return (x, tlen, plen, last, cand, r_prev), psi, r


def ctc_fp32_dev():
    dev = 0.0
    for args in CTC_SINGLE:
        (_, p64, r64), (_, p32, r32) = ctc_single_case(*args, dtype=np.float64), ctc_single_case(*args, dtype=np.float32)
        dev = max(dev, rel_dev(p32, p64), rel_dev(r32, r64))
    for args in CTC_BATCHED:
        (_, p64, r64), (_, p32, r32) = ctc_batched_case(*args, dtype=np.float64), ctc_batched_case(*args, dtype=np.float32)
        ok = ~np.isnan(r64)
        dev = max(dev, rel_dev(p32, p64), rel_dev(r32[ok], r64[ok]))
    for batched in (False, True):
        dev = max(dev, max(rel_dev(a, b) for a, b in zip(ctc_chain(np.float32, batched), ctc_chain(np.float64, batched))))
    return dev


def _check_ctc(psi_g, r_g, case, valid=None):
    _, p64, r64 = case(np.float64)
    _, p32, r32 = case(np.float32)
    valid = ~np.isnan(r64) if valid is None else valid
    d64 = max(rel_dev(psi_g, p64), rel_dev(r_g[valid], r64[valid]))
    d32 = max(rel_dev(psi_g, p32), rel_dev(r_g[valid], r32[valid]))
    print('deviation from float64 %.3g, from the fp32 transcription %.3g (allowed %.3g)' % (d64, d32, TOL_FACTOR * CTC_DEV))
    assert d64 <= TOL_FACTOR * CTC_DEV
    assert d32 <= (TOL_FACTOR + 1) * CTC_DEV                 # triangle: the transcription is within CTC_DEV of float64
    assert (r_g[~valid] == CAN_F).all(), 'frames past tlen written'


@pytest.mark.gpu
@pytest.mark.parametrize('T,V,N,C', CTC_SINGLE)
def test_ctc_prefix_score_single(T, V, N, C):
    from src import hipabi as H
    (x, plen, last, cand, r_prev), _, _ = ctc_single_case(T, V, N, C, np.float64)
    d = lambda a: torch.from_numpy(a).cuda()
    xd, pd, ld, cd, rd = d(x), d(plen), d(last), d(cand), d(r_prev)
    psi, r_out = Guarded((N, C), torch.float32), Guarded((N, C, T, 2), torch.float32)
    H.call('asr_ctc_prefix_score', H.ptr(xd), H.ptr(rd), H.ptr(cd), H.ptr(pd), H.ptr(ld), psi.ptr(), r_out.ptr(), N, C, T, V, H.stream_ptr())
    torch.cuda.synchronize()
    _check_ctc(psi.host(), r_out.host(), lambda dt: ctc_single_case(T, V, N, C, dt))
    r0 = Guarded((T, 2), torch.float32)
    H.call('asr_ctc_prefix_init', H.ptr(xd), r0.ptr(), T, V, H.stream_ptr())
    torch.cuda.synchronize()
    assert rel_dev(r0.host(), R.ctc_prefix_init(x)) <= TOL_FACTOR * CTC_DEV


@pytest.mark.gpu
@pytest.mark.parametrize('Tmax,V,rpu,C', CTC_BATCHED)
def test_ctc_prefix_score_batched(Tmax, V, rpu, C):
    from src import hipabi as H
    (x, tlen, plen, last, cand, r_prev), _, r64 = ctc_batched_case(Tmax, V, rpu, C, np.float64)
    N = 3 * rpu
    d = lambda a: torch.from_numpy(a).cuda()
    xd, td, pd, ld, cd, rd = d(x), d(tlen), d(plen), d(last), d(cand), d(r_prev)
    psi, r_out = Guarded((N, C), torch.float32), Guarded((N, C, Tmax, 2), torch.float32)
    H.call('asr_ctc_prefix_score_batched', H.ptr(xd), H.ptr(td), H.ptr(rd), H.ptr(cd), H.ptr(pd), H.ptr(ld), psi.ptr(), r_out.ptr(),
           N, C, Tmax, V, rpu, H.stream_ptr())
    torch.cuda.synchronize()
    _check_ctc(psi.host(), r_out.host(), lambda dt: ctc_batched_case(Tmax, V, rpu, C, dt))
    assert np.isnan(r64[0, :, 1:]).all()                   # utterance 0 has one frame: the rest of its rows is canary (checked above)
    r0 = Guarded((N, Tmax, 2), torch.float32)
    H.call('asr_ctc_prefix_init_batched', H.ptr(xd), H.ptr(td), r0.ptr(), N, rpu, Tmax, V, H.stream_ptr())
    torch.cuda.synchronize()
    assert rel_dev(r0.host(), R.ctc_prefix_init_batched(x, tlen, rpu, N)) <= TOL_FACTOR * CTC_DEV


@pytest.mark.gpu
@pytest.mark.parametrize('T,V,N,C', CTC_SINGLE)
def test_ctc_prefix_single_is_the_batched_scorer_on_one_utterance(T, V, N, C):
    """asr_ctc_prefix_score / _init and the batched entries with U = 1, rows_per_utt = N, tlen = [T] run one body
    (csrc/ctc_prefix.hip): psi, r_out and r0 bit for bit identical, guards intact."""
    from src import hipabi as H
    (x, plen, last, cand, r_prev), _, _ = ctc_single_case(T, V, N, C, np.float64)
    d = lambda a: torch.from_numpy(a).cuda()
    xd, td, pd, ld, cd, rd, st = d(x), d(np.array([T], dtype=np.int32)), d(plen), d(last), d(cand), d(r_prev), H.stream_ptr()
    psi = [Guarded((N, C), torch.float32) for _ in range(2)]
    r_out = [Guarded((N, C, T, 2), torch.float32) for _ in range(2)]
    r0 = [Guarded((1, T, 2), torch.float32) for _ in range(2)]
    H.call('asr_ctc_prefix_score', H.ptr(xd), H.ptr(rd), H.ptr(cd), H.ptr(pd), H.ptr(ld), psi[0].ptr(), r_out[0].ptr(), N, C, T, V, st)
    H.call('asr_ctc_prefix_score_batched', H.ptr(xd), H.ptr(td), H.ptr(rd), H.ptr(cd), H.ptr(pd), H.ptr(ld), psi[1].ptr(), r_out[1].ptr(),
           N, C, T, V, N, st)
    H.call('asr_ctc_prefix_init', H.ptr(xd), r0[0].ptr(), T, V, st)
    H.call('asr_ctc_prefix_init_batched', H.ptr(xd), H.ptr(td), r0[1].ptr(), 1, N, T, V, st)
    torch.cuda.synchronize()
    for what, (a, b) in (('psi', psi), ('r_out', r_out), ('r0', r0)):
        ha, hb = a.host(), b.host()
        assert (ha.view(np.uint32) == hb.view(np.uint32)).all(), (what, np.argwhere(ha != hb)[:4].tolist())


CHAIN = dict(T=37, V=31, C=6, rpu=2, picks=[(2, 0, 5, 3, 1, 4), (1, 1, 0, 5, 2, 3)])


def ctc_chain(dtype, batched, kernels=None):
    """init -> score (empty prefix) -> gather the state of a chosen candidate per row -> score -> gather -> score: an error
    in the layout of the state compounds.  kernels: None (the restatement) or the device callables.  -> (psi3, r3)."""
    T, V, C, rpu = CHAIN['T'], CHAIN['V'], CHAIN['C'], CHAIN['rpu']
    U = 3 if batched else 1
    N = U * rpu if batched else 4
    tlen = np.array([5, T, T // 2], dtype=np.int32) if batched else np.array([T], dtype=np.int32)
    x = R.log_softmax32(3.0 * np.random.RandomState(99 + batched).randn(U, T, V))
    rng = np.random.RandomState(7)
    cands = [np.stack([rng.permutation(np.arange(1, V))[:C] for _ in range(N)]).astype(np.int32) for _ in range(3)]
    utt = lambda n: n // rpu if batched else 0
    if kernels is not None:
        return kernels(x, tlen, cands, N, C, T, V, rpu)
    r = np.stack([np.pad(R.ctc_prefix_init(x[utt(n), :tlen[utt(n)]], dtype), ((0, T - tlen[utt(n)]), (0, 0)), constant_values=R.DO.LOGZERO_CTC)
                  for n in range(N)])
    plen, last = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    for k in range(3):
        psi, rn = R.ctc_prefix_score_batched(x, tlen, r, cands[k], plen, last, rpu, dtype) if batched else \
            R.ctc_prefix_score_batched(x, np.array([T] * N), r, cands[k], plen, last, 10 ** 6, dtype)
        if k < 2:
            pick = np.array([CHAIN['picks'][k][n % 6] for n in range(N)])
            r = np.nan_to_num(rn[np.arange(N), pick], nan=0.0)            # frames past tlen: never read again
            plen, last = plen + 1, cands[k][np.arange(N), pick]
    return psi, np.nan_to_num(rn, nan=0.0)


def _device_chain(batched):
    from src import hipabi as H

    def run(x, tlen, cands, N, C, T, V, rpu):
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        st = H.stream_ptr()
        xd, td = d(x), d(tlen)
        r = torch.zeros(N, T, 2, device='cuda')
        if batched:
            H.call('asr_ctc_prefix_init_batched', H.ptr(xd), H.ptr(td), H.ptr(r), N, rpu, T, V, st)
        else:
            H.call('asr_ctc_prefix_init', H.ptr(xd), H.ptr(r), T, V, st)
            r.copy_(r[0].expand(N, T, 2).clone())
        plen, last = torch.zeros(N, dtype=torch.int32, device='cuda'), torch.zeros(N, dtype=torch.int32, device='cuda')
        for k in range(3):
            psi, rn = torch.zeros(N, C, device='cuda'), torch.zeros(N, C, T, 2, device='cuda')
            cd = d(cands[k])
            if batched:
                H.call('asr_ctc_prefix_score_batched', H.ptr(xd), H.ptr(td), H.ptr(r), H.ptr(cd), H.ptr(plen), H.ptr(last), H.ptr(psi), H.ptr(rn),
                       N, C, T, V, rpu, st)
            else:
                H.call('asr_ctc_prefix_score', H.ptr(xd), H.ptr(r), H.ptr(cd), H.ptr(plen), H.ptr(last), H.ptr(psi), H.ptr(rn), N, C, T, V, st)
            if k < 2:
                pick = torch.tensor([CHAIN['picks'][k][n % 6] for n in range(N)], device='cuda')
                idx = (torch.arange(N, device='cuda') * C + pick).to(torch.int64)          # ctc_index as asr_beam_step writes it
                r = torch.zeros(N, T, 2, device='cuda')
                H.call('asr_gather_rows', H.ptr(rn), H.ptr(idx), H.ptr(r), N, T * 2, T * 2, T * 2, N * C, st)
                plen, last = plen + 1, cd[torch.arange(N, device='cuda'), pick].contiguous()
        torch.cuda.synchronize()
        return psi.cpu().numpy(), rn.cpu().numpy()
    return run


@pytest.mark.gpu
@pytest.mark.parametrize('batched', [False, True])
def test_ctc_prefix_chain_of_three_calls(batched):
    psi_g, r_g = ctc_chain(None, batched, _device_chain(batched))
    psi, r = ctc_chain(np.float64, batched)
    T, rpu = CHAIN['T'], CHAIN['rpu']
    tl = [5, T, T // 2] if batched else [T]
    for n in range(psi.shape[0]):
        t_ = tl[n // rpu] if batched else T
        dev = max(rel_dev(psi_g[n], psi[n]), rel_dev(r_g[n, :, :t_], r[n, :, :t_]))
        assert dev <= TOL_FACTOR * CTC_DEV, (n, dev)


# ---- asr_lstm_cell -------------------------------------------------------------------------------------------------------
LSTM_CASES = [(N, D, cp, sc) for (N, D) in ((1, 1), (5, 257), (3, 1024)) for cp in (True, False) for sc in (1.0, 30.0)]


def lstm_inputs(N, D, with_c, scale):
    rng = np.random.RandomState(N * 10000 + D + int(scale))
    pre = (scale * rng.uniform(-1, 1, size=(N, 4 * D))).astype(np.float32)
    pre.flat[::7] = np.sign(pre.flat[::7]) * scale                         # the extremes are present
    bih, bhh = (0.5 * rng.randn(4 * D)).astype(np.float32), (0.5 * rng.randn(4 * D)).astype(np.float32)
    c_prev = (2.0 * rng.randn(N, D)).astype(np.float32) if with_c else None
    return pre, bih, bhh, c_prev


def lstm_fp32_dev():
    dev = 0.0
    for N, D, cp, sc in LSTM_CASES:
        a, b = R.lstm_cell(*lstm_inputs(N, D, cp, sc)), R.lstm_cell(*lstm_inputs(N, D, cp, sc), dtype=np.float32)
        dev = max(dev, rel_dev(b[0], a[0]), rel_dev(b[1], a[1]))
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize('N,D,with_c,scale', LSTM_CASES)
def test_lstm_cell_equals_float64(N, D, with_c, scale):
    from src import hipabi as H
    pre, bih, bhh, c_prev = lstm_inputs(N, D, with_c, scale)
    d = lambda a: None if a is None else torch.from_numpy(a).cuda()
    pd, bi, bh, cp = d(pre), d(bih), d(bhh), d(c_prev)
    h, c = Guarded((N, D), torch.float32), Guarded((N, D), torch.float32)
    H.call('asr_lstm_cell', H.ptr(pd), H.ptr(bi), H.ptr(bh), H.ptr(cp), h.ptr(), c.ptr(), N, D, H.stream_ptr())
    torch.cuda.synchronize()
    h64, c64 = R.lstm_cell(pre, bih, bhh, c_prev)
    dev = max(rel_dev(h.host(), h64), rel_dev(c.host(), c64))
    print('lstm cell (%d,%d) c_prev %s scale %g: deviation %.3g (allowed %.3g)' % (N, D, with_c, scale, dev, TOL_FACTOR * LSTM_DEV))
    assert dev <= TOL_FACTOR * LSTM_DEV


# ---- asr_gather_rows -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('rows,width,src_ld,dst_ld,nsrc', [(5, 7, 9, 11, 4), (1, 1, 1, 1, 1), (64, 256, 256, 300, 64),
                                                           (9, 116537, 116537, 116538, 3)])       # the last: 4096*256 + 257 elements
def test_gather_rows_is_exact(rows, width, src_ld, dst_ld, nsrc):
    from src import hipabi as H
    rng = np.random.RandomState(rows + width)
    src = rng.randn(nsrc, src_ld).astype(np.float32)
    idx = rng.randint(0, nsrc, size=rows).astype(np.int64)
    idx[0] = -3
    idx[-1] = nsrc + 5
    if rows > 3:
        idx[1] = idx[2] = nsrc - 1
    dst = Guarded((rows, dst_ld), torch.float32)
    sd, idd = torch.from_numpy(src).cuda(), torch.from_numpy(idx).cuda()
    H.call('asr_gather_rows', H.ptr(sd), H.ptr(idd), dst.ptr(), rows, width, src_ld, dst_ld, nsrc, H.stream_ptr())
    torch.cuda.synchronize()
    got = dst.host()
    assert (got[:, :width] == R.gather_rows(src, idx)[:, :width]).all()
    assert (got[:, width:] == CAN_F).all()


# ---- asr_sample_tokens ---------------------------------------------------------------------------------------------------
SAMPLE_SEEDS = (12345, 7, 2 ** 32 + 5)                   # the last: the high key word matters
SAMPLE_CASES = [(V, seed, V + 3 * ((i + j) % 2), (1, 7)[(i + j + 1) % 2]) for i, V in enumerate((2, 31, 64, 65, 300, 2048))
                for j, seed in enumerate(SAMPLE_SEEDS)]


SAMPLE_REDRAW = {(2048, 12345): 2, (2048, 2 ** 32 + 5): 1}       # logits drawn again until at most 2 % of the rows sit near a bracket


def sample_logits(V, seed, rows=64):
    return (3.0 * np.random.RandomState(V + seed % 1000 + 7919 * SAMPLE_REDRAW.get((V, seed), 0)).randn(rows, V)).astype(np.float32)


def test_sample_cases_have_few_rows_near_a_bracket():
    for V, seed, _, _ in SAMPLE_CASES:
        _, margin = R.sample_tokens(sample_logits(V, seed), seed)
        assert (margin < R.sample_bracket_threshold(V)).mean() <= 0.02, (V, seed)


@pytest.mark.gpu
@pytest.mark.parametrize('V,seed,ld,out_ld', SAMPLE_CASES)
def test_sample_tokens_equal_the_restatement(V, seed, ld, out_ld):
    from src import hipabi as H
    rows = 64
    x = sample_logits(V, seed)
    for perm in (np.arange(rows), np.random.RandomState(1).permutation(rows)):           # a row's uniform belongs to (seed, row), not to its logits
        xp = x[perm]
        buf = np.full((rows, ld), 50.0, dtype=np.float32)              # the padding would win every draw if it were read
        buf[:, :V] = xp
        out = Guarded((rows, out_ld), torch.int64)
        bd = torch.from_numpy(buf).cuda()
        H.call('asr_sample_tokens', H.ptr(bd), ld, out.ptr(), out_ld, rows, V, seed, H.stream_ptr())
        torch.cuda.synchronize()
        got = out.host()
        assert (got[:, 1:] == CAN_I).all()
        pick, margin = R.sample_tokens(xp, seed)
        off = got[:, 0] != pick
        assert (np.abs(got[off, 0] - pick[off]) == 1).all() and (margin[off] < R.sample_bracket_threshold(V)).all(), \
            (np.nonzero(off)[0].tolist(), got[off, 0].tolist(), pick[off].tolist(), margin[off].tolist())


@pytest.mark.gpu
def test_sampler_follows_softmax_at_v300():
    from src import hipabi as H
    V, rows = 300, 20000
    logit = (1.5 * np.random.RandomState(3).randn(V)).astype(np.float32)
    logits = torch.from_numpy(logit).repeat(rows, 1).cuda().contiguous()
    out = torch.full((rows,), -1, dtype=torch.int64, device='cuda')
    H.call('asr_sample_tokens', H.ptr(logits), V, H.ptr(out), 1, rows, V, 2 ** 33 + 1, H.stream_ptr())
    got = out.cpu().numpy()
    assert got.min() >= 0 and got.max() < V
    p = np.exp(logit.astype(np.float64) - logit.max())
    p /= p.sum()
    freq = np.bincount(got, minlength=V) / rows
    sigma = np.sqrt(0.25 / rows)                          # no class has a larger standard deviation than p = 1/2 would
    assert np.abs(freq - p).max() < 4 * sigma             # 0.0141: at least 4 sigma for every class


# ---- the recorded deviations, re-measured without a GPU --------------------------------------------------------------------
def test_fp32_transcription_within_the_recorded_deviation():
    for what, dev, rec in (('step', step_fp32_dev(), STEP_DEV), ('ctc', ctc_fp32_dev(), CTC_DEV), ('lstm', lstm_fp32_dev(), LSTM_DEV)):
        print('%s: fp32 transcription deviates by %.4g (recorded %.4g)' % (what, dev, rec))
        assert dev <= rec
