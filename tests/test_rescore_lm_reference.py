"""The yardstick of the RNN-LM in two-pass decoding's second pass: plain-numpy restatements of asr_rescore_lm_input,
asr_rescore_token_logp and asr_rescore_rank_lm (csrc/rescore.hip), written from the comments of include/asr_hip.h and checked
here against torch.log_softmax in float64, against the LM term of the fused search (tests/test_ctc_beam_lm_reference.py::lm_term)
and on hand-made lists.  tests/test_hip_rescore_lm.py imports the restatements, the case table and its seeds from this file;
nothing here imports the code under test except the chunk rule and the export check at the end.

Row r = u*K + i is beam slot i of utterance u, its hypothesis l_1..l_n with n = len[r]:
  lm_in[r,0] = sos, lm_in[r,t] = teacher[r,t-1]                                         (the LM's input, teacher = pack()'s table)
  tok_logp[r,t] = log_softmax(logits[r,t,:])[teacher[r,t]] for t < min(max(len[r],0), L), else 0
  lm_score[r] = sum_{t < len} tok_logp[r,t]                                              (0 for the empty hypothesis)
  total[r]    = (1 - w) * att_score[r] + w * ctc_score[r] + lm_weight * lm_score[r] + len_bonus * len[r]
att_score, ctc_score or (with lm_weight > 0) lm_score at -inf give total = -inf, never NaN; lm_weight = 0 leaves the LM term out.
Unused slots (i >= n[u]) get lm_score = total = -inf.  order lists the slots by descending total, ties to the lower slot, unused
slots last.

The case table (CASES) holds, per case, the shapes, weights, paddings and the seeds of its utterances.  The seeds were searched
with the restatement alone (`case_ok`): adjacent totals of every utterance are more than GAP apart, so fp32 rounding cannot
reorder them and a device's `order` must match exactly; every single-utterance case with K >= 4 and an LM weight has an order that
the LM term changes.  test_committed_seeds_hold_the_gaps re-checks that here.

Score tolerance: the restatement transcribed to fp32 numpy deviates from float64 by at most FP32_DEV, relative to
max(1, |score| / 20), over every tok_logp, lm_score and total of the table; a kernel is allowed SCORE_TOL = 4 x FP32_DEV in the same
units (the factor covers the order of the sums across lanes and the device's exp / log)."""
import types

import numpy as np
import pytest
import torch

from test_ctc_beam_lm_reference import lm_term, trigram_table
from test_rescore_reference import EOS, NEG_INF, make_utterance, pack, targets_of

SOS = 0
GAP = 1e-3
# largest deviation of the fp32 transcription from float64 over every tok_logp, lm_score and total of every case, relative to
# max(1, |score| / 20) (fp32_deviation): case magnitude_80, whose LM scores near -5900 carry an fp32 ulp of 4.9e-4 per addition
FP32_DEV = 3.0642148382262176e-06
SCORE_TOL = 4 * FP32_DEV
TL_BLOCK_V = 1024                      # asr_rescore_token_logp takes a row in blocks of this many columns: the first V with a second block is one above


# ---- the restatements ------------------------------------------------------------------------------------------------------
def lm_input(teacher, L, sos=SOS):
    """teacher (R, >= L) int64 -> lm_in (R,L) int64."""
    teacher = np.asarray(teacher)
    out = np.empty((teacher.shape[0], L), dtype=np.int64)
    out[:, 0] = sos
    out[:, 1:] = teacher[:, :L - 1]
    return out


def token_logp(logits, target, lens, L, dtype=np.float64):
    """logits (R, >= L, V), target (R, >= L), lens (R) -> (R,L).  Only logits[r, :min(max(len,0),L), :] is read."""
    dt = dtype
    R, V = logits.shape[0], logits.shape[2]
    out = np.zeros((R, L), dtype=dt)
    with np.errstate(all='ignore'):
        for r in range(R):
            for t in range(max(0, min(int(lens[r]), L))):
                row = np.asarray(logits[r, t], dtype=dt)
                c = int(target[r, t])
                x = row[c] if 0 <= c < V else dt(NEG_INF)
                if x == NEG_INF:
                    out[r, t] = NEG_INF
                    continue
                m = row.max()
                out[r, t] = dt(dt(x - m) - np.log(np.exp(row - m).sum(dtype=dt)))
    return out


def rank_lm(att, ctc, tok_logp, lens, n_used, L, ctc_weight, lm_weight, len_bonus, dtype=np.float64):
    """One utterance: att, ctc (K), tok_logp (K, >= L), lens (K), n_used -> (lm_score (K), total (K), order)."""
    dt = dtype
    K = len(att)
    lm, total = np.full(K, NEG_INF, dtype=dt), np.full(K, NEG_INF, dtype=dt)
    w, lw, bonus = dt(ctc_weight), dt(lm_weight), dt(len_bonus)
    with np.errstate(all='ignore'):
        for i in range(n_used):
            n = max(0, min(int(lens[i]), L))
            s = dt(0.0)
            for t in range(n):
                s = dt(s + dt(tok_logp[i, t]))
            lm[i] = s
            a, c = dt(att[i]), dt(ctc[i])
            if a == NEG_INF or c == NEG_INF or (lw != 0 and s == NEG_INF):
                continue
            tot = dt(dt(dt(dt(1.0) - w) * a) + dt(w * c))
            if lw != 0:
                tot = dt(tot + dt(lw * s))
            total[i] = dt(tot + dt(bonus * dt(n)))
    order = sorted(range(K), key=lambda i: (i >= n_used, -float(total[i]), i))
    return lm, total, order


def total_gap(total, order, n_used):
    """Smallest distance between adjacent finite totals of the ranked used slots (inf for fewer than two)."""
    s = [float(total[i]) for i in order if i < n_used and total[i] > NEG_INF]
    return min([a - b for a, b in zip(s, s[1:])] + [float('inf')])


# ---- the case table (shared with tests/test_hip_rescore_lm.py) -----------------------------------------------------------------
W3 = float(np.float32(0.3))             # weights a device's fp32 argument holds exactly
# name -> K, V, L, scale, ctc_weight, lm_weight, len_bonus, special, pad (extra elements per position / row / table row),
#         [(seed, used slots) per utterance]
# special, beyond make_utterance's: 'over' gives slot 2 (which 'full' fills to L targets) len = L + 1, clamped to L; 'exact' gives
# it len = L, so that its last position is scored too; 'att_hole' puts the attention score of slot 0 at -inf.
CASES = {
    'v2_l1_k1': (1, 2, 1, 3.0, 0.5, W3, 0.25, (), 0, [(0, 1)]),
    'v31_l2_k4': (4, 31, 2, 3.0, W3, 0.5, 0.25, ('empty', 'eos', 'full', 'over'), 3, [(0, 4)]),
    'v64_l37_k4': (4, 64, 37, 3.0, W3, 0.5, 0.0, ('empty', 'eos', 'full', 'exact'), 0, [(0, 4)]),
    'v65_l37_k16': (16, 65, 37, 3.0, 0.5, W3, 0.25, ('empty', 'eos', 'full', 'over'), 3, [(0, 16)]),
    'v300_l37_k4_ragged_u3': (4, 300, 37, 3.0, W3, 0.5, 0.25, ('eos',), 1, [(0, 4), (1, 0), (2, 2)]),
    'v5003_l2_k4': (4, 5003, 2, 3.0, W3, 0.5, 0.0, ('full', 'over'), 5, [(0, 3)]),
    'v1024_l2_k4_one_block': (4, TL_BLOCK_V, 2, 3.0, W3, 0.5, 0.25, ('full', 'exact'), 1, [(0, 4)]),
    'v1025_l2_k4_second_block': (4, TL_BLOCK_V + 1, 2, 3.0, W3, 0.5, 0.25, ('full', 'exact'), 3, [(0, 4)]),
    'v31_l37_k1_u3': (1, 31, 37, 3.0, W3, 0.5, 0.25, (), 2, [(0, 1), (1, 0), (2, 1)]),
    'v31_l37_k16_ragged_u3': (16, 31, 37, 3.0, W3, W3, 0.5, ('empty', 'eos', 'full', 'over'), 2, [(0, 16), (1, 0), (2, 5)]),
    'magnitude_80': (4, 31, 37, 80.0, 0.5, 0.5, 0.0, ('full',), 3, [(0, 4)]),
    'holes': (4, 31, 37, 3.0, W3, 0.5, 0.25, ('holes', 'full'), 3, [(0, 4), (1, 1), (2, 3)]),
    'target_hole': (4, 65, 37, 3.0, W3, 0.5, 0.25, ('target_hole', 'eos'), 0, [(0, 4)]),
    'lm_weight_0': (4, 31, 37, 3.0, W3, 0.0, 0.25, ('target_hole', 'att_hole'), 0, [(0, 4)]),
    'ctc_weight_0': (4, 31, 37, 3.0, 0.0, 0.5, 0.25, ('att_hole',), 0, [(0, 4)]),
    'ctc_weight_1': (4, 31, 37, 3.0, 1.0, 0.5, 0.0, ('target_hole', 'att_hole'), 0, [(0, 4)]),
}


def case_inputs(name, seeds=None):
    """-> K, V, L, (ctc_weight, lm_weight, len_bonus), pad, [per utterance: dict(hyps, logits (K,L,V) fp32, ctc, att, lens, n)].
    The logits, hypotheses and ctc scores are make_utterance's; lens[i] = the hypothesis' own token count (0 in an unused slot)
    but for 'over' / 'exact'; att (K) fp32 = a random attention score per slot."""
    K, V, L, scale, w, lw, bonus, special, pad, utts = CASES[name]
    out = []
    for u, (seed, n) in enumerate(utts):
        seed = seed if seeds is None else seeds[u]
        s = 1000 * seed + 7 * V + L + u
        hyps, logits, ctc, _ = make_utterance(s, K, n, L, V, scale, tuple(x for x in special if x in ('empty', 'eos', 'full', 'holes', 'target_hole')))
        lens = np.array([len(h) if h is not None else 0 for h in hyps], dtype=np.int32)
        if n > 2 and 'over' in special:
            lens[2] = L + 1
        if n > 2 and 'exact' in special:
            lens[2] = L
        att = (-np.random.RandomState(s + 977).rand(K) * 2.0 * L).astype(np.float32)
        if 'att_hole' in special and n > 0:
            att[0] = NEG_INF
        out.append({'hyps': hyps, 'logits': logits, 'ctc': ctc, 'att': att, 'lens': lens, 'n': n})
    return K, V, L, (w, lw, bonus), pad, out


def restate(name, dtype=np.float64, seeds=None):
    """Per utterance (teacher (K,L), lm_in (K,L), tok_logp (K,L), lm_score, total, order) of a case."""
    K, V, L, (w, lw, bonus), pad, utts = case_inputs(name, seeds)
    out = []
    for c in utts:
        teacher, _ = pack(c['hyps'], L)
        tl = token_logp(c['logits'], teacher, c['lens'], L, dtype)
        out.append((teacher, lm_input(teacher, L), tl) + rank_lm(c['att'], c['ctc'], tl, c['lens'], c['n'], L, w, lw, bonus, dtype))
    return out


_REF = {}


def reference(name):
    """The float64 restatement of a case, computed once."""
    if name not in _REF:
        _REF[name] = restate(name)
    return _REF[name]


def lm_changes_the_order(name, seeds=None):
    K, V, L, (w, lw, bonus), pad, utts = case_inputs(name, seeds)
    res = restate(name, seeds=seeds)
    for c, (teacher, _, tl, lm, total, order) in zip(utts, res):
        if rank_lm(c['att'], c['ctc'], tl, c['lens'], c['n'], L, w, 0.0, 0.0)[2] != order:
            return True
    return False


def case_ok(name, seeds=None):
    """The conditions the seed search asked of a case, on the restatement alone."""
    K, V, L, (w, lw, bonus), pad, utts = case_inputs(name, seeds)
    special = CASES[name][7]
    for c, (teacher, _, tl, lm, total, order) in zip(utts, restate(name, seeds=seeds)):
        n = c['n']
        if total_gap(total, order, n) <= GAP:
            return False
        if 'target_hole' in special and n > 0 and not (lm[n - 1] == NEG_INF and np.isfinite(lm[:n - 1]).all()):
            return False
        if 'full' in special and n > 2 and len(targets_of(c['hyps'][2])) != L:
            return False
        if 'empty' in special and n > 0 and not (c['lens'][0] == 0 and lm[0] == 0):
            return False
    if K >= 4 and len(utts) == 1 and lw > 0 and 'att_hole' not in special and not lm_changes_the_order(name, seeds):
        return False
    return True


def rel(got, want):
    return abs(got - want) / max(1.0, abs(want) / 20)


def fp32_deviation(name):
    """Largest deviation, relative to max(1, |score| / 20), of the fp32 transcription from float64 over a case's scores."""
    worst = 0.0
    for (_, _, tl32, lm32, tot32, o32), (_, _, tl, lm, tot, order) in zip(restate(name, np.float32), reference(name)):
        assert o32 == order
        for got, want in zip(np.concatenate([tl32.ravel(), lm32, tot32]), np.concatenate([tl.ravel(), lm, tot])):
            if want == NEG_INF:
                assert got == NEG_INF
            else:
                worst = max(worst, rel(float(got), float(want)))
    return worst


@pytest.mark.parametrize('name', sorted(CASES))
def test_committed_seeds_hold_the_gaps(name):
    assert case_ok(name)
    dev = fp32_deviation(name)
    # numpy's fp32 exp differs in the last bit between hosts, so the recorded maximum is printed beside the measured value and
    # the transcription is held to what the kernel is held to
    print('%s: fp32 transcription deviates by %.3g relative to max(1, |score|/20) (recorded maximum %.3g)' % (name, dev, FP32_DEV))
    assert dev <= SCORE_TOL


def test_the_lm_term_changes_an_order_with_k_at_least_4():
    assert any(CASES[name][0] >= 4 and lm_changes_the_order(name) for name in CASES)


def test_the_table_covers_what_it_must():
    Vs, Ls, Ks = {c[1] for c in CASES.values()}, {c[2] for c in CASES.values()}, {c[0] for c in CASES.values()}
    assert {2, 31, 64, 65, 300, 5003, TL_BLOCK_V, TL_BLOCK_V + 1} <= Vs and {1, 2, 37} <= Ls and {1, 4, 16} <= Ks
    assert any(len(c[9]) == 3 and any(n == 0 for _, n in c[9]) and any(0 < n < c[0] for _, n in c[9]) for c in CASES.values())
    assert any((len(c[9]) * c[0]) % 4 for c in CASES.values())                    # rows that do not fill a workgroup's four waves
    lens = [(int(l), L) for name in CASES for L, cs in [(CASES[name][2], case_inputs(name)[5])] for c in cs for l in c['lens'][:c['n']]]
    assert any(l == 0 for l, L in lens) and any(l == L for l, L in lens) and any(l == L + 1 for l, L in lens)
    assert any(c[3] == 80.0 for c in CASES.values()) and any('holes' in c[7] for c in CASES.values())
    assert any(c[5] == 0.0 for c in CASES.values()) and {0.0, 1.0} <= {c[4] for c in CASES.values()}
    assert any(c[8] > 0 for c in CASES.values())


# ---- the restatements themselves -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V,L,scale', [(2, 1, 3.0), (31, 5, 3.0), (65, 9, 80.0), (300, 4, 1.0)])
def test_token_logp_equals_torch_log_softmax(V, L, scale):
    hyps, logits, _, _ = make_utterance(5 + V, 4, 4, L, V, scale, special=('empty', 'eos', 'full'))
    teacher, tgt_len = pack(hyps, L)
    got = token_logp(logits, teacher, tgt_len, L)                               # every target, the <eos> included
    lsm = torch.log_softmax(torch.from_numpy(logits).double(), dim=-1)
    want = lsm.gather(2, torch.from_numpy(teacher).unsqueeze(-1)).squeeze(-1).numpy()
    for i in range(4):
        n = int(tgt_len[i])
        assert np.abs(got[i, :n] - want[i, :n]).max() <= 1e-12 * max(1.0, np.abs(want[i, :n]).max())
        assert (got[i, n:] == 0).all()


def test_the_shift_rule():
    teacher, tgt_len = pack([[5, 7], [5, 1], [], None], 4)
    assert lm_input(teacher, 4).tolist() == [[0, 5, 7, 1], [0, 5, 1, 0], [0, 1, 0, 0], [0, 0, 0, 0]]     # empty: <sos> and the <eos> nobody scores
    assert lm_input(teacher, 3).tolist() == [[0, 5, 7], [0, 5, 1], [0, 1, 0], [0, 0, 0]]
    assert lm_input(teacher, 1).tolist() == [[0]] * 4 and lm_input(teacher, 2, sos=9)[:, 0].tolist() == [9] * 4
    assert lm_input(teacher, 4).dtype == np.int64
    # the empty hypothesis and the unused slot score nothing: no logit is read (NaN everywhere), lm_score 0 and -inf
    logits = np.full((4, 4, 8), np.nan)
    logits[0, :2], logits[1, :2] = 0.0, 0.0
    lens = np.array([2, 2, 0, 0])
    tl = token_logp(logits, teacher, lens, 4)
    assert not np.isnan(tl).any() and (tl[2:] == 0).all() and np.allclose(tl[:2, :2], -np.log(8)) and (tl[:2, 2:] == 0).all()
    lm, total, order = rank_lm(np.zeros(4), np.zeros(4), tl, lens, 3, 4, 0.5, 1.0, 0.0)
    assert lm[2] == 0 and lm[3] == NEG_INF and total[3] == NEG_INF and order == [2, 0, 1, 3]


@pytest.mark.parametrize('w,bonus', [(0.5, 0.0), (0.3, 0.25), (1.0, -0.5)])
def test_lm_score_is_the_lm_term_of_the_fused_search(w, bonus):
    V, L = 5, 7
    table = trigram_table(3, V)
    hyps = [[2, 3, 4, 2], [], [4], [3, 3, 1], [2, 4, 4, 3, 2, 2]]
    teacher, _ = pack(hyps, L)
    lens = np.array([len(h) for h in hyps])
    lm_in = lm_input(teacher, L)
    # what a trigram LM answers to lm_in: position t sees <sos> = 0 in front and the tokens up to t
    logits = np.array([[table[tuple(((0,) + tuple(lm_in[i, :t + 1]))[-2:])] for t in range(L)] for i in range(len(hyps))])
    tl = token_logp(logits, teacher, lens, L)
    lm, total, _ = rank_lm(np.zeros(len(hyps)), np.zeros(len(hyps)), tl, lens, len(hyps), L, 0.0, w, bonus)
    for i, h in enumerate(hyps):
        want = lm_term(table, h, w, bonus)
        assert abs(w * lm[i] + bonus * len(h) - want) < 1e-12 and abs(total[i] - want) < 1e-12


def test_ties_go_to_the_lower_slot_and_unused_slots_come_last():
    tl = np.zeros((6, 3))
    tl[:, 0] = [-1.0, -2.0, -1.0, -1.0, -9.0, -9.0]
    lens = np.array([1, 1, 1, 1, 1, 1])
    lm, total, order = rank_lm(np.zeros(6), np.zeros(6), tl, lens, 4, 3, 0.5, 1.0, 0.0)
    assert order == [0, 2, 3, 1, 4, 5] and total[0] == total[2] == total[3] > total[1]
    assert (lm[4:] == NEG_INF).all() and (total[4:] == NEG_INF).all()
    # a used slot at -inf is still ahead of the unused ones
    tl[0, 0] = NEG_INF
    lm, total, order = rank_lm(np.zeros(6), np.zeros(6), tl, lens, 4, 3, 0.5, 1.0, 0.0)
    assert order == [2, 3, 1, 0, 4, 5] and total[0] == NEG_INF


@pytest.mark.parametrize('w', [0.0, 0.3, 1.0])
@pytest.mark.parametrize('lw', [0.0, 0.5])
def test_minus_infinity_gives_minus_infinity_not_nan(w, lw):
    tl = np.array([[-1.0, NEG_INF], [-1.0, -2.0], [-1.0, -1.0], [-3.0, -1.0]])
    att, ctc, lens = np.array([-1.0, NEG_INF, -2.0, -1.0]), np.array([-1.0, -1.0, -2.0, NEG_INF]), np.array([2, 2, 2, 2])
    for dt in (np.float64, np.float32):
        lm, total, order = rank_lm(att, ctc, tl, lens, 4, 2, w, lw, 0.25, dt)
        assert not np.isnan(lm).any() and not np.isnan(total).any()
        assert lm[0] == NEG_INF and np.isfinite(lm[1:]).all()
        assert total[1] == NEG_INF and total[3] == NEG_INF and np.isfinite(total[2])
        assert (total[0] == NEG_INF) == (lw > 0)                  # lm_weight = 0 leaves the LM term out
        assert order[0] in (0, 2) and set(order[-2:]) <= {0, 1, 3}
    # a logit row that is -inf throughout, a target at -inf and a target outside 0..V-1
    logits = np.zeros((1, 3, 4))
    logits[0, 0], logits[0, 1, 2] = NEG_INF, NEG_INF
    got = token_logp(logits, np.array([[1, 2, 7]]), np.array([3]), 3)
    assert (got == NEG_INF).all()


# ---- the chunk rule of the host path, and the exports ------------------------------------------------------------------------------
def _chunk_rows(V, L, lm, rows=None):
    from src.decode import BeamDecoder
    bd = types.SimpleNamespace(lm=lm, asr=types.SimpleNamespace(vocab_size=V), lm_rescore_rows=rows)
    return BeamDecoder._rescore_lm_chunk_rows(bd, L)


def test_lm_chunk_rows():
    from src.decode import RESCORE_STATE_BYTES
    from src.lm import RNNLM
    small = RNNLM(31, False, 32, 'LSTM', 32, 2, 0.0)
    per_row = 4 * 37 * (31 + 32 + 6 * 32)
    assert _chunk_rows(31, 37, small) == RESCORE_STATE_BYTES // per_row > 10000
    assert _chunk_rows(31, 37, small, rows=3) == 3 and _chunk_rows(31, 37, small, rows=10 ** 9) == RESCORE_STATE_BYTES // per_row
    # emb_dim < dim (its shapes only: RNNLM refuses an untied model whose emb_dim differs from dim)
    gru = types.SimpleNamespace(dim=32, module='GRU', emb=types.SimpleNamespace(weight=torch.empty(1, 16)))
    assert _chunk_rows(31, 37, gru) == RESCORE_STATE_BYTES // (4 * 37 * (31 + 32 + 8 * 32))
    # a word vocabulary: the config's 4 x 1024 tied LM at V = 65 536 (its shapes only: the embedding alone would be 256 MiB)
    big = types.SimpleNamespace(dim=1024, module='LSTM', emb=types.SimpleNamespace(weight=torch.empty(1, 1024)))
    per_row = 4 * 300 * (65536 + 1024 + 6 * 1024)
    rows = _chunk_rows(65536, 300, big)
    assert rows == RESCORE_STATE_BYTES // per_row == 12 and rows * per_row <= RESCORE_STATE_BYTES < 128 * per_row
    assert _chunk_rows(65536, 300, big, rows=5) == 5 and _chunk_rows(65536, 300, big, rows=64) == 12
    assert _chunk_rows(65536, 10 ** 6, big) == 1 and _chunk_rows(65536, 10 ** 6, big, rows=4) == 1      # never below one row


def test_rescore_lm_entries_are_exported():
    from src import hipabi
    import ctypes
    for name in ('asr_rescore_lm_input', 'asr_rescore_token_logp', 'asr_rescore_rank_lm'):
        assert name in hipabi.exported_symbols()
        assert hasattr(ctypes.CDLL(hipabi.LIB_PATH), name)
