"""The yardstick of two-pass decoding's second pass: a plain-numpy restatement of what csrc/rescore.hip computes
(asr_rescore_pack, asr_rescore_nbest), checked here against torch.log_softmax in float64 and on hand-made lists.
tests/test_hip_rescore.py imports `rescore_nbest`, `pack` and the seeded case generator from this file; nothing here imports
the code under test except the export check at the end.

One utterance, K beam slots.  `hyps[i]` is the token list of slot i, or None for an unused slot.  A hypothesis is scored
with an <eos> appended unless its last token is <eos> already (so the empty hypothesis scores the one <eos>):
  att_score[i] = sum_{t < tgt_len} log_softmax(logits[i, t, :])[target[t]]        added in order of t
  total[i]     = (1 - w) * att_score[i] + w * ctc_score[i] + (first_score[i] - ctc_score[i])
first_score is what the first pass ranked by: the CTC score plus, with a language model, its LM and length-bonus terms, which
so ride along unweighted.  A target whose logit is -inf makes att_score = total = -inf (never NaN, whatever w).  order lists
the slots by descending total, ties to the lower slot, unused slots (att_score = total = -inf) last."""
import numpy as np
import pytest
import torch

NEG_INF = float('-inf')
EOS = 1


def targets_of(hyp, eos=EOS):
    """The tokens the decoder is asked for: the hypothesis and its <eos>, not doubled."""
    hyp = [int(c) for c in hyp]
    return hyp if hyp and hyp[-1] == eos else hyp + [eos]


def pack(hyps, Lr, eos=EOS):
    """hyps (K token lists, None = unused slot) -> teacher (K,Lr) int64 zero-padded, tgt_len (K) int32."""
    teacher, tgt_len = np.zeros((len(hyps), Lr), dtype=np.int64), np.zeros(len(hyps), dtype=np.int32)
    for i, h in enumerate(hyps):
        if h is None:
            continue
        t = targets_of(h, eos)
        assert len(t) <= Lr
        teacher[i, :len(t)], tgt_len[i] = t, len(t)
    return teacher, tgt_len


def rescore_nbest(logits, hyps, ctc_scores, first_scores, ctc_weight, eos=EOS, dtype=np.float64):
    """logits (K,L,V) -> (att_scores (K), totals (K), order: list of slots by rank).  Only logits[i, :tgt_len[i], :] is read.
    `dtype` is the arithmetic: float64 is the yardstick, float32 its transcription that sizes the kernel's tolerance."""
    dt = dtype
    K = len(hyps)
    att, total = np.full(K, NEG_INF, dtype=dt), np.full(K, NEG_INF, dtype=dt)
    w = dt(ctc_weight)
    with np.errstate(all='ignore'):
        for i, h in enumerate(hyps):
            if h is None:
                continue
            a = dt(0.0)
            for t, c in enumerate(targets_of(h, eos)):
                row = np.asarray(logits[i, t], dtype=dt)
                x = row[c]
                if x == NEG_INF:
                    a = dt(NEG_INF)
                    continue
                m = row.max()
                a = dt(a + dt(dt(x - m) - np.log(np.exp(row - m).sum(dtype=dt))))
            att[i] = a
            if a > NEG_INF:
                ctc, first = dt(ctc_scores[i]), dt(first_scores[i])
                total[i] = dt(dt(dt(dt(1.0) - w) * a) + dt(w * ctc)) + dt(first - ctc)
    order = sorted(range(K), key=lambda i: (hyps[i] is None, -float(total[i]), i))
    return att, total, order


def final_gap(total, order, hyps):
    """Smallest distance between adjacent totals of the ranked used slots (inf for fewer than two finite ones)."""
    s = [float(total[i]) for i in order if hyps[i] is not None and total[i] > NEG_INF]
    return min([a - b for a, b in zip(s, s[1:])] + [float('inf')])


# ---- seeded cases (shared with tests/test_hip_rescore.py) ---------------------------------------------------------------
def make_utterance(seed, K, n, L, V, scale, special=(), lm=False, eos=EOS):
    """One utterance of a case: n used slots of K.  Hypotheses of 0..Lcap tokens, Lcap = max(1, L - 1), none scoring more than L
    tokens; `special` forces 'empty' (slot 0), 'eos' (slot 1 ends in <eos>) and 'full' (slot 2 has Lcap tokens) where those slots
    are used.  logits (K,L,V) = scale * randn in fp32; 'holes' puts a fifth of the logits at -inf sparing the targets,
    'target_hole' puts the first target of the last used slot at -inf.  ctc_scores descend as a first pass's do;
    first_scores = ctc_scores, plus with `lm` a random LM part per slot.  All scores are fp32-representable."""
    rng = np.random.RandomState(seed)
    Lcap = max(1, L - 1)
    lo = 2 if V > 2 else 0
    hyps = []
    for i in range(K):
        if i >= n:
            hyps.append(None)
            continue
        l = int(rng.randint(0, Lcap + 1))
        if 'empty' in special and i == 0:
            l = 0
        if 'full' in special and i == 2:
            l = Lcap
        h = [int(c) for c in rng.randint(lo, V, size=l)]
        if 'eos' in special and i == 1:
            h = (h or [eos])[:-1] + [eos]
        if len(targets_of(h, eos)) > L:
            h[-1] = eos
        hyps.append(h)
    logits = (scale * rng.randn(K, L, V)).astype(np.float32)
    if 'holes' in special:
        hole = rng.rand(K, L, V) < 0.2
        for i, h in enumerate(hyps):
            for t, c in enumerate(targets_of(h, eos) if h is not None else []):
                hole[i, t, c] = False
        logits[hole] = NEG_INF
    if 'target_hole' in special and n > 0:
        logits[n - 1, 0, targets_of(hyps[n - 1], eos)[0]] = NEG_INF
    ctc = np.sort(-rng.rand(K) * 4.0 * L)[::-1].astype(np.float32)
    first = (ctc + (rng.randn(K) * 3.0 if lm else 0.0)).astype(np.float32)
    return hyps, logits, ctc, first


# ---- the restatement itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V,L,scale', [(2, 1, 3.0), (31, 5, 3.0), (65, 9, 80.0), (300, 4, 1.0)])
def test_att_score_equals_torch_log_softmax(V, L, scale):
    hyps, logits, ctc, first = make_utterance(5 + V, 4, 4, L, V, scale, special=('empty', 'eos', 'full'))
    att, _, _ = rescore_nbest(logits, hyps, ctc, first, 0.5)
    lsm = torch.log_softmax(torch.from_numpy(logits).double(), dim=-1)
    for i, h in enumerate(hyps):
        tgt = torch.tensor(targets_of(h))
        want = float(lsm[i, torch.arange(len(tgt)), tgt].sum())
        assert abs(float(att[i]) - want) <= 1e-12 * max(1.0, abs(want)), (i, float(att[i]), want)


def test_eos_is_appended_not_doubled_and_the_empty_hypothesis_scores_one_eos():
    assert targets_of([5, 7]) == [5, 7, 1] and targets_of([5, 1]) == [5, 1] and targets_of([]) == [1] and targets_of([1]) == [1]
    teacher, tgt_len = pack([[5, 7], [5, 1], [], None], 4)
    assert teacher.tolist() == [[5, 7, 1, 0], [5, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]] and teacher.dtype == np.int64
    assert tgt_len.tolist() == [3, 2, 1, 0] and tgt_len.dtype == np.int32
    logits = np.log(np.array([[[0.1, 0.2, 0.3, 0.4]] * 3] * 3))           # (3 slots, 3 positions, V = 4)
    att, _, _ = rescore_nbest(logits, [[3, 2], [3, 1], []], [0.0] * 3, [0.0] * 3, 0.0)
    assert abs(att[0] - np.log(0.4 * 0.3 * 0.2)) < 1e-12              # 3, 2 and the appended <eos>
    assert abs(att[1] - np.log(0.4 * 0.2)) < 1e-12                    # 3 and its own <eos>, no second one
    assert abs(att[2] - np.log(0.2)) < 1e-12                          # the one <eos>


def test_ties_go_to_the_lower_first_pass_slot():
    logits = np.zeros((4, 2, 5))
    hyps = [[2], [3], [4], [2]]                                       # every slot scores 2 log(1/5)
    att, total, order = rescore_nbest(logits, hyps, [-1.0, -2.0, -1.0, -1.0], [-1.0, -2.0, -1.0, -1.0], 0.5)
    assert len(set(att.tolist())) == 1
    assert order == [0, 2, 3, 1]                                      # slots 0, 2, 3 tie and keep their order; slot 1 is behind
    assert total[order[0]] == total[order[1]] == total[order[2]] > total[order[3]]


def test_unused_slots_come_last():
    hyps, logits, ctc, first = make_utterance(3, 6, 3, 4, 31, 3.0)
    assert hyps[3:] == [None] * 3
    logits[3:] = np.nan                                               # never read
    att, total, order = rescore_nbest(logits, hyps, ctc, first, 0.3)
    assert sorted(order[:3]) == [0, 1, 2] and order[3:] == [3, 4, 5]
    assert np.isfinite(att[:3]).all() and (att[3:] == NEG_INF).all() and (total[3:] == NEG_INF).all()
    assert [float(total[i]) for i in order[:3]] == sorted((float(x) for x in total[:3]), reverse=True)
    # a used slot at -inf is still ahead of the unused ones
    logits[0, 0, targets_of(hyps[0])[0]] = NEG_INF
    _, total, order = rescore_nbest(logits, hyps, ctc, first, 0.3)
    assert order[2:] == [0, 3, 4, 5] and total[0] == NEG_INF


@pytest.mark.parametrize('w', [0.0, 0.3, 1.0])
def test_minus_infinity_at_a_target_gives_minus_infinity_not_nan(w):
    hyps, logits, ctc, first = make_utterance(4, 4, 4, 5, 31, 3.0, special=('holes', 'target_hole'))
    assert np.isinf(logits).mean() > 0.1
    att, total, order = rescore_nbest(logits, hyps, ctc, first, w)
    assert not np.isnan(att).any() and not np.isnan(total).any()
    assert att[3] == NEG_INF and total[3] == NEG_INF and np.isfinite(att[:3]).all() and np.isfinite(total[:3]).all()
    assert order[-1] == 3
    a32, t32, o32 = rescore_nbest(logits, hyps, ctc, first, w, dtype=np.float32)
    assert not np.isnan(a32).any() and not np.isnan(t32).any() and o32 == order


def test_the_first_pass_term_is_additive():
    hyps, logits, ctc, first = make_utterance(6, 5, 5, 6, 31, 3.0)
    c = np.array([0.5, -2.0, 3.25, 0.0, -7.5])
    att0, total0, _ = rescore_nbest(logits, hyps, ctc, ctc, 0.3)
    att1, total1, _ = rescore_nbest(logits, hyps, ctc, ctc.astype(np.float64) + c, 0.3)
    assert (att0 == att1).all()
    assert np.abs((total1 - total0) - c).max() < 1e-12
    # without an LM (first = ctc) the total is the plain interpolation
    assert np.abs(total0 - (0.7 * att0 + 0.3 * ctc.astype(np.float64))).max() < 1e-12


def test_rescore_entries_are_exported():
    from src import hipabi
    import ctypes
    for name in ('asr_rescore_pack', 'asr_rescore_nbest'):
        assert name in hipabi.exported_symbols()
        assert hasattr(ctypes.CDLL(hipabi.LIB_PATH), name)
