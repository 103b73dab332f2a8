"""The yardstick of CTC-only decoding: a plain-Python restatement of the frame-synchronous CTC prefix beam search that
csrc/ctc_decode.hip runs on the device (asr_ctc_beam_search), checked here against exhaustive enumeration of every
alignment.  tests/test_hip_ctc_beam.py imports `prefix_beam_search` from this file; nothing here imports the code under
test except the export check at the end.

The algorithm (blank = 0).  The beam holds at most K prefixes, each with (pb, pnb) = log-probability of the alignments
of the frames so far that collapse to the prefix and end in blank / in non-blank; it starts as the empty prefix with
(0, -inf).  Frame t, for every beam prefix l in slot i with last token e and p = logaddexp(pb, pnb):
  stay    l    : pb' (+)= p + lp[t,0];  pnb' (+)= pnb + lp[t,e] when l is not empty
  extend  l+c  : pnb' (+)= (pb if c == e else p) + lp[t,c]   for every allowed token c != 0
where (+) is logaddexp with -inf (+) -inf = -inf.  An extension l+c that is itself a beam member accumulates into that
member's entry, together with the member's own stay terms.  Allowed tokens: every non-blank one (cand = 0), else the
`cand` non-blank tokens with the largest lp[t,.] (ties: lower index).  The K entries with the largest
logaddexp(pb', pnb') survive; ties go to the smaller (parent slot, token), where a beam member's own entry counts as
(its slot, 0); entries at -inf are never kept.  The order of the survivors is the slot order of the next frame and,
after the last frame, the order of the hypotheses."""
import itertools

import numpy as np
import pytest

NEG_INF = float('-inf')


def _lse(a, b, dt):
    m = a if a > b else b
    if m == NEG_INF:
        return dt(NEG_INF)
    return dt(m + np.log1p(np.exp(-abs(a - b))))


def prefix_beam_search(lp, K, cand=0, dtype=np.float64):
    """lp (T,V) log-probabilities -> (hyps, gaps): hyps = [(tokens, score)] best first, at most K; gaps = the smallest
    margins any decision of the search had: 'keep' (K-th kept entry against the best rejected one, over the frames),
    'cand' (lp at the `cand` boundary, over the frames), 'final' (adjacent hypotheses of the result).  `dtype` is the
    arithmetic the search runs in: float64 is the yardstick, float32 its transcription that sizes the score tolerance."""
    dt = dtype
    lp = np.asarray(lp, dtype=dt)
    T, V = lp.shape
    beam = [((), dt(0.0), dt(NEG_INF))]
    keep_gap = cand_gap = float('inf')
    with np.errstate(all='ignore'):
        for t in range(T):
            row = lp[t]
            order = sorted(range(1, V), key=lambda c: (-row[c], c))
            if 0 < cand < V - 1:
                cand_gap = min(cand_gap, float(row[order[cand - 1]]) - float(row[order[cand]]))
                order = order[:cand]
            entries = {pre: [dt(NEG_INF), dt(NEG_INF), (i, 0)] for i, (pre, _, _) in enumerate(beam)}
            for i, (pre, pb, pnb) in enumerate(beam):
                p = _lse(pb, pnb, dt)
                e = pre[-1] if pre else 0
                own = entries[pre]
                own[0] = _lse(own[0], dt(p + row[0]), dt)
                if pre:
                    own[1] = _lse(own[1], dt(pnb + row[e]), dt)
                for c in order:
                    ent = entries.setdefault(pre + (c,), [dt(NEG_INF), dt(NEG_INF), (i, c)])
                    ent[1] = _lse(ent[1], dt((pb if c == e else p) + row[c]), dt)
            scored = [(_lse(pb, pnb, dt), key, pre, pb, pnb) for pre, (pb, pnb, key) in entries.items()]
            scored = sorted((s for s in scored if s[0] > NEG_INF), key=lambda s: (-s[0], s[1]))
            if len(scored) > K:
                keep_gap = min(keep_gap, float(scored[K - 1][0]) - float(scored[K][0]))
            beam = [(pre, pb, pnb) for _, _, pre, pb, pnb in scored[:K]]
    hyps = [(list(pre), float(_lse(pb, pnb, dt))) for pre, pb, pnb in beam]
    final_gap = min([a[1] - b[1] for a, b in zip(hyps, hyps[1:])] + [float('inf')])
    return hyps, {'keep': keep_gap, 'cand': cand_gap, 'final': final_gap}


def peaked_logp(seed, T, V, scale):
    """log_softmax(scale * randn) in float64, then rounded to the fp32 the device reads."""
    x = scale * np.random.RandomState(seed).randn(T, V)
    x = x - x.max(axis=1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=1, keepdims=True))).astype(np.float32)


def enumerate_labellings(lp):
    """Every one of the V**T alignments, collapsed (repeats merged, blanks dropped): labelling -> log-probability."""
    lp = np.asarray(lp, dtype=np.float64)
    T, V = lp.shape
    prob = {}
    for path in itertools.product(range(V), repeat=T):
        lab = tuple(c for c, prev in zip(path, (None,) + path[:-1]) if c != 0 and c != prev)
        prob[lab] = prob.get(lab, 0.0) + float(np.exp(sum(lp[t, c] for t, c in enumerate(path))))
    return {lab: float(np.log(v)) for lab, v in prob.items()}


# The K = 16 search drops whatever probability ran through a pruned prefix.  At V = 4 the beam overflows from frame 2 on, and
# what it drops is of the order exp(-scale * (a few standard deviations)) of the total: measured on these seeds 4e-6 at
# scale 6, 2e-11 at scale 12, below 1e-15 at scale 20.  So the 1e-10 check of the pruned search runs at scale 20, and the
# unpruned search (K >= number of labellings, nothing dropped) is held to 1e-10 on EVERY labelling at scale 6, where
# repeated symbols and merged prefixes carry weight: that is the check a wrong merge or repeat rule cannot pass.
@pytest.mark.parametrize('V,T', [(3, 5), (3, 6), (4, 5), (4, 6)])
@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_restatement_finds_the_most_probable_labelling(V, T, seed):
    lp = peaked_logp(100 * V + 10 * T + seed, T, V, 20.0).astype(np.float64)
    want = enumerate_labellings(lp)
    best = max(want, key=want.get)
    hyps, _ = prefix_beam_search(lp, 16)
    assert len(hyps) <= 16
    assert tuple(hyps[0][0]) == best
    assert abs(hyps[0][1] - want[best]) < 1e-10, (hyps[0][1], want[best])


@pytest.mark.parametrize('V,T', [(3, 5), (3, 6), (4, 5), (4, 6)])
def test_unpruned_restatement_equals_enumeration(V, T):
    lp = peaked_logp(7 * V + T, T, V, 6.0).astype(np.float64)
    want = enumerate_labellings(lp)
    hyps, _ = prefix_beam_search(lp, len(want))
    assert len(hyps) == len(want)
    assert tuple(hyps[0][0]) == max(want, key=want.get)
    for toks, score in hyps:
        assert abs(score - want[tuple(toks)]) < 1e-10, (toks, score, want[tuple(toks)])
    assert [s for _, s in hyps] == sorted((s for _, s in hyps), reverse=True)


def test_repeated_symbol_needs_a_blank_between():
    """Two frames that both favour symbol 1: '1' (the repeat collapses) must beat '1 1' (needs a blank that is not there),
    and the probabilities are those of the four alignments each."""
    lp = np.log(np.array([[0.1, 0.8, 0.1], [0.1, 0.8, 0.1]]))
    hyps, _ = prefix_beam_search(lp, 8)
    got = {tuple(h): s for h, s in hyps}
    assert hyps[0][0] == [1]
    assert abs(got[(1,)] - np.log(0.8 * 0.8 + 0.8 * 0.1 + 0.1 * 0.8)) < 1e-12
    assert (1, 1) not in got                   # two frames cannot hold 1, blank, 1
    assert abs(got[()] - np.log(0.01)) < 1e-12


def test_cand_pruning_and_minus_infinity():
    lp = peaked_logp(5, 6, 7, 3.0).astype(np.float64)
    lp[:, 3] = NEG_INF
    hyps, gaps = prefix_beam_search(lp, 4, cand=2)
    assert gaps['cand'] > 0
    assert all(np.isfinite(s) for _, s in hyps) and all(3 not in h for h, _ in hyps)
    allowed = [set(sorted(range(1, 7), key=lambda c: (-lp[t, c], c))[:2]) for t in range(6)]
    for h, _ in hyps:                            # a token can only have entered at a frame that allowed it
        assert all(any(c in a for a in allowed) for c in h)
    assert prefix_beam_search(np.zeros((0, 5)), 4)[0] == [([], 0.0)]


def test_ctc_beam_search_is_exported():
    from src import hipabi
    import ctypes
    for name in ('asr_ctc_beam_search', 'asr_ctc_beam_search_workspace_bytes'):
        assert name in hipabi.exported_symbols()
        assert hasattr(ctypes.CDLL(hipabi.LIB_PATH), name)
