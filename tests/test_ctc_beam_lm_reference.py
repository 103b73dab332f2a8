"""The yardstick of CTC-only decoding with RNN-LM shallow fusion: a plain-Python restatement of the search that the resumable
kernels of csrc/ctc_decode.hip run (asr_ctc_beam_lm_init / _advance / _readout), checked here against exhaustive enumeration
of every alignment.  tests/test_hip_ctc_beam_lm.py imports `prefix_beam_search_lm` from this file; nothing here imports the
code under test except the export check at the end.

A prefix l = l_1..l_n is ranked, at every frame and in the result, by
    score(l) = log P_ctc(l | frames so far) + lm_weight * sum_j log P_lm(l_j | <sos>, l_1..l_{j-1}) + len_bonus * n
log P_ctc = logaddexp(pb, pnb) is what tests/test_ctc_beam_reference.py states (same stay, extend and merge rules; pb and pnb
stay pure CTC); <sos> = 0 is the LM's own convention and lives inside `lm`; <eos> = 1 is an ordinary label.  The LM part is one
additive value per beam entry: a stay inherits it, the extension of slot i by c gets lms_i + lm_weight * lm(l)[c] + len_bonus, an
extension that is a beam member itself keeps the member's value.  The allowed tokens are the `cand` largest CTC log-probs of
the frame (the LM has no say); the K entries with the largest score survive, ties to the smaller (parent slot, token), entries
at -inf never.

A launch of the kernel must stop after the first frame whose survivors include an extension (some slot then needs a new LM
row) and after the last frame: `stops` lists those frame counts."""
import numpy as np
import pytest

from test_ctc_beam_reference import NEG_INF, _lse, enumerate_labellings, peaked_logp, prefix_beam_search


def prefix_beam_search_lm(lp, K, cand, lm, lm_weight, len_bonus, dtype=np.float64):
    """lp (T,V) log-probabilities; lm(prefix tuple) -> (V,) log-probabilities of the next token.  Returns (hyps, gaps, info):
    hyps = [(tokens, fused score, CTC score)] best first, at most K; gaps = the smallest margins of the decisions ('keep' and
    'final' on the fused score, 'cand' on the frame's CTC log-probs); info = {'stops': frame counts after which a launch must
    stop, 'merges': extensions that went into a beam member's entry, 'returns': survivors that had been in the beam before,
    had left it and came back as an extension}.  `dtype` is the arithmetic of the search."""
    dt = dtype
    lp = np.asarray(lp, dtype=dt)
    T, V = lp.shape
    w, bonus = dt(lm_weight), dt(len_bonus)
    beam = [((), dt(0.0), dt(NEG_INF), dt(0.0))]
    keep_gap = cand_gap = float('inf')
    stops, merges, returns, seen = [], 0, 0, {()}
    with np.errstate(all='ignore'):
        for t in range(T):
            row = lp[t]
            order = sorted(range(1, V), key=lambda c: (-row[c], c))
            if 0 < cand < V - 1:
                cand_gap = min(cand_gap, float(row[order[cand - 1]]) - float(row[order[cand]]))
                order = order[:cand]
            members = {pre for pre, _, _, _ in beam}
            entries = {pre: [dt(NEG_INF), dt(NEG_INF), (i, 0), lms] for i, (pre, _, _, lms) in enumerate(beam)}
            for i, (pre, pb, pnb, lms) in enumerate(beam):
                p = _lse(pb, pnb, dt)
                e = pre[-1] if pre else 0
                own = entries[pre]
                own[0] = _lse(own[0], dt(p + row[0]), dt)
                if pre:
                    own[1] = _lse(own[1], dt(pnb + row[e]), dt)
                lm_row = None
                for c in order:
                    ext = pre + (c,)
                    if ext in members:
                        merges += 1
                    elif ext not in entries:
                        if lm_row is None:
                            lm_row = np.asarray(lm(pre), dtype=dt)
                        entries[ext] = [dt(NEG_INF), dt(NEG_INF), (i, c), dt(dt(lms + dt(w * lm_row[c])) + bonus)]
                    ent = entries[ext]
                    ent[1] = _lse(ent[1], dt((pb if c == e else p) + row[c]), dt)
            scored = [(dt(_lse(pb, pnb, dt) + lms), key, pre, pb, pnb, lms) for pre, (pb, pnb, key, lms) in entries.items()]
            scored = sorted((s for s in scored if s[0] > NEG_INF), key=lambda s: (-s[0], s[1]))
            if len(scored) > K:
                keep_gap = min(keep_gap, float(scored[K - 1][0]) - float(scored[K][0]))
            kept = scored[:K]
            extended = [s for s in kept if s[1][1] != 0]
            returns += sum(1 for s in extended if s[2] in seen)
            seen.update(s[2] for s in kept)
            if extended or t == T - 1:
                stops.append(t + 1)
            beam = [(pre, pb, pnb, lms) for _, _, pre, pb, pnb, lms in kept]
    hyps = [(list(pre), float(dt(_lse(pb, pnb, dt) + lms)), float(_lse(pb, pnb, dt))) for pre, pb, pnb, lms in beam]
    final_gap = min([a[1] - b[1] for a, b in zip(hyps, hyps[1:])] + [float('inf')])
    return hyps, {'keep': keep_gap, 'cand': cand_gap, 'final': final_gap}, {'stops': stops, 'merges': merges, 'returns': returns}


def trigram_table(seed, V):
    """Seeded (V,V,V) float64 log_softmax table: [a, b] = distribution after the tokens a, b."""
    x = 2.0 * np.random.RandomState(seed).randn(V, V, V)
    x = x - x.max(axis=2, keepdims=True)
    return x - np.log(np.exp(x).sum(axis=2, keepdims=True))


def table_lm(table):
    """prefix -> the table's row of its last two tokens, <sos> = 0 in front."""
    return lambda pre: table[((0, 0) + tuple(pre))[-2], ((0, 0) + tuple(pre))[-1]]


def lm_term(table, lab, lm_weight, len_bonus):
    ctx, tot = (0, 0), 0.0
    for c in lab:
        tot += table[ctx[0], ctx[1], c]
        ctx = (ctx[1], c)
    return lm_weight * tot + len_bonus * len(lab)


@pytest.mark.parametrize('V,T', [(3, 5), (3, 6), (4, 5)])
def test_unpruned_search_equals_enumeration_plus_lm(V, T):
    lp = peaked_logp(7 * V + T, T, V, 6.0).astype(np.float64)
    table = trigram_table(11 * V + T, V)
    want = enumerate_labellings(lp)
    hyps, _, info = prefix_beam_search_lm(lp, len(want), 0, table_lm(table), 0.7, 0.3)
    assert len(hyps) == len(want)
    assert info['stops'][-1] == T
    for toks, fused, ctc in hyps:
        lab = tuple(toks)
        assert abs(ctc - want[lab]) < 1e-10, (toks, ctc, want[lab])
        assert abs(fused - (want[lab] + lm_term(table, lab, 0.7, 0.3))) < 1e-10, (toks, fused)
    assert [h[1] for h in hyps] == sorted((h[1] for h in hyps), reverse=True)
    best = max(want, key=lambda lab: want[lab] + lm_term(table, lab, 0.7, 0.3))
    assert tuple(hyps[0][0]) == best


@pytest.mark.parametrize('K,cand,V,T,scale', [(4, 0, 31, 24, 3.0), (8, 12, 31, 24, 3.0), (16, 0, 4, 6, 6.0), (1, 0, 31, 20, 60.0)])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_without_lm_weight_it_is_the_plain_search(K, cand, V, T, scale, dtype):
    lp = peaked_logp(1000 + T, T, V, scale)
    table = trigram_table(5, V)
    hyps, gaps, info = prefix_beam_search_lm(lp, K, cand, table_lm(table), 0.0, 0.0, dtype=dtype)
    want, want_gaps = prefix_beam_search(lp, K, cand, dtype=dtype)
    assert [(h, s) for h, s, _ in hyps] == want                 # scores included, exactly
    assert [(h, c) for h, _, c in hyps] == want
    assert gaps == want_gaps
    assert info['stops'][-1] == T and all(a < b for a, b in zip(info['stops'], info['stops'][1:]))


def test_the_lm_changes_the_best_hypothesis():
    """Two frames; CTC alone prefers '1', an LM that all but forbids 1 after <sos> turns the result to '2'."""
    lp = np.log(np.array([[0.2, 0.5, 0.3], [0.6, 0.25, 0.15]]))
    table = np.log(np.full((3, 3, 3), 1.0 / 3))
    table[0, 0] = np.log(np.array([0.05, 0.05, 0.9]))
    plain, _ = prefix_beam_search(lp, 8)
    assert plain[0][0] == [1]
    hyps, _, info = prefix_beam_search_lm(lp, 8, 0, table_lm(table), 1.0, 0.0)
    assert hyps[0][0] == [2]
    ctc = {tuple(h): s for h, s in plain}
    for toks, fused, c in hyps:
        assert abs(c - ctc[tuple(toks)]) < 1e-12
        assert abs(fused - (c + lm_term(table, tuple(toks), 1.0, 0.0))) < 1e-12
    assert info['stops'] == [1, 2]
    # the bonus alone: a longer labelling gains len_bonus per token
    hyps_b, _, _ = prefix_beam_search_lm(lp, 8, 0, table_lm(table), 0.0, 0.5)
    for toks, fused, c in hyps_b:
        assert abs(fused - (c + 0.5 * len(toks))) < 1e-12


def test_merges_returns_and_stops_are_counted():
    """V = 3, K = 2: the beam overflows at once, prefixes leave and come back; a frame of stays only is no stop."""
    lp = peaked_logp(3, 8, 3, 1.5).astype(np.float64)
    _, _, info = prefix_beam_search_lm(lp, 2, 0, table_lm(trigram_table(1, 3)), 0.5, 0.0)
    assert info['merges'] > 0
    assert info['stops'][-1] == 8
    one_hot = peaked_logp(24020, 20, 31, 60.0).astype(np.float64)
    hyps, _, info = prefix_beam_search_lm(one_hot, 1, 0, table_lm(trigram_table(2, 31)), 0.1, 0.0)
    assert len(info['stops']) <= len(hyps[0][0]) + 1            # K = 1: one stop per new token, and the last frame


def test_ctc_beam_lm_is_exported():
    from src import hipabi
    import ctypes
    for name in ('asr_ctc_beam_lm_workspace_bytes', 'asr_ctc_beam_lm_init', 'asr_ctc_beam_lm_advance', 'asr_ctc_beam_lm_readout',
                 'asr_masked_copy_rows'):
        assert name in hipabi.exported_symbols()
        assert hasattr(ctypes.CDLL(hipabi.LIB_PATH), name)
