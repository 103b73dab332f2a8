"""The yardstick of CTC forced alignment: a numpy restatement of the Viterbi recursion that csrc/ctc_align.hip runs on the
device (asr_ctc_align), checked here against exhaustive enumeration of every frame path that collapses to the target.
tests/test_hip_ctc_align.py imports `viterbi_align` and the input recipe from this file; nothing here imports the code under
test except the export check at the end.

Lattice (blank = 0): l' = (0, y1, 0, ..., yL, 0), S = 2L+1 states.
  d[t][s] = lp[t][l'_s] + max(d[t-1][s], d[t-1][s-1], d[t-1][s-2])      (s-2 only when l'_s != 0 and l'_s != l'_{s-2})
from d[0][0], d[0][1]; the end is the better of d[T-1][S-1], d[T-1][S-2].  Tie rules: among predecessors stay, then s-1, then
s-2 (a candidate replaces the best so far only when strictly greater); at the end S-1 wins a tie; -inf never wins over a finite
value; an end value of -inf means there is no alignment (ok = False)."""
import collections
import itertools

import numpy as np
import pytest

NEG_INF = float('-inf')

Viterbi = collections.namedtuple('Viterbi', 'ok states score gap')


def extended(target):
    ext = [0]
    for y in target:
        ext += [int(y), 0]
    return np.asarray(ext, dtype=np.int64)


def _shift(v, k, fill):
    """out[s] = v[s-k] (k > 0) or v[s+|k|] (k < 0), `fill` where that runs off the lattice."""
    out = np.full_like(v, fill)
    if k > 0:
        out[k:] = v[:-k] if k < len(v) else v[:0]
    else:
        out[:k] = v[-k:] if -k < len(v) else v[:0]
    return out


def viterbi_align(lp, target, dtype=np.float64):
    """lp (T,V) log-probabilities, target: token ids in 1..V-1 -> Viterbi(ok, states, score, gap).  states: the lattice state
    of every frame (None when not ok); score: log-probability of that path (-inf when not ok); gap: score minus the score of
    the second-best path (inf when there is no other path of finite score).  `dtype` is the arithmetic of the recursion:
    float64 is the yardstick, float32 its transcription that sizes the score tolerance."""
    dt = dtype
    lp = np.asarray(lp, dtype=dt)
    T, V = lp.shape
    ext = extended(target)
    S = len(ext)
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (ext[2:] != 0) & (ext[2:] != ext[:-2])
    ninf = dt(NEG_INF)
    emit = lp[:, ext]                                          # (T,S)
    fwd = np.full((T, S), ninf, dtype=dt)
    move = np.zeros((T, S), dtype=np.int64)
    with np.errstate(all='ignore'):
        fwd[0, :2] = emit[0, :2]
        for t in range(1, T):
            prev = fwd[t - 1]
            best = prev.copy()
            b1 = _shift(prev, 1, ninf)
            sel = b1 > best
            best[sel], move[t, sel] = b1[sel], 1
            b2 = np.where(skip, _shift(prev, 2, ninf), ninf)
            sel = b2 > best
            best[sel], move[t, sel] = b2[sel], 2
            fwd[t] = best + emit[t]
        end, score = S - 1, fwd[T - 1, S - 1]
        if S > 1 and fwd[T - 1, S - 2] > score:
            end, score = S - 2, fwd[T - 1, S - 2]
        if not score > ninf:
            return Viterbi(False, None, NEG_INF, float('inf'))
        states = [0] * T
        s = end
        for t in range(T - 1, -1, -1):
            states[t] = s
            s -= int(move[t, s]) if t > 0 else 0
        # second-best path: every other path visits a node off the optimal one, and the best path through node (t,s) scores
        # fwd[t,s] + bwd[t,s] - emit[t,s]
        bwd = np.full((T, S), ninf, dtype=dt)
        bwd[T - 1, max(S - 2, 0):] = emit[T - 1, max(S - 2, 0):]
        skip_from = _shift(skip, -2, False)                    # state s may jump to s+2
        for t in range(T - 2, -1, -1):
            nxt = bwd[t + 1]
            best = np.maximum(nxt, _shift(nxt, -1, ninf))
            best = np.maximum(best, np.where(skip_from, _shift(nxt, -2, ninf), ninf))
            bwd[t] = best + emit[t]
        live = (fwd > ninf) & (bwd > ninf)
        through = np.where(live, fwd + bwd - np.where(live, emit, 0), ninf)
        through[np.arange(T), states] = ninf
        second = through.max() if through.size else ninf
    return Viterbi(True, states, float(score), float(score) - float(second))


def frames_of(states, target):
    """(frame_token, frame_pos) of a state path."""
    ext = extended(target)
    return [int(ext[s]) for s in states], [(s >> 1) if s & 1 else -1 for s in states]


def spans_of(states, L):
    """(tok_start, tok_end), inclusive, of every target token from a state path."""
    start, end = [-1] * L, [-1] * L
    for t, s in enumerate(states):
        if s & 1:
            j = s >> 1
            if start[j] < 0:
                start[j] = t
            end[j] = t
    return start, end


def collapse(frame_token):
    return [c for c, prev in zip(frame_token, [None] + list(frame_token[:-1])) if c != 0 and c != prev]


def random_alignment(rng, T, target):
    """A random frame path of length T that collapses to `target` (T must leave room for the forced blanks)."""
    L = len(target)
    count = [0] * (2 * L + 1)                                   # frames spent in every lattice state
    for j in range(L):
        count[2 * j + 1] = 1
        if j and target[j] == target[j - 1]:
            count[2 * j] = 1
    extra = T - sum(count)
    assert extra >= 0, 'T too short for this target'
    for s in rng.randint(0, 2 * L + 1, size=extra):
        count[s] += 1
    ext = extended(target)
    return [int(ext[s]) for s in range(2 * L + 1) for _ in range(count[s])]


def bumped_logp(seed, T, V, target, scale, bump, with_path=False):
    """log_softmax(scale * randn + bump along a random valid alignment of the target), float64, rounded to the fp32 the
    device reads; with_path: (that, the alignment the bump runs along)."""
    rng = np.random.RandomState(seed)
    x = scale * rng.randn(T, V)
    path = random_alignment(rng, T, target)
    x[np.arange(T), path] += bump
    x = x - x.max(axis=1, keepdims=True)
    lp = (x - np.log(np.exp(x).sum(axis=1, keepdims=True))).astype(np.float32)
    return (lp, path) if with_path else lp


def enumerate_alignments(lp, target):
    """Every one of the V**T frame paths that collapses to `target`, with its log-probability, best first."""
    lp = np.asarray(lp, dtype=np.float64)
    T, V = lp.shape
    target = [int(y) for y in target]
    found = []
    for path in itertools.product(range(V), repeat=T):
        if collapse(path) == target:
            found.append((float(sum(lp[t, c] for t, c in enumerate(path))), list(path)))
    return sorted(found, key=lambda x: -x[0])


def _plain_logp(seed, T, V, scale=2.0):
    x = scale * np.random.RandomState(seed).randn(T, V)
    x = x - x.max(axis=1, keepdims=True)
    return x - np.log(np.exp(x).sum(axis=1, keepdims=True))


# targets: without and with a repeated symbol, the empty one, and (per T) one that fits only without blanks
@pytest.mark.parametrize('V', [3, 4])
@pytest.mark.parametrize('T', [4, 5, 6])
@pytest.mark.parametrize('kind', ['distinct', 'repeat', 'empty', 'full'])
def test_restatement_equals_enumeration(V, T, kind):
    target = {'distinct': [1, 2], 'repeat': [2, 2, 1], 'empty': [],
              'full': [1 + (j % (V - 1)) for j in range(T)]}[kind]
    for seed in range(3):
        lp = _plain_logp(1000 * V + 100 * T + seed, T, V)
        want = enumerate_alignments(lp, target)
        got = viterbi_align(lp, target)
        assert got.ok and len(want) >= 1
        if kind == 'full':
            assert len(want) == 1 and want[0][1] == target and got.gap == float('inf')
        assert frames_of(got.states, target)[0] == want[0][1]
        assert abs(got.score - want[0][0]) < 1e-12
        if len(want) > 1:
            assert abs(got.gap - (want[0][0] - want[1][0])) < 1e-12, (got.gap, want[0][0] - want[1][0])
        h32 = viterbi_align(lp.astype(np.float32), target, dtype=np.float32)
        assert h32.ok and abs(h32.score - got.score) < 1e-4


@pytest.mark.parametrize('V,T,target', [(3, 4, [1, 1, 1]), (4, 5, [1, 2, 2, 2]), (3, 2, [1, 2, 1]), (4, 4, [3, 3, 1, 1])])
def test_infeasible_target(V, T, target):
    lp = _plain_logp(7, T, V)
    assert enumerate_alignments(lp, target) == []
    got = viterbi_align(lp, target)
    assert not got.ok and got.states is None and got.score == NEG_INF


def test_minus_infinity_never_wins_and_can_block_every_path():
    lp = _plain_logp(3, 5, 4)
    lp[2, 0] = NEG_INF                                          # a hole the best path has to avoid
    want = enumerate_alignments(lp, [1, 3])
    got = viterbi_align(lp, [1, 3])
    assert got.ok and np.isfinite(got.score) and frames_of(got.states, [1, 3])[0] == want[0][1]
    assert abs(got.score - want[0][0]) < 1e-12
    lp[3, :] = NEG_INF                                          # a frame no path gets through
    assert not viterbi_align(lp, [1, 3]).ok


def test_tie_rules():
    """Every path scores the same (all entries -2, exact in any float type): the rules alone pick the path.  The end is S-1
    (the trailing blank), and a state is left as late as it can be - 'stay' wins - so the tokens come as early as possible."""
    lp = np.full((5, 4), -2.0)
    got = viterbi_align(lp, [1, 2])
    assert got.ok and got.states == [1, 3, 4, 4, 4] and got.gap == 0.0 and got.score == -10.0
    assert frames_of(got.states, [1, 2]) == ([1, 2, 0, 0, 0], [0, 1, -1, -1, -1])
    got = viterbi_align(lp, [3, 3])                             # s-2 is closed between equal tokens: s-1 twice
    assert got.states == [1, 2, 3, 4, 4]
    got = viterbi_align(np.full((2, 4), -2.0), [1, 2])          # no room for the trailing blank: the end is S-2
    assert got.states == [1, 3]
    got32 = viterbi_align(lp.astype(np.float32), [1, 2], dtype=np.float32)
    assert got32.states == [1, 3, 4, 4, 4]


def test_helpers():
    assert spans_of([0, 1, 1, 2, 3, 4], 2) == ([1, 4], [2, 4])
    assert collapse([0, 1, 1, 0, 1, 2, 2, 0]) == [1, 1, 2]
    rng = np.random.RandomState(0)
    for T, target in ((3, [1, 1]), (9, [2, 2, 3]), (4, []), (5, [1, 2, 3, 4, 1])):
        path = random_alignment(rng, T, target)
        assert len(path) == T and collapse(path) == target


def test_ctc_align_is_exported():
    from src import hipabi
    import ctypes
    for name in ('asr_ctc_align', 'asr_ctc_align_workspace_bytes'):
        assert name in hipabi.exported_symbols()
        assert hasattr(ctypes.CDLL(hipabi.LIB_PATH), name)
