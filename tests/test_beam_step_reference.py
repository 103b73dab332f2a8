"""The yardstick of the attention beam search's bookkeeping kernels (csrc/beam_step.hip, csrc/ctc_prefix.hip,
csrc/decode.hip): a plain numpy restatement of
asr_beam_candidates, asr_ctc_prefix_{init,score}[_batched], asr_beam_step, asr_sample_tokens, asr_lstm_cell and
asr_gather_rows, with its own checks.  tests/test_hip_beam_step.py imports the restatement, the cases and their generator
from this file; nothing here imports the code under test except the export check at the end.

Every function takes the arithmetic as `dtype`: float64 is the yardstick, float32 its transcription, which sizes the
tolerances of the GPU file.  beam_step is written from the rules of the reference (src/decode.py:104-177, 214-263 as
restated in oracle/decode_oracle.py::beam_search), not from the kernel's loops:
  fused score  (1-w) att + w (psi - ctc_prob) with LOG_ZERO for non-candidates and for token 0, + lm_w lm;
  per live hypothesis the `beam` best tokens, LOWER TOKEN FIRST among equals (the kernel's stated rule; torch.topk leaves
  it open), fewer when fewer than `beam` tokens are above -inf;
  token 1 (<eos>) among them ends the hypothesis when att[1] > eos_threshold * max(att[2:]); it joins the finals only
  when t >= min_len; with beam 1 the first final ends the utterance;
  the children are pruned to the `beam` best by sum/len in stable order (earlier parent, then earlier pick, first);
  the finals are the `beam` best by average in stable order, a new entry behind equal ones;
  when t + 1 reaches max_len the surviving rows join the finals in their order and the utterance is done;
  a done utterance (or t >= max_len) has dead rows: alive, sum, ctc_prob, len, last_token and its token-table column 0,
  parent = the row itself, ctc_index = row * max(C, 1); its finals are not touched.

Pins: the replay of oracle/decode_oracle.py::beam_search (itself pinned to the genuine reference by test_oracle_golden.py)
through beam_step; beam_candidates against a stable argsort; Philox4x32-10 against the known-answer vectors that
Random123 publishes for it (kat_vectors: zero counter and key, all-ones counter and key, and the digits-of-pi vector),
written here from the published values - numpy's Philox generator is the 4x64 variant and cannot serve; hand-made steps."""
import numpy as np
import pytest

from oracle import decode_oracle as DO

LOG_ZERO = -10000000.0           # src/decode.py:11
NEG_INF = float('-inf')
GAP = 1e-3
INF = float('inf')


# ---- top-k with the lower token first --------------------------------------------------------------------------------
def _top(x, k):
    """(sel, rest): the k largest entries above -inf, descending, ties to the lower index; rest = the best one left."""
    x = np.array(x)
    sel = []
    for _ in range(k):
        j = int(np.argmax(x))                    # the first of equal maxima
        if not x[j] > NEG_INF:
            break
        sel.append(j)
        x[j] = NEG_INF
    rest = int(np.argmax(x))
    return sel, (rest if x[rest] > NEG_INF else None)


def beam_candidates(att, C):
    """att (rows, V) -> (rows, C) int: the C largest per row, descending, ties to the lower token; a row with fewer than
    C entries above -inf is filled up with token 0."""
    att = np.asarray(att)
    out = np.zeros((att.shape[0], C), dtype=np.int64)
    for r in range(att.shape[0]):
        sel, _ = _top(att[r], C)
        out[r, :len(sel)] = sel
    return out


def candidate_gap(att, C):
    """smallest margin between the C-th candidate of a row and the next token."""
    gap = INF
    for row in np.asarray(att, dtype=np.float64):
        s = np.sort(row)[::-1]
        if C < len(s) and s[C] > NEG_INF:
            gap = min(gap, float(s[C - 1] - s[C]))
    return gap


# ---- CTC prefix scorer: oracle/decode_oracle.py in the requested arithmetic -------------------------------------------
def ctc_prefix_init(x, dtype=np.float64):
    return DO.ctc_prefix_init(x, dtype)


def ctc_prefix_cheap(x, plen, last, r_prev, cand, dtype=np.float64):
    """One hypothesis row as the kernels see it: prefix LENGTH and LAST token, candidates (C,) -> (psi (C,), r (C,T,2)).
    Specified for plen <= T.  Every candidate is scored on its own, so a candidate list may name a token twice.
    The reference's aliasing is part of the specification: with no frame left to sweep (plen == T, or T == 1) its psi is
    a view of r[T-1, 0, :], so the <eos> candidate's r[T-1, 0] receives psi[<eos>] (src/ctc.py:85, 107) - and the next
    step of such a hypothesis reads it back."""
    g = [int(last)] * int(plen)
    assert len(g) <= x.shape[0]
    psi, r = [], []
    for c in cand:
        p, rr = DO.ctc_prefix_cheap(x, g, r_prev, [int(c)], dtype)
        psi.append(p[0])
        r.append(rr[0])
    return np.array(psi, dtype=dtype), np.stack(r)


def ctc_prefix_init_batched(x, tlen, rows_per_utt, rows, dtype=np.float64):
    """x (U,Tmax,V) -> r (rows,Tmax,2): row n scores utterance n // rows_per_utt over its tlen frames; log zero behind them."""
    Tmax = x.shape[1]
    r = np.full((rows, Tmax, 2), DO.LOGZERO_CTC, dtype=dtype)
    for n in range(rows):
        u = n // rows_per_utt
        T = min(max(int(tlen[u]), 1), Tmax)
        r[n, :T] = ctc_prefix_init(x[u, :T], dtype)
    return r


def ctc_prefix_score_batched(x, tlen, r_prev, cand, plen, last, rows_per_utt, dtype=np.float64):
    """-> psi (N,C), r (N,C,Tmax,2) with NaN in the frames t >= tlen[utt], which the kernel does not write."""
    N, C = cand.shape
    Tmax = x.shape[1]
    psi = np.zeros((N, C), dtype=dtype)
    r = np.full((N, C, Tmax, 2), np.nan, dtype=dtype)
    for n in range(N):
        u = n // rows_per_utt
        T = min(max(int(tlen[u]), 1), Tmax)
        psi[n], r[n, :, :T] = ctc_prefix_cheap(x[u, :T], plen[n], last[n], r_prev[n, :T], cand[n], dtype)
    return psi, r


# ---- one step of the bookkeeping -----------------------------------------------------------------------------------------
def init_state(U, beam, dtype=np.float64):
    R = U * beam
    st = {'alive': np.zeros(R, dtype=np.int64), 'sum': np.zeros(R, dtype=dtype), 'ctcp': np.zeros(R, dtype=dtype),
          'len': np.zeros(R, dtype=np.int64), 'seq': [[] for _ in range(R)], 'score': [[] for _ in range(R)],
          'done': np.zeros(U, dtype=np.int64), 'finals': [[] for _ in range(U)]}
    st['alive'][::beam] = 1
    return st


def _final_insert(finals, beam, avg, seq, score, info):
    """stable descending insert, the new entry behind equal ones; the best `beam` stay.  finals: [(avg, seq, score)]."""
    pos = sum(1 for f in finals if f[0] >= avg)
    for f in finals[max(pos - 1, 0):pos + 1]:
        info['final'] = min(info['final'], abs(float(f[0]) - float(avg)))
    info['events'].append(('final', len(finals), pos))
    if pos >= beam:
        return
    finals.insert(pos, (avg, list(seq), list(score)))
    del finals[beam:]


def new_info():
    return {'topk': INF, 'pool': INF, 'final': INF, 'eos': INF, 'noncand': False, 'events': [], 'picked': [], 'ties': []}


def beam_step(state, tables, params, dtype=np.float64, sum_dtype=None, info=None):
    """One call of asr_beam_step.  state: init_state()'s layout; tables: 'att' (R,V), 'lm' (R,V) or None, 'psi' / 'cand'
    (R,C) or None; params: beam, t, min_len (U), max_len (U), ctc_w, lm_w, eos_thr, tok_ld.  Returns the state after the
    step plus 'last_token', 'parent', 'ctc_index' (R), 'tok_col' and 'tok_val' (R): the token-table column written.
    `dtype` is the arithmetic of the scores, `sum_dtype` (default: the same) that of the running sum and the averages.
    `info` (new_info()) collects the smallest margin of every kind of decision, the events and the picked tokens."""
    dt = dtype
    sdt = sum_dtype or dtype
    info = new_info() if info is None else info
    beam, t = int(params['beam']), int(params['t'])
    att_all, lm_all, psi_all, cand_all = tables['att'], tables.get('lm'), tables.get('psi'), tables.get('cand')
    C = cand_all.shape[1] if cand_all is not None else 0
    U = len(state['done'])
    R, V = U * beam, att_all.shape[1]
    rows = np.arange(R)
    out = {'alive': np.zeros(R, dtype=np.int64), 'sum': np.zeros(R, dtype=sdt), 'ctcp': np.zeros(R, dtype=dt),
           'len': np.zeros(R, dtype=np.int64), 'seq': [[] for _ in range(R)], 'score': [[] for _ in range(R)],
           'done': np.array(state['done'], dtype=np.int64), 'finals': [list(f) for f in state['finals']],
           'last_token': np.zeros(R, dtype=np.int64), 'parent': rows.copy(), 'ctc_index': rows * max(C, 1),
           'tok_col': min(t + 1, int(params['tok_ld']) - 1), 'tok_val': np.zeros(R, dtype=np.int64)}
    for u in range(U):
        r0 = u * beam
        finals = out['finals'][u]
        if state['done'][u] or t >= params['max_len'][u]:
            out['done'][u] = 1
            continue
        pool, stop = [], False
        for i in range(beam):
            row = r0 + i
            if not state['alive'][row]:
                continue
            att = np.asarray(att_all[row], dtype=dt)
            cur = att.copy()
            cand = None
            if cand_all is not None:
                cand = [int(c) for c in cand_all[row]]
                hack = np.full(V, LOG_ZERO, dtype=dt)
                for j, ch in enumerate(cand):
                    hack[ch] = dt(psi_all[row, j]) - dt(state['ctcp'][row])
                cur = dt(1 - params['ctc_w']) * cur + dt(params['ctc_w']) * hack
                cur[0] = LOG_ZERO
            if lm_all is not None:
                cur = cur + dt(params['lm_w']) * np.asarray(lm_all[row], dtype=dt)
            sel, rest = _top(cur, beam)
            if rest is not None and sel:
                info['topk'] = min(info['topk'], float(cur[sel[-1]]) - float(cur[rest]))
            for va, vb in zip(sel, sel[1:] + ([rest] if rest is not None else [])):
                if cur[va] == cur[vb]:
                    info['ties'].append((va, vb))
            sum_i, len_i = sdt(state['sum'][row]), int(state['len'][row])
            term = None
            for v in sel:
                info['picked'].append(v)
                if cand is not None and (v == 0 or v not in cand):
                    info['noncand'] = True
                if v == 1:
                    mx = att[2:].max() if V > 2 else dt(NEG_INF)
                    rhs = dt(params['eos_thr']) * mx
                    info['eos'] = min(info['eos'], abs(float(att[1]) - float(rhs)))
                    if att[1] > rhs:
                        term = cur[1]
                        continue
                ci, cp = 0, dt(0)
                if cand is not None and v in cand:
                    ci = cand.index(v)
                    cp = dt(psi_all[row, ci])
                s = sum_i + sdt(cur[v])
                pool.append({'par': i, 'tok': v, 'topv': cur[v], 'sum': s, 'avg': s / sdt(len_i + 1), 'ci': ci, 'cp': cp})
            if term is not None:
                info['events'].append(('term', u, t >= params['min_len'][u]))
                if t >= params['min_len'][u]:
                    s = sum_i + sdt(term)
                    _final_insert(finals, beam, s / sdt(len_i + 1), state['seq'][row] + [1], state['score'][row] + [term], info)
                    if beam == 1:
                        stop = True
                        break
        if stop:
            out['done'][u] = 1
            continue
        order = sorted(range(len(pool)), key=lambda e: -pool[e]['avg'])                  # stable
        for a, b in zip(order[:beam], order[1:beam + 1]):
            info['pool'] = min(info['pool'], float(pool[a]['avg']) - float(pool[b]['avg']))
        kept = order[:beam]
        info['events'].append(('kept', u, len(kept), int(state['alive'][r0:r0 + beam].sum())))
        for rk, e in enumerate(kept):
            ent = pool[e]
            src, dst = r0 + ent['par'], r0 + rk
            out['alive'][dst], out['sum'][dst], out['ctcp'][dst] = 1, ent['sum'], ent['cp']
            out['len'][dst] = state['len'][src] + 1
            out['seq'][dst] = state['seq'][src] + [ent['tok']]
            out['score'][dst] = state['score'][src] + [ent['topv']]
            out['last_token'][dst] = out['tok_val'][dst] = ent['tok']
            out['parent'][dst], out['ctc_index'][dst] = src, src * max(C, 1) + ent['ci']
        if not kept:
            out['done'][u] = 1
            continue
        if t + 1 >= params['max_len'][u]:
            for rk in range(len(kept)):
                dst = r0 + rk
                _final_insert(finals, beam, out['sum'][dst] / sdt(out['len'][dst]), out['seq'][dst], out['score'][dst], info)
            out['done'][u] = 1
    return out


# ---- sampler -----------------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11): counter (4 x uint32), key (2 x uint32) -> 4 x uint32."""
    c0, c1, c2, c3 = [int(c) & 0xffffffff for c in ctr]
    k0, k1 = [int(k) & 0xffffffff for k in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xffffffff, (p0 >> 32) ^ c3 ^ k1, p0 & 0xffffffff
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return c0, c1, c2, c3


def sample_uniform(row, seed):
    r0 = philox4x32_10((row, 0, 0x53414d50, 0), (seed & 0xffffffff, seed >> 32))[0]
    return ((r0 >> 8) + 0.5) / 16777216.0


def sample_tokens(logits, seed, dtype=np.float64):
    """logits (rows, V) -> (pick (rows,), margin (rows,)): inverse CDF over exp(x - max) in token order at the uniform of
    (seed, row); margin = distance of the target to the nearer of the two cumulative sums that bracket it, as a fraction
    of the whole sum."""
    logits = np.asarray(logits, dtype=dtype)
    rows, V = logits.shape
    pick, margin = np.zeros(rows, dtype=np.int64), np.zeros(rows)
    for r in range(rows):
        e = np.exp(logits[r] - logits[r].max())
        cum = np.cumsum(e)
        target = dtype(sample_uniform(r, seed)) * cum[-1]
        hit = np.nonzero(cum >= target)[0]
        p = int(hit[0]) if len(hit) else V - 1
        below = cum[p - 1] if p > 0 else dtype(0)
        pick[r], margin[r] = p, float(min(target - below, cum[p] - target) / cum[-1])
    return pick, margin


def sample_bracket_threshold(V):
    """Below this margin an fp32 sampler may pick the neighbouring token.  The kernel's whole sum and each of its running
    sums pass through at most V/64 + 6 fp32 additions per value (64-lane strides, a 6-stage scan or butterfly) on
    exponentials that are 2 ulp off at the most, so each is within (V/64 + 8) 2^-24 of the sum; the comparison sees both."""
    return (V / 64.0 + 8.0) * 2.0 ** -23


# ---- the two one-liners ------------------------------------------------------------------------------------------------
def lstm_cell(pre, bih, bhh, c_prev, dtype=np.float64):
    """gate sums (N,4D) in the order i, f, g, o -> (h, c)."""
    sig = lambda z: 1 / (1 + np.exp(-z))
    i, f, g, o = np.split(np.asarray(pre, dtype) + np.asarray(bih, dtype) + np.asarray(bhh, dtype), 4, axis=1)
    c = sig(f) * (0 if c_prev is None else np.asarray(c_prev, dtype)) + sig(i) * np.tanh(g)
    return sig(o) * np.tanh(c), c


def gather_rows(src, idx):
    return src[np.clip(idx, 0, src.shape[0] - 1)]


# ---- cases of the step kernel: committed seeds, generator, conditions ---------------------------------------------------
def log_softmax32(x):
    x = x - x.max(axis=-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)


# name -> V, beam, mode, C, min_len / max_len per utterance, seed, and options:
#   p_eos: share of rows whose <eos> logit is raised (terminations);  hi: tokens 2..63 are pushed down, so that the winners
#   sit in the lanes' k >= 1 registers;  done0: utterance 0 is done before the first step and holds one final already;
#   scale: of the logits, where it is not SCALE;  tie: attention-only dyadic log-probs -k/4 (exact in fp32, ties everywhere);  want: what the case must exercise.
# CTC cases use C >= beam + 2, not int(1.5 beam), where the latter is smaller: a top-`beam` of candidates other than token 0
# needs that many (non-candidates sit near w LOG_ZERO, where fp32 cannot tell scores apart).
def _c(V, beam, mode, C, min_len, max_len, seed, **opt):
    return dict(V=V, beam=beam, mode=mode, C=C, min_len=list(min_len), max_len=list(max_len), seed=seed, opt=opt)


CASES = {
    'v3_b2_att': _c(3, 2, 'att', 0, [0], [5], 0, p_eos=0.3),
    'v3_b8_att_few_alive': _c(3, 8, 'att', 0, [0], [4], 0, want=['kept_lt_beam']),
    'v31_b5_ctc': _c(31, 5, 'ctc', 8, [1], [6], 0, p_eos=0.3),
    'v31_b2_ctc_lm': _c(31, 2, 'ctc_lm', 4, [0], [6], 0, p_eos=0.2),
    'v64_b8_lm': _c(64, 8, 'lm', 0, [0], [5], 0, p_eos=0.2),
    'v65_b8_att': _c(65, 8, 'att', 0, [0], [5], 0, hi=True, want=['k1']),
    'v129_b5_ctc_lm': _c(129, 5, 'ctc_lm', 8, [2], [6], 0, hi=True, p_eos=0.3, want=['k1']),
    'v300_b16_att_finals_full': _c(300, 16, 'att', 0, [0], [4], 1, hi=True, p_eos=0.6, scale=6.0, want=['k1', 'fin_full', 'multi_term']),
    'v300_b16_ctc_lm': _c(300, 16, 'ctc_lm', 24, [1], [5], 13, hi=True, p_eos=0.3, want=['k1']),
    'v2047_b8_ctc': _c(2047, 8, 'ctc', 12, [0], [4], 1, p_eos=0.3, want=['k1']),
    'v2048_b16_lm': _c(2048, 16, 'lm', 0, [0], [4], 1, p_eos=0.3, want=['k1', 'multi_term']),
    'v2048_b2_att': _c(2048, 2, 'att', 0, [0], [6], 0, want=['k1']),
    'ragged_u3_b4_ctc_lm': _c(31, 4, 'ctc_lm', 6, [0, 2, 1], [4, 7, 3], 0, p_eos=0.3, done0=True, want=['early_term']),
    'ragged_u3_b8_att_v300': _c(300, 8, 'att', 0, [0, 0, 3], [5, 2, 6], 1, hi=True, p_eos=0.4, done0=True, want=['k1', 'multi_term']),
    'b1_stop_att': _c(31, 1, 'att', 0, [0], [8], 0, p_eos=0.4, want=['b1_stop']),
    'b1_stop_ctc': _c(31, 1, 'ctc', 3, [1], [8], 0, p_eos=0.4, want=['b1_stop']),
    'b1_runs_out_lm': _c(65, 1, 'lm', 0, [0], [4], 0, want=['b1_flush']),
    'min_len_b5_att': _c(31, 5, 'att', 0, [3], [5], 1, p_eos=0.5, want=['early_term', 'multi_term']),
    'tie_v130_b4': _c(130, 4, 'att', 0, [0], [5], 0, tie=True),
    'tie_v300_b8': _c(300, 8, 'att', 0, [1], [5], 0, tie=True),
    'tie_v2048_b16': _c(2048, 16, 'att', 0, [0], [4], 0, tie=True),
}
SCALE, CTC_W, LM_W, EOS_THR = 3.0, np.float32(0.3), np.float32(0.5), np.float32(1.5)     # the weights as the fp32 the device reads


def case_dims(name):
    c = CASES[name]
    U = len(c['max_len'])
    Lmax = max(c['max_len'])
    return U, U * c['beam'], Lmax, Lmax + 1          # U, R, Lmax, tok_ld


def case_tables(name, t, seed=None):
    """The tables of step t: they depend on (seed, t) alone, not on the hypotheses."""
    c = CASES[name]
    U, R, _, _ = case_dims(name)
    V, opt = c['V'], c['opt']
    rng = np.random.RandomState(100003 * (c['seed'] if seed is None else seed) + 17 * t + V)
    if opt.get('tie'):
        att = -rng.randint(2, 7, size=(R, V)) / 4.0
        for r in range(0, R, 2):                      # every other row: its best value on the tokens of ONE lane
            att[r, rng.randint(2, 64)::64] = -0.25
        return {'att': att.astype(np.float32), 'lm': None, 'psi': None, 'cand': None}
    scale = opt.get('scale', SCALE)
    x = scale * rng.randn(R, V)
    if opt.get('hi') and V > 64:
        x[:, 2:64] -= 4 * scale
    x[rng.rand(R) < opt.get('p_eos', 0.0), 1] += 4 * scale
    tab = {'att': log_softmax32(x), 'lm': None, 'psi': None, 'cand': None}
    if 'lm' in c['mode']:
        tab['lm'] = log_softmax32(SCALE * rng.randn(R, V))
    if 'ctc' in c['mode']:
        tab['cand'] = beam_candidates(tab['att'], c['C'])
        tab['psi'] = (-2.0 * (t + 1) + 2.0 * rng.randn(R, c['C'])).astype(np.float32)
    return tab


def case_params(name, t):
    c = CASES[name]
    return {'beam': c['beam'], 't': t, 'min_len': c['min_len'], 'max_len': c['max_len'], 'ctc_w': CTC_W if 'ctc' in c['mode'] else 0.0,
            'lm_w': LM_W if 'lm' in c['mode'] else 0.0, 'eos_thr': EOS_THR, 'tok_ld': case_dims(name)[3]}


DONE0_FINAL = (-0.75, [5, 4, 1], [-0.5, -1.0, -0.75])       # what utterance 0 of a `done0` case holds from the start


def case_state0(name, dtype=np.float64):
    c = CASES[name]
    st = init_state(len(c['max_len']), c['beam'], dtype)
    if c['opt'].get('done0'):
        st['done'][0] = 1
        st['finals'][0] = [(dtype(DONE0_FINAL[0]), list(DONE0_FINAL[1]), [dtype(s) for s in DONE0_FINAL[2]])]
    return st


def run_case(name, dtype=np.float64, seed=None, step=beam_step):
    """The whole drive on the restatement alone -> ([state after step t], info)."""
    info = new_info()
    info['cand'] = INF
    st, outs = case_state0(name, dtype), []
    for t in range(max(CASES[name]['max_len']) + 1):              # one call more: every utterance is done then, all rows die
        tab = case_tables(name, t, seed)
        info['events'].append(('step', t))
        if tab['cand'] is not None:
            info['cand'] = min(info['cand'], candidate_gap(tab['att'], CASES[name]['C']))
        st = step(st, tab, case_params(name, t), dtype, info=info)
        outs.append(st)
    return outs, info


def _multi_term(ev):
    """two or more terminations of one utterance made finals in one step."""
    n, t = {}, None
    for e in ev:
        if e[0] == 'step':
            t = e[1]
        elif e[0] == 'term' and e[2]:
            n[(t, e[1])] = n.get((t, e[1]), 0) + 1
    return any(v >= 2 for v in n.values())


def case_ok(name, seed=None):
    """The conditions a seed must meet, on the float64 restatement alone."""
    c = CASES[name]
    outs, info = run_case(name, np.float64, seed)
    # events: ('step', t); ('term', u, it made a final); ('final', finals held before, position of the new one: >= beam is a
    # rejection); ('kept', u, rows kept, rows alive on entry)
    ev = info['events']
    has = {'k1': any(v >= 64 for v in info['picked']),
           'kept_lt_beam': any(e[0] == 'kept' and 0 < e[2] < c['beam'] and e[3] < c['beam'] for e in ev),
           'fin_full': any(e[0] == 'final' and e[1] == c['beam'] and e[2] >= c['beam'] for e in ev)
           and any(e[0] == 'final' and e[1] == c['beam'] and e[2] < c['beam'] - 1 for e in ev),
           'multi_term': _multi_term(ev),
           'early_term': any(e[0] == 'term' and not e[2] for e in ev),
           'b1_stop': len(outs[-1]['finals'][0]) == 1 and len(outs[-1]['finals'][0][0][1]) < c['max_len'][0]
           and outs[-1]['finals'][0][0][1][-1] == 1,
           'b1_flush': len(outs[-1]['finals'][0]) == 1 and len(outs[-1]['finals'][0][0][1]) == c['max_len'][0]}
    if not all(has[w] for w in c['opt'].get('want', [])):
        return False
    if c['opt'].get('tie'):
        return info['topk'] == 0 and info['pool'] == 0 and info['final'] == 0
    if 'ctc' in c['mode'] and info['noncand']:
        return False
    return min(info['topk'], info['pool'], info['final'], info['eos'], info['cand']) > GAP


@pytest.mark.parametrize('name', sorted(CASES))
def test_committed_seeds_hold_the_conditions(name):
    assert case_ok(name)


def test_tie_cases_hold_ties_in_one_lane_and_across_lanes():
    ties = []
    for name in CASES:
        if CASES[name]['opt'].get('tie'):
            ties += run_case(name)[1]['ties']
    assert any((b - a) % 64 == 0 for a, b in ties)           # v and v + 64k: one lane's registers
    assert any((b - a) % 64 != 0 for a, b in ties)           # different lanes
    assert all(a < b for a, b in ties)                       # the lower token was the one taken


def test_fp32_transcription_decides_alike():
    for name in CASES:
        o64, o32 = run_case(name)[0], run_case(name, np.float32)[0]
        for a, b in zip(o64, o32):
            assert a['seq'] == b['seq'] and [[f[1] for f in u] for u in a['finals']] == [[f[1] for f in u] for u in b['finals']]
            for k in ('alive', 'len', 'parent', 'ctc_index', 'last_token', 'tok_val', 'done'):
                assert (a[k] == b[k]).all(), (name, k)


# ---- pin 1: replay of the reference-pinned oracle ------------------------------------------------------------------------
def _replay(trace, V, beam, min_len, max_len, ctc_w, lm_w):
    """The oracle fuses in fp32 tensors and averages Python floats, so the replay scores in float32 and sums in float64:
    then every score is the oracle's bit for bit."""
    tab = {(t, seq): (att, cand, ctcp, lm) for t, seq, att, cand, ctcp, lm in trace}
    C = len(trace[0][3]) if trace[0][3] is not None else 0
    st = init_state(1, beam, np.float32)
    st['sum'] = st['sum'].astype(np.float64)
    for t in range(max_len):
        tables = {'att': np.zeros((beam, V), np.float32), 'lm': np.zeros((beam, V), np.float32) if lm_w > 0 else None,
                  'psi': np.zeros((beam, C), np.float32) if C else None, 'cand': np.zeros((beam, C), np.int64) if C else None}
        for i in range(beam):
            if st['alive'][i]:
                att, cand, ctcp, lm = tab[(t, tuple(st['seq'][i]))]
                tables['att'][i] = att.numpy()
                if C:
                    tables['cand'][i], tables['psi'][i] = cand, ctcp
                if lm_w > 0:
                    tables['lm'][i] = lm.numpy()[0]
        st = beam_step(st, tables, {'beam': beam, 't': t, 'min_len': [min_len], 'max_len': [max_len], 'ctc_w': ctc_w, 'lm_w': lm_w,
                                    'eos_thr': 1.5, 'tok_ld': max_len + 1}, np.float32, np.float64)
        if st['done'][0]:
            break
    assert st['done'][0]
    return st['finals'][0]


@pytest.mark.parametrize('beam', [4, 1])
@pytest.mark.parametrize('tag,ctc_w,lm_w', [('att', 0.0, 0.0), ('ctc', 0.3, 0.0), ('ctc_lm', 0.3, 0.5)])
def test_replay_of_the_oracle_beam_search(golden_dir, tag, ctc_w, lm_w, beam):
    import torch
    from test_oracle_golden import _decode_setup, load
    meta, z = load(golden_dir, 'g7_decode')
    D, cfg, P, lm = _decode_setup(meta)
    trace = []
    feat_len = torch.from_numpy(z['feat_len'])
    want = D.beam_search(torch.from_numpy(z['feat']), feat_len, P, cfg, beam, meta['min_len_ratio'], meta['max_len_ratio'],
                         ctc_weight=ctc_w, lm=lm if lm_w > 0 else None, lm_weight=lm_w, trace=trace)
    max_len = int(np.ceil(int(feat_len[0]) * meta['max_len_ratio']))
    min_len = int(np.ceil(int(feat_len[0]) * meta['min_len_ratio']))
    got = _replay(trace, int(trace[0][2].shape[0]), beam, min_len, max_len, ctc_w, lm_w)
    assert len(got) == len(want) >= 1
    for (avg, seq, score), (wseq, wscore) in zip(got, want):
        assert seq == wseq
        np.testing.assert_allclose(np.array(score, np.float64), np.array(wscore, np.float64), rtol=1e-14, atol=0)
        assert abs(float(avg) - sum(wscore) / len(wscore)) <= 1e-14 * abs(float(avg))


# ---- pin 2: candidates against a stable argsort ---------------------------------------------------------------------------
@pytest.mark.parametrize('V,C', [(3, 3), (31, 12), (65, 24), (300, 24), (2048, 1), (2048, 24)])
def test_beam_candidates_against_stable_argsort(V, C):
    rng = np.random.RandomState(V + C)
    x = rng.randn(7, V).astype(np.float32)
    x[1] = -rng.randint(1, 4, size=V) / 2.0              # ties
    x[2, rng.rand(V) < 0.5] = NEG_INF
    want = np.argsort(-x.astype(np.float64), axis=1, kind='stable')[:, :C]
    want = np.where(np.take_along_axis(x, want, axis=1) > NEG_INF, want, 0)
    assert (beam_candidates(x, C) == want).all()


# ---- pin 3: Philox4x32-10 known answers -----------------------------------------------------------------------------------
def test_philox_known_answers():
    f = 0xffffffff
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert philox4x32_10((f, f, f, f), (f, f)) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


def test_sampler_brackets_its_target():
    x = np.random.RandomState(0).randn(64, 300) * 3
    pick, margin = sample_tokens(x, 2 ** 32 + 5)
    p = np.exp(x - x.max(axis=1, keepdims=True))
    cum = np.cumsum(p, axis=1) / p.sum(axis=1, keepdims=True)
    for r in range(64):
        u = sample_uniform(r, 2 ** 32 + 5)
        assert 0 < u < 1 and (cum[r, pick[r] - 1] if pick[r] else 0) < u <= cum[r, pick[r]] + 1e-15
        assert margin[r] >= 0
    assert sample_uniform(3, 5) != sample_uniform(3, 2 ** 32 + 5)           # the high key word matters
    assert len(set(pick.tolist())) > 10


# ---- pin 4: hand-made steps ------------------------------------------------------------------------------------------------
def _hand(att, beam=2, t=0, min_len=0, max_len=9, state=None, V=4):
    att = np.array(att, dtype=np.float64)
    st = state or init_state(1, beam)
    info = new_info()
    out = beam_step(st, {'att': att, 'lm': None, 'psi': None, 'cand': None},
                    {'beam': beam, 't': t, 'min_len': [min_len], 'max_len': [max_len], 'ctc_w': 0.0, 'lm_w': 0.0, 'eos_thr': 1.5, 'tok_ld': 10},
                    info=info)
    return out, info


def test_hand_eos_rule_at_its_threshold():
    # max(att[2:]) = -1, threshold 1.5 * -1 = -1.5; <eos> is the best token either way
    dead = [0.0] * 4
    out, _ = _hand([[-9, -1.4999, -1, -2], dead])          # just above: the empty hypothesis ends
    assert out['finals'][0] == [(-1.4999, [1], [-1.4999])]
    assert out['seq'][0] == [2] and out['alive'].tolist() == [1, 0]       # <eos> took a top-2 slot: one child only
    out, _ = _hand([[-9, -1.5, -1, -2], dead])             # at the threshold (not above): <eos> is an ordinary token
    assert out['finals'][0] == [] and out['seq'][:2] == [[2], [1]]
    out, _ = _hand([[-9, -1.5001, -1, -2], dead])          # just below
    assert out['finals'][0] == [] and out['seq'][:2] == [[2], [1]] and out['sum'].tolist() == [-1, -1.5001]


def test_hand_termination_before_min_len():
    out, info = _hand([[-9, -0.5, -1, -2], [0.0] * 4], min_len=1)
    assert ('term', 0, False) in info['events']
    assert out['finals'][0] == [] and out['seq'][0] == [2] and out['alive'].tolist() == [1, 0] and out['done'][0] == 0


def test_hand_two_terminations_in_one_step():
    st = init_state(1, 2)
    st['alive'][:] = 1
    st['len'][:] = 1
    st['seq'], st['score'], st['sum'] = [[2], [3]], [[-1.0], [-2.0]], np.array([-1.0, -2.0])
    out, _ = _hand([[-9, -0.5, -1, -3], [-9, -0.25, -1, -3]], t=1, state=st)
    assert out['finals'][0] == [(-0.75, [2, 1], [-1.0, -0.5]), (-1.125, [3, 1], [-2.0, -0.25])]
    assert out['seq'][:2] == [[2, 2], [3, 2]] and out['parent'].tolist() == [0, 1] and out['done'][0] == 0


def test_hand_last_step_flush_goes_behind_an_equal_average():
    st = init_state(1, 2)
    st['len'][0], st['seq'][0], st['score'][0], st['sum'][0] = 1, [2], [-1.0], -1.0
    st['finals'][0] = [(-1.0, [3, 1], [-1.5, -0.5])]
    out, _ = _hand([[-9, -9, -1, -2], [0.0] * 4], t=1, max_len=2, state=st)          # children: [2,2] avg -1, [2,3] avg -1.5
    assert out['done'][0] == 1
    assert out['finals'][0] == [(-1.0, [3, 1], [-1.5, -0.5]), (-1.0, [2, 2], [-1.0, -1.0])]       # equal: the old one stays ahead; -1.5 is third, dropped


def test_hand_kept_below_beam():
    out, info = _hand([[-1, -9, -2, NEG_INF]] + [[0.0] * 4] * 3, beam=4)
    assert out['alive'].tolist() == [1, 1, 1, 0] and out['seq'][:3] == [[0], [2], [1]]          # three tokens above -inf
    assert out['parent'].tolist() == [0, 0, 0, 3] and out['len'].tolist() == [1, 1, 1, 0] and out['tok_val'].tolist() == [0, 2, 1, 0]


def test_hand_done_utterance_is_left_alone():
    st = init_state(1, 2)
    st['done'][0] = 1
    st['finals'][0] = [(-1.0, [3, 1], [-1.5, -0.5])]
    out, _ = _hand([[-1, -2, -3, -4]] * 2, state=st)
    assert out['alive'].tolist() == [0, 0] and out['parent'].tolist() == [0, 1] and out['finals'][0] == st['finals'][0] and out['done'][0] == 1


def test_hand_ctc_fusion():
    # candidates 2 and 3 with psi - ctc_prob = -1 and -3; w = 0.5: fused 2 -> -1, 3 -> -1.5; tokens 0 and 1 at about LOG_ZERO / 2
    st = init_state(1, 2)
    st['ctcp'][0] = -1.0
    out = beam_step(st, {'att': np.array([[-0.5, -4, -1, 0.0], [0.0] * 4]), 'lm': None, 'psi': np.array([[-2.0, -4.0], [0, 0]]),
                         'cand': np.array([[2, 3], [0, 0]])},
                    {'beam': 2, 't': 0, 'min_len': [0], 'max_len': [9], 'ctc_w': 0.5, 'lm_w': 0.0, 'eos_thr': 1.5, 'tok_ld': 10})
    assert out['seq'][:2] == [[2], [3]] and out['sum'].tolist() == [-1.0, -1.5] and out['ctcp'].tolist() == [-2.0, -4.0]
    assert out['ctc_index'].tolist() == [0, 1]


def test_lstm_cell_and_gather_rows_by_hand():
    h, c = lstm_cell(np.array([[0.0, 30.0, 0.0, 0.0]]), np.zeros(4), np.zeros(4), np.array([[2.0]]))
    assert abs(c[0, 0] - 2.0) < 1e-12 and abs(h[0, 0] - 0.5 * np.tanh(2.0)) < 1e-12           # i*g = 0, f = 1, o = 1/2
    assert gather_rows(np.arange(6).reshape(3, 2), np.array([-4, 2, 2, 7])).tolist() == [[0, 1], [4, 5], [4, 5], [4, 5]]


def test_bookkeeping_kernels_are_exported():
    from src import hipabi
    for name in ('asr_beam_step', 'asr_beam_candidates', 'asr_ctc_prefix_init', 'asr_ctc_prefix_score', 'asr_ctc_prefix_init_batched',
                 'asr_ctc_prefix_score_batched', 'asr_lstm_cell', 'asr_gather_rows', 'asr_sample_tokens'):
        assert name in hipabi.exported_symbols()
