"""Float64 restatements of the embedding-regulariser entry points (csrc/emb_fuse.hip), written from the header comments of
include/asr_hip.h, the case tables the GPU tests import (tests/test_hip_emb_fuse.py, tests/test_hip_emb_plugin.py), and the
checks that hold the restatements themselves:

  cos_loss_ref        against torch.nn.functional.cosine_embedding_loss in float64 and its autograd
  fuse_fwd_ref / fuse_bwd_ref   against torch softmax / sigmoid / relu / log in float64 and autograd, d_temp and d_lam_raw in all
                      three lambda / temperature modes
  normalize_fwd_ref / normalize_bwd_ref   against F.normalize in float64 and its autograd (all-zero rows apart: the library
                      gives them a zero gradient, torch dy / 1e-12 - include/asr_hip.h)
  plugin_ref          the whole module from the restatements, against tests/golden/g13_emb_plugin.npz: the reference's own
                      EmbeddingRegularizer in float32 (tests/golden/gen_emb_plugin.py)

CPU only; nothing here needs the library."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

F64 = torch.float64
# ATen's cosine_embedding_loss adds a FLOAT constant 1e-12 to both squared magnitudes, whatever the tensors' type
FUSE_EPS, COS_EPS, NORM_EPS = 1e-8, float(np.float32(1e-12)), 1e-12
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g13_emb_plugin.npz')


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------
# restatements
# ---------------------------------------------------------------------------------------------------------------------
def cos_loss_ref(x, table, label):
    """x (B,L,E), table (V,E), label (B,L) -> loss, dx (B,L,E), dy (B,L,E) [gradient wrt the gathered rows], float64."""
    x, table = x.to(F64), table.to(F64)
    B, L = label.shape
    V = table.shape[0]
    on = (label > 0) & (label < V)
    cnt = on.sum(1, keepdim=True).expand(B, L)
    w = torch.where(on, 1.0 / (B * cnt.clamp(min=1).to(F64)), torch.zeros((), dtype=F64))
    y = table[label.clamp(0, V - 1)]
    pxy, a, b = (x * y).sum(-1), (x * x).sum(-1) + COS_EPS, (y * y).sum(-1) + COS_EPS
    den = torch.sqrt(a * b)
    c = pxy / den
    loss = (w * (1.0 - c)).sum()
    dx = -w[..., None] * (y / den[..., None] - (c / a)[..., None] * x)
    dy = -w[..., None] * (x / den[..., None] - (c / b)[..., None] * y)
    return loss, dx, dy


def _lam(lam_raw, lam_sigmoid):
    return torch.sigmoid(lam_raw) if lam_sigmoid else lam_raw


def _probs(dec, emb, temp_raw, lam_raw, lam_sigmoid):
    a = torch.relu(temp_raw) * emb
    pd = torch.exp(dec - dec.max(-1, keepdim=True).values)
    pd = pd / pd.sum(-1, keepdim=True)
    pe = torch.exp(a - a.max(-1, keepdim=True).values)
    pe = pe / pe.sum(-1, keepdim=True)
    lam = _lam(lam_raw, lam_sigmoid)
    return pd, pe, lam, (1.0 - lam) * pd + lam * pe


def fuse_fwd_ref(dec, emb, temp_raw, lam_raw, lam_sigmoid):
    """dec, emb (N,V); temp_raw, lam_raw (1,) or (V,) -> out (N,V), stats (N,2), argmax (N) (lowest index on a tie), float64."""
    dec, emb, temp_raw, lam_raw = (t.to(F64) for t in (dec, emb, temp_raw, lam_raw))
    pd, pe, lam, f = _probs(dec, emb, temp_raw, lam_raw, lam_sigmoid)
    out = torch.log(f + FUSE_EPS)
    stats = torch.stack([torch.logsumexp(dec, -1), torch.logsumexp(torch.relu(temp_raw) * emb, -1)], -1)
    top = out.max(-1, keepdim=True).values
    V = out.shape[-1]
    amax = torch.where(out == top, torch.arange(V).expand_as(out), torch.full_like(out, V, dtype=torch.int64)).min(-1).values
    return out, stats, amax


def fuse_bwd_ref(dout, dec, emb, temp_raw, lam_raw, lam_sigmoid):
    """-> d_dec, d_emb (N,V), d_temp, d_lam_raw (shaped like the raw parameters), float64."""
    dout, dec, emb, temp_raw, lam_raw = (t.to(F64) for t in (dout, dec, emb, temp_raw, lam_raw))
    pd, pe, lam, f = _probs(dec, emb, temp_raw, lam_raw, lam_sigmoid)
    g = dout / (f + FUSE_EPS)
    dpd, dpe = g * (1.0 - lam), g * lam
    d_dec = pd * (dpd - (dpd * pd).sum(-1, keepdim=True))
    da = pe * (dpe - (dpe * pe).sum(-1, keepdim=True))
    d_emb = da * torch.relu(temp_raw)
    t_terms = da * emb * (temp_raw > 0).to(F64)
    l_terms = g * (pe - pd) * (lam * (1.0 - lam) if lam_sigmoid else torch.ones_like(lam))
    d_temp = t_terms.sum(0) if temp_raw.numel() > 1 else t_terms.sum().reshape(1)
    d_lam = l_terms.sum(0) if lam_raw.numel() > 1 else l_terms.sum().reshape(1)
    return d_dec, d_emb, d_temp, d_lam


def normalize_fwd_ref(x):
    x = x.to(F64)
    return x / torch.sqrt((x * x).sum(-1, keepdim=True)).clamp(min=NORM_EPS)


def normalize_bwd_ref(dy, x):
    dy, x = dy.to(F64), x.to(F64)
    n = torch.sqrt((x * x).sum(-1, keepdim=True))
    den = n.clamp(min=NORM_EPS)
    dot = (dy * x).sum(-1, keepdim=True)
    k2 = torch.where(n >= NORM_EPS, dot / (den * den * n.clamp(min=1e-300)), torch.zeros_like(n))
    dx = dy / den - x * k2
    return torch.where((x == 0).all(-1, keepdim=True), torch.zeros_like(dx), dx)


def plugin_ref(sd, dec_state, dec_logit, label, weight, fuse, fuse_normalize, dout=None):
    """The whole module (reference src/plugin.py:125-160) from the restatements, float64.  sd: the reference's state_dict.
    Returns loss, out, and the gradients of weight * loss + <dout, out> (dout = ones when None) wrt dec_state, dec_logit and
    every trainable parameter, keyed by the state_dict names."""
    P = {k: torch.as_tensor(v).to(F64) for k, v in sd.items()}
    B, L, Dd = dec_state.shape
    x0 = dec_state.to(F64).reshape(B * L, Dd)
    h_pre = x0 @ P['emb_net.0.weight'].T + P['emb_net.0.bias']
    h = torch.relu(h_pre)
    xe = h @ P['emb_net.2.weight'].T + P['emb_net.2.bias']
    table = P['emb_table.weight']
    loss, dxe, _ = cos_loss_ref(xe.view(B, L, -1), table, label)
    dxe = weight * dxe.reshape(B * L, -1)
    out, grads = None, {}
    d_logit = torch.zeros_like(dec_logit, dtype=F64)
    if fuse != 0:
        lam_sig = fuse < 0
        a, b = (normalize_fwd_ref(xe), normalize_fwd_ref(table)) if fuse_normalize else (xe, table)
        emb_logit = a @ b.T
        dl = dec_logit.to(F64).reshape(B * L, -1)
        out, _, _ = fuse_fwd_ref(dl, emb_logit, P['temp'], P['fuse_lambda'], lam_sig)
        do = torch.ones_like(out) if dout is None else dout.to(F64).reshape(out.shape)
        d_dec, d_emb, d_temp, d_lam = fuse_bwd_ref(do, dl, emb_logit, P['temp'], P['fuse_lambda'], lam_sig)
        d_logit = d_dec.view(dec_logit.shape)
        da = d_emb @ b
        dxe = dxe + (normalize_bwd_ref(da, xe) if fuse_normalize else da)
        grads['fuse_lambda'], grads['temp'] = d_lam, d_temp           # meaningful where the parameter is learnable
        out = out.view(dec_logit.shape)
    grads['emb_net.2.weight'] = dxe.T @ h
    grads['emb_net.2.bias'] = dxe.sum(0)
    dh = (dxe @ P['emb_net.2.weight']) * (h_pre > 0).to(F64)
    grads['emb_net.0.weight'] = dh.T @ x0
    grads['emb_net.0.bias'] = dh.sum(0)
    grads['dec_state'] = (dh @ P['emb_net.0.weight']).view(B, L, Dd)
    grads['dec_logit'] = d_logit
    return loss, out, grads


# ---------------------------------------------------------------------------------------------------------------------
# case tables (imported by the GPU tests)
# ---------------------------------------------------------------------------------------------------------------------
# (N, V, row stride of dec_logit - V, magnitude of both logit matrices, raw temp, lambda, per-token strides, sigmoid inside)
# V: 2 and 31 inside one sweep of a wave, 64 / 65 at the sweep edge, 2048 / 2049 at the edge between the wave-per-row and the
# workgroup-per-row kernel, 65 536 the largest vocabulary (N = 1).  N: 1, 3 (part of a four-row workgroup), 65 (17 workgroups).
FUSE_CASES = [
    dict(N=1, V=2, pad=0, mag=1.0, temp=2.0, lam=0.3, vec=False, sig=False),
    dict(N=3, V=31, pad=0, mag=1.0, temp=2.0, lam=0.3, vec=False, sig=False),
    dict(N=65, V=31, pad=7, mag=1.0, temp=2.0, lam=0.3, vec=True, sig=True),
    dict(N=3, V=31, pad=0, mag=1.0, temp=-1.0, lam=0.3, vec=False, sig=False),
    dict(N=3, V=31, pad=0, mag=1.0, temp=0.0, lam=0.3, vec=True, sig=False),
    dict(N=3, V=31, pad=0, mag=1.0, temp=2.0, lam=0.0, vec=False, sig=False),
    dict(N=3, V=31, pad=0, mag=1.0, temp=2.0, lam=1.0, vec=False, sig=False),
    dict(N=3, V=31, pad=5, mag=80.0, temp=2.0, lam=0.3, vec=False, sig=True),
    dict(N=65, V=64, pad=0, mag=1.0, temp=2.0, lam=0.3, vec=True, sig=True),
    dict(N=65, V=65, pad=3, mag=1.0, temp=2.0, lam=0.3, vec=False, sig=True),
    dict(N=3, V=2048, pad=0, mag=1.0, temp=2.0, lam=0.3, vec=True, sig=True),
    dict(N=3, V=2049, pad=0, mag=1.0, temp=2.0, lam=0.3, vec=True, sig=True),
    dict(N=3, V=2049, pad=9, mag=80.0, temp=2.0, lam=0.3, vec=False, sig=False),
    dict(N=1, V=65536, pad=0, mag=1.0, temp=2.0, lam=0.3, vec=True, sig=True),
]


def fuse_case_id(c):
    return 'N%d-V%d-pad%d-mag%g-t%g-l%g-%s-%s' % (c['N'], c['V'], c['pad'], c['mag'], c['temp'], c['lam'],
                                                    'vec' if c['vec'] else 'scalar', 'sig' if c['sig'] else 'raw')


def fuse_inputs(c):
    """float32 inputs of a case: dec (N,V), emb (N,V), temp_raw, lam_raw (1 or V entries), dout (N,V).  With `sig` the lambda
    entries are raw values whose sigmoid is near c['lam']; per-token temperatures spread around c['temp'] with their sign."""
    g = _gen(1000 + c['N'] * 7 + c['V'])
    N, V = c['N'], c['V']
    dec = torch.randn(N, V, generator=g) * c['mag']
    emb = torch.randn(N, V, generator=g) * c['mag']
    n = V if c['vec'] else 1
    temp = torch.full((n,), float(c['temp'])) + (0.25 * torch.randn(n, generator=g) if c['vec'] and c['temp'] > 0 else 0.0)
    lam = torch.full((n,), float(c['lam']))
    if c['sig']:
        lam = torch.logit(lam.clamp(1e-3, 1 - 1e-3)) + (0.5 * torch.randn(n, generator=g) if c['vec'] else 0.0)
    dout = torch.randn(N, V, generator=g)
    return dec, emb, temp, lam, dout


# (B, L, E, V): E 1 / 7 inside one sweep, 300 = 4 sweeps + 44; the rows hold an all-pad utterance, a zero x row and twice the
# same label (cos_inputs)
COS_CASES = [(3, 5, 1, 11), (3, 5, 7, 11), (3, 5, 300, 40), (2, 67, 7, 11)]


def cos_inputs(B, L, E, V):
    g = _gen(2000 + E + L)
    x = torch.randn(B, L, E, generator=g)
    table = torch.randn(V, E, generator=g)
    table[0] = 0.0
    label = torch.randint(1, V, (B, L), generator=g)
    label[0, 1] = label[0, 0]              # the same token twice: the scatter of dy adds two rows
    label[0, L - 1] = 0
    label[B - 1, :] = 0                    # an utterance without a label
    x[0, 2] = 0.0                          # a zero prediction
    return x, table, label


NORM_CASES = [(4, 1), (4, 7), (5, 300), (67, 7)]


def norm_inputs(N, E):
    g = _gen(3000 + E + N)
    x = torch.randn(N, E, generator=g)
    x[1] = 0.0                             # a zero row (row 0 of the table)
    x[2] = 0.0
    x[2, 0] = 1e-20                        # a row far below the epsilon
    return x, torch.randn(N, E, generator=g)


def load_fixture():
    z = np.load(GOLDEN)
    cases = []
    for c in range(int(z['n_cases'])):
        pre = 'c%d_' % c
        cases.append({'fuse': float(z[pre + 'fuse']), 'temperature': float(z[pre + 'temperature']),
                      'fuse_normalize': bool(z[pre + 'fuse_normalize']),
                      'sd': {k[len(pre) + 3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre + 'sd_')},
                      'loss': torch.from_numpy(z[pre + 'loss']), 'out': torch.from_numpy(z[pre + 'out']),
                      'grads': {k[len(pre) + 2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre + 'g_')}})
    shared = {k: torch.from_numpy(z[k]) for k in ('dec_state', 'dec_logit', 'label', 'vectors')}
    shared['weight'] = float(z['weight'])
    return shared, cases


def fixture_case_id(c):
    return 'fuse%g-temp%g-%s' % (c['fuse'], c['temperature'], 'norm' if c['fuse_normalize'] else 'plain')


# ---------------------------------------------------------------------------------------------------------------------
# the restatements against torch in float64
# ---------------------------------------------------------------------------------------------------------------------
def _close(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max())


@pytest.mark.parametrize('B,L,E,V', COS_CASES)
def test_cos_loss_restatement_is_torch(B, L, E, V):
    x, table, label = cos_inputs(B, L, E, V)
    loss, dx, dy = cos_loss_ref(x, table, label)
    xt = x.double().requires_grad_(True)
    yt = table.double()[label].requires_grad_(True)
    per = F.cosine_embedding_loss(xt.view(-1, E), yt.view(-1, E), torch.ones(1, dtype=F64), reduction='none').view(B, L)
    per = torch.where(label != 0, per, torch.zeros_like(per))
    cnt = (label != 0).sum(-1)
    keep = cnt > 0                          # the reference divides 0 by 0 for the empty utterance; the library counts it as 0
    want = (per.sum(-1)[keep] / cnt[keep].double()).sum() / B
    want.backward()
    _close(loss, want.detach())
    # the zero x row has gradients of 1e6: judged on their own scale
    _close(dx, xt.grad, 1e-10)
    _close(dy, yt.grad, 1e-10)
    assert float(dx[B - 1].abs().max()) == 0.0 and float(dy[B - 1].abs().max()) == 0.0
    assert float(dx[0, L - 1].abs().max()) == 0.0


MODES = [('const', False, False), ('scalar', False, True), ('vector', True, True)]


@pytest.mark.parametrize('mode,vec,sig', MODES)
@pytest.mark.parametrize('temp', [2.0, 0.0, -1.0])
def test_fuse_restatement_is_torch(mode, vec, sig, temp):
    c = dict(N=5, V=13, pad=0, mag=3.0, temp=temp, lam=0.3, vec=vec, sig=sig)
    dec, emb, t_raw, l_raw, dout = fuse_inputs(c)
    if vec:
        t_raw[4] = -0.5
    d, e, t, l = (v.double().requires_grad_(True) for v in (dec, emb, t_raw, l_raw))
    lam = torch.sigmoid(l) if sig else l
    fused = (1 - lam) * d.softmax(-1) + lam * (F.relu(t) * e).softmax(-1)
    want = (fused + 1e-8).log()
    (want * dout.double()).sum().backward()
    out, stats, amax = fuse_fwd_ref(dec, emb, t_raw, l_raw, sig)
    _close(out, want.detach())
    _close(stats[:, 0], torch.logsumexp(d.detach(), -1))
    assert torch.equal(amax, want.detach().argmax(-1))
    d_dec, d_emb, d_temp, d_lam = fuse_bwd_ref(dout, dec, emb, t_raw, l_raw, sig)
    _close(d_dec, d.grad)
    _close(d_emb, e.grad)
    _close(d_temp, t.grad)
    _close(d_lam, l.grad)
    if temp <= 0 and not vec:
        assert float(d_temp.abs().max()) == 0.0 and float(d_emb.abs().max()) == 0.0


def test_fuse_restatement_edges():
    dec = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0]])
    emb = torch.tensor([[0.0, 5.0, 5.0, 1.0], [1.0, 1.0, 1.0, 1.0]])
    one = torch.ones(1)
    out, _, amax = fuse_fwd_ref(dec, emb, one, 0.5 * one, False)
    assert amax.tolist() == [1, 0]                                   # the lowest index of an exact tie
    out0, _, _ = fuse_fwd_ref(dec, emb, one, 0.0 * one, False)
    assert torch.equal(out0, torch.log(dec.double().softmax(-1) + 1e-8))
    out1, _, _ = fuse_fwd_ref(dec, emb, one, one, False)
    _close(out1, torch.log(emb.double().softmax(-1) + 1e-8))
    outu, _, _ = fuse_fwd_ref(dec, emb, -one, one, False)           # temp <= 0: uniform p_emb
    _close(outu, torch.full_like(outu, float(np.log(0.25 + 1e-8))))


@pytest.mark.parametrize('N,E', NORM_CASES)
def test_normalize_restatement_is_torch(N, E):
    x, dy = norm_inputs(N, E)
    xt = x.double().requires_grad_(True)
    want = F.normalize(xt, dim=-1)
    (want * dy.double()).sum().backward()
    y = normalize_fwd_ref(x)
    _close(y, want.detach())
    dx = normalize_bwd_ref(dy, x)
    zero = (x == 0).all(-1)
    _close(dx[~zero], xt.grad[~zero], 1e-12)
    assert float(dx[zero].abs().max()) == 0.0 and float(y[zero].abs().max()) == 0.0
    # the row below the epsilon is x / eps with dx = dy / eps
    _close(y[2], x[2].double() / 1e-12)
    _close(dx[2], dy[2].double() / 1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# the whole module against the reference's own output (float32 fixture: its rounding bounds the agreement)
# ---------------------------------------------------------------------------------------------------------------------
_SHARED, _CASES = load_fixture() if os.path.exists(GOLDEN) else (None, [])


def test_fixture_is_present_and_complete():
    assert os.path.exists(GOLDEN), 'tests/golden/gen_emb_plugin.py <reference checkout> writes it'
    assert len(_CASES) == 6
    assert {(c['fuse'], c['temperature'], c['fuse_normalize']) for c in _CASES} == {
        (0.3, 2.0, False), (0.3, 2.0, True), (-1.0, -1.0, False), (-1.0, -1.0, True), (-2.0, -2.0, False), (-2.0, -2.0, True)}
    lab = _SHARED['label']
    assert lab[2].tolist()[1:] == [1, 0, 0, 0] and tuple(lab.shape) == (3, 5)
    assert float(_SHARED['vectors'][0].abs().max()) == 0.0


@pytest.mark.parametrize('case', _CASES, ids=fixture_case_id)
def test_restated_module_matches_the_reference(case):
    """The fixture is float32: a gradient of it carries the float32 rounding of sums of up to B L V = 165 terms whose largest
    is ~ max |g|; 1e-4 of that scale is 100x the expected rounding and far below any wrong term."""
    s = _SHARED
    loss, out, grads = plugin_ref(case['sd'], s['dec_state'], s['dec_logit'], s['label'], s['weight'], case['fuse'],
                                  case['fuse_normalize'])
    _close(loss, case['loss'].double(), 1e-6)
    _close(out, case['out'].double(), 1e-5)
    assert set(case['grads']) <= set(grads), sorted(set(case['grads']) - set(grads))
    for k, want in case['grads'].items():
        got = grads[k].reshape(want.shape)
        scale = max(1.0, float(want.abs().max()))
        err = float((got - want.double()).abs().max())
        assert err <= 1e-4 * scale, (k, err, scale)


# ---------------------------------------------------------------------------------------------------------------------
# the vector file reader
# ---------------------------------------------------------------------------------------------------------------------
def test_load_embedding_reads_the_fasttext_text_format(tmp_path):
    """`count E` header; `</s>` is <eos>; unknown tokens are averaged into <unk>; a token without a line keeps zeros; the later of
    two lines wins; a line that begins with a blank is the blank symbol's vector (character vocabularies)."""
    from src.text import CharacterTextEncoder, WordTextEncoder
    from src.util import load_embedding
    path = tmp_path / 'vec.txt'
    path.write_text('6 2\nTHE 1 2\n</s> 3 4\nDOG 5 6\nBIRD 7 10\nCAT 0.5 -1.5\nCAT 9 8\n\n')
    w = WordTextEncoder(['THE', 'CAT', 'SAT'])                    # ids: <pad> 0 <eos> 1 <unk> 2 THE 3 CAT 4 SAT 5
    e = load_embedding(w, str(path))
    assert e.shape == (6, 2) and e.dtype == np.float64
    assert e.tolist() == [[0, 0], [3, 4], [6, 8], [1, 2], [9, 8], [0, 0]]
    path.write_text('3 3\nA 1 2 3\n  4 5 6\n</s> 7 8 9\n')
    c = CharacterTextEncoder([' ', 'A'])                          # ' ' 3, 'A' 4
    assert load_embedding(c, str(path)).tolist() == [[0, 0, 0], [7, 8, 9], [0, 0, 0], [4, 5, 6], [1, 2, 3]]
