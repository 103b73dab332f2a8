#!/usr/bin/env python
"""Writes tests/golden/g13_emb_plugin.npz: the reference's own EmbeddingRegularizer (its src/plugin.py, imported from a read-only
checkout) on the CPU in float32 at B = 3, L = 5, Dd = 8, E = 7, V = 11; the third transcript is <eos> after one token and pad
from there on.  The embedding table is read by the reference's load_embedding from a vector file written here (fastText text
format, no vector for <pad>: row 0 of the table stays zero).

    python tests/golden/gen_emb_plugin.py <path of the reference checkout>      (or ASR_REFERENCE=<path>)

pytorch_pretrained_bert and matplotlib are not needed by the table variant; they are imported through inert stand-ins.
Six cases, (fuse, temperature) = constant (0.3, 2.0), learnable (-1, -1), per-token (-2, -2), each with fuse_normalize off and
on; the learnable parameters are moved off their initial values (some per-token temperatures below zero) so that their
gradients differ.  Stored once: dec_state, dec_logit, label, vectors (the table), weight.  Stored per case c (prefix 'c{c}_'):
fuse, temperature, fuse_normalize, sd_<state_dict key> for every entry of the module's state_dict, loss, out (log_fused_prob)
and g_<name>: the autograd gradient of weight * loss + out.sum() wrt dec_state, dec_logit and every parameter that requires one."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
B, L, DD, E, V = 3, 5, 8, 7, 11
WEIGHT = 0.7
CASES = [(0.3, 2.0, False), (0.3, 2.0, True), (-1, -1, False), (-1, -1, True), (-2, -2, False), (-2, -2, True)]


class Tokens:
    """What load_embedding needs of a text encoder: the words are 't<id>'."""
    token_type, vocab_size, unk_idx = 'word', V, 2

    def encode(self, s):
        return [int(s[1:]), 1]


def reference_plugin(ref):
    for name in ('matplotlib', 'matplotlib.pyplot', 'pytorch_pretrained_bert', 'pytorch_pretrained_bert.modeling'):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.use = lambda *a, **k: None
            m.BertForMaskedLM = m.BertOnlyMLMHead = object
            sys.modules[name] = m
            if '.' in name:
                setattr(sys.modules[name.split('.')[0]], name.split('.')[1], m)
    sys.path.insert(0, ref)
    import src.plugin as P
    assert os.path.abspath(P.__file__).startswith(os.path.abspath(ref)), P.__file__
    return P


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('ASR_REFERENCE')
    if not ref:
        sys.exit(__doc__)
    P = reference_plugin(ref)
    torch.set_num_threads(1)
    g = np.random.Generator(np.random.PCG64(1313))
    vectors = g.standard_normal((V, E)).astype(np.float32)
    vectors[0] = 0.0
    dec_state = g.standard_normal((B, L, DD)).astype(np.float32)
    dec_logit = (2.0 * g.standard_normal((B, L, V))).astype(np.float32)
    label = g.integers(1, V, (B, L)).astype(np.int64)
    label[1, 4] = 0
    label[2, 1:] = [1, 0, 0, 0]
    arrays = {'dec_state': dec_state, 'dec_logit': dec_logit, 'label': label, 'vectors': vectors, 'weight': np.array(WEIGHT),
              'n_cases': np.array(len(CASES))}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'vectors.txt')
        with open(path, 'w') as f:
            f.write('%d %d\n' % (V - 1, E))
            for v in range(1, V):
                f.write('t%d %s\n' % (v, ' '.join(repr(float(x)) for x in vectors[v])))
        for c, (fuse, temp, norm) in enumerate(CASES):
            torch.manual_seed(100 + c)
            m = P.EmbeddingRegularizer(Tokens(), DD, True, path, 'CosEmb', WEIGHT, fuse, temp, fuse_normalize=norm)
            assert np.array_equal(m.emb_table.weight.detach().numpy(), vectors)
            with torch.no_grad():
                for p in m.emb_net.parameters():
                    p.copy_(torch.from_numpy(0.5 * g.standard_normal(tuple(p.shape)).astype(np.float32)))
                if fuse < 0:
                    m.fuse_lambda.copy_(torch.from_numpy(g.standard_normal(tuple(m.fuse_lambda.shape)).astype(np.float32)))
                    t = 1.0 + g.standard_normal(tuple(m.temp.shape)).astype(np.float32)
                    if t.size > 1:
                        t[3] = -0.5
                    m.temp.copy_(torch.from_numpy(np.abs(t) if t.size == 1 else t))
            pre = 'c%d_' % c
            arrays.update({pre + 'fuse': np.array(fuse), pre + 'temperature': np.array(temp), pre + 'fuse_normalize': np.array(norm)})
            for k, v in m.state_dict().items():
                arrays[pre + 'sd_' + k] = v.numpy().copy()
            ds = torch.from_numpy(dec_state).requires_grad_(True)
            dl = torch.from_numpy(dec_logit).requires_grad_(True)
            loss, out = m(ds, dl, torch.from_numpy(label))
            (WEIGHT * loss + out.sum()).backward()
            arrays.update({pre + 'loss': loss.detach().numpy().copy(), pre + 'out': out.detach().numpy().copy(),
                           pre + 'g_dec_state': ds.grad.numpy().copy(), pre + 'g_dec_logit': dl.grad.numpy().copy()})
            for k, p in m.named_parameters():
                if p.requires_grad:
                    arrays[pre + 'g_' + k] = p.grad.numpy().copy()
    path = os.path.join(HERE, 'g13_emb_plugin.npz')
    np.savez_compressed(path, **arrays)
    print('wrote %s (%.1f KB, %d arrays)' % (path, os.path.getsize(path) / 1024.0, len(arrays)))


if __name__ == '__main__':
    main()
