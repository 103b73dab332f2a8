"""RNNLM(module='GRU') on the host: construction, the reference's parameter layout (nn.GRU under `rnn.`), fixture checkpoints,
the state kind, and the hidden-size rule of asr_gru_rec_fwd / _bwd (1 <= H <= 2048, any H in that range; larger refused)."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ASR_E_ARG, ASR_E_UNSUPPORTED = -1, -3


@pytest.mark.parametrize('n_layers,tying', [(1, True), (2, False), (4, True)])
def test_state_dict_matches_torch_gru(n_layers, tying):
    from src.lm import RNNLM
    lm = RNNLM(31, tying, 16, 'GRU', 16, n_layers, 0.0)
    ref = torch.nn.GRU(16, 16, num_layers=n_layers, batch_first=True)
    want = {'emb.weight': (31, 16)}
    want.update({'rnn.' + k: tuple(v.shape) for k, v in ref.state_dict().items()})
    if not tying:
        want.update({'trans.weight': (31, 16), 'trans.bias': (31,)})
    got = {k: tuple(v.shape) for k, v in lm.state_dict().items()}
    assert got == want
    assert list(got)[:1 + 4 * n_layers] == list(want)[:1 + 4 * n_layers]
    # nn.GRU's initialisation: U(-1/sqrt(dim), 1/sqrt(dim)) (finite, inside the bound, not all zero)
    k = 1.0 / 16 ** 0.5
    for name, p in lm.rnn.named_parameters():
        p = p.detach()
        assert torch.isfinite(p).all() and float(p.abs().max()) <= k and float(p.abs().max()) > 0.5 * k, name


def test_fixture_checkpoints_load_unchanged():
    import yaml
    from src.lm import RNNLM
    paths = sorted(glob.glob(os.path.join(GOLDEN, 'g12_lm_gru_train_*.npz')))
    assert len(paths) == 4
    for p in paths:
        z = np.load(p)
        meta = yaml.safe_load(str(z['meta']))
        lm = RNNLM(meta['V'], meta['emb_tying'], meta['emb_dim'], meta['module'], meta['dim'], meta['n_layers'], meta['dropout'])
        sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('w:')}
        lm.load_state_dict(sd)                              # strict: same names and shapes as the reference's RNNLM
        for k, v in lm.state_dict().items():
            assert torch.equal(v, sd[k]), k


def test_init_state_is_one_tensor():
    from src.lm import RNNLM
    lm = RNNLM(31, True, 16, 'gru', 16, 3, 0.0)
    s = lm.init_state(5, 'cpu')
    assert isinstance(s, torch.Tensor) and s.shape == (3, 5, 16) and float(s.abs().max()) == 0.0
    assert lm.state_rows(torch.arange(30.).view(3, 5, 2), 2).shape == (3, 2, 2)
    h, c = RNNLM(31, True, 16, 'LSTM', 16, 3, 0.0).init_state(5, 'cpu')
    assert h.shape == c.shape == (3, 5, 16)


def test_other_modules_and_sizes_are_refused():
    from src.lm import GRU_MAX_DIM, RNNLM
    assert GRU_MAX_DIM == 2048
    RNNLM(31, False, 2048, 'GRU', 2048, 1, 0.0)
    RNNLM(31, False, 37, 'GRU', 37, 1, 0.0)                # ragged sizes are handled, not refused
    with pytest.raises(NotImplementedError, match='outside'):
        RNNLM(31, False, 2049, 'GRU', 2049, 1, 0.0)
    with pytest.raises(NotImplementedError, match='emb_dim'):
        RNNLM(31, False, 8, 'GRU', 37, 1, 0.0)             # untied with emb_dim != dim: the reference's model fails at its first forward
    with pytest.raises(NotImplementedError):
        RNNLM(31, True, 16, 'RNN', 16, 1, 0.0)
    lm = RNNLM(31, True, 16, 'GRU', 16, 1, 0.0)
    with pytest.raises(NotImplementedError):
        lm(torch.zeros(2, 3, dtype=torch.long), None, hidden=torch.zeros(1, 2, 16))


def test_kernel_refuses_hidden_sizes_above_2048_before_touching_memory():
    """The C ABI's rule, checked on the host: the size test comes before any launch or memory access."""
    from src import hipabi as H
    lib = H.lib()
    bogus = ctypes.c_void_p(16)                              # never dereferenced: the call must return first
    assert lib.asr_gru_rec_fwd(bogus, bogus, bogus, None, 4, 3, 2049, H.BF16, bogus, None, None) == ASR_E_UNSUPPORTED
    assert lib.asr_gru_rec_fwd(bogus, bogus, bogus, None, 4, 3, 0, H.BF16, bogus, None, None) == ASR_E_ARG
    assert lib.asr_gru_rec_fwd(bogus, bogus, bogus, None, 4, 3, 64, 7, bogus, None, None) == ASR_E_ARG
    ws = lib.asr_gru_rec_workspace_bytes(4, 2049)
    assert lib.asr_gru_rec_bwd(bogus, bogus, bogus, None, bogus, 4, 3, 2049, H.F32, bogus, bogus, None, bogus, ws, None) == ASR_E_UNSUPPORTED
    small = lib.asr_gru_rec_workspace_bytes(4, 64) - 4
    assert lib.asr_gru_rec_bwd(bogus, bogus, bogus, None, bogus, 4, 3, 64, H.F32, bogus, bogus, None, bogus, small, None) == ASR_E_ARG
    # transposed W_hh (3H*H floats, padded to 64) + carry (B*H floats)
    assert lib.asr_gru_rec_workspace_bytes(5, 37) == 4 * ((3 * 37 * 37 + 63) // 64 * 64 + 5 * 37)
