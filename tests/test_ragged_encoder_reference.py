"""The yardstick of the length-aware batched encoder pass (src/ragged.py, csrc/ragged.hip), in float64 torch.nn.LSTM on the
CPU: a padded BiLSTM pass whose direction-1 inputs are RIGHT-ALIGNED per row, and whose direction-1 outputs are shifted
back, equals the unpadded pass of every row on every valid frame - and the naive padded pass does not.  Plus the length
chain of the down-sampling layers as a plain function, the grouping helper of --decode-batch, the export check, and the
float64 restatement of the encoder + CTC head (encoder_f64) that tests/test_hip_ragged_encoder.py measures both passes with."""
import ctypes

import pytest
import torch

H_, D_ = 8, 5
SEED = 0            # test_naive_padded_pass_differs asserts that this seed shows the difference; change it there if it does not


def _lstms(seed):
    """A float64 BiLSTM and its two directions as unidirectional LSTMs with the same weights."""
    torch.manual_seed(seed)
    bi = torch.nn.LSTM(D_, H_, batch_first=True, bidirectional=True).double()
    fwd = torch.nn.LSTM(D_, H_, batch_first=True).double()
    rev = torch.nn.LSTM(D_, H_, batch_first=True).double()
    for n in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0'):
        getattr(fwd, n).data.copy_(getattr(bi, n).data)
        getattr(rev, n).data.copy_(getattr(bi, n + '_reverse').data)
    return bi, fwd, rev


def _batch(seed, lens):
    g = torch.Generator().manual_seed(seed + 1)
    T = max(lens)
    x = torch.zeros(len(lens), T, D_, dtype=torch.float64)
    for b, n in enumerate(lens):
        x[b, :n] = torch.randn(n, D_, generator=g, dtype=torch.float64)
    return x


def right_aligned_pass(fwd, rev, x, lens):
    """Padded batch: direction 0 as it is; direction 1 over inputs right-aligned per row (frame t at t + T - n), walked from
    T-1 down from the zero state, its outputs shifted back.  Returns (B,T,2H), zeros past each row's length."""
    B, T, _ = x.shape
    xa = torch.zeros_like(x)
    for b, n in enumerate(lens):
        xa[b, T - n:] = x[b, :n]
    y0 = fwd(x)[0]
    y1a = rev(xa.flip(1))[0].flip(1)
    out = torch.zeros(B, T, 2 * H_, dtype=torch.float64)
    for b, n in enumerate(lens):
        out[b, :n, :H_] = y0[b, :n]
        out[b, :n, H_:] = y1a[b, T - n:]
    return out


@pytest.mark.parametrize('lens', [(7, 4, 1), (5, 5, 5)])
def test_right_aligned_pass_equals_the_unpadded_pass(lens):
    bi, fwd, rev = _lstms(SEED)
    x = _batch(SEED, lens)
    with torch.no_grad():
        got = right_aligned_pass(fwd, rev, x, lens)
        for b, n in enumerate(lens):
            want = bi(x[b:b + 1, :n])[0][0]
            err = float((got[b, :n] - want).abs().max())
            print('row %d (n = %d): max |diff| %.3g' % (b, n, err))
            assert err <= 1e-12
            assert (got[b, n:] == 0).all()


def test_naive_padded_pass_differs():
    """The reverse direction of a zero-padded pass starts inside the padding: on the same inputs the shortest row's last valid
    frame, direction 1, is off by more than 1e-2 - the difference the test above would show if the construction were wrong."""
    lens = (7, 4, 1)
    bi, fwd, rev = _lstms(SEED)
    x = _batch(SEED, lens)
    b = lens.index(min(lens))
    n = lens[b]
    with torch.no_grad():
        naive = bi(x)[0]
        want = bi(x[b:b + 1, :n])[0][0]
        good = right_aligned_pass(fwd, rev, x, lens)
    diff = float((naive[b, n - 1, H_:] - want[n - 1, H_:]).abs().max())
    print('naive padded pass, row %d frame %d direction 1: max |diff| %.3g' % (b, n - 1, diff))
    assert diff > 1e-2, 'SEED = %d does not show the difference: choose another' % SEED
    assert float((good[b, n - 1, H_:] - want[n - 1, H_:]).abs().max()) <= 1e-12


def length_chain(n, rates, style):
    """(tlen, enc_len) of an utterance of n frames: 'drop' keeps ceil(n/r) frames, 'concat' n // r stacked groups; the
    reference's length is n // r per layer either way."""
    tlen = enc_len = n
    for r in rates:
        tlen = -(-tlen // r) if style == 'drop' else tlen // r
        enc_len //= r
    return tlen, enc_len


@pytest.mark.parametrize('rates', [[1, 2], [2, 2]])
@pytest.mark.parametrize('style', ['drop', 'concat'])
def test_length_chain_equals_the_unpadded_shapes(rates, style):
    from src.ragged import ragged_lengths
    for n in range(1, 10):
        x, ref_len = torch.zeros(n, 3), n
        for r in rates:                                  # what the unpadded pass does to the time axis (src/module.py:1059-1076 of the reference)
            if r > 1:
                x = x[::r] if style == 'drop' else x[:x.shape[0] - x.shape[0] % r].reshape(x.shape[0] // r, r * x.shape[1])
                ref_len //= r
        assert length_chain(n, rates, style) == (x.shape[0], ref_len), (n, rates, style)
        assert ragged_lengths(n, rates, style) == (x.shape[0], ref_len), (n, rates, style)


def test_grouping_helper():
    from src.ragged import group_consecutive
    items = list(range(10))
    groups = list(group_consecutive(items, 4))
    assert groups == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]                   # N consecutive items, the last group short
    assert [i for g in groups for i in g] == items                          # order preserved
    assert list(group_consecutive(items, 1)) == [[i] for i in items]
    assert list(group_consecutive(items, 10)) == [items] and list(group_consecutive(items, 16)) == [items]
    assert list(group_consecutive(iter('abcde'), 2)) == [['a', 'b'], ['c', 'd'], ['e']]
    assert list(group_consecutive([], 3)) == []


def test_main_routes_decode_batch_to_the_batched_solver():
    import main
    import bin.align_asr
    import bin.batch_asr
    import bin.test_asr
    parse = main.parser.parse_args
    assert parse(['--config', 'x', '--test']).decode_batch == 1                                     # default: today's path
    assert main.select_solver(parse(['--config', 'x', '--test', '--decode-batch', '1'])) == (bin.test_asr.Solver, 'test')
    assert main.select_solver(parse(['--config', 'x', '--test', '--decode-batch', '4'])) == (bin.batch_asr.Solver, 'test')
    assert main.select_solver(parse(['--config', 'x', '--align', '--decode-batch', '4'])) == (bin.align_asr.Solver, 'test')
    assert issubclass(bin.batch_asr.Solver, bin.test_asr.Solver)
    assert bin.batch_asr.decode_batch_of(parse(['--config', 'x', '--decode-batch', '0'])) == 1


def test_pad_group_pads_to_the_longest_with_zeros():
    from bin.batch_asr import pad_group
    rows = [torch.full((n, 3), float(n)) for n in (4, 1, 6)]
    out, lens = pad_group(rows)
    assert out.shape == (3, 6, 3) and lens.tolist() == [4, 1, 6] and lens.dtype == torch.int64
    for u, r in enumerate(rows):
        assert torch.equal(out[u, :r.shape[0]], r) and not out[u, r.shape[0]:].any()


def test_ragged_kernels_are_exported():
    from src import hipabi
    for name in ('asr_ragged_align', 'asr_ragged_unalign'):
        assert name in hipabi.exported_symbols()
        assert hasattr(ctypes.CDLL(hipabi.LIB_PATH), name)


# ---- float64 restatement of the encoder + CTC head, per utterance and unpadded, from a state dict --------------------------
def encoder_f64(sd, enc_cfg, x, with_ctc=True):
    """x (n,D) -> (enc (T',E), ctc log-probs (T',V) or None) in float64.  `sd`: the ASR's state dict, `enc_cfg`: its
    encoder section (LSTM layers, no front-end).  LSTM -> [LayerNorm] -> time down-sampling -> [tanh(Linear)] per layer
    (reference src/module.py:1040-1081), head log_softmax(ReLU(Linear)) (reference src/asr.py:116-120)."""
    x = x.double().unsqueeze(0)
    nl = len(enc_cfg['dim'])
    with torch.no_grad():
        for l in range(nl):
            pre = 'encoder.layers.%d.' % l
            Hd = enc_cfg['dim'][l]
            rnn = torch.nn.LSTM(x.shape[2], Hd, batch_first=True, bidirectional=enc_cfg['bidirection']).double()
            for name, p in rnn.named_parameters():
                p.data.copy_(sd[pre + 'layer.' + name].double())
            x = rnn(x)[0]
            if enc_cfg['layer_norm'][l]:
                x = torch.nn.functional.layer_norm(x, x.shape[-1:], sd[pre + 'ln.weight'].double(), sd[pre + 'ln.bias'].double(), 1e-5)
            r = enc_cfg['sample_rate'][l]
            if r > 1:
                if enc_cfg['sample_style'] == 'drop':
                    x = x[:, ::r]
                else:
                    n = x.shape[1]
                    x = x[:, :n - n % r].reshape(1, n // r, r * x.shape[2])
            if enc_cfg['proj'][l]:
                x = torch.tanh(x @ sd[pre + 'pj.weight'].double().t() + sd[pre + 'pj.bias'].double())
        ctc = None
        if with_ctc:
            ctc = torch.log_softmax(torch.relu(x @ sd['ctc_layer.0.weight'].double().t() + sd['ctc_layer.0.bias'].double()), dim=-1)[0]
    return x[0], ctc
