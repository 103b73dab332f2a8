"""The yardstick of the batched encoder pass for models with a front-end (vgg 1..7; src/ragged.py, src/vgg.forward_lens,
asr_ragged_zero_tail), in float64 torch on the CPU.  A conv front-end over a zero-padded batch equals the unpadded pass of
every utterance on its valid frames when (1) the n % time_div frames the unpadded pass drops are masked, (2) the tail of every
convolution's activation is zeroed before the next convolution (or pooling) reads it, (3) the lengths are halved at each time
pooling - and without (2) it does not.  Plus the front-end length chain, eligibility, the export check, and the float64
restatement of front-end + encoder + CTC head (encoder_f64) that tests/test_hip_ragged_frontend.py measures both passes with."""
import ctypes

import pytest
import torch
import torch.nn.functional as tF

D_, V_ = 40, 31
SEED = 0             # test_unmasked_padded_batch_differs asserts that this seed shows the difference; change it there if it does not
LENS_CASES = [(50, 37, 44), (9, 4, 6)]
ENC = {'vgg': 0, 'vgg_freq': -1, 'vgg_low_filt': -1, 'module': 'LSTM', 'bidirection': True, 'dim': [32, 32], 'dropout': [0.0, 0.0],
       'layer_norm': [False, False], 'proj': [True, True], 'sample_rate': [1, 2], 'sample_style': 'drop'}
FREQ = {'vgg_freq': 12, 'vgg_low_filt': 4}

# conv stacks as data: indices of the four convolutions in the nn.Sequential, CNNLayerNorm behind each one or not, ceil-mode
# pooling or not, second pooling over frequency only or not (then time is halved once: time_div 2)
STACKS = {1: ((0, 2, 5, 7), False, True, False), 5: ((0, 3, 7, 10), True, False, False), 3: ((0, 2, 5, 7), False, False, True),
          2: ((0, 2, 5, 7), False, False, False), 4: ((0, 2, 5, 7), False, False, True)}


def enc_cfg(vgg):
    return dict(ENC, vgg=vgg, **(FREQ if vgg in (2, 4) else {}))


def time_div(vgg):
    return None if vgg not in STACKS else (2 if STACKS[vgg][3] else 4)


def seeded_state_dict(shapes, seed, head_scale=1.0):
    """Seeded weights that keep every activation O(1) whatever the fan-in (a conv stack of 128 channels in front of a 2560-wide
    LSTM input would saturate the gates with a fixed 0.3): matrices and filters randn * min(0.3, 1.5 / sqrt(fan_in)), biases
    randn * 0.1, LayerNorm gains 1 + randn * 0.1."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in shapes.items():
        r = torch.randn(shape, generator=g)
        if len(shape) > 1:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            sd[k] = r * min(0.3, 1.5 / fan_in ** 0.5)
        elif k.endswith('ln.weight') or k.endswith('layer_norm.weight'):
            sd[k] = 1.0 + 0.1 * r
        else:
            sd[k] = 0.1 * r
    if 'ctc_layer.0.weight' in sd:
        sd['ctc_layer.0.weight'] = sd['ctc_layer.0.weight'] * head_scale
    return sd


_MODELS = {}


def cpu_model(vgg, module='LSTM'):
    """The project's model on the host (parameters only; nothing runs): its state-dict shapes and its front-end module."""
    from src.asr import ASR
    key = (vgg, module)
    if key not in _MODELS:
        torch.manual_seed(SEED)
        _MODELS[key] = ASR(D_, V_, 1, ctc_weight=1, encoder=dict(enc_cfg(vgg), module=module), prec='fp32')
    return _MODELS[key]


def model_sd(vgg, seed=SEED, head_scale=1.0):
    return seeded_state_dict({k: tuple(v.shape) for k, v in cpu_model(vgg).state_dict().items()}, seed, head_scale)


# ---- float64 restatement of the front-ends ------------------------------------------------------------------------------------
def _zero_tails(x, lens):
    """x (B,C,T,F): exact zeros at t >= lens[b]."""
    x = x.clone()
    for b, n in enumerate(lens):
        x[b, :, n:] = 0
    return x


def conv_stack_f64(sd, pre, spec, x, lens=None):
    """x (B,C,T,F) float64 through conv3x3 [-> LayerNorm over F] -> ReLU, twice, 2 x 2 max pooling, the same again with the
    second pooling 2 x 2 or 1 x 2 (torch.nn.functional, reference src/module.py:582-1001).  lens: the masked padded-batch
    construction - the tail of every activation zeroed at the row's length, the lengths halved with the time axis."""
    idx, has_ln, ceil, freq_only2 = spec
    lens = None if lens is None else list(lens)
    for li, i in enumerate(idx):
        x = tF.conv2d(x, sd['%s%d.weight' % (pre, i)].double(), sd['%s%d.bias' % (pre, i)].double(), padding=1)
        if has_ln:
            x = tF.layer_norm(x, x.shape[-1:], sd['%s%d.layer_norm.weight' % (pre, i + 1)].double(),
                              sd['%s%d.layer_norm.bias' % (pre, i + 1)].double(), 1e-5)
        x = torch.relu(x)
        if lens is not None:
            x = _zero_tails(x, lens)
        if li == 3 and freq_only2:
            x = tF.max_pool2d(x, (1, 2), stride=(1, 2))
        elif li in (1, 3):
            x = tF.max_pool2d(x, 2, stride=2, ceil_mode=ceil)
            lens = None if lens is None else [n // 2 for n in lens]
    return x


def frontend_batch_f64(sd, cfg, x, lens=None):
    """x (B,T,D) float64 -> (B,T',D'): the front-end cfg['vgg'] over the batch as it stands (conv extractors: T a multiple of
    time_div, image (B,C,T,F) with the channels stacked in D, output channel-major).  lens: see conv_stack_f64."""
    vgg, pre = cfg['vgg'], 'encoder.layers.0.'
    if vgg == 6:
        return x[:, ::4]
    if vgg == 7:
        return x @ sd[pre + 'dense.weight'].double().t() + sd[pre + 'dense.bias'].double()
    B, T, D = x.shape
    img = x.reshape(B, T, D // 40, 40).transpose(1, 2)

    def flat(y):
        return y.transpose(1, 2).reshape(B, y.shape[2], y.shape[1] * y.shape[3])
    if vgg in (2, 4):
        f0 = cfg['vgg_freq']
        return torch.cat((flat(conv_stack_f64(sd, pre + 'low_extractor.', STACKS[vgg], img[..., :f0], lens)),
                          flat(conv_stack_f64(sd, pre + 'high_extractor.', STACKS[vgg], img[..., f0:], lens))), dim=-1)
    return flat(conv_stack_f64(sd, pre + 'extractor.', STACKS[vgg], img, lens))


def frontend_out_dim(cfg):
    vgg = cfg['vgg']
    if vgg in (2, 4):
        lo = cfg['vgg_low_filt']
        return cfg['vgg_freq'] // 4 * 2 * lo + (40 - cfg['vgg_freq']) // 4 * (128 - 2 * lo)
    return {1: 2560, 3: 1280, 5: 1280, 6: D_, 7: 256}[vgg]


def frontend_f64(sd, cfg, x):
    """One utterance x (n,D), unpadded -> (out (t',D') float64, enc_len): the conv extractors drop n % time_div trailing frames
    and report n // time_div; vgg 6 keeps every 4th frame and reports n // 4; vgg 7 is one Linear."""
    n, div = x.shape[0], time_div(cfg['vgg'])
    x = x.double()
    with torch.no_grad():
        if div is None:
            return frontend_batch_f64(sd, cfg, x[None])[0], (n // 4 if cfg['vgg'] == 6 else n)
        if n < div:
            return torch.zeros((0, frontend_out_dim(cfg)), dtype=torch.float64), 0
        return frontend_batch_f64(sd, cfg, x[None, :n - n % div])[0], n // div


def encoder_f64(sd, cfg, x, with_ctc=True):
    """x (n,D) -> (enc (T',E), ctc log-probs (T',V) or None, enc_len) in float64: front-end (layer 0 of the encoder when
    cfg['vgg'] != 0), then LSTM -> [LayerNorm] -> time down-sampling -> [tanh(Linear)] per layer (reference
    src/module.py:1040-1081) with the layer keys shifted behind the front-end, head log_softmax(ReLU(Linear))."""
    first = 0 if cfg['vgg'] == 0 else 1
    x, enc_len = (x.double(), x.shape[0]) if first == 0 else frontend_f64(sd, cfg, x)
    x = x.unsqueeze(0)
    with torch.no_grad():
        for l in range(len(cfg['dim'])):
            pre = 'encoder.layers.%d.' % (l + first)
            rnn = torch.nn.LSTM(x.shape[2], cfg['dim'][l], batch_first=True, bidirectional=cfg['bidirection']).double()
            for name, p in rnn.named_parameters():
                p.data.copy_(sd[pre + 'layer.' + name].double())
            x = rnn(x)[0]
            if cfg['layer_norm'][l]:
                x = tF.layer_norm(x, x.shape[-1:], sd[pre + 'ln.weight'].double(), sd[pre + 'ln.bias'].double(), 1e-5)
            r = cfg['sample_rate'][l]
            if r > 1:
                enc_len //= r
                if cfg['sample_style'] == 'drop':
                    x = x[:, ::r]
                else:
                    n = x.shape[1]
                    x = x[:, :n - n % r].reshape(1, n // r, r * x.shape[2])
            if cfg['proj'][l]:
                x = torch.tanh(x @ sd[pre + 'pj.weight'].double().t() + sd[pre + 'pj.bias'].double())
        ctc = None
        if with_ctc:
            ctc = torch.log_softmax(torch.relu(x @ sd['ctc_layer.0.weight'].double().t() + sd['ctc_layer.0.bias'].double()), dim=-1)[0]
    return x[0], ctc, enc_len


# ---- the construction ---------------------------------------------------------------------------------------------------------
def _utterances(lens, seed=SEED):
    g = torch.Generator().manual_seed(seed + 1)
    return [torch.randn(n, D_, generator=g, dtype=torch.float64) for n in lens]


def padded_batch(utts, valid):
    """(B, max(valid), D): row b holds the first valid[b] frames of utterance b, zeros behind them."""
    x = torch.zeros(len(utts), max(valid), D_, dtype=torch.float64)
    for b, (u, n) in enumerate(zip(utts, valid)):
        x[b, :n] = u[:n]
    return x


@pytest.mark.parametrize('lens', LENS_CASES)
@pytest.mark.parametrize('vgg', [1, 2, 3, 4, 5, 6, 7])
def test_masked_padded_batch_equals_the_unpadded_pass(vgg, lens):
    cfg, sd = enc_cfg(vgg), model_sd(vgg)
    utts, div = _utterances(lens), time_div(vgg)
    valid = list(lens) if div is None else [n - n % div for n in lens]
    with torch.no_grad():
        got = frontend_batch_f64(sd, cfg, padded_batch(utts, valid), None if div is None else valid)
    assert got.shape[1] == max(frontend_f64(sd, cfg, u)[0].shape[0] for u in utts)
    for b, u in enumerate(utts):
        want, _ = frontend_f64(sd, cfg, u)
        t = want.shape[0]
        err = float((got[b, :t] - want).abs().max())
        print('vgg %d row %d (n = %d -> %d frames): max |diff| %.3g' % (vgg, b, lens[b], t, err))
        assert t > 0 and err <= 1e-12
        if div is not None:
            assert (got[b, t:] == 0).all()


@pytest.mark.parametrize('vgg', [1, 2, 3, 4, 5])
def test_unmasked_padded_batch_differs(vgg):
    """The same zero-padded batch without the tail zeroing: behind a row's last frame the first convolution leaves
    ReLU(bias + taps that reach back), which the second one reads where the unpadded pass reads zero padding.  The shorter
    rows' last output frame is off by more than 1e-3 - the difference the test above would show if the masks were missing."""
    lens = LENS_CASES[0]
    cfg, sd = enc_cfg(vgg), model_sd(vgg)
    utts, div = _utterances(lens), time_div(vgg)
    valid = [n - n % div for n in lens]
    with torch.no_grad():
        naive = frontend_batch_f64(sd, cfg, padded_batch(utts, valid))
    for b, u in enumerate(utts):
        want, _ = frontend_f64(sd, cfg, u)
        diff = float((naive[b, :want.shape[0]] - want).abs().max())
        print('vgg %d row %d unmasked: max |diff| %.3g' % (vgg, b, diff))
        if valid[b] < max(valid):
            assert diff > 1e-3, 'SEED = %d does not show the difference: choose another' % SEED
        else:
            assert diff <= 1e-12                   # the longest row has no padding behind it


# ---- lengths, eligibility, exports --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vgg', [1, 2, 3, 4, 5, 6, 7])
def test_frontend_lengths_equal_the_unpadded_shapes(vgg):
    from src.ragged import frontend_lengths
    cfg, sd = enc_cfg(vgg), model_sd(vgg)
    ext = cpu_model(vgg).encoder.layers[0]
    for n in range(1, 14):
        out, enc_len = frontend_f64(sd, cfg, torch.zeros(n, D_))
        assert frontend_lengths(ext, n) == (out.shape[0], enc_len), (vgg, n)
        assert out.shape[1] == ext.out_dim


@pytest.mark.parametrize('vgg', [1, 3, 5, 6, 7])
def test_front_ends_are_eligible(vgg):
    from src.ragged import ineligible_reason
    assert ineligible_reason(cpu_model(vgg)) is None
    assert 'GRU' in ineligible_reason(cpu_model(vgg, 'GRU'))


def test_no_front_end_is_still_eligible_and_gru_still_named():
    from src.ragged import ineligible_reason
    assert ineligible_reason(cpu_model(0)) is None
    assert ineligible_reason(cpu_model(0, 'GRU')) == 'GRU encoder layer'


def test_zero_tail_kernel_is_exported():
    from src import hipabi
    assert 'asr_ragged_zero_tail' in hipabi.exported_symbols()
    assert hasattr(ctypes.CDLL(hipabi.LIB_PATH), 'asr_ragged_zero_tail')


def test_front_end_chunk_size_follows_the_byte_budget(monkeypatch):
    """frontend_max_batch: rows whose largest activation fits the budget, at least one, unbounded without a conv extractor;
    the largest activation is the full-resolution fp32 image of init_dim channels on the fp32-operand path."""
    from src import ragged
    from src.vgg import largest_activation_bytes
    m1 = cpu_model(1)
    row = largest_activation_bytes(m1.encoder.layers[0], 48, m1.prec)
    assert row == 48 * 40 * 128 * 4
    assert ragged.frontend_max_batch(m1, 48) == ragged.FRONTEND_ACT_BYTES // row
    monkeypatch.setattr(ragged, 'FRONTEND_ACT_BYTES', 2 * row + 1)
    assert ragged.frontend_max_batch(m1, 48) == 2
    monkeypatch.setattr(ragged, 'FRONTEND_ACT_BYTES', 1)
    assert ragged.frontend_max_batch(m1, 48) == 1
    for vgg in (0, 6, 7):
        assert ragged.frontend_max_batch(cpu_model(vgg), 48) >= 1 << 30
    assert ragged.max_batch(cpu_model(1)) == ragged.max_batch(cpu_model(0))          # the one-argument call keeps working
