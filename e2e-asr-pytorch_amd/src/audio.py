"""GPU acoustic front-end with the reference's module names (src/audio.py): ExtractAudioFeature (fbank),
Delta, CMVN, Postprocess, Augment (SpecAugment), create_transform, and WaveAugment for the reference's waveform augmenter
(time_aug); SpecAugmentPolicy (augment as a mapping: time warp, several masks, mean or zero fill) has no counterpart there.
Unlike the reference — one utterance at a time on CPU DataLoader workers — these modules take a zero-padded BATCH on the device plus lengths and run
the HIP kernels of csrc/frontend.hip, csrc/specaug_policy.hip and csrc/wave_aug.hip.  Only constant tables (window, DFT basis, mel filterbank, delta
filters, FFT twiddles) are built on the host."""
import math

import numpy as np
import torch
import torch.nn as nn

from src import hipabi as H

SAMPLE_RATE = 16000


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    mel = f / f_sp
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = math.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, mel)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = math.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def create_mel_filterbank(sr, n_fft, n_mels=128, fmin=0.0, fmax=None):
    """Slaney-style, area-normalised triangular filterbank over the 1 + n_fft//2 FFT bins — the table the
    reference builds at src/audio.py:149-156, 491-605 (pinned against its output in tests/golden)."""
    fmax = float(sr) / 2 if fmax is None else fmax
    nb = 1 + n_fft // 2
    fftfreqs = np.linspace(0, float(sr) / 2, nb)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    w = np.zeros((n_mels, nb))
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        w[i] = np.maximum(0, np.minimum(lower, upper))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w.astype(np.float32)


def delta_filters(order, window_size):
    """Delta._create_filters (src/audio.py:73-93): rows = [static, delta, (delta-delta)], zero-padded to equal length."""
    scales = [[1.0]]
    for i in range(1, order + 1):
        prev_off = (len(scales[i - 1]) - 1) // 2
        cur_off = prev_off + window_size
        cur = [0.0] * (len(scales[i - 1]) + 2 * window_size)
        norm = 0.0
        for j in range(-window_size, window_size + 1):
            norm += j * j
            for k in range(-prev_off, prev_off + 1):
                cur[j + k + cur_off] += j * scales[i - 1][k + prev_off]
        scales.append([x / norm for x in cur])
    n = len(scales[-1])
    out = np.zeros((order + 1, n), dtype=np.float32)
    for i, sc in enumerate(scales):
        pad = (n - len(sc)) // 2
        out[i, pad:pad + len(sc)] = sc
    return out


class ExtractAudioFeature(nn.Module):
    """wav (B,N) fp32 on the device + wav_len (B) -> (B,T,num_mel_bins) in [0,1], frame lengths."""

    def __init__(self, mode='fbank', num_mel_bins=80, frame_length=25, frame_shift=10, ref_level_db=20, min_level_db=-100,
                 preemphasis_coeff=0.97, sample_rate=SAMPLE_RATE):
        super().__init__()
        assert mode == 'fbank'
        self.n_fft = 1025
        self.hop = int(frame_shift / 1000 * sample_rate)
        self.win = int(frame_length / 1000 * sample_rate)
        self.nmel, self.ref_db, self.min_db, self.preemph = num_mel_bins, float(ref_level_db), float(min_level_db), float(preemphasis_coeff)
        nb = self.n_fft // 2 + 1
        m = np.arange(self.win, dtype=np.float64) + (self.n_fft - self.win) // 2
        ang = 2.0 * np.pi * np.arange(nb, dtype=np.float64)[:, None] * m[None, :] / self.n_fft
        table = np.concatenate([np.cos(ang), -np.sin(ang)], 0).astype(np.float32)
        self.register_buffer('dft_table', torch.from_numpy(table), persistent=False)
        self.register_buffer('mel_fb', torch.from_numpy(create_mel_filterbank(sample_rate, self.n_fft, num_mel_bins)), persistent=False)
        self.register_buffer('window', torch.hann_window(self.win, periodic=True), persistent=False)

    def forward(self, wav, wav_len):
        wav = wav.contiguous().float()
        wav_len = wav_len.to(wav.device, torch.int64).contiguous()
        B, N = wav.shape
        T = 1 + (N - 1) // self.hop      # torch.stft(center=True) with odd n_fft
        out = torch.empty((B, T, self.nmel), dtype=torch.float32, device=wav.device)
        nbytes = H.lib().asr_fbank_workspace_bytes(B, T, self.win, self.n_fft)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=wav.device)
        H.call('asr_fbank', H.ptr(wav), H.ptr(wav_len), H.ptr(out), H.ptr(self.dft_table), H.ptr(self.mel_fb), H.ptr(self.window),
               B, N, T, self.win, self.hop, self.n_fft, self.nmel, self.preemph, self.ref_db, self.min_db, H.ptr(ws), nbytes,
               H.stream_ptr())
        return out, 1 + (wav_len - 1) // self.hop


class Delta(nn.Module):
    """(B,T,F) + lens -> (B,T,(order+1)*F), channel-major like Postprocess emits it."""

    def __init__(self, order=2, window_size=2):
        super().__init__()
        self.order = order
        self.register_buffer('filters', torch.from_numpy(delta_filters(order, window_size)), persistent=False)

    def forward(self, x, lens):
        x = x.contiguous()
        B, T, F = x.shape
        C, taps = self.filters.shape
        out = torch.empty((B, T, C * F), dtype=torch.float32, device=x.device)
        lens = lens.to(x.device, torch.int64).contiguous()
        H.call('asr_delta_stack', H.ptr(x), H.ptr(lens), H.ptr(out), H.ptr(self.filters), B, T, F, C, taps, H.stream_ptr())
        return out, lens


class CMVN(nn.Module):
    """Per-utterance mean / variance normalisation (src/audio.py:14-37), in place on the padded batch: every column of an
    utterance over its own valid frames, (x - mean) / (eps + unbiased std)."""

    def __init__(self, mode='global', dim=2, eps=1e-10):
        super().__init__()
        if mode != 'global':
            raise NotImplementedError('Only support global mean variance normalization.')
        self.mode, self.dim, self.eps = mode, dim, eps

    def forward(self, x, lens):
        B, T, D = x.shape
        lens = lens.to(x.device, torch.int64).contiguous()
        nbytes = H.lib().asr_cmvn_workspace_bytes(B, D)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
        H.call('asr_cmvn', H.ptr(x), H.ptr(lens), None, B, T, D, self.eps, H.ptr(ws), nbytes, H.stream_ptr())
        return x, lens

    def extra_repr(self):
        return 'mode={}, dim={}, eps={}'.format(self.mode, self.dim, self.eps)


class Postprocess(nn.Module):
    """Kept for name compatibility: the HIP front-end already emits the (T, C*F) layout."""

    def forward(self, x, lens):
        return x, lens


class Augment(nn.Module):
    """SpecAugment (one time mask <= T, one frequency mask <= F, mean fill), in place on the padded batch."""

    def __init__(self, T=40, num_masks=1, replace_with_zero=False, F=27, seed=0):
        super().__init__()
        assert num_masks == 1 and not replace_with_zero
        self.T, self.F, self.seed, self.calls = T, F, seed, 0

    def forward(self, x, lens, draws=None):
        B, T, D = x.shape
        lens = lens.to(x.device, torch.int64).contiguous()
        d_in = None
        if draws is not None:
            d_in = draws.to(x.device, torch.int32).contiguous()
        self.calls += 1
        ws = torch.empty(B * 16 * 2, dtype=torch.float64, device=x.device)          # asr_specaug_workspace_bytes(B)
        H.call('asr_specaug_ws', H.ptr(x), H.ptr(lens), H.ptr(d_in), None, B, T, D, self.T, self.F,
               (self.seed * 1000003 + self.calls) & 0xFFFFFFFFFFFF, H.ptr(ws), ws.numel() * 8, H.stream_ptr())
        return x, lens


POLICY_KEYS = {'time_warp': 0, 'freq_masks': 0, 'freq_width': 27, 'time_masks': 0, 'time_width': 100, 'time_ratio': 1.0,
               'time_count_ratio': 0, 'fill': 'mean'}
POLICY_MAX_FREQ_MASKS, POLICY_MAX_TIME_MASKS, POLICY_RECORD = 8, 32, 82


def parse_policy(cfg):
    """A mapping under data.audio.augment -> the settings asr_specaug_policy takes (seven integers and the fill), as a dict.  Missing keys take the values
    of POLICY_KEYS (an empty mapping is the identity); ratios become per-mille with round(x * 1000).  ValueError names the key."""
    cfg = dict(cfg)
    for k in cfg:
        if k not in POLICY_KEYS:
            raise ValueError('augment: unknown key %r (known: %s)' % (k, ', '.join(POLICY_KEYS)))
    v = dict(POLICY_KEYS, **cfg)
    out = {}
    for k, cap in (('time_warp', None), ('freq_masks', POLICY_MAX_FREQ_MASKS), ('freq_width', None),
                   ('time_masks', POLICY_MAX_TIME_MASKS), ('time_width', None)):
        x = v[k]
        if isinstance(x, bool) or not isinstance(x, int) or x < 0 or x >= 2 ** 31 or (cap is not None and x > cap):
            raise ValueError('augment: %s = %r must be an integer in 0..%s' % (k, x, cap if cap is not None else '2^31 - 1'))
        out[k] = x
    for k in ('time_ratio', 'time_count_ratio'):
        x = v[k]
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not 0.0 <= x <= 1.0:
            raise ValueError('augment: %s = %r must be a number in 0..1' % (k, x))
        out[k + '_pm'] = int(round(x * 1000))
    if v['fill'] not in ('mean', 'zero'):
        raise ValueError("augment: fill = %r must be 'mean' or 'zero'" % (v['fill'],))
    out['fill'] = v['fill']
    return out


class SpecAugmentPolicy(nn.Module):
    """A SpecAugment policy on the padded batch (csrc/specaug_policy.hip): time warp W, freq_masks masks of at most freq_width bins,
    time_masks masks of at most min(time_width, time_ratio * len) frames (their count min(time_masks, time_count_ratio * len) when
    that ratio is > 0), filled with the utterance's mean or with zero.  Out of place - the warp gathers along time: x (B,T,D)
    fp32 + lens -> (out, lens), out a buffer the module keeps between calls.  draws (B,82) int32 = {w0, c, (f0, fend) x 8,
    (t0, tend) x 32} skips the device RNG, as Augment's draws do."""

    def __init__(self, time_warp=0, freq_masks=0, freq_width=27, time_masks=0, time_width=100, time_ratio=1.0, time_count_ratio=0,
                 fill='mean', seed=0):
        super().__init__()
        self.policy = parse_policy({'time_warp': time_warp, 'freq_masks': freq_masks, 'freq_width': freq_width, 'time_masks': time_masks,
                                    'time_width': time_width, 'time_ratio': time_ratio, 'time_count_ratio': time_count_ratio, 'fill': fill})
        self.seed, self.calls = seed, 0
        self._ws = self._out = None

    def forward(self, x, lens, draws=None):
        if x.dtype != torch.float32 or x.dim() != 3:
            raise ValueError('SpecAugmentPolicy takes a float32 (B,T,D) batch')
        x = x.contiguous()
        B, T, D = x.shape
        lens = lens.to(x.device, torch.int64).contiguous()
        d_in = None
        if draws is not None:
            d_in = draws.to(x.device, torch.int32).contiguous()
            if d_in.numel() != B * POLICY_RECORD:
                raise ValueError('SpecAugmentPolicy: draws must be (B, %d)' % POLICY_RECORD)
        self.calls += 1
        nbytes = H.lib().asr_specaug_policy_workspace_bytes(B)
        if self._ws is None or self._ws.numel() * 8 < nbytes or self._ws.device != x.device:
            self._ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
        if self._out is None or self._out.numel() < x.numel() or self._out.device != x.device:
            self._out = torch.empty(x.numel(), dtype=torch.float32, device=x.device)
        out = self._out[:x.numel()].view(B, T, D)
        p = self.policy
        H.call('asr_specaug_policy', H.ptr(x), H.ptr(lens), H.ptr(out), H.ptr(d_in), None, B, T, D, p['time_warp'], p['freq_masks'],
               p['freq_width'], p['time_masks'], p['time_width'], p['time_ratio_pm'], p['time_count_ratio_pm'],
               1 if p['fill'] == 'zero' else 0, (self.seed * 1000003 + self.calls) & 0xFFFFFFFFFFFF, H.ptr(self._ws),
               self._ws.numel() * 8, H.stream_ptr())
        return out, lens

    def extra_repr(self):
        p = self.policy
        return ('time_warp={time_warp}, freq_masks={freq_masks}, freq_width={freq_width}, time_masks={time_masks}, '
                'time_width={time_width}, time_ratio={tr}, time_count_ratio={tc}, fill={fill}, seed={seed}').format(
                    tr=p['time_ratio_pm'] / 1000.0, tc=p['time_count_ratio_pm'] / 1000.0, seed=self.seed, **p)


def wave_aug_table(n_fft):
    """What the FFT kernels of csrc/wave_aug.hip read: n_fft/2 twiddles (cos, -sin)(2 pi k / n_fft) interleaved, then the periodic
    Hann window, 2 * n_fft float32 in all, rounded once from float64."""
    k = np.arange(n_fft // 2, dtype=np.float64)
    tw = np.stack([np.cos(2.0 * np.pi * k / n_fft), -np.sin(2.0 * np.pi * k / n_fft)], 1).reshape(-1)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)
    return np.concatenate([tw, win]).astype(np.float32)


class WaveAugment(nn.Module):
    """The reference's ReadAudio.augmenter (src/audio.py:283-309: Gaussian noise, time stretch, pitch shift) on a zero-padded
    waveform batch, in place: wav (B,N) fp32 + wav_len (B) -> the same two.  draws (B,6) float32 = {noise_on, amp, stretch_on,
    rate, pitch_on, semitones} skips the device RNG, as Augment's draws do."""

    def __init__(self, seed=0, n_fft=2048):
        super().__init__()
        self.seed, self.n_fft, self.calls = seed, n_fft, 0
        self.register_buffer('table', torch.from_numpy(wave_aug_table(n_fft)), persistent=False)
        self._ws = None

    def forward(self, wav, wav_len, draws=None):
        if wav.dtype != torch.float32 or not wav.is_contiguous():
            raise ValueError('WaveAugment works in place on a contiguous float32 (B,N) batch')
        B, N = wav.shape
        lens = wav_len.to(wav.device, torch.int64).contiguous()
        d_in = None
        if draws is not None:
            d_in = draws.to(wav.device, torch.float32).contiguous()
        self.calls += 1
        nbytes = H.lib().asr_wave_augment_workspace_bytes(B, N, self.n_fft)
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != wav.device:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=wav.device)
        H.call('asr_wave_augment', H.ptr(wav), H.ptr(lens), H.ptr(d_in), None, H.ptr(self.table), B, N, self.n_fft,
               (self.seed * 1000003 + self.calls) & 0xFFFFFFFFFFFF, H.ptr(self._ws), self._ws.numel(), H.stream_ptr())
        return wav, wav_len

    def extra_repr(self):
        return 'seed={}, n_fft={}'.format(self.seed, self.n_fft)


class FrontEnd(nn.Module):
    def __init__(self, stages):
        super().__init__()
        self.stages = nn.ModuleList(stages)

    def forward(self, x, lens):
        for s in self.stages:
            x, lens = s(x, lens)
        return x, lens


def create_transform(audio_config, mode='train'):
    """Same keys as the reference's create_transform (src/audio.py:453-486); returns (module, feature dim).  augment may also be
    a mapping (POLICY_KEYS): the training chain then ends in SpecAugmentPolicy instead of Augment."""
    cfg = dict(audio_config)
    delta_order = cfg.pop('delta_order', 0)
    delta_window = cfg.pop('delta_window_size', 2)
    apply_cmvn = cfg.pop('apply_cmvn', False)
    feat_type, feat_dim = cfg.pop('feat_type'), cfg.pop('feat_dim')
    augment = cfg.pop('augment', False)
    time_aug = cfg.pop('time_aug', False)
    policy = parse_policy(augment) if isinstance(augment, dict) else None          # checked in every mode
    stages = [WaveAugment()] if time_aug and mode == 'train' else []
    stages.append(ExtractAudioFeature(mode=feat_type, num_mel_bins=feat_dim, sample_rate=SAMPLE_RATE, **cfg))
    if delta_order >= 1:
        stages.append(Delta(delta_order, delta_window))
    if apply_cmvn:
        stages.append(CMVN())
    stages.append(Postprocess())
    if policy is not None and mode == 'train':
        stages.append(SpecAugmentPolicy(policy['time_warp'], policy['freq_masks'], policy['freq_width'], policy['time_masks'],
                                        policy['time_width'], policy['time_ratio_pm'] / 1000.0, policy['time_count_ratio_pm'] / 1000.0,
                                        policy['fill']))
    elif policy is None and augment and mode == 'train':
        stages.append(Augment())
    return FrontEnd(stages), feat_dim * (delta_order + 1)
