"""The yardstick of csrc/wave_aug.hip (waveform augmentation, data.audio.time_aug): a float64 restatement of every stage and of the
chain, the case tables, the bounds and their pins.  tests/test_hip_wave_aug.py imports all of it; nothing here runs a kernel.

Recipe.  draws (B,6) float32 = {noise_on, amp, stretch_on, rate, pitch_on, semitones}.

  draws      Philox4x32-10 blocks (b, 0, 3, 0) -> r0..r3 and (b, 0, 4, 0) -> r4, r5, keyed by the seed.  u_i = float32(r_i) * 2^-32 in
             float32; switches u0 < 0.3, u2 < 0.3, u4 < 0.5; amp = 0.001 + u1 (0.01 - 0.001), rate = 0.8 + u3 (1.25 - 0.8),
             semitones = -4 + u5 * 8: float32 multiply, then float32 add, no fused multiply-add.  Pitch rate = float32(2^(-s/12)),
             the power in float64.  A stretch / pitch switch is recorded 0 when len <= n_fft/2 or the rate is outside [0.5, 2].
  noise      sample n of utterance b takes Philox block (n // 4, b, 5, 0) -> r0..r3; with p = (n % 4) // 2:
                 u1 = ((r[2p] >> 8) + 1) 2^-24 in (0, 1],     u2 = (r[2p+1] >> 8) 2^-24 in [0, 1)
                 z = sqrt(-2 ln u1) * (cos(2 pi u2) if n even else sin(2 pi u2)),        x[n] += amp z.
  stft       n_fft, hop = n_fft/4, periodic Hann, centred with reflect padding, n_frames = 1 + len // hop, n_fft/2 + 1 bins.
  pvoc       librosa's phase_vocoder: frame t at s = t rate for t < ceil(n_frames / rate); magnitudes interpolated linearly, phase
             accumulated from angle(D[:, 0]) by phi + wrap(angle(c1) - angle(c0) - phi), phi[k] = k pi / 2.
  istft      irfft, window, overlap-add, divided by the window's sum of squares where that is above float32 tiny (0 elsewhere), the
             centre padding trimmed, length M = round(len / rate) (half to even), zeros beyond the last frame's reach.
  stretch    y[n] for n < min(M, len), 0 for M <= n < len.
  pitch      r = 2^(-s/12): stretch by r to M samples, then out[i] = sum_j y[j] h(i / r - j), h(t) = c sinc(c t) kaiser(t / W),
             c = 0.9475937167399596 min(1, r), W = 64 / min(1, r), Kaiser beta 14.769656459379492 (resampy's kaiser_best).

Bounds, u = 2^-24 the unit roundoff of float32.  The ulp figures of the device functions are those of the OpenCL full profile, which
the device library implements: log 3, sqrt 3, sinpi / cospi 4, atan2 6, hypot 4.
  noise      z, relative, with 1 ulp <= 2u: (3 ulp of log + one product) / 2 = 3.5u under the root, the root 6u, the sine 8u, their
             product u: 18.5u; amp z one more rounding: 19.5u, 21u with the second-order terms; the sum one rounding:
                 |y - y64| <= u |y64| + 21 u |amp z64|.
  fft        Higham, Accuracy and Stability, thm 24.2: ||fl(Fx) - Fx||_2 <= log2(n) eta ||Fx||_2 / (1 - log2(n) eta), eta = mu + g4 (sqrt 2 +
             mu), g4 = 4u / (1 - 4u), mu the twiddle error: the table is rounded once from float64, each component off by <= 2^-25,
             so mu <= 2^-24.  ||Fx||_2 = sqrt(n) ||x||_2.  The STFT transforms two windowed frames (a, b) as a + ib - one more
             rounding (window times sample) on the way in - and separates them by (Z[k] +- conj Z[n-k]) / 2, one rounding each:
                 ||D - D64||_2 per frame <= sqrt(n) sqrt(||a||^2 + ||b||^2) (log2(n) eta' + u) + u ||D64||_2
  pvoc       both angles of a step are off by <= 6 ulp(pi) = 6 * 2^-22 rad; the accumulator is a double in turns reduced exactly,
             so after t steps the phase is off by (1 + 2t) 6 * 2^-22 + pi 2^-24 (its float32 rounding); sincospi 4 ulp per
             component; magnitudes hypot 4 ulp, three roundings of the interpolation, the float32 rounding of the weight a:
                 |o - o64| <= mag64 ((1 + 2t) 6 * 2^-22 + pi u + 4 sqrt 2 * 2u + 2u) + (4 * 2u + 4u) mag64 + u (m0 + m1)
  istft      inverse FFT as above on the pair's spectrum, ||z||_2 the time-domain norm of the pair: every element of a frame is off by
             <= e_f = log2(n) eta' ||z_pair||_2; the gather sums <= 4 products w y (one rounding each, <= 4 additions) and the
             envelope likewise, then one division:
                 |y - y64| <= (sum_f w e_f + 6u sum_f |w y_f|) / env + 8u |y64|
  resample   weights and sum in float64 (I0 by its series of positive terms, sinpi), rounded once:
                 |y - y64| <= u |y64| + (taps + 160) 2^-53 sum_j |y_j h_j|"""
import functools

import numpy as np
import pytest
import torch

from test_encoder_glue_reference import philox_blocks

F32 = np.float32
U24, U53 = 2.0 ** -24, 2.0 ** -53
TINY32 = float(np.finfo(np.float32).tiny)
M32 = np.uint64(0xffffffff)
SENTINEL = F32(-777.25)
KAISER_BETA, ROLLOFF, ZEROS = 14.769656459379492, 0.9475937167399596, 64.0
P_NOISE, P_STRETCH, P_PITCH = F32(0.3), F32(0.3), F32(0.5)
ULP_LOG, ULP_SQRT, ULP_SINPI, ULP_ATAN2, ULP_HYPOT = 3, 3, 4, 6, 4
G4 = 4 * U24 / (1 - 4 * U24)
ETA = U24 + G4 * (np.sqrt(2.0) + U24)


# ---- Philox with a full counter -----------------------------------------------------------------------------------------------
def philox4(c0, c1, c2, c3, seed):
    """Counter words (arrays or scalars, broadcast) -> (n, 4) uint32; the function of csrc/common.h."""
    c0, c1, c2, c3 = [np.atleast_1d(np.asarray(c, dtype=np.uint64)) for c in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & M32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return np.stack([c0, c1, c2, c3], 1).astype(np.uint32)


# ---- draws ------------------------------------------------------------------------------------------------------------------
def raw_draws(B, seed):
    """(B,6) float32 by the draw rule, before the switches an utterance cannot take are cleared."""
    b = np.arange(B)
    r = np.concatenate([philox4(b, 0, 3, 0, seed), philox4(b, 0, 4, 0, seed)[:, :2]], 1)
    u = r.astype(F32) * F32(2.0 ** -32)
    d = np.zeros((B, 6), dtype=F32)
    d[:, 0] = u[:, 0] < P_NOISE
    d[:, 1] = F32(0.001) + u[:, 1] * (F32(0.01) - F32(0.001))
    d[:, 2] = u[:, 2] < P_STRETCH
    d[:, 3] = F32(0.8) + u[:, 3] * (F32(1.25) - F32(0.8))
    d[:, 4] = u[:, 4] < P_PITCH
    d[:, 5] = F32(-4.0) + u[:, 5] * F32(8.0)
    return d


def pitch_rate(semitones):
    return np.exp2(-np.asarray(semitones, dtype=F32).astype(np.float64) / 12.0).astype(F32)


def rate_ok(r):
    with np.errstate(invalid='ignore'):
        return (np.asarray(r) >= F32(0.5)) & (np.asarray(r) <= F32(2.0))


def finish_draws(d, lens, N, n_fft):
    """draws as given or drawn -> (draws as applied (B,6), rates (B,2)): asr_wave_draws."""
    d = np.array(d, dtype=F32)
    ln = np.clip(np.asarray(lens, dtype=np.int64), 0, N)
    pr = pitch_rate(d[:, 5])
    d[:, 0] = d[:, 0] != 0
    d[:, 2] = (d[:, 2] != 0) & rate_ok(d[:, 3]) & (ln > n_fft // 2)
    d[:, 4] = (d[:, 4] != 0) & rate_ok(pr) & (ln > n_fft // 2)
    rates = np.stack([np.where(d[:, 2] != 0, d[:, 3], F32(0)), np.where(d[:, 4] != 0, pr, F32(0))], 1).astype(F32)
    return d, rates


# ---- noise -------------------------------------------------------------------------------------------------------------------
def normals64(b, n, seed):
    """z[0..n) of utterance b in float64 by the exact map of the module docstring."""
    q = (n + 3) // 4
    r = philox4(np.arange(q), b, 5, 0, seed).astype(np.uint64)
    z = np.zeros((q, 4))
    for p in range(2):
        u1 = ((r[:, 2 * p] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
        u2 = (r[:, 2 * p + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        rad = np.sqrt(-2.0 * np.log(u1))
        z[:, 2 * p], z[:, 2 * p + 1] = rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2)
    return z.reshape(-1)[:n]


def noise64(x, lens, draws, seed):
    """x (B,N) float32 -> (y float64 (B,N), amp z float64 (B,N), 0 where nothing is added)."""
    B, N = x.shape
    y, az = x.astype(np.float64), np.zeros((B, N))
    for b in range(B):
        n = max(0, min(int(lens[b]), N))
        if draws[b, 0] != 0 and n > 0:
            az[b, :n] = float(draws[b, 1]) * normals64(b, n, seed)
            y[b, :n] += az[b, :n]
    return y, az


def noise_bound(y64, az64):
    return U24 * np.abs(y64) + 21 * U24 * np.abs(az64)


# ---- tables, counts ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(n_fft):
    """The (2 n_fft) float32 table the FFT kernels read: n_fft/2 twiddles (cos, -sin) interleaved, then the periodic Hann window."""
    k = np.arange(n_fft // 2, dtype=np.float64)
    tw = np.stack([np.cos(2.0 * np.pi * k / n_fft), -np.sin(2.0 * np.pi * k / n_fft)], 1).reshape(-1)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)
    return np.concatenate([tw, win]).astype(F32)


def window64(n_fft):
    return table(n_fft)[n_fft:].astype(np.float64)


def n_frames(length, n_fft):
    return 1 + length // (n_fft // 4)


def out_frames(nfr, rate):
    return int(np.ceil(np.float64(nfr) / np.float64(rate)))


def out_len(length, rate):
    return int(np.rint(np.float64(length) / np.float64(rate)))


# ---- STFT / vocoder / ISTFT ------------------------------------------------------------------------------------------------------
def frames64(x, n_fft):
    """x (len,) -> the windowed frames (n_frames, n_fft) in float64 (float32 window, float32 samples: exact products)."""
    x = np.asarray(x, dtype=np.float64)
    hop = n_fft // 4
    xp = np.pad(x, n_fft // 2, mode='reflect')
    idx = np.arange(n_frames(len(x), n_fft))[:, None] * hop + np.arange(n_fft)[None, :]
    return xp[idx] * window64(n_fft)[None, :]


def stft64(x, n_fft):
    return np.fft.rfft(frames64(x, n_fft), axis=1)                  # (n_frames, n_fft/2 + 1)


def stft_bound(x, n_fft):
    """Per frame (n_frames,): the bound on ||D - D64||_2, frames paired (0,1), (2,3), ... as the kernel transforms them."""
    fr = frames64(x, n_fft)
    e2 = (fr * fr).sum(1)
    pair = e2.copy()
    pair[0:len(e2) - len(e2) % 2:2] += e2[1::2]
    pair[1::2] = pair[0:len(e2) - len(e2) % 2:2]
    lg = np.log2(n_fft)
    d = np.sqrt((np.abs(np.fft.rfft(fr, axis=1)) ** 2).sum(1))
    return np.sqrt(n_fft * pair) * (lg * ETA / (1 - lg * ETA) + U24) + U24 * d


def _wrap(d):
    return d - 2.0 * np.pi * np.round(d / (2.0 * np.pi))


def pvoc64(D, rate, with_parts=False):
    """D (n_frames, nb) complex -> (ceil(n_frames / rate), nb) complex128, the loop of librosa.phase_vocoder.  The accumulator is
    kept within a turn (phi[k] = k pi / 2 grows by 800 k rad per frame at n_fft = 2048, and a float64 at 3e4 rad resolves 4e-12);
    pvoc64_cumsum is the literal, unreduced form."""
    D = np.asarray(D, dtype=np.complex128)
    nfr, nb = D.shape
    rate = np.float64(rate)
    nout = out_frames(nfr, rate)
    phi = np.pi * (np.arange(nb) % 4) / 2.0               # k pi / 2 less whole turns: the same under wrap and exp, and exact
    Dp = np.concatenate([D, np.zeros((2, nb), dtype=np.complex128)], 0)
    out = np.zeros((nout, nb), dtype=np.complex128)
    mags, sums = np.zeros((nout, nb)), np.zeros((nout, nb))
    acc = np.angle(D[0])
    for t in range(nout):
        st = t * rate
        fl = int(np.floor(st))
        a = st - fl
        c0, c1 = Dp[min(fl, nfr)], Dp[min(fl + 1, nfr)]
        mags[t] = (1.0 - a) * np.abs(c0) + a * np.abs(c1)
        sums[t] = np.abs(c0) + np.abs(c1)
        out[t] = mags[t] * np.exp(1j * acc)
        acc = _wrap(acc + phi + _wrap(np.angle(c1) - np.angle(c0) - phi))
    return (out, mags, sums) if with_parts else out


def pvoc64_cumsum(D, rate):
    """The same as one gather and one cumulative sum."""
    D = np.asarray(D, dtype=np.complex128)
    nfr, nb = D.shape
    nout = out_frames(nfr, rate)
    phi = np.pi * np.arange(nb) / 2.0
    Dp = np.concatenate([D, np.zeros((2, nb), dtype=np.complex128)], 0)
    st = np.arange(nout) * np.float64(rate)
    fl = np.floor(st).astype(np.int64)
    a = (st - fl)[:, None]
    c0, c1 = Dp[np.minimum(fl, nfr)], Dp[np.minimum(fl + 1, nfr)]
    adv = phi[None, :] + _wrap(np.angle(c1) - np.angle(c0) - phi[None, :])
    acc = np.angle(D[0])[None, :] + np.concatenate([np.zeros((1, nb)), np.cumsum(adv, 0)[:-1]], 0)
    return ((1.0 - a) * np.abs(c0) + a * np.abs(c1)) * np.exp(1j * acc)


def pvoc_bound(mags, sums):
    t = np.arange(mags.shape[0])[:, None]
    phase = (1 + 2 * t) * ULP_ATAN2 * 2.0 ** -22 + np.pi * U24 + ULP_SINPI * np.sqrt(2.0) * 2 * U24 + 2 * U24
    return mags * (phase + ULP_HYPOT * 2 * U24 + 4 * U24) + U24 * sums


def istft64(O, M, n_fft, with_bound=False):
    """O (n_out, nb) complex -> y (M,) float64 [, the bound per sample]."""
    O = np.asarray(O, dtype=np.complex128)
    nout = O.shape[0]
    hop, w = n_fft // 4, window64(n_fft)
    fr = np.fft.irfft(O, n=n_fft, axis=1)
    total = n_fft + hop * (nout - 1)
    y, env, ea, eb = np.zeros(total), np.zeros(total), np.zeros(total), np.zeros(total)
    # the kernel transforms frames in pairs (f_first + 2w, f_first + 2w + 1) with f_first = 5g - 3: a frame's partner depends on the
    # workgroup, so the pair norm is bounded by the frame with its larger neighbour on either side
    e2 = (fr * fr).sum(1)
    nb2 = np.maximum(np.concatenate([[0.0], e2[:-1]]), np.concatenate([e2[1:], [0.0]]))
    lg = np.log2(n_fft)
    ef = lg * ETA / (1 - lg * ETA) * np.sqrt(e2 + nb2)
    for f in range(nout):
        sl = slice(f * hop, f * hop + n_fft)
        y[sl] += w * fr[f]
        env[sl] += w * w
        ea[sl] += w * ef[f]
        eb[sl] += np.abs(w * fr[f])
    ok = env > TINY32
    out = np.where(ok, y / np.where(ok, env, 1.0), 0.0)
    bnd = np.where(ok, (ea + 6 * U24 * eb) / np.where(ok, env, 1.0), 0.0) + 8 * U24 * np.abs(out)
    out, bnd = out[n_fft // 2:], bnd[n_fft // 2:]
    if len(out) < M:
        out, bnd = np.concatenate([out, np.zeros(M - len(out))]), np.concatenate([bnd, np.zeros(M - len(bnd))])
    return (out[:M], bnd[:M]) if with_bound else out[:M]


# ---- resampler -------------------------------------------------------------------------------------------------------------------
def resample_weights(n_out, M, rate):
    """-> (j (n_out, taps) int64 clipped into [0, M), h (n_out, taps) float64, 0 outside the window or the wave)."""
    rate = np.float64(rate)
    mn = min(1.0, rate)
    c, W = ROLLOFF * mn, ZEROS / mn
    pos = np.arange(n_out, dtype=np.float64) / rate
    taps = 2 * int(np.ceil(W)) + 2
    j = np.ceil(pos - W).astype(np.int64)[:, None] + np.arange(taps)[None, :]
    t = pos[:, None] - j
    s2 = 1.0 - (t * (mn / ZEROS)) ** 2
    ok = (s2 >= 0.0) & (j >= 0) & (j < M) & (j <= np.floor(pos + W)[:, None])
    h = c * np.sinc(c * t) * np.i0(KAISER_BETA * np.sqrt(np.maximum(s2, 0.0))) / np.i0(KAISER_BETA)
    return np.clip(j, 0, max(M - 1, 0)), np.where(ok, h, 0.0)


def resample64(y, n_out, rate, with_bound=False):
    y = np.asarray(y, dtype=np.float64)
    j, h = resample_weights(n_out, len(y), rate)
    terms = y[j] * h
    out = terms.sum(1)
    if with_bound:
        return out, U24 * np.abs(out) + (h.shape[1] + 160) * U53 * np.abs(terms).sum(1)
    return out


# ---- stages and the chain ----------------------------------------------------------------------------------------------------------
def stretch64(x, rate, n_fft, keep_len=True):
    """x (len,) -> the stretched wave: len samples (zeros from M on) or, keep_len False, M = round(len / rate) samples."""
    n = len(x)
    M = out_len(n, rate)
    y = istft64(pvoc64(stft64(x, n_fft), rate), M, n_fft)
    if not keep_len:
        return y
    out = np.zeros(n)
    out[:min(M, n)] = y[:min(M, n)]
    return out


def pitch64(x, rate, n_fft):
    """rate = 2^(-semitones / 12) as the float32 the kernels read."""
    return resample64(stretch64(x, rate, n_fft, keep_len=False), len(x), rate)


def chain64(x, lens, draws, seed, n_fft, stft=None):
    """x (B,N) float32, draws as applied (finish_draws) -> (B,N) float64; samples n >= len as they came.  stft: replaces stft64
    (the end-to-end yardstick feeds a float32 torch.stft here)."""
    B, N = x.shape
    d, rates = finish_draws(draws, lens, N, n_fft)
    y, _ = noise64(x, lens, d, seed)
    for b in range(B):
        n = max(0, min(int(lens[b]), N))
        for stage in range(2):
            r = rates[b, stage]
            if r == 0:
                continue
            v = y[b, :n]
            M = out_len(n, r)
            s = istft64(pvoc64((stft or stft64)(v, n_fft), r), M, n_fft)
            if stage == 0:
                v = np.zeros(n)
                v[:min(M, n)] = s[:min(M, n)]
            else:
                v = resample64(s, n, r)
            y[b, :n] = v
    return y


# ---- case tables (shared with the GPU file) ----------------------------------------------------------------------------------------
RATES = [0.8, 1.25, 1.0, 0.5, 2.0, float(pitch_rate(4.0)), float(pitch_rate(-4.0))]
# (n_fft, [(len, recipe)]): 0 and n_fft/2 are skipped, n_fft/2 + 1 is the smallest legal length (every reflect index is used), then a
# hop multiple, + 1, + hop - 1, and one length beyond N
CASES = {
    64: [(0, 'normal'), (32, 'normal'), (33, 'normal'), (64, 'normal'), (192, 'normal'), (193, 'normal'), (207, 'normal'), (300, 'normal'),
         (192, 'zero'), (193, 'cosine'), (207, 'impulse')],
    256: [(129, 'normal'), (700, 'normal'), (769, 'normal'), (769, 'cosine'), (640, 'impulse')],
    2048: [(512 * 12 + 5, 'normal')],
}
CASE_RATES = {64: RATES, 256: RATES, 2048: [0.8]}
CASE_N = {64: 207, 256: 769, 2048: 512 * 12 + 5}


def recipe(name, b, n, n_fft, seed=11):
    g = np.random.Generator(np.random.PCG64([seed, b, n, n_fft]))
    if name == 'normal':
        return (0.3 * g.standard_normal(n)).astype(F32)
    if name == 'zero':
        return np.zeros(n, dtype=F32)
    if name == 'cosine':
        return np.cos(2.0 * np.pi * (n_fft // 8) * np.arange(n) / n_fft).astype(F32)          # the centre of bin n_fft / 8
    if name == 'impulse':
        v = np.zeros(n, dtype=F32)
        v[n // 3] = 1.0
        return v
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def wave_case(n_fft):
    """-> dict(N, lens, x (B + 1, N) float32): utterance b holds its recipe in [0, min(len, N)), SENTINEL behind it; row B is the
    NaN guard utterance."""
    rows, N = CASES[n_fft], CASE_N[n_fft]
    B = len(rows)
    x = np.full((B + 1, N), SENTINEL, dtype=F32)
    for b, (n, name) in enumerate(rows):
        m = min(n, N)
        x[b, :m] = recipe(name, b, m, n_fft)
    x[B] = np.nan
    x.setflags(write=False)
    return {'N': N, 'lens': [n for n, _ in rows], 'x': x, 'B': B}


# ---- pins ---------------------------------------------------------------------------------------------------------------------------
def test_philox4_is_the_pinned_philox():
    for seed in (99, 0x9E3779B97F4A7C15):
        blk = np.array([0, 1, 5, 2 ** 32 + 7, 2 ** 40 + 3], dtype=np.uint64)
        assert np.array_equal(philox4(blk & M32, blk >> np.uint64(32), 0, 0, seed), philox_blocks(blk, seed))
    assert not np.array_equal(philox4([0, 1], 0, 3, 0, 7), philox4([0, 1], 0, 4, 0, 7))


def test_draw_rule():
    d = raw_draws(4096, 1000004)
    assert d.dtype == F32
    for col, p in ((0, 0.3), (2, 0.3), (4, 0.5)):
        assert set(np.unique(d[:, col])) <= {0.0, 1.0}
        assert abs(d[:, col].mean() - p) <= 4 * np.sqrt(p * (1 - p) / 4096)
    for col, lo, hi in ((1, 0.001, 0.01), (3, 0.8, 1.25), (5, -4.0, 4.0)):
        assert (d[:, col] >= F32(lo)).all() and (d[:, col] <= F32(hi)).all()
        assert abs(d[:, col].mean() - (lo + hi) / 2) < 4 * (hi - lo) / np.sqrt(12 * 4096)
    # the switches an utterance cannot take
    raw = np.array([[1, 0.01, 1, 0.8, 1, 4.0]] * 5 + [[1, 0.01, 1, 0.4, 1, 13.0], [0, 0.01, 2, 2.0, -1, -12.0], [1, 0, 1, np.nan, 1, np.nan]], dtype=F32)
    dd, rates = finish_draws(raw, [0, 32, 33, 64, 500, 64, 64, 64], 100, 64)
    assert dd[:, 2].tolist() == [0, 0, 1, 1, 1, 0, 1, 0] and dd[:, 4].tolist() == [0, 0, 1, 1, 1, 0, 1, 0] and dd[:, 0].tolist() == [1] * 6 + [0, 1]
    assert rates[2].tolist() == [F32(0.8), pitch_rate(4.0)] and rates[5].tolist() == [0, 0] and rates[6].tolist() == [2.0, 2.0]
    assert float(pitch_rate(4.0)) == float(F32(2.0 ** (-4.0 / 12))) and rate_ok(pitch_rate(4.0)) and rate_ok(pitch_rate(-4.0))


def test_box_muller_map_and_moments():
    z = normals64(3, 2 ** 16, 12345)
    assert np.isfinite(z).all()
    n = len(z)
    assert abs(z.mean()) < 4 / np.sqrt(n) and abs(z.var() - 1) < 4 * np.sqrt(2.0 / n)
    assert abs((z ** 3).mean()) < 4 * np.sqrt(15.0 / n) and abs((z ** 4).mean() - 3) < 4 * np.sqrt(96.0 / n)
    assert abs(np.corrcoef(z[0::2], z[1::2])[0, 1]) < 4 / np.sqrt(n / 2)
    # the first uniform is never 0: the largest |z| the map can give is sqrt(-2 ln 2^-24)
    assert np.abs(z).max() <= np.sqrt(48 * np.log(2.0))
    # keyed by utterance and by n // 4: a prefix is a prefix, another utterance is another stream
    assert np.array_equal(normals64(3, 10, 12345), z[:10]) and not np.array_equal(normals64(4, 10, 12345), z[:10])


@pytest.mark.parametrize('n_fft', [64, 256, 2048])
def test_stft_istft_against_torch(n_fft):
    g = np.random.Generator(np.random.PCG64(n_fft))
    n = n_fft * 5 + 3
    x = g.standard_normal(n)
    w = torch.from_numpy(window64(n_fft))
    assert np.abs(w.numpy() - torch.hann_window(n_fft, periodic=True, dtype=torch.float64).numpy()).max() < 2.0 ** -24
    D = stft64(x, n_fft)
    T = torch.stft(torch.from_numpy(x), n_fft, hop_length=n_fft // 4, window=w, center=True, pad_mode='reflect', return_complex=True).numpy().T
    assert D.shape == (n_frames(n, n_fft), n_fft // 2 + 1) == T.shape
    assert np.abs(D - T).max() <= 3e-12 * np.abs(T).max()
    # the round trip, and the inverse against torch on a length the frames reach
    M = (D.shape[0] - 1) * (n_fft // 4)
    y = istft64(D, M, n_fft)
    ty = torch.istft(torch.from_numpy(T.T.copy()), n_fft, hop_length=n_fft // 4, window=w, center=True, length=M).numpy()
    assert np.abs(y - x[:M]).max() <= 3e-12 * np.abs(x).max() and np.abs(y - ty).max() <= 3e-12 * np.abs(x).max()
    # rate 1 reproduces D
    assert np.abs(pvoc64(D, 1.0) - D).max() <= 3e-12 * np.abs(D).max()


@pytest.mark.parametrize('n_fft', [64, 256])
@pytest.mark.parametrize('rate', RATES)
def test_vocoder_loop_is_the_cumulative_sum(n_fft, rate):
    g = np.random.Generator(np.random.PCG64([n_fft, int(rate * 1000)]))
    n = n_fft * 6 + 5
    D = stft64(g.standard_normal(n), n_fft)
    a, c = pvoc64(D, rate), pvoc64_cumsum(D, rate)
    assert a.shape == (out_frames(D.shape[0], rate), n_fft // 2 + 1)
    assert np.abs(a - c).max() <= 1e-9 * np.abs(D).max()
    assert len(stretch64(np.zeros(n), rate, n_fft, keep_len=False)) == out_len(n, rate)
    assert out_frames(D.shape[0], rate) <= 2 * D.shape[0] and out_len(n, rate) <= 2 * n


def _tone_amplitude(y, freq):
    """Amplitude of the component of y at `freq` cycles per sample, over a Hann-weighted stretch (leakage of the rest ~ 0)."""
    n = np.arange(len(y))
    w = np.hanning(len(y))
    return 2.0 * np.abs((y * w * np.exp(-2j * np.pi * freq * n)).sum()) / w.sum()


@pytest.mark.parametrize('n_fft', [64, 256, 2048])
def test_cosine_under_stretch_and_pitch(n_fft):
    k0 = n_fft // 8
    n = n_fft * 10
    x = np.cos(2.0 * np.pi * k0 * np.arange(n) / n_fft)
    # stretched by 0.8: the same bin, unit amplitude
    y = stretch64(x, 0.8, n_fft, keep_len=False)
    assert len(y) == out_len(n, 0.8)
    mid = y[2 * n_fft:len(y) - 2 * n_fft]
    spec = np.abs(np.fft.rfft(mid[:n_fft * 4] * np.hanning(n_fft * 4)))
    assert int(spec.argmax()) == k0 * 4
    assert abs(_tone_amplitude(mid, k0 / n_fft) - 1.0) < 1e-7
    # shifted by +-4 semitones: the peak at f 2^(+-4/12) within the analysis resolution, amplitude 1
    for s in (4.0, -4.0):
        r = float(pitch_rate(s))
        z = pitch64(x, r, n_fft)
        assert len(z) == n
        mid = z[2 * n_fft:n - 2 * n_fft]
        f = k0 / n_fft / r
        L = len(mid)
        spec = np.abs(np.fft.rfft(mid * np.hanning(L)))
        assert abs(int(spec.argmax()) / L - f) <= 1.0 / n_fft
        assert abs(_tone_amplitude(mid, f) - 1.0) < 1e-7, (s, _tone_amplitude(mid, f))


def test_resampler_at_ratio_one_is_the_identity_to_the_stop_band():
    g = np.random.Generator(np.random.PCG64(5))
    y = g.standard_normal(700)
    out, bnd = resample64(y, 700, 1.0, with_bound=True)
    # at ratio 1 the taps sit on the integers: h(j) = c sinc(c j) kaiser(j / 64), which is not a delta (c < 1); what is left of the
    # signal is a low-pass at 0.9476 of Nyquist, so white noise loses its top band.  A band-limited input comes back.
    n = np.arange(700)
    s = np.cos(2 * np.pi * 0.11 * n) + 0.5 * np.sin(2 * np.pi * 0.31 * n)
    o = resample64(s, 700, 1.0)
    assert np.abs(o - s)[128:-128].max() < 1e-6                       # kaiser_best: stop band below -120 dB
    assert (bnd >= U24 * np.abs(out)).all() and out.shape == (700,)
    # taps: 2 W + 1 at most, none outside the wave
    j, h = resample_weights(50, 40, 0.5)
    assert (np.count_nonzero(h, axis=1) <= 2 * 128 + 1).all() and (h[:, :][j >= 40] == 0).all()


def test_float32_stft_moves_the_chain_little():
    """Feeding the float64 vocoder a float32 torch.stft moves a 40-frame white-noise output by ~3e-5 of the spectrogram's peak and the
    waveform by ~1e-6 at amplitude 0.32: the chain is not chaotic on such input (printed, with a loose assertion)."""
    n_fft = 2048
    n = 512 * 39 + 7
    x = (0.1 * np.random.Generator(np.random.PCG64(40)).standard_normal(n)).astype(F32)
    for rate in (0.8, 1.25):
        a = stretch64(x, rate, n_fft)
        b = stretch64_f32stft(x, rate, n_fft)
        print('float32-stft yardstick rate %.2f: max |dy| %.3g at amplitude %.3g' % (rate, np.abs(a - b).max(), np.abs(a).max()))
        assert np.abs(a - b).max() < 1e-4 * np.abs(a).max()


def stft32_torch(x, n_fft):
    """float32 torch.stft of x with the float32 window, as complex128 (n_frames, nb)."""
    w = torch.from_numpy(table(n_fft)[n_fft:].copy())
    t = torch.stft(torch.from_numpy(np.asarray(x, dtype=F32).copy()), n_fft, hop_length=n_fft // 4, window=w, center=True, pad_mode='reflect',
                   return_complex=True)
    return t.numpy().T.astype(np.complex128)


def stretch64_f32stft(x, rate, n_fft):
    n = len(x)
    M = out_len(n, rate)
    y = istft64(pvoc64(stft32_torch(x, n_fft), rate), M, n_fft)
    out = np.zeros(n)
    out[:min(M, n)] = y[:min(M, n)]
    return out


def test_bounds_are_small_and_cover_float32_arithmetic():
    """The bounds are derived, not measured; here each is shown to admit the correctly rounded float32 result of its stage (the
    least any float32 kernel commits) and to be of the order of float32 roundoff."""
    n_fft = 64
    c = wave_case(n_fft)
    x = c['x'][4, :192]
    D = stft64(x, n_fft)
    sb = stft_bound(x, n_fft)
    assert (sb < 1e-5 * np.sqrt((np.abs(D) ** 2).sum(1)).max()).all()
    assert (np.sqrt((np.abs(D.astype(np.complex64) - D) ** 2).sum(1)) <= sb).all()
    out, mags, sums = pvoc64(D.astype(np.complex64), 0.8, with_parts=True)
    pb = pvoc_bound(mags, sums)
    assert (np.abs(out.astype(np.complex64) - out) <= pb).all() and pb.max() < 1e-3 * mags.max()
    y, yb = istft64(out.astype(np.complex64), out_len(192, 0.8), n_fft, with_bound=True)
    assert (np.abs(y.astype(F32) - y) <= yb).all()
    r, rb = resample64(y.astype(F32), 192, 0.8, with_bound=True)
    assert (np.abs(r.astype(F32) - r) <= rb).all()


def test_table_is_the_modules():
    from src.audio import wave_aug_table
    for n_fft in (64, 256, 2048):
        assert np.array_equal(wave_aug_table(n_fft), table(n_fft))
