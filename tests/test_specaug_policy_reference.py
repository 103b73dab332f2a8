"""The yardstick of asr_specaug_policy (csrc/specaug_policy.hip): the integer draw rule restated in numpy on the
Philox of tests/test_frontend_reference.py, the float64 restatement policy64, the derived float32 bound of the warp, the case
table, and their own pins.  tests/test_hip_specaug_policy.py imports all of it; nothing here runs a kernel.

  policy_draws   the 82-word record {w0, c, (f0, fend) x 8, (t0, tend) x 32} of utterance b with n = min(max(len, 0), T) frames;
  clamp_record   what the kernel makes of a caller-supplied record (draws_in);
  warp_index     per destination frame t < n the integers (i, r, den) of the stated rule: the source position is i + r / den;
  policy64       float64: warp, then the fill (mean of the n D valid INPUT values, or 0) inside every band; rows >= n as they came;
  warp32         the stated float32 arithmetic in numpy, with the product rounded (mul + add) or not (fused multiply-add).

The bound of a warped value.  With a = x[i], b = x[i + 1], q = r / den and u = 2^-24 the kernel forms
      fl(a + fl(fl(q) * fl(b - a)))          or, fused,          fl(a + fl(q) * fl(b - a))
so, with |e_k| <= u for the four roundings (quotient, difference, product, sum) and P = q (b - a) the exact increment,
      y_hat = (a + P (1 + e1)(1 + e2)(1 + e3)) (1 + e4)
      y_hat - y = e4 y + P (1 + e4) ((1 + e1)(1 + e2)(1 + e3) - 1),        |y_hat - y| <= u |y| + |P| (1 + u) ((1 + u)^3 - 1).
|P| <= |b - a| <= |a| + |b| and (1 + u)((1 + u)^3 - 1) < 3 u (1 + 2^-22), which gives the form
      |y_hat - y| <= 2^-24 (|y| + K (|a| + |b|)),      K = 3 (1 + 2^-22)
(K = 2 would do for the fused form alone, which has no e3).  r == 0 is exact: the bound is 0 there.  float(r) and float(den)
are exact below 2^24 frames; nothing in the table comes near the subnormal range.  The bound is never measured on the kernel;
test_bound_holds_for_the_float32_emulation holds both emulations inside it on the whole table (worst ratio printed: 0.68
without and 0.52 with the fused multiply-add; |b - a| reaches |a| + |b| only for neighbours of opposite sign)."""
import collections
import functools

import numpy as np
import pytest
import torch

import test_frontend_reference as FR

SA_SEEDS = FR.SA_SEEDS
REC, N_FM, N_TM = 82, 8, 32
U24 = 2.0 ** -24
K_WARP = 3.0 * (1.0 + 2.0 ** -22)
SENTINEL = 9.0

Policy = collections.namedtuple('Policy', 'warp fm fw tm tw tr_pm tc_pm fill')        # fill: 0 mean, 1 zero
IDENTITY = Policy(0, 0, 27, 0, 100, 1000, 0, 0)


def policy_n(length, T):
    return min(max(int(length), 0), int(T))


def _group(b, k, seed):
    return FR.philox4x32_10((b, k, 3, 0), (seed & 0xffffffff, (seed >> 32) & 0xffffffff))


def policy_draws(b, n, D, p, seed):
    """The device draws of utterance b with n valid frames: a list of 82 ints."""
    rec = [0] * REC
    r = _group(b, 0, seed)
    if p.warp > 0 and n >= 2 * p.warp + 1:
        w0 = p.warp + r[0] % (n - 2 * p.warp)
        w = r[1] % (2 * p.warp + 1) - p.warp
        rec[0], rec[1] = w0, min(max(w0 + w, 1), n - 2)
    for j in range(p.fm):
        r = _group(b, 1 + j, seed)
        f = r[0] % (min(p.fw, D) + 1)
        f0 = r[1] % (D - f + 1)
        rec[2 + 2 * j], rec[3 + 2 * j] = f0, f0 + f
    cnt = min(p.tm, n * p.tc_pm // 1000) if p.tc_pm else p.tm
    for j in range(cnt):
        r = _group(b, 1 + N_FM + j, seed)
        t = r[0] % (min(p.tw, n * p.tr_pm // 1000) + 1)
        t0 = r[1] % (n - t + 1)
        rec[2 + 2 * N_FM + 2 * j], rec[3 + 2 * N_FM + 2 * j] = t0, t0 + t
    return rec


def clamp_record(rec, n, D):
    """A caller-supplied record as the kernel applies it."""
    rec = [int(v) for v in rec]
    out = [0] * REC
    if 1 <= rec[0] <= n - 2 and 1 <= rec[1] <= n - 2:
        out[0], out[1] = rec[0], rec[1]
    for k in range(1, 1 + N_FM + N_TM):
        ext = D if k < 1 + N_FM else n
        lo = min(max(rec[2 * k], 0), ext)
        out[2 * k], out[2 * k + 1] = lo, min(max(rec[2 * k + 1], lo), ext)
    return out


def bands(rec):
    """-> (frequency bands, time bands), the non-empty ones as (start, end)."""
    fb = [(rec[2 + 2 * j], rec[3 + 2 * j]) for j in range(N_FM) if rec[3 + 2 * j] > rec[2 + 2 * j]]
    tb = [(rec[18 + 2 * j], rec[19 + 2 * j]) for j in range(N_TM) if rec[19 + 2 * j] > rec[18 + 2 * j]]
    return fb, tb


def band_mask(rec, n, T, D):
    """(T, D) bool: inside any band of a valid row."""
    m = np.zeros((T, D), dtype=bool)
    fb, tb = bands(rec)
    for lo, hi in fb:
        m[:n, lo:hi] = True
    for lo, hi in tb:
        m[lo:min(hi, n)] = True
    return m


def warp_index(n, w0, c):
    """(i, r, den) int64 arrays over t = 0..n-1: destination frame t reads source position i + r / den."""
    t = np.arange(n, dtype=np.int64)
    first = t <= c
    num = np.where(first, t * w0, (t - c) * (n - 1 - w0))
    den = np.where(first, c, n - 1 - c)
    return np.where(first, 0, w0) + num // den, num % den, den


def warp64(x, n, w0, c):
    """x (T, D) -> (n, D) float64: the warped valid rows."""
    x = np.asarray(x, dtype=np.float64)
    if w0 <= 0:
        return x[:n].copy()
    i, r, den = warp_index(n, w0, c)
    a, b = x[i], x[np.minimum(i + 1, n - 1)]
    y = a + (r / den)[:, None] * (b - a)
    y[r == 0] = a[r == 0]
    return y


def warp32(x, n, w0, c, fma):
    """The kernel's stated arithmetic in numpy float32; fma: the product is not rounded (emulated through float64, where the
    product of two float32 is exact)."""
    x = np.asarray(x, dtype=np.float32)
    if w0 <= 0:
        return x[:n].copy()
    i, r, den = warp_index(n, w0, c)
    a, b = x[i], x[np.minimum(i + 1, n - 1)]
    q = (r.astype(np.float32) / den.astype(np.float32))[:, None]
    d = b - a
    assert q.dtype == np.float32 and d.dtype == np.float32
    if fma:
        y = (a.astype(np.float64) + q.astype(np.float64) * d.astype(np.float64)).astype(np.float32)
    else:
        y = a + q * d
    y[r == 0] = a[r == 0]
    return y


def warp_bound(x, n, w0, c, y64):
    """(n, D): the derived bound of the module docstring; 0 where the rule copies."""
    x = np.asarray(x, dtype=np.float64)
    if w0 <= 0:
        return np.zeros((n, x.shape[1]))
    i, r, den = warp_index(n, w0, c)
    bd = U24 * (np.abs(y64) + K_WARP * (np.abs(x[i]) + np.abs(x[np.minimum(i + 1, n - 1)])))
    bd[r == 0] = 0.0
    return bd


def policy64(x, length, rec, fill):
    """x (T, D), rec as applied (inside the utterance) -> (out (T, D) float64, mean64 or None).  Rows >= n are returned as they came."""
    x = np.asarray(x, dtype=np.float64)
    T, D = x.shape
    n = policy_n(length, T)
    out = x.copy()
    if n == 0:
        return out, None
    mean = float(x[:n].sum() / (n * D))
    out[:n] = warp64(x, n, rec[0], rec[1])
    out[band_mask(rec, n, T, D)] = 0.0 if fill else mean
    return out, mean


# ---- case table ------------------------------------------------------------------------------------------------------------------
SA_DIMS = [8, 26, 27, 40, 160]
T_SMALL = 96


def len_cycle(W, T):
    return [0, 1, 2, 3, 2 * W, 2 * W + 1, 2 * W + 2, T - 1, T, T + 5]


# name -> policy.  T = 96: the adaptive count min(4, n * 42 / 1000) is 0 up to n = 12, 3 at n = 95 and 4, the cap, at n = 96
SETTINGS = collections.OrderedDict([
    ('identity', IDENTITY),
    ('warp1', Policy(1, 1, 27, 2, 10, 1000, 0, 0)),
    ('warp5-full', Policy(5, 8, 27, 32, 10, 1000, 0, 1)),
    ('warp5-ratio', Policy(5, 1, 27, 2, 100, 200, 0, 0)),
    ('adaptive', Policy(5, 2, 27, 4, 100, 100, 42, 1)),
    ('adaptive-mean', Policy(0, 2, 8, 4, 100, 100, 42, 0)),
    ('masks-only', Policy(0, 8, 27, 32, 10, 1000, 0, 0)),
    ('warp80', Policy(80, 2, 27, 2, 100, 1000, 0, 0)),
])
RECIPES = ['integer', 'unit', 'normal', 'scaled']

# (name, D, T, setting, recipe, seed, lens or None for the cycle of the setting's warp)
POLICY_CASES = [
    ('id-8', 8, T_SMALL, 'identity', 'normal', SA_SEEDS[0], None),
    ('int-26', 26, T_SMALL, 'masks-only', 'integer', SA_SEEDS[1], None),
    ('int-160', 160, T_SMALL, 'adaptive-mean', 'integer', SA_SEEDS[2], None),
    ('w1-8', 8, T_SMALL, 'warp1', 'unit', SA_SEEDS[0], None),
    ('w1-27', 27, T_SMALL, 'warp1', 'scaled', SA_SEEDS[1], None),
    ('w1-160', 160, T_SMALL, 'warp1', 'normal', SA_SEEDS[2], None),
    ('w5-26', 26, T_SMALL, 'warp5-full', 'normal', SA_SEEDS[0], None),
    ('w5-40', 40, T_SMALL, 'warp5-full', 'scaled', SA_SEEDS[1], None),
    ('w5-160', 160, T_SMALL, 'warp5-full', 'unit', SA_SEEDS[2], None),
    ('ratio-27', 27, T_SMALL, 'warp5-ratio', 'normal', SA_SEEDS[0], None),
    ('ratio-40', 40, T_SMALL, 'warp5-ratio', 'unit', SA_SEEDS[1], None),
    ('adapt-8', 8, T_SMALL, 'adaptive', 'normal', SA_SEEDS[2], None),
    ('adapt-160', 160, T_SMALL, 'adaptive', 'scaled', SA_SEEDS[0], None),
    ('adaptm-26', 26, T_SMALL, 'adaptive-mean', 'unit', SA_SEEDS[1], None),
    ('w80-40', 40, 200, 'warp80', 'normal', SA_SEEDS[2], [160, 161, 162, 199, 200, 205]),
    # more (row, vector) pairs per utterance than one pass of the apply grid (64 workgroups x 256 threads): the strided path,
    # float4 (450 x 40 = 18000 pairs) and scalar (640 x 26 = 16640)
    ('stride-160', 160, 450, 'warp5-ratio', 'normal', SA_SEEDS[0], [450, 449, 300]),
    ('stride-26', 26, 640, 'warp5-full', 'unit', SA_SEEDS[1], [640, 333]),
]
CASE_NAMES = [c[0] for c in POLICY_CASES]
APPLY_PASS = 64 * 256


def policy_input(recipe, B, T, D, seed):
    """(B, T, D) float32."""
    g = np.random.Generator(np.random.PCG64([91, D, T, seed & 0xffff]))
    if recipe == 'integer':
        x = g.integers(-8, 9, size=(B, T, D)).astype(np.float64)
    elif recipe == 'unit':
        x = g.random((B, T, D))
    elif recipe == 'normal':
        x = g.standard_normal((B, T, D))
    elif recipe == 'scaled':
        x = g.standard_normal((B, T, D)) * 10.0 ** np.linspace(-6, 6, T)[None, :, None]
    else:
        raise KeyError(recipe)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def policy_case(name):
    """One case, computed once: x (B + 1, T, D) float32 with a NaN guard utterance behind the B and SENTINEL in the padding rows,
    lens as handed to the kernel, n, the policy, and the device-draw records (with the masks, and with all counts 0)."""
    _, D, T, setting, recipe, seed, lens = POLICY_CASES[CASE_NAMES.index(name)]
    p = SETTINGS[setting]
    if recipe == 'integer':
        assert p.warp == 0
    lens = list(lens) if lens is not None else len_cycle(p.warp, T)
    B = len(lens)
    ns = [policy_n(v, T) for v in lens]
    x = np.full((B + 1, T, D), SENTINEL, dtype=np.float32)
    body = policy_input(recipe, B, T, D, seed)
    for b, n in enumerate(ns):
        x[b, :n] = body[b, :n]
    x[B] = np.nan
    x.setflags(write=False)
    rec = [policy_draws(b, n, D, p, seed) for b, n in enumerate(ns)]
    bare = p._replace(fm=0, tm=0)
    rec_bare = [policy_draws(b, n, D, bare, seed) for b, n in enumerate(ns)]
    return {'name': name, 'D': D, 'T': T, 'B': B, 'policy': p, 'bare': bare, 'recipe': recipe, 'seed': seed, 'lens': lens, 'n': ns,
            'x': x, 'rec': rec, 'rec_bare': rec_bare}


def foreign_record(c, b):
    """A record for draws_in that needs every clamp: the draws of another seed for an utterance of T + 7 frames and D + 5 bins."""
    p = c['policy']._replace(fm=N_FM, tm=N_TM, tc_pm=0, warp=max(c['policy'].warp, 1))
    return policy_draws(b, c['T'] + 7, c['D'] + 5, p, c['seed'] + 12345)


# =================================================================================================================================
# pins
# =================================================================================================================================
LD = Policy(80, 2, 27, 2, 100, 1000, 0, 0)


def test_policy_draws_known_rows():
    """Rows written out: the LD policy at seed 7 (utterances 0 and 5, 1200 frames, 160 bins), a short utterance, the adaptive count."""
    r0 = policy_draws(0, 1200, 160, LD, 7)
    r5 = policy_draws(5, 1200, 160, LD, 7)
    assert len(r0) == REC
    assert r0[:6] == [953, 918, 103, 109, 63, 68] and r0[18:22] == [915, 1009, 674, 737]
    assert r5[:6] == [1006, 993, 115, 126, 115, 140] and r5[18:22] == [780, 833, 289, 389]
    assert r0[6:18] == [0] * 12 and r0[22:] == [0] * 60                   # masks beyond the counts are (0, 0)
    # no warp below 2 W + 1 frames; the first length that has one; time masks at most p n = 6 frames wide
    s = policy_draws(3, 160, 160, LD._replace(tr_pm=40), 7)
    assert s[:2] == [0, 0] and s[18:22] == [21, 27, 130, 131]
    assert policy_draws(3, 161, 160, LD, 7)[:2] == [80, 95]
    # adaptive multiplicity: min(20, n * 40 / 1000) masks, nothing behind them
    a = Policy(0, 0, 27, 20, 100, 40, 40, 0)
    for n, cnt in ((0, 0), (24, 0), (25, 1), (300, 12), (1200, 20)):
        rec = policy_draws(1, n, 160, a, 7)
        assert rec[18 + 2 * cnt:] == [0] * (64 - 2 * cnt) and (cnt == 0 or rec[18 + 2 * cnt - 1] > 0), n
    e = policy_draws(2, 0, 40, LD, 7)                                       # an empty utterance still draws its frequency bands
    assert e[:2] == [0, 0] and e[18:] == [0] * 64 and e[2:6] == [9, 34, 9, 13]
    # the group's third counter word is 3: today's rule (1 and 2) shares no block with it
    assert _group(4, 0, 7) != FR.philox4x32_10((4, 0, 1, 0), (7, 0)) and _group(4, 0, 7) != FR.philox4x32_10((4, 0, 2, 0), (7, 0))


def test_policy_draws_stay_inside_the_utterance():
    for T, W in ((T_SMALL, 0), (T_SMALL, 1), (T_SMALL, 5), (200, 80)):
        for n in sorted(set(policy_n(v, T) for v in len_cycle(W, T))):
            for p in SETTINGS.values():
                for seed in SA_SEEDS:
                    for D in (8, 27, 160):
                        for b in range(12):
                            rec = policy_draws(b, n, D, p, seed)
                            w0, c = rec[:2]
                            if p.warp > 0 and n >= 2 * p.warp + 1:
                                assert p.warp <= w0 <= n - 1 - p.warp and 1 <= c <= n - 2 and abs(c - w0) <= p.warp, (n, p, rec[:2])
                            else:
                                assert (w0, c) == (0, 0)
                            cnt = min(p.tm, n * p.tc_pm // 1000) if p.tc_pm else p.tm
                            for j in range(N_FM):
                                lo, hi = rec[2 + 2 * j], rec[3 + 2 * j]
                                assert 0 <= lo <= hi <= D and hi - lo <= min(p.fw, D) and (j < p.fm or (lo, hi) == (0, 0))
                            for j in range(N_TM):
                                lo, hi = rec[18 + 2 * j], rec[19 + 2 * j]
                                assert 0 <= lo <= hi <= n and hi - lo <= min(p.tw, n * p.tr_pm // 1000) and (j < cnt or (lo, hi) == (0, 0))
                            assert clamp_record(rec, n, D) == rec               # what the device draws is inside already


def test_adaptive_count_reaches_zero_between_and_cap():
    p = SETTINGS['adaptive']
    c = policy_case('adapt-8')
    cnts = {n: min(p.tm, n * p.tc_pm // 1000) for n in c['n']}
    assert cnts[12] == 0 and cnts[95] == 3 and cnts[96] == p.tm == 4


def test_clamp_record():
    rec = [0] * REC
    rec[:2] = [4, 9]
    rec[2:6] = [-3, 5, 30, 99]
    rec[18:24] = [8, 15, 7, 3, -2, 400]
    got = clamp_record(rec, 10, 8)
    assert got[:2] == [0, 0]                                   # c = 9 > n - 2: the warp is off
    assert got[2:6] == [0, 5, 8, 8] and got[18:24] == [8, 10, 7, 7, 0, 10]
    rec[:2] = [8, 1]
    assert clamp_record(rec, 10, 8)[:2] == [8, 1]
    assert clamp_record(rec, 9, 8)[:2] == [0, 0] and clamp_record(rec, 2, 8)[:2] == [0, 0]
    assert clamp_record(rec, 0, 8)[18:24] == [0] * 6


def test_warp64_is_linear_interpolation_with_aligned_corners():
    """Both segments against torch.nn.functional.interpolate(mode='linear', align_corners=True) in float64."""
    g = np.random.Generator(np.random.PCG64(5))
    for k in range(60):
        n = int(g.integers(3, 120))
        w0, c = int(g.integers(1, n - 1)), int(g.integers(1, n - 1))
        x = g.standard_normal((n, 3))
        y = warp64(x, n, w0, c)
        xt = torch.from_numpy(x.T.copy())[None]                                   # (1, D, n)
        first = torch.nn.functional.interpolate(xt[:, :, :w0 + 1], size=c + 1, mode='linear', align_corners=True)[0].numpy().T
        second = torch.nn.functional.interpolate(xt[:, :, w0:], size=n - c, mode='linear', align_corners=True)[0].numpy().T
        assert np.abs(y[:c + 1] - first).max() <= 1e-12 * max(1.0, np.abs(x).max()), (n, w0, c)
        assert np.abs(y[c:] - second).max() <= 1e-12 * max(1.0, np.abs(x).max()), (n, w0, c)
        assert np.array_equal(y[0], x[0]) and np.array_equal(y[c], x[w0]) and np.array_equal(y[n - 1], x[n - 1])
    # the knot at either end of its range
    x = np.arange(10.0)[:, None] * np.ones((1, 2))
    assert np.allclose(warp64(x, 10, 5, 1)[:, 0], [0, 5, 5.5, 6, 6.5, 7, 7.5, 8, 8.5, 9])
    assert np.allclose(warp64(x, 10, 5, 8)[:, 0], [0, .625, 1.25, 1.875, 2.5, 3.125, 3.75, 4.375, 5, 9])
    i, r, den = warp_index(10, 1, 8)
    assert (i + (r > 0)).max() <= 9 and i.min() == 0


def test_policy64_identity_and_hand_made_cases():
    g = np.random.Generator(np.random.PCG64(6))
    x = g.standard_normal((12, 8)).astype(np.float32)
    for n in (0, 1, 5, 12, 40):
        out, _ = policy64(x, n, [0] * REC, 0)
        assert np.array_equal(out, x.astype(np.float64))
    # overlapping bands, a band at each edge, mean fill: one value, the mean of the INPUT's valid region
    rec = [0] * REC
    rec[2:6] = [0, 2, 1, 3]                      # frequency [0, 2) and [1, 3): overlap, at the lower edge
    rec[6:8] = [6, 8]                            # at the upper edge
    rec[18:22] = [0, 2, 7, 9]                    # time [0, 2) at the start, [7, 9) at the end of n = 9
    out, mean = policy64(x, 9, rec, 0)
    assert mean == float(x[:9].astype(np.float64).mean())
    m = band_mask(rec, 9, 12, 8)
    assert m[:9, :3].all() and m[:9, 6:].all() and m[:2].all() and m[7:9].all() and not m[9:].any() and not m[2:7, 3:6].any()
    assert (out[m] == mean).all() and np.array_equal(out[~m], x.astype(np.float64)[~m])
    outz, _ = policy64(x, 9, rec, 1)
    assert (outz[m] == 0.0).all() and np.array_equal(outz[~m], out[~m])
    # c == 1 and c == n - 2, with a mask on top: rows outside the bands are the warped ones, padding rows as they came
    for w0, c in ((4, 1), (3, 7), (1, 7), (7, 1)):
        rec[:2] = [w0, c]
        out, mean = policy64(x, 9, rec, 0)
        y = warp64(x, 9, w0, c)
        assert np.array_equal(out[:9][~m[:9]], y[~m[:9]]) and (out[m] == mean).all() and np.array_equal(out[9:], x[9:].astype(np.float64))
        assert np.array_equal(y[c], x[w0].astype(np.float64))


def test_case_table_covers_what_it_claims():
    ds, fills, recipes, warps = set(), set(), set(), set()
    for name in CASE_NAMES:
        c = policy_case(name)
        ds.add(c['D']); fills.add(c['policy'].fill); recipes.add(c['recipe']); warps.add(c['policy'].warp)
        assert np.isnan(c['x'][c['B']]).all()
        for b, n in enumerate(c['n']):
            assert (c['x'][b, n:] == SENTINEL).all() and c['rec_bare'][b][2:] == [0] * 80 and c['rec_bare'][b][:2] == c['rec'][b][:2]
    assert ds == set(SA_DIMS) and fills == {0, 1} and recipes == set(RECIPES) and warps == {0, 1, 5, 80}
    assert {SETTINGS[s].fm for s in SETTINGS} >= {0, 1, 8} and {SETTINGS[s].tm for s in SETTINGS} >= {0, 2, 32}
    for name, vec in (('stride-160', 4), ('stride-26', 1)):
        c = policy_case(name)
        assert c['T'] * (c['D'] // vec) > APPLY_PASS
    # the warp is on for some utterance of every warped case, and off below 2 W + 1 frames
    for name in CASE_NAMES:
        c = policy_case(name)
        W = c['policy'].warp
        on = [r[0] > 0 for r in c['rec']]
        assert on == [W > 0 and n >= 2 * W + 1 for n in c['n']], name
    # the frequency width is below, at and above D
    assert any(min(SETTINGS[s].fw, D) == D for s in SETTINGS for D in SA_DIMS) and 27 in SA_DIMS and 26 in SA_DIMS


def test_bound_holds_for_the_float32_emulation():
    worst = {False: 0.0, True: 0.0}
    for name in CASE_NAMES:
        c = policy_case(name)
        for b, n in enumerate(c['n']):
            w0, cc = c['rec'][b][:2]
            if w0 <= 0:
                assert np.array_equal(warp32(c['x'][b], n, w0, cc, False), c['x'][b, :n])
                continue
            y64 = warp64(c['x'][b], n, w0, cc)
            bd = warp_bound(c['x'][b], n, w0, cc, y64)
            for fma in (False, True):
                err = np.abs(warp32(c['x'][b], n, w0, cc, fma).astype(np.float64) - y64)
                assert (err[bd == 0.0] == 0.0).all()
                ratio = float((err[bd > 0] / bd[bd > 0]).max(initial=0.0))
                worst[fma] = max(worst[fma], ratio)
                assert ratio <= 1.0, (name, b, fma, ratio)
    print('RATIO warp emulation: mul + add %.4f, fused %.4f (bound 1)' % (worst[False], worst[True]))
    assert worst[False] > 0.05 and worst[True] > 0.05                 # the bound is not slack by orders of magnitude


# ---- create_transform -------------------------------------------------------------------------------------------------------------
AUDIO = {'feat_type': 'fbank', 'feat_dim': 40, 'delta_order': 2}
LD_MAP = {'time_warp': 80, 'freq_masks': 2, 'freq_width': 27, 'time_masks': 2, 'time_width': 100, 'time_ratio': 1.0,
          'time_count_ratio': 0, 'fill': 'mean'}


def test_create_transform_builds_the_policy_stage_from_a_mapping():
    from src.audio import Augment, SpecAugmentPolicy, create_transform
    fe, dim = create_transform(dict(AUDIO, augment=dict(LD_MAP)), 'train')
    assert dim == 120 and [type(s).__name__ for s in fe.stages] == ['ExtractAudioFeature', 'Delta', 'Postprocess', 'SpecAugmentPolicy']
    st = fe.stages[-1]
    assert isinstance(st, SpecAugmentPolicy) and not any(isinstance(s, Augment) for s in fe.stages)
    assert st.policy == {'time_warp': 80, 'freq_masks': 2, 'freq_width': 27, 'time_masks': 2, 'time_width': 100, 'time_ratio_pm': 1000,
                         'time_count_ratio_pm': 0, 'fill': 'mean'}
    assert 'time_warp=80' in repr(fe) and 'fill=mean' in repr(fe)
    fe, _ = create_transform(dict(AUDIO, augment=dict(LD_MAP)), 'eval')
    assert [type(s).__name__ for s in fe.stages] == ['ExtractAudioFeature', 'Delta', 'Postprocess']
    # True / False as before
    fe, _ = create_transform(dict(AUDIO, augment=True), 'train')
    assert [type(s).__name__ for s in fe.stages] == ['ExtractAudioFeature', 'Delta', 'Postprocess', 'Augment']
    assert (fe.stages[-1].T, fe.stages[-1].F) == (40, 27)
    for aug in (False, None):
        fe, _ = create_transform(dict(AUDIO, augment=aug), 'train')
        assert [type(s).__name__ for s in fe.stages] == ['ExtractAudioFeature', 'Delta', 'Postprocess']
    fe, _ = create_transform(dict(AUDIO, augment=True), 'eval')
    assert [type(s).__name__ for s in fe.stages] == ['ExtractAudioFeature', 'Delta', 'Postprocess']
    # defaults: an empty mapping is the identity policy; ratios become per-mille
    fe, _ = create_transform(dict(AUDIO, augment={}), 'train')
    assert fe.stages[-1].policy == {'time_warp': 0, 'freq_masks': 0, 'freq_width': 27, 'time_masks': 0, 'time_width': 100,
                                    'time_ratio_pm': 1000, 'time_count_ratio_pm': 0, 'fill': 'mean'}
    fe, _ = create_transform(dict(AUDIO, augment={'time_masks': 20, 'time_ratio': 0.04, 'time_count_ratio': 0.0405, 'fill': 'zero'}), 'train')
    p = fe.stages[-1].policy
    assert (p['time_masks'], p['time_ratio_pm'], p['time_count_ratio_pm'], p['fill']) == (20, 40, 40, 'zero')


@pytest.mark.parametrize('key,value', [('time_wrap', 5), ('freq_masks', 9), ('time_masks', 33), ('freq_masks', -1), ('time_warp', -1),
                                       ('freq_width', -2), ('time_width', -1), ('time_ratio', 1.5), ('time_ratio', -0.1),
                                       ('time_count_ratio', 1.001), ('time_count_ratio', -1), ('fill', 'median'), ('time_width', 2.5),
                                       ('freq_masks', True)])
def test_create_transform_refuses_bad_policies(key, value):
    from src.audio import create_transform
    for mode in ('train', 'eval'):
        with pytest.raises(ValueError, match=key):
            create_transform(dict(AUDIO, augment={key: value}), mode)


def test_shipped_policy_configs_parse():
    import os
    import yaml
    from src.audio import parse_policy
    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'e2e-asr-pytorch_amd', 'config')
    ld = yaml.safe_load(open(os.path.join(cfg, 'librispeech_asr_ld.yaml')))
    base = yaml.safe_load(open(os.path.join(cfg, 'librispeech_asr.yaml')))
    assert parse_policy(ld['data']['audio']['augment']) == parse_policy(LD_MAP)
    assert base['data']['audio']['augment'] is True
    ld['data']['audio']['augment'] = True
    assert ld == base                                                    # nothing else differs
    dbg = yaml.safe_load(open(os.path.join(cfg, 'debug_specaug.yaml')))
    p = parse_policy(dbg['data']['audio']['augment'])
    assert (p['time_warp'], p['freq_masks'], p['freq_width'], p['time_masks'], p['time_width']) == (5, 2, 8, 2, 10)
    assert dbg['data']['audio']['time_aug'] is False and dbg['data']['corpus']['path'] == 'synthetic-wav'
