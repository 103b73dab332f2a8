"""The yardstick of asr_cmvn (csrc/frontend.hip): a float64 restatement of per-utterance CMVN, its pins, the case table with its
input recipes, and the error bound.  tests/test_hip_cmvn.py imports all of it; nothing here runs a kernel.

  cmvn64       per utterance b and column d over the len = min(lens[b], T) valid frames, in float64 and two passes:
               mean = sum x / len,  std = sqrt(sum (x - mean)^2 / (len - 1)),  y = (x - mean) / (eps + std).
               Rows >= len come back as they went in.  len <= 0: untouched, (mean, std) = (0, 0); len == 1: NaN (0 / 0 under the
               root, as torch.std gives it), mean = the row.  eps is the float32 the C entry point is handed.
               Pins: torch's float64 mean(0) / std(0) on unpadded slices; the reference's own Delta(2,2) -> CMVN -> Postprocess in
               tests/golden/g12_cmvn.npz (written by tests/golden/gen_cmvn_golden.py; the reference runs in float32).

The bound.  With u the unit roundoff of the arithmetic, n = len >= 2, X = max_t |x_t| of the column, s = eps + std64:

      |y - y64|  <=  2^-24 |y64|  +  C n u (X / s) (1 + |y64|),          C = 70

The first term is the one rounding of the result to float32; the second is the arithmetic before it, u = 2^-53 for the kernel.
C comes from the scheme the kernel implements - per-thread Welford, Chan merges of (count, mean, M2) in a fixed order, empty
sides skipped - to first order in u; it is not fitted to anything measured:
  (a) Every mean held anywhere (a thread's, a partial's, a merged one) is the mean of a subset, so it and every difference d
      against it are bounded by X and 2X.  A Welford step  mean += (v - mean) / k  commits three roundings, <= u (2X + 2X/k + X)
      <= 5uX; a merge  ma += (mb - ma) f, f = nb / n,  commits three on a quantity <= 2X and one on the sum, <= 7uX.  Inherited errors
      pass on with weights (1 - 1/k) resp. (na/n, nb/n), which sum to at most 1.  There are n steps and at most n - 1 merges
      of non-empty sides in all, so every mean is off by at most  E = (5n + 7(n-1)) u X <= 12 n u X.
  (b) In exact arithmetic M2 = sum_j w_j d_j^2 over all steps (w = (k-1)/k) and merges (w = na nb / (na + nb)): non-negative
      terms, nothing cancels.  A computed difference is off by <= 2E + u|d_j|, a term by <= 4 E w_j |d_j| + 6u w_j d_j^2.  By
      Cauchy-Schwarz sum w|d| <= sqrt(sum w) sqrt(M2); a step has w < 1, a merge w <= the size of the side that is added, and
      every row is added once per level (lanes, partials): sum w <= 3n.  An element of the sum passes through at most 3n
      additions.  Together  dM2 <= 4E sqrt(3n M2) + (3n + 6) u M2.
  (c) std = sqrt(M2 / (n-1)):  dstd <= dM2 / (2 sqrt((n-1) M2)) + 2u std <= 2 sqrt(3n/(n-1)) E + (1.5n + 5) u std
      <= 4.9 E + 4 n u std, and std <= sqrt(n/(n-1)) X <= 1.42 X, so  dstd <= (4.9 * 12 + 5.7) n u X <= 65 n u X.
  (d) y = (v - mean) / (eps + std):  dy <= E / s + |y| dstd / s + 3u |y|.  For a column with std >= eps, X / s >= 1 / 2.83, so
      3u|y| <= 4.5 n u (X/s) |y|  (columns with std < eps are the constant ones of the recipes, which are held to exactly 0).
      dy <= (12 + 69.5 |y|) n u X / s <= 70 n u (X/s) (1 + |y|).
Against the float32 reference of the fixture the same steps hold with u = 2^-24 for any mean that is a recursive sum over n
(<= n u X <= E) and any M2 formed from differences against it (Welford or two passes): bound(..., u=2^-24).

What the bound excludes.  The one-pass form (sum x^2 - (sum x)^2 / n) / (n - 1) in float64 breaks it on the `jitter` recipe by
orders of magnitude (test_one_pass_sum_of_squares_violates_the_bound): a column that moves by one float32 ulp around its level
has mean^2 / var = 2^48, and n = 600 additions into a sum of squares carry more than 2^-48 of it.  The recipe also puts an
outlier in the first frame, the input on which a shift by x_0 is as poor a guess of the mean as no shift.  What the shifted form
makes of it is printed, not asserted: in float64 its differences on this recipe are small multiples of one ulp and it comes out
near exact.  It is excluded by the rule (its error grows with (x_0 - mean)^2 / var, which no input bounds), not by this case."""
import functools
import os

import numpy as np
import pytest
import torch

U24, U53 = 2.0 ** -24, 2.0 ** -53
C_BOUND = 70.0
EPS = float(np.float32(1e-10))             # CMVN's default as the C entry point receives it
CM_SPLIT, CM_COLS, CM_LANES = 16, 64, 4    # csrc/frontend.hip: partials per utterance, columns per workgroup, rows in flight
SENTINEL = np.float32(-777.25)             # what the padding rows of every GPU case hold


def rows_per_partial(T):
    return (T + CM_SPLIT - 1) // CM_SPLIT


def cmvn64(x, lens, eps=EPS):
    """x (B, T, D), lens (B) -> (y (B, T, D) float64, mean (B, D), std (B, D))."""
    x = np.asarray(x)
    B, T, D = x.shape
    y = x.astype(np.float64)
    mean, std = np.zeros((B, D)), np.zeros((B, D))
    for b in range(B):
        n = max(0, min(int(lens[b]), T))
        if n == 0:
            continue
        v = y[b, :n].copy()
        mean[b] = v.sum(0) / n
        dev = v - mean[b]
        with np.errstate(invalid='ignore', divide='ignore'):
            std[b] = np.sqrt((dev * dev).sum(0) / np.float64(n - 1))
            y[b, :n] = dev / (np.float64(eps) + std[b])
    return y, mean, std


def bound(xv, y64, std64, eps=EPS, u=U53):
    """xv, y64 (n, D): the valid rows of one utterance and their reference; std64 (D) -> the bound per element (n, D)."""
    n = xv.shape[0]
    X = np.abs(np.asarray(xv, dtype=np.float64)).max(0)
    with np.errstate(invalid='ignore'):
        return U24 * np.abs(y64) + C_BOUND * n * u * (X / (np.float64(eps) + std64))[None, :] * (1.0 + np.abs(y64))


def one_pass64(xv, eps=EPS, shift=False):
    """The excluded scheme on the valid rows (n, D): float64 running sums of x and x^2 in frame order (cumsum adds in order),
    optionally of x - x_0."""
    v = np.asarray(xv, dtype=np.float64)
    n = v.shape[0]
    k = v[0] if shift else 0.0
    w = v - k
    s1 = w.cumsum(0)[-1]
    s2 = (w * w).cumsum(0)[-1]
    with np.errstate(invalid='ignore'):
        sd = np.sqrt((s2 - s1 * s1 / n) / (n - 1))
        return (v - (k + s1 / n)) / (eps + sd)


# ---- recipes: the n valid rows (n, D) float32 of utterance b ----------------------------------------------------------------------
def _rng(*key):
    return np.random.Generator(np.random.PCG64(list(key)))


def recipe_integer(b, n, D, seed):
    """Integers whose mean and unbiased variance are exact: column d has mean m_d (an integer up to 2^16 in size) and, for n >= 3,
    an integer std s_d.  Deviations from the mean in units of s = 2, 4, 8 or 16, shuffled per column:
      n even   (3/2, -1/2, -1/2, -1/2, +1, -1, +1, -1, ...)          sum 0, sum of squares n - 1
      n odd    (3/2, -1, -1/2, 1/2, -1/2, +1, -1, ...)               the same
      n == 3   (3, 5, -8) s / 2: std = 7 s / 2, y = 3/7, 5/7, -8/7   (no three dyadic deviations without a zero exist)
      n == 2   (+s, -s): std = s sqrt 2.
    No element sits on the mean: an exact zero would turn one ulp of the float64 mean into a non-zero float32.  For n >= 4 y64 is
    a multiple of 1/2 to within eps / s, so its float32 rounding is out of doubt (test_integer_recipe_is_exact holds the margin
    for every case of the table)."""
    d = np.arange(D)
    m = ((d * 37 + b * 11) % 2001 - 1000).astype(np.float64) + np.where(d % 3 == 1, 2.0 ** 16, 0.0)
    s = 2.0 ** (1 + (d + b) % 4)
    if n <= 1:
        unit = np.zeros(n)
    elif n == 2:
        unit = np.array([1.0, -1.0])
    elif n == 3:
        unit = np.array([1.5, 2.5, -4.0])
    elif n % 2:
        unit = np.concatenate([[1.5, -1.0, -0.5, 0.5, -0.5], np.tile([1.0, -1.0], (n - 5) // 2)])
    else:
        unit = np.concatenate([[1.5, -0.5, -0.5, -0.5], np.tile([1.0, -1.0], (n - 4) // 2)])
    dev = _rng(1, seed, b, n, D).permuted(np.tile(unit[:, None], (1, D)), axis=0)
    x = m[None, :] + dev * s[None, :]
    assert np.array_equal(x, x.astype(np.float32))
    return x.astype(np.float32)


def recipe_normal(b, n, D, seed):
    """Normals with a level and a spread per column (levels up to 50 spreads away from zero)."""
    g = _rng(2, seed, b, n, D)
    d = np.arange(D)
    return (g.standard_normal((n, D)) * (0.1 + (d % 5)) + ((d % 11) - 5.0) * 10.0).astype(np.float32)


def recipe_clamped(b, n, D, seed):
    """What asr_fbank emits: values clamped to [0, 1] with runs of exact zeros (silence) and ones; columns d % 7 == 0 are all
    zero and d % 7 == 3 all one (constant: the output is exactly 0)."""
    g = _rng(3, seed, b, n, D)
    x = np.clip(0.35 + 0.45 * g.standard_normal((n, D)), 0.0, 1.0)
    x[n // 3:n // 2] = 0.0
    d = np.arange(D)
    x[:, d % 7 == 0] = 0.0
    x[:, d % 7 == 3] = 1.0
    return x.astype(np.float32)


JITTER_OUTLIER = 64        # float32 ulps the first frame sits above the column's level


def recipe_jitter(b, n, D, seed):
    """Column d sits at a level L_d in [1, 2) * 2^(d % 5) and moves by one float32 ulp of L_d from frame to frame (0 or 1 ulp,
    at random); the first frame is an outlier, JITTER_OUTLIER ulps above the level."""
    g = _rng(4, seed, b, n, D)
    d = np.arange(D)
    level = (1.0 + ((d * 29 + b) % 64) / 64.0).astype(np.float32).astype(np.float64)
    k = g.integers(0, 2, size=(n, D)).astype(np.float64)
    if n:
        k[0] = JITTER_OUTLIER
    x = (level[None, :] + k * 2.0 ** -23) * (2.0 ** (d % 5))[None, :]
    assert np.array_equal(x, x.astype(np.float32))
    return x.astype(np.float32)


RECIPES = {'integer': recipe_integer, 'normal': recipe_normal, 'clamped': recipe_clamped, 'jitter': recipe_jitter}
CONSTANT_COLUMNS = {'clamped': lambda D: (np.arange(D) % 7 == 0) | (np.arange(D) % 7 == 3)}

# (T, D, lens): B = 6 utterances of mixed lengths; with R = rows_per_partial(T): 0, 1, 2, 3, T, T + 5 (taken as T), R - 1, R, R + 1,
# k R +- 1.  D below, at and past a wave of columns (63, 64, 65), the real widths (120, 240), past one and four tiles (65, 257).
CMVN_SHAPES = [
    (37, 1, [0, 1, 2, 3, 37, 42]),              # R = 3: 2, 3 are R - 1, R
    (64, 3, [3, 4, 5, 64, 69, 31]),             # R = 4: R - 1, R, R + 1, 8R - 1
    (100, 63, [6, 7, 8, 13, 15, 100]),          # R = 7: R - 1, R, R + 1, 2R - 1, 2R + 1
    (100, 64, [0, 1, 50, 48, 105, 99]),         # 7R + 1, 7R - 1
    (129, 65, [8, 9, 10, 1, 134, 2]),           # R = 9: R - 1, R, R + 1
    (600, 120, [37, 38, 39, 600, 605, 303]),    # R = 38: R - 1, R, R + 1, 8R - 1
    (600, 240, [305, 1, 0, 600, 75, 77]),       # 8R + 1, 2R - 1, 2R + 1
    (200, 257, [12, 13, 14, 200, 205, 3]),      # R = 13: R - 1, R, R + 1
]
CMVN_CASES = [(si, name) for si in range(len(CMVN_SHAPES)) for name in RECIPES]


@functools.lru_cache(maxsize=None)
def cmvn_case(si, name):
    """One case, built once and never changed: x (B + 1, T, D) float32 - valid rows from the recipe, SENTINEL in the padding
    rows, NaN in the guard utterance behind the B that are passed - and the float64 reference (y, mean, std) of the first B."""
    T, D, lens = CMVN_SHAPES[si]
    B = len(lens)
    x = np.full((B + 1, T, D), SENTINEL, dtype=np.float32)
    for b, n in enumerate(lens):
        nn = min(n, T)
        x[b, :nn] = RECIPES[name](b, nn, D, si)
    x[B] = np.nan
    y, mean, std = cmvn64(x[:B], lens)
    for a in (x, y, mean, std):
        a.setflags(write=False)
    return {'name': '%s T %d D %d' % (name, T, D), 'T': T, 'D': D, 'lens': list(lens), 'x': x, 'y': y, 'mean': mean, 'std': std,
            'constant': CONSTANT_COLUMNS.get(name, lambda D: np.zeros(D, dtype=bool))(D)}


def judge(c, got, what):
    """got (B, T, D) float32 against case c: padding bit-identical, len == 1 rows NaN, constant columns exactly 0, the integer
    recipe bit for bit, everything else inside the bound -> largest error / bound."""
    worst = 0.0
    name = c['name'].split()[0]
    for b, n in enumerate(c['lens']):
        nn = min(n, c['T'])
        assert np.array_equal(got[b, nn:], c['x'][b, nn:]), (what, c['name'], b, 'padding rows')
        if nn == 0:
            continue
        g, ref = got[b, :nn].astype(np.float64), c['y'][b, :nn]
        if nn == 1:
            assert np.isnan(ref).all() and np.isnan(g).all(), (what, c['name'], b, 'a single frame is NaN in the reference')
            continue
        assert np.isfinite(g).all(), (what, c['name'], b)
        const = c['std'][b] == 0.0                                            # silence, saturation, the recipe's constant columns
        assert (const | ~c['constant']).all()
        assert (g[:, const] == 0.0).all(), (what, c['name'], b, 'constant columns')
        if name == 'integer':
            assert np.array_equal(got[b, :nn], ref.astype(np.float32)), (what, c['name'], b, float(np.abs(g - ref).max()))
        bd = bound(c['x'][b, :nn], ref, c['std'][b])
        ratio = np.abs(g - ref)[:, ~const] / bd[:, ~const]
        if ratio.size:
            worst = max(worst, float(ratio.max()))
            assert (ratio <= 1.0).all(), (what, c['name'], b, n, float(ratio.max()))
    return worst


# =================================================================================================================================
# pins
# =================================================================================================================================
@pytest.fixture(scope='module')
def g12(golden_dir):
    return np.load(os.path.join(golden_dir, 'g12_cmvn.npz'))


def test_cmvn64_is_torch_mean_and_unbiased_std_on_unpadded_slices():
    for si, name in CMVN_CASES:
        c = cmvn_case(si, name)
        for b, n in enumerate(c['lens']):
            nn = min(n, c['T'])
            if nn < 2:
                continue
            v = torch.from_numpy(c['x'][b, :nn].astype(np.float64))
            mean, std = v.mean(0).numpy(), v.std(0).numpy()
            assert np.abs(c['mean'][b] - mean).max() <= 1e-12 * max(1.0, np.abs(mean).max())
            assert np.abs(c['std'][b] - std).max() <= 1e-9 * std.max() + 1e-300, (c['name'], b)
            assert ((c['std'][b] == 0.0) == (std == 0.0)).all()
            nz = c['std'][b] != 0.0
            want = ((v - v.mean(0)) / (EPS + v.std(0))).numpy()
            tol = 1e-9 * (1.0 + np.abs(want)) if name != 'jitter' else 1e-6 * (1.0 + np.abs(want))     # torch's own float64 rounding
            assert (np.abs(c['y'][b, :nn] - want)[:, nz] <= tol[:, nz]).all(), (c['name'], b)


def test_cmvn64_edges():
    x = np.arange(24, dtype=np.float32).reshape(2, 4, 3) ** 2
    y, mean, std = cmvn64(x, [0, 1])
    assert np.array_equal(y[0], x[0]) and (mean[0] == 0).all() and (std[0] == 0).all()
    assert np.isnan(y[1, 0]).all() and np.array_equal(y[1, 1:], x[1, 1:])
    assert np.array_equal(mean[1], x[1, 0]) and np.isnan(std[1]).all()
    y, mean, std = cmvn64(x, [9, -3])                                        # beyond T is T; below 0 is 0
    assert np.array_equal(y[1], x[1]) and np.allclose(y[0].mean(0), 0.0, atol=1e-15)
    assert np.allclose(y[0].std(0, ddof=1), 1.0, atol=1e-9)
    c = np.full((1, 5, 2), 0.25, dtype=np.float32)
    assert (cmvn64(c, [5])[0] == 0.0).all()


def test_integer_recipe_is_exact():
    """mean and std of the integer recipe are the integers it was built from; no y64 is zero; and every y64 of the case table
    keeps its float32 rounding under a relative change of 1e-9, a hundred times what float64 moments of these sizes can move it."""
    for n in (3, 4, 5, 38, 600):
        x = recipe_integer(2, n, 65, 0)[None]
        y, mean, std = cmvn64(x, [n])
        d = np.arange(65)
        assert np.array_equal(std[0], 2.0 ** (1 + (d + 2) % 4) * (3.5 if n == 3 else 1.0))
        assert np.array_equal(mean[0], np.round(mean[0]))
        if n > 3:
            near = np.round(y[0] * 2) / 2
            assert set(np.unique(near)) <= {-1.0, -0.5, 0.5, 1.0, 1.5}
            assert np.abs(y[0] - near).max() <= 1e-10
    for si in range(len(CMVN_SHAPES)):
        c = cmvn_case(si, 'integer')
        for b, n in enumerate(c['lens']):
            nn = min(n, c['T'])
            if nn < 2:
                continue
            y = c['y'][b, :nn]
            assert (y != 0.0).all()
            r = y.astype(np.float32)
            assert np.array_equal((y * (1 + 1e-9)).astype(np.float32), r) and np.array_equal((y * (1 - 1e-9)).astype(np.float32), r)


def test_fixture_pins_cmvn64_and_the_reference_stays_inside_the_float32_bound(g12):
    """Delta's float32 output as the reference handed it to its CMVN -> cmvn64, against what the reference made of it."""
    worst = 0.0
    for i in range(int(g12['n'])):
        T = int(g12['len%d' % i])
        d = g12['delta%d' % i]                                                # (C, F, T)
        x = d.transpose(2, 0, 1).reshape(1, T, -1)                            # Postprocess's layout: (T, C F), channel-major
        y, mean, std = cmvn64(x, [T], eps=float(g12['eps']))
        out = g12['out%d' % i].astype(np.float64)
        assert out.shape == y[0].shape
        if T == 1:
            assert np.isnan(out).all() and np.isnan(y[0]).all()               # the reference's single frame
            continue
        bd = bound(x[0], y[0], std[0], eps=float(g12['eps']), u=U24)
        ratio = np.abs(out - y[0]) / bd
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (i, float(ratio.max()))
        np.testing.assert_allclose(out, y[0], atol=2e-5, rtol=2e-5)           # and plainly: it is the same function
    print('RATIO reference (float32) vs cmvn64, bound at u = 2^-24: %.4f' % worst)
    assert [int(g12['len%d' % i]) for i in range(int(g12['n']))] == [5, 17, 40, 1]


def test_case_table_covers_what_it_claims():
    widths = sorted({D for _, D, _ in CMVN_SHAPES})
    assert widths == [1, 3, 63, 64, 65, 120, 240, 257]
    seen = set()
    for T, D, lens in CMVN_SHAPES:
        assert len(lens) <= 6 and T <= 600
        R = rows_per_partial(T)
        for n in lens:
            for tag, v in (('0', 0), ('1', 1), ('2', 2), ('3', 3), ('T', T), ('T+5', T + 5), ('R-1', R - 1), ('R', R), ('R+1', R + 1)):
                if n == v:
                    seen.add(tag)
            if n > R + 1 and n < T and (n + 1) % R == 0:
                seen.add('kR-1')
            if n > R + 1 and n < T and (n - 1) % R == 0:
                seen.add('kR+1')
    assert seen == {'0', '1', '2', '3', 'T', 'T+5', 'R-1', 'R', 'R+1', 'kR-1', 'kR+1'}, seen
    for si, name in CMVN_CASES:
        c = cmvn_case(si, name)
        assert np.isnan(c['x'][-1]).all()
        for b, n in enumerate(c['lens']):
            assert (c['x'][b, min(n, c['T']):] == SENTINEL).all()


def test_cmvn64_sits_well_inside_the_bound():
    """cmvn64 against itself in higher precision (numpy longdouble, two passes): a hundredth of the bound at most."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, 'numpy longdouble is no wider than float64 on this host'
    worst = 0.0
    for si, name in CMVN_CASES:
        c = cmvn_case(si, name)
        for b, n in enumerate(c['lens']):
            nn = min(n, c['T'])
            if nn < 2:
                continue
            v = c['x'][b, :nn].astype(np.longdouble)
            mean = v.sum(0) / nn
            dev = v - mean
            sd = np.sqrt((dev * dev).sum(0) / (nn - 1))
            want = (dev / (np.longdouble(EPS) + sd)).astype(np.float64)
            nz = c['std'][b] != 0.0
            bd = bound(c['x'][b, :nn], c['y'][b, :nn], c['std'][b])
            ratio = np.abs(c['y'][b, :nn] - want)[:, nz] / bd[:, nz]
            worst = max(worst, float(ratio.max(initial=0.0)))
    print('RATIO cmvn64 vs extended precision: %.5f' % worst)
    assert worst <= 0.01


def test_one_pass_sum_of_squares_violates_the_bound():
    """The jitter case bites: float64 running sums of x and x^2 break the bound on the long utterances of the jitter recipe, by
    orders of magnitude; on the normal recipe at the same shape they do not (so it is the case, not the bound, that excludes
    them)."""
    si = 5
    for name, expect in (('jitter', True), ('normal', False)):
        c = cmvn_case(si, name)
        for b, n in enumerate(c['lens']):
            nn = min(n, c['T'])
            if nn < 300:
                continue
            xv, ref = c['x'][b, :nn], c['y'][b, :nn]
            bd = bound(xv, ref, c['std'][b])
            with np.errstate(invalid='ignore'):
                r0 = np.abs(one_pass64(xv) - ref) / bd
                r1 = np.abs(one_pass64(xv, shift=True) - ref) / bd
            bad = ~(r0 <= 1.0)                                                # NaN (a negative variance) is a violation too
            print('RATIO one-pass float64 on %-20s b %d n %3d: plain %.3g (%.0f %% of the elements outside), shifted by x_0 %.3g'
                  % (c['name'], b, nn, np.nanmax(r0), 100.0 * bad.mean(), np.nanmax(r1)))
            if expect:
                assert bad.mean() > 0.5 and np.nanmax(r0) > 100.0, (c['name'], b)
            else:
                assert not bad.any()
