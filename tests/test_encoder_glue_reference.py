"""The yardstick of the bf16 encoder glue (csrc/elementwise16.hip) and of the fp32 dropout kernels (csrc/elementwise.hip): plain
numpy restatements of every operation, written from the header comments of include/asr_hip.h, the case tables, and the CPU
checks of both.  tests/test_hip_encoder_glue_vs_float64.py imports them; nothing here imports the code under test.

Almost everything is a data movement or a single rounding, so the restatements are EXACT: the GPU module compares bits.

Operations
  philox_blocks   Philox4x32-10 (Salmon et al., SC'11) vectorised over 64-bit block indices: counter (lo, hi, 0, 0), key
                  (seed lo, seed hi).  Pinned to the scalar philox4x32_10 of tests/test_beam_step_reference.py, which is pinned to
                  the published known answers, on blocks below and above 2^32 and seeds with and without a high word.
  keep_mask       element i is kept iff word i & 3 of block i >> 2 is >= floor(float32(p) 2^32) saturated at 2^32 - 1; p <= 0
                  keeps everything.  drop_scale(p) is the float32 quotient 1 / (1 - p).
  downsample_ref / downsample_bwd_ref   style 0: z[b,t2,:] = drop(y)[b, t2 rate, :]; style 1: z[b,t2,i D + :] = drop(y)[b, t2 rate + i, :];
                  kept values are the float32 product y scale (bf16 form: rounded to bf16, nearest-even); the backward writes all
                  of dy, +0 where nothing flowed.
  bf16_bits       float32 -> bfloat16 bit patterns, nearest-even, subnormals rounded like everything else; pinned to torch.
  pack_ref        asr_rnn_pack_weights: destination row d 4H + 4u + g <- source row d 4H + g H + u, bf16 values, the transpose with
                  the same values, the float32 sum b_ih + b_hh in destination order, pj16 = bf16(pj) and its transpose.
  colsum_perm     the column a sum lands in when perm_h > 0 (gate-minor column -> reference row); rows_per_block restates the host
                  rule, only to show which of its values a case takes.
  act_bwd16_ref   bf16(g (1 - o o)) resp. bf16(o > 0 ? g : 0), the float32 expression.

Block indices >= 2^32 of the device Philox would need a 64 GB tensor; they are covered by philox_blocks on the CPU only.
"""
import math

import numpy as np
import torch

from test_beam_step_reference import philox4x32_10

F32 = np.float32
ACT_TANH, ACT_RELU = 1, 2
P_MAX = float(np.nextafter(F32(1), F32(0)))            # the largest float32 below 1
SEEDS = [99, 0x9E3779B97F4A7C15]
M32 = np.uint64(0xffffffff)


# ---------------------------------------------------------------------------------------------------------------------
# Philox and the dropout map
# ---------------------------------------------------------------------------------------------------------------------
def philox_blocks(blk, seed):
    """blk: array of block indices (any integer dtype, < 2^64) -> (len, 4) uint32 words."""
    blk = np.asarray(blk, dtype=np.uint64)
    c0, c1 = blk & M32, blk >> np.uint64(32)
    c2, c3 = np.zeros_like(blk), np.zeros_like(blk)
    k0, k1 = int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2          # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & M32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return np.stack([c0, c1, c2, c3], 1).astype(np.uint32)


def drop_thresh(p):
    p = F32(p)
    if p <= 0:
        return 0
    return min(int(math.floor(float(p) * 4294967296.0)), 4294967295)            # float32(p) 2^32 is exact in float64


def drop_scale(p):
    return F32(1) / (F32(1) - F32(p))


_MASKS = {}


def keep_mask(n, p, seed):
    """-> bool (n,), computed once per (n, p, seed)."""
    key = (int(n), float(F32(p)), int(seed))
    if key not in _MASKS:
        th = drop_thresh(p)
        if th == 0:
            m = np.ones(n, dtype=bool)
        else:
            m = philox_blocks(np.arange((n + 3) // 4, dtype=np.uint64), seed).reshape(-1)[:n] >= np.uint32(th)
        m.setflags(write=False)
        if len(_MASKS) > 64:
            _MASKS.clear()
        _MASKS[key] = m
    return _MASKS[key]


def out_frames(T, rate, style):
    """The caller's T2 (src/functions.py::out_frames): 'drop' keeps ceil(T / rate) frames, 'concat' stacks T // rate groups."""
    if rate == 1:
        return T
    return (T + rate - 1) // rate if style == 0 else T // rate


def t2_is_legal(T, T2, rate, style):
    return T2 >= 1 and ((T2 - 1) * rate < T if style == 0 else T2 * rate <= T)


def selected_rows(T, T2, rate, style):
    """bool (T,): the time rows of y the forward reads."""
    t = np.arange(T)
    return ((t % rate == 0) & (t // rate < T2)) if style == 0 else (t < T2 * rate)


def downsample_ref(y, mask, scale, rate, style, T2):
    """y (B,T,D), mask bool (B,T,D), scale a scalar of y's dtype -> z (B,T2,D) resp. (B,T2,rate D) in y's dtype.  Rows of y that
    are not selected are not looked at (they may hold NaN)."""
    B, T, D = y.shape
    assert t2_is_legal(T, T2, rate, style)
    sel = selected_rows(T, T2, rate, style)
    ys, ms = y[:, sel], mask[:, sel]
    with np.errstate(over='ignore', invalid='ignore'):
        d = np.where(ms, ys * y.dtype.type(scale), y.dtype.type(0))
    return d if style == 0 else d.reshape(B, T2, rate * D)


def downsample_bwd_ref(dz, mask, scale, rate, style, T):
    """dz (B,T2,Dz) -> dy (B,T,D): dz scale where the element was selected and kept, +0 elsewhere."""
    B, T2 = dz.shape[0], dz.shape[1]
    D = mask.shape[2]
    sel = selected_rows(T, T2, rate, style)
    g = np.zeros((B, T, D), dtype=dz.dtype)
    g[:, sel] = dz.reshape(B, -1, D)
    with np.errstate(over='ignore', invalid='ignore'):
        return np.where(mask & sel[None, :, None], g * dz.dtype.type(scale), dz.dtype.type(0))


# ---------------------------------------------------------------------------------------------------------------------
# bfloat16
# ---------------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """float32 array -> uint16 bfloat16 patterns: nearest, ties to even, on the bit pattern (so subnormals round like every
    other value and FLT_MAX carries into infinity); NaN -> a quiet NaN of the same sign."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7fff) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    nan = (u & np.uint64(0x7fffffff)) > np.uint64(0x7f800000)
    return np.where(nan, ((u >> np.uint64(16)) | np.uint64(0x40)).astype(np.uint16), r)


def bf16_value(bits):
    """uint16 patterns -> float32 values."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(F32)


def bf16_round(x):
    return bf16_value(bf16_bits(x))


# fp32 inputs of asr_cast_bf16 that randn never produces.  -0 comes first: the shortest cases hold nothing else.
SPECIAL_F32 = np.array([-0.0, 0.0,
                        1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8),          # ties: down / up to even
                        1 + 2.0 ** -8 + 2.0 ** -23, -(1 + 2.0 ** -8 + 2.0 ** -23),                          # one ulp above a tie
                        1 + 2.0 ** -8 - 2.0 ** -23,                                                          # one ulp below
                        float(np.finfo(F32).max), -float(np.finfo(F32).max),                                 # -> infinity
                        float(np.array([0x7f7f8000], dtype=np.uint32).view(F32)[0]),                         # the tie above the largest bf16: -> infinity
                        float(np.array([0x7f7f7fff], dtype=np.uint32).view(F32)[0]),                         # one ulp below it: stays finite
                        float('inf'), float('-inf'),
                        2.0 ** -126, -2.0 ** -126,                                                           # the smallest normal
                        2.0 ** -127, 2.0 ** -133, 3 * 2.0 ** -134, 2.0 ** -134, 2.0 ** -149, -2.0 ** -140,     # subnormals (a bf16 one, ties, the smallest)
                        float('nan')], dtype=F32)
SPECIAL_SUBNORMAL = (np.abs(SPECIAL_F32) < 2.0 ** -126) & (SPECIAL_F32 != 0)
# bf16 inputs of asr_cast_f32: signed zeros, infinities, the extremes, subnormals, NaN
SPECIAL_BF16 = np.array([0x8000, 0x0000, 0x7f80, 0xff80, 0x7f7f, 0xff7f, 0x0080, 0x8080, 0x0001, 0x8001, 0x007f, 0x3f80, 0xbf81, 0x7fc0],
                        dtype=np.uint16)
CAST_N = [1, 7, 8, 9, 16, 1003, 8388608, 8388608 + 2048 + 3]


def cast_inputs(n):
    """fp32 source of asr_cast_bf16 (specials tiled over the first and the last 32 elements, so that the n & 7 tail of every n holds
    some), the bf16 source of asr_cast_f32 likewise, and the random start values of accum = 1."""
    g = np.random.default_rng(7100 + n % 1009)
    src = g.standard_normal(n).astype(F32)
    src16 = bf16_bits(g.standard_normal(n).astype(F32))
    for lo in ((0, n - 32) if n > 64 else (0,)):
        k = min(32, n - lo)
        src[lo:lo + k] = SPECIAL_F32[np.arange(k) % len(SPECIAL_F32)]
        src16[lo:lo + k] = SPECIAL_BF16[np.arange(k) % len(SPECIAL_BF16)]
    return src, src16, g.standard_normal(n).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# packing of an RNN layer's weights
# ---------------------------------------------------------------------------------------------------------------------
# (H, ND, Din, D or None = no projection)
# (5, 2, 7, None): without a projection AND with H > 1 - at H = 1 the row permutation is the identity
PACK_CASES = [(1, 1, 1, None), (5, 2, 7, None), (3, 2, 5, 6), (16, 2, 24, 32), (20, 1, 33, 20), (48, 2, 70, 96), (320, 2, 640, 640)]


def pack_rows(H, ND):
    """src[r] = the reference row (d 4H + g H + u) that destination row r = d 4H + 4u + g holds."""
    r = np.arange(ND * 4 * H)
    d, rr = r // (4 * H), r % (4 * H)
    return d * 4 * H + (rr % 4) * H + rr // 4


def pack_ref(w_ih, b_ih, b_hh, pj, H, ND):
    src = pack_rows(H, ND)
    w16 = bf16_bits(w_ih[src])
    out = dict(wih16=w16, wihT16=np.ascontiguousarray(w16.T), bias=(b_ih + b_hh)[src].astype(F32))
    if pj is not None:
        out['pj16'] = bf16_bits(pj)
        out['pjT16'] = np.ascontiguousarray(out['pj16'].T)
    return out


def pack_inputs(case):
    H, ND, Din, D = case
    g = np.random.default_rng(7200 + PACK_CASES.index(case))
    G = ND * 4 * H
    w = g.standard_normal((G, Din)).astype(F32)
    w.reshape(-1)[:6] = SPECIAL_F32[2:8][:w.size]                                  # rounding ties among the weights
    pj = None if D is None else g.standard_normal((D, D)).astype(F32)
    return dict(w_ih=w, b_ih=g.standard_normal(G).astype(F32), b_hh=g.standard_normal(G).astype(F32), pj=pj)


def pack_jobs(case):
    """32 x 32 tiles the kernel walks (its workgroups stride over them by 1024)."""
    H, ND, Din, D = case
    t = lambda n: (n + 31) // 32
    return t(ND * 4 * H) * t(Din) + (0 if D is None else t(D) ** 2)


# ---------------------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------------------
COLSUM_M = [1, 7, 8, 9, 16, 17, 33, 300]
COLSUM_N = [8, 64, 248, 256, 264]
COLSUM_BIG = [(6600, 2560), (13100, 2560)]


def colsum_perm(N, perm_h):
    """dst[c] = the output column the sum of input column c is added to."""
    c = np.arange(N)
    if perm_h == 0:
        return c
    assert N % (4 * perm_h) == 0
    h4 = 4 * perm_h
    blk, rr = c // h4, c % h4
    return blk * h4 + (rr % 4) * perm_h + rr // 4


def rows_per_block(M, N):
    cdiv = lambda a, b: (a + b - 1) // b
    rpb = 512
    while rpb > 32 and cdiv(N, 256) * cdiv(M, rpb) < 1024:
        rpb >>= 1
    return rpb


def colsum_inputs(M, N, lda, recipe):
    """A (M, lda) float32 holding bf16 values, columns past N poisoned with NaN, and two start vectors.  'integer': A in [-4, 4],
    starts in [-64, 64], so every partial sum is an integer below 2^24; 'random': bf16-rounded normals, fp32 normal starts."""
    g = torch.Generator().manual_seed(7300 + 31 * (M % 997) + N + (lda - N) + (0 if recipe == 'integer' else 5))
    if recipe == 'integer':
        A = torch.randint(-4, 5, (M, lda), generator=g).to(torch.float32)
        o1, o2 = [torch.randint(-64, 65, (N,), generator=g).to(torch.float32) for _ in range(2)]
    else:
        A = torch.randn(M, lda, generator=g).to(torch.bfloat16).to(torch.float32)
        o1, o2 = torch.randn(N, generator=g), torch.randn(N, generator=g)
    A[:, N:] = float('nan')
    return A, o1, o2


# ---------------------------------------------------------------------------------------------------------------------
# activation backward
# ---------------------------------------------------------------------------------------------------------------------
ACT_N = [8, 16, 2048, 8 * 1048576 + 8 * 257]
BF16_TINY = float(bf16_value([0x0001])[0])               # the smallest positive bf16 (a subnormal)


def act_bwd16_ref(g, o, act):
    """g, o float32 arrays of bf16 values -> bf16 patterns of the float32 expression."""
    if act == ACT_TANH:
        return bf16_bits(g * (F32(1) - o * o))
    return bf16_bits(np.where(o > 0, g, F32(0)))


def act_inputs(n, act):
    g = np.random.default_rng(7400 + n % 1009 + act)
    gr = bf16_round(g.standard_normal(n).astype(F32))
    if act == ACT_TANH:
        o = bf16_round(np.tanh(3 * g.standard_normal(n)).astype(F32))
        o[:4] = [1.0, -1.0, 0.0, -0.0]
    else:
        o = bf16_round(np.maximum(g.standard_normal(n), 0).astype(F32))            # what a ReLU leaves: half of it exact zeros
        o[:8] = [0.0, -0.0, BF16_TINY, -BF16_TINY, -1.5, 2.0 ** -126, -2.0 ** -126, 3.0]
    return gr, o


# ---------------------------------------------------------------------------------------------------------------------
# dropout case tables
# ---------------------------------------------------------------------------------------------------------------------
DROP_B, DROP_T, DROP_RATES, DROP_P = [1, 3], [1, 2, 5, 11], [1, 2, 3], [0.0, 0.3, 0.5, P_MAX]
DROP_D32, DROP_D16 = [4, 5, 8, 24], [8, 24, 320]
DROP_SHAPES32 = [(B, T, D) for B in DROP_B for T in DROP_T for D in DROP_D32]
DROP_SHAPES16 = [(B, T, D) for B in DROP_B for T in DROP_T for D in DROP_D16]
# grid-stride cases (B, T, D, rate, style): work items beyond the capped grid of 4096 x 256 threads
DROP_BIG_VEC4 = (4, 1030, 1024, 2, 0)
DROP_BIG_SCALAR = (3, 70001, 5, 3, 1)
DROP_BIG_16 = (4, 2050, 1024, 2, 0)
GRID_CAP = 4096 * 256


def drop_variants(T):
    """(rate, style, T2) of a shape: the caller's T2 and one less where that is >= 1."""
    out = []
    for rate in DROP_RATES:
        for style in (0, 1):
            t2 = out_frames(T, rate, style)
            out += [(rate, style, v) for v in (t2, t2 - 1) if v >= 1]
    return out


def drop_inputs(B, T, D, T2, rate, style, tag=0, rounded=True):
    """y (B,T,D) float32 normals and dz of the matching shape.  rounded: bf16 values, for the bf16 kernels; the fp32 kernels get
    full 24-bit significands, so that the float32 product y scale really rounds (a division by 1 - p would differ)."""
    g = np.random.default_rng(7500 + 1000 * tag + 97 * B + 13 * T + D + 7 * rate + style + 3 * T2)
    y = g.standard_normal((B, T, D)).astype(F32)
    dz = g.standard_normal((B, T2, D if style == 0 else rate * D)).astype(F32)
    return (bf16_round(y), bf16_round(dz)) if rounded else (y, dz)


# ---------------------------------------------------------------------------------------------------------------------
# CPU checks
# ---------------------------------------------------------------------------------------------------------------------
def test_philox_blocks_is_philox4x32_10():
    blocks = [0, 1, 2, 0xffffffff, 1 << 32, (1 << 32) + 5, 0x123456789abcdef, (1 << 64) - 1]
    for seed in SEEDS + [0, 77, 0xffffffffffffffff, 1 << 32]:
        got = philox_blocks(blocks, seed)
        for b, row in zip(blocks, got):
            want = philox4x32_10((b & 0xffffffff, b >> 32, 0, 0), (seed & 0xffffffff, seed >> 32))
            assert tuple(int(v) for v in row) == want, (b, seed)
    # the published known answer of Random123 (counter and key all zero)
    assert [int(v) for v in philox_blocks([0], 0)[0]] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    # both key words matter, and so does the high counter word
    assert not np.array_equal(philox_blocks([3], SEEDS[1]), philox_blocks([3], SEEDS[1] & 0xffffffff))
    assert not np.array_equal(philox_blocks([3], SEEDS[1]), philox_blocks([3], (SEEDS[1] & 0xffffffff) * 0x100000001))
    assert not np.array_equal(philox_blocks([1 << 32], 99), philox_blocks([0], 99))
    assert SEEDS[1] >> 32 != 0 and SEEDS[0] >> 32 == 0


def test_threshold_scale_and_keep_rate():
    assert drop_thresh(0.0) == 0 and drop_thresh(-1.0) == 0
    assert drop_thresh(0.5) == 1 << 31
    assert drop_thresh(0.3) == int(math.floor(float(F32(0.3)) * 2 ** 32)) == 1288490240
    assert drop_thresh(P_MAX) == 2 ** 32 - 256 and P_MAX == 1 - 2.0 ** -24
    assert drop_thresh(1.0) == 4294967295                                           # saturates (the entry points refuse p = 1)
    assert drop_scale(0.0) == 1 and drop_scale(0.5) == 2 and drop_scale(P_MAX) == 2.0 ** 24
    assert drop_scale(0.3) == F32(1) / F32(0.7) and drop_scale(0.3).dtype == F32
    assert float(drop_scale(0.3)) != 1 / (1 - 0.3)                                  # not the float64 quotient
    n = 10 ** 6
    for p in (0.3, 0.5):
        for seed in SEEDS:
            rate = float(keep_mask(n, p, seed).mean())
            assert abs(rate - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n), (p, seed, rate)
    assert keep_mask(1000, 0.0, 99).all()
    assert int(keep_mask(n, P_MAX, 99).sum()) <= 4                                  # expectation 2^-24 n = 0.06
    # element i reads word i & 3 of block i >> 2
    w = philox_blocks([0, 1, 2], SEEDS[1]).reshape(-1)
    assert np.array_equal(keep_mask(11, 0.5, SEEDS[1]), w[:11] >= np.uint32(1 << 31))
    assert not np.array_equal(keep_mask(4096, 0.5, SEEDS[1]), keep_mask(4096, 0.5, SEEDS[1] & 0xffffffff))


def _torch_downsample(y, rate, style, T2):
    B, T, D = y.shape
    return y[:, ::rate][:, :T2] if style == 0 else y[:, :T2 * rate].reshape(B, T2, rate * D)


def test_downsample_refs():
    for (B, T, D) in [(1, 1, 4), (3, 5, 5), (3, 11, 8), (1, 2, 24)]:
        for (rate, style, T2) in drop_variants(T):
            y, dz = drop_inputs(B, T, D, T2, rate, style)
            ones = np.ones((B, T, D), dtype=bool)
            # p = 0: plain indexing
            assert np.array_equal(downsample_ref(y, ones, F32(1), rate, style, T2), _torch_downsample(torch.from_numpy(y), rate, style, T2).numpy())
            for p in (0.3, P_MAX):
                mask = keep_mask(B * T * D, p, SEEDS[1]).reshape(B, T, D)
                sc = drop_scale(p)
                # rows that are not selected are not looked at
                yn = y.copy()
                yn[:, ~selected_rows(T, T2, rate, style)] = np.nan
                z = downsample_ref(yn, mask, sc, rate, style, T2)
                assert not np.isnan(z).any() and z.dtype == F32
                assert np.array_equal(z, _torch_downsample(torch.from_numpy(np.where(mask, y * sc, F32(0))), rate, style, T2).numpy())
                # the backward is the float64 autograd of the forward
                yt = torch.from_numpy(y.astype(np.float64)).requires_grad_(True)
                zt = _torch_downsample(yt * torch.from_numpy(mask.astype(np.float64)) * float(sc), rate, style, T2)
                zt.backward(torch.from_numpy(dz.astype(np.float64)))
                got = downsample_bwd_ref(dz.astype(np.float64), mask, float(sc), rate, style, T)
                assert np.array_equal(got, yt.grad.numpy()) and got.shape == (B, T, D)
                d32 = downsample_bwd_ref(dz, mask, sc, rate, style, T)
                assert d32.dtype == F32 and not np.signbit(d32[d32 == 0] if p == P_MAX else d32[~mask]).any()          # unreached elements are +0
    # the fp32 inputs are not bf16 values, and there the product by the float32 scale is not the quotient by 1 - p
    y, _ = drop_inputs(3, 11, 24, 11, 1, 0, rounded=False)
    assert not np.array_equal(bf16_round(y), y)
    assert float(((y * drop_scale(0.3)) != (y / (F32(1) - F32(0.3)))).mean()) > 0.05
    assert drop_variants(1) == [(1, 0, 1), (1, 1, 1), (2, 0, 1), (3, 0, 1)]          # concat of one frame at rate 2 has no output
    assert drop_variants(5) == [(1, 0, 5), (1, 0, 4), (1, 1, 5), (1, 1, 4), (2, 0, 3), (2, 0, 2), (2, 1, 2), (2, 1, 1), (3, 0, 2), (3, 0, 1), (3, 1, 1)]
    for T in DROP_T:
        for (rate, style, T2) in drop_variants(T):
            assert t2_is_legal(T, T2, rate, style)
            assert not t2_is_legal(T, out_frames(T, rate, style) + 1, rate, style)
    # the grid-stride cases need a second pass of the capped grid
    B, T, D, _, _ = DROP_BIG_VEC4
    assert B * T * D // 4 > GRID_CAP and D % 4 == 0
    B, T, D, _, _ = DROP_BIG_SCALAR
    assert B * T * D > GRID_CAP and D % 4 != 0
    B, T, D, _, _ = DROP_BIG_16
    assert B * T * D // 8 > GRID_CAP and D % 8 == 0


def test_bf16_bits_is_nearest_even():
    g = np.random.default_rng(1)
    x = np.concatenate([g.standard_normal(100000).astype(F32) * F32(10.0) ** g.integers(-30, 30, 100000).astype(F32),
                        g.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(F32), SPECIAL_F32])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = bf16_bits(x)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.isnan(bf16_value(got[nan])).all() and nan.sum() > 0
    v = bf16_round(SPECIAL_F32)
    assert v[:9].tolist() == [-0.0, 0.0, 1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6), 1 + 2.0 ** -7, -(1 + 2.0 ** -7), 1.0]
    assert np.signbit(v[0]) and not np.signbit(v[1])
    assert v[9:15].tolist() == [np.inf, -np.inf, np.inf, float(bf16_value([0x7f7f])[0]), np.inf, -np.inf]
    assert v[15:17].tolist() == [2.0 ** -126, -2.0 ** -126]
    # subnormals: 2^-127 and 2^-133 are bf16 values; 3 2^-134 ties up to even (2^-132), 2^-134 ties down to even (0); 2^-149 -> 0
    # and -2^-140 -> -0
    assert v[17:23].tolist() == [2.0 ** -127, 2.0 ** -133, 2.0 ** -132, 0.0, 0.0, 0.0] and np.signbit(v[22]) and not np.signbit(v[21])
    assert int(SPECIAL_SUBNORMAL.sum()) == 6 and np.array_equal(np.nonzero(SPECIAL_SUBNORMAL)[0], np.arange(17, 23))
    assert np.array_equal(bf16_bits(bf16_value(SPECIAL_BF16[:-1])), SPECIAL_BF16[:-1])          # bf16 values pass through
    for n in CAST_N:
        src, src16, init = cast_inputs(n)
        assert src.shape == (n,) and src16.dtype == np.uint16
        tail = src[n - (n & 7):]
        assert (n & 7) == 0 or np.signbit(tail[tail == 0]).any() or n > 64 or n == 9          # a -0 sits in the short tails
    assert (CAST_N[-1] // 8 + 1 + 255) // 256 > 4096 and (CAST_N[-2] // 8 + 1 + 255) // 256 > 4096          # second grid-stride pass


def test_pack_ref():
    for case in PACK_CASES:
        H, ND, Din, D = case
        c = pack_inputs(case)
        r = pack_ref(c['w_ih'], c['b_ih'], c['b_hh'], c['pj'], H, ND)
        G = ND * 4 * H
        assert r['wih16'].shape == (G, Din) and r['wihT16'].shape == (Din, G) and r['bias'].shape == (G,)
        src = pack_rows(H, ND)
        assert sorted(src.tolist()) == list(range(G))
        # written out: destination d 4H + 4u + g <- source d 4H + g H + u
        for d in range(ND):
            for u in (0, H - 1):
                for gt in range(4):
                    assert src[d * 4 * H + 4 * u + gt] == d * 4 * H + gt * H + u
        # x @ packed^T read as (ND, H, 4) == x @ W_ih^T read as (ND, 4, H), in float64
        x = np.random.default_rng(2).standard_normal((3, Din))
        w16 = bf16_value(bf16_bits(c['w_ih'])).astype(np.float64)
        a = (x @ bf16_value(r['wih16']).astype(np.float64).T).reshape(3, ND, H, 4)
        b = (x @ w16.T).reshape(3, ND, 4, H)
        assert np.array_equal(a, b.transpose(0, 1, 3, 2))
        assert np.array_equal(r['bias'].reshape(ND, H, 4), (c['b_ih'] + c['b_hh']).reshape(ND, 4, H).transpose(0, 2, 1))
        assert (D is None) == ('pj16' not in r)
        if D is not None:
            assert np.array_equal(r['pjT16'].T, r['pj16']) and np.array_equal(r['pj16'], bf16_bits(c['pj']))
    assert pack_jobs(PACK_CASES[-1]) == 2000 and pack_jobs(PACK_CASES[-1]) > 1024
    assert [pack_jobs(c) for c in PACK_CASES[:-1]] == [1, 2, 2, 5, 7, 45]
    assert any(c[3] is None and c[0] > 1 and not np.array_equal(pack_rows(c[0], c[1]), np.arange(c[1] * 4 * c[0])) for c in PACK_CASES)
    assert any(c[2] % 32 and (c[1] * 4 * c[0]) % 32 for c in PACK_CASES)            # Din and G both off the 32 x 32 tile


def test_colsum_tables():
    seen = set()
    for M in COLSUM_M:
        for N in COLSUM_N:
            seen.add(rows_per_block(M, N))
            assert N % 8 == 0 and N % (4 * (N // 8)) == 0
            p = colsum_perm(N, N // 8)
            assert sorted(p.tolist()) == list(range(N))
    assert seen == {32}
    assert [rows_per_block(M, N) for (M, N) in COLSUM_BIG] == [64, 128]
    assert colsum_perm(8, 0).tolist() == list(range(8))
    assert colsum_perm(8, 1).tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
    assert colsum_perm(16, 2).tolist() == [0, 2, 4, 6, 1, 3, 5, 7, 8, 10, 12, 14, 9, 11, 13, 15]
    # the permutation undoes the packing: gate-minor column r lands on the reference row pack_rows names
    assert np.array_equal(colsum_perm(2 * 4 * 5, 5), pack_rows(5, 2))
    # the integer recipe is exact in fp32 for every committed case, the largest included
    for (M, N) in [(300, 264)] + COLSUM_BIG:
        assert 4 * M + 64 < 2 ** 24
    A, o1, o2 = colsum_inputs(17, 8, 16, 'integer')
    assert float(A[:, :8].abs().max()) <= 4 and float(o1.abs().max()) <= 64 and bool(torch.isnan(A[:, 8:]).all())
    A, _, _ = colsum_inputs(17, 8, 8, 'random')
    assert torch.equal(A.to(torch.bfloat16).to(torch.float32), A)


def test_act_bwd16_ref():
    """With bf16 operands o o is exact in float32, so g (1 - o o) has one rounding before the bf16 one whether or not the compiler
    contracts 1 - o o into a fused operation."""
    g = np.random.default_rng(3)
    gr = bf16_round(g.standard_normal(100000).astype(F32))
    o = bf16_round(np.tanh(3 * g.standard_normal(100000)).astype(F32))
    o64, g64 = o.astype(np.float64), gr.astype(np.float64)
    assert np.array_equal((o * o).astype(np.float64), o64 * o64)
    plain = gr * (F32(1) - o * o)
    fused = (g64 * (1.0 - o64 * o64).astype(F32).astype(np.float64)).astype(F32)   # the product of two float32 values is exact in float64
    assert np.array_equal(plain.view(np.uint32), fused.view(np.uint32))
    assert np.array_equal(act_bwd16_ref(gr, o, ACT_TANH), bf16_bits(fused))
    # autograd of tanh in float64 agrees to bf16 accuracy
    xs = torch.atanh(torch.from_numpy(o64).clamp(-1 + 1e-12, 1 - 1e-12)).requires_grad_(True)
    torch.tanh(xs).backward(torch.from_numpy(g64))
    inner = np.abs(o) < 1
    got = bf16_value(act_bwd16_ref(gr, o, ACT_TANH)).astype(np.float64)
    assert np.abs(got - xs.grad.numpy())[inner].max() <= 2.0 ** -8 * np.abs(xs.grad.numpy()).max()
    gr, o = act_inputs(2048, ACT_RELU)
    r = bf16_value(act_bwd16_ref(gr, o, ACT_RELU))
    assert r[0] == 0 and r[1] == 0 and r[2] == gr[2] and r[3] == 0 and r[4] == 0 and r[5] == gr[5] and r[6] == 0 and r[7] == gr[7]
    assert BF16_TINY == 2.0 ** -133 and 0.3 < float((o == 0).mean()) < 0.7
    assert ACT_N[-1] // 8 > GRID_CAP
