"""Parity of the MFMA contraction (asr_gemm) against a plain fp32 torch matmul on the CPU.

fp32 mode must match to accumulation-order noise; bf16 mode is compared with the same product on
bf16-rounded operands (so a wrong fragment/lane map cannot hide behind the loose bf16 tolerance).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _ref(A, B, a_kc, b_kc, prec):
    a = A if a_kc else A.transpose(-1, -2)
    b = B.transpose(-1, -2) if b_kc else B
    if prec == 1:
        a, b = _bf(a), _bf(b)
    return a.double() @ b.double()


CASES = [
    # M, N, K
    (128, 128, 32), (130, 257, 160), (300, 31, 70), (64, 640, 640), (513, 96, 33), (17, 5, 3), (1000, 300, 941),
]


@pytest.mark.parametrize('prec', [0, 1])
@pytest.mark.parametrize('a_kc,b_kc', [(1, 1), (1, 0), (0, 0), (0, 1)])
@pytest.mark.parametrize('M,N,K', CASES)
def test_gemm_layouts(M, N, K, a_kc, b_kc, prec):
    from src import hipabi
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = torch.randn((M, K) if a_kc else (K, M), generator=g)
    B = torch.randn((N, K) if b_kc else (K, N), generator=g)
    ref = _ref(A, B, a_kc, b_kc, prec)
    Ad, Bd = A.cuda(), B.cuda()
    C = torch.full((M, N), float('nan'), device='cuda')
    hipabi.gemm(Ad, Bd, C, M, N, K, A.shape[1], B.shape[1], N, a_kc=a_kc, b_kc=b_kc, prec=prec)
    torch.cuda.synchronize()
    err = (C.cpu().double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= 2e-5 * max(scale, 1.0) * (K ** 0.5), (err, scale)


@pytest.mark.parametrize('prec', [0, 1])
def test_gemm_bias_act_accum(prec):
    from src import hipabi
    g = torch.Generator().manual_seed(5)
    M, N, K = 200, 70, 100
    A, W, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g)
    C0 = torch.randn(M, N, generator=g)
    for act, fn in ((0, lambda x: x), (1, torch.tanh), (2, torch.relu)):
        ref = fn(_ref(A, W, 1, 1, prec) + b.double())
        C = torch.empty(M, N, device='cuda')
        hipabi.gemm(A.cuda(), W.cuda(), C, M, N, K, K, K, N, bias=b.cuda(), act=act, prec=prec)
        assert (C.cpu().double() - ref).abs().max().item() < 1e-4
    # accumulate into existing C
    C = C0.cuda()
    hipabi.gemm(A.cuda(), W.cuda(), C, M, N, K, K, K, N, accum=1, prec=prec)
    ref = C0.double() + _ref(A, W, 1, 1, prec)
    assert (C.cpu().double() - ref).abs().max().item() < 1e-4


@pytest.mark.parametrize('prec', [0, 1])
def test_gemm_split_reduction_and_views(prec):
    """Weight-gradient form: dW[n,k] += sum_m dY[m,n] X[m,k] with dY a column slice of a wider buffer."""
    from src import hipabi
    g = torch.Generator().manual_seed(9)
    Mr, N, K, wide = 1500, 96, 80, 256
    dYw = torch.randn(Mr, wide, generator=g)
    X = torch.randn(Mr, K, generator=g)
    off = 64
    dY = dYw[:, off:off + N]
    ref = _ref(dY.contiguous(), X, 0, 0, prec)  # A stored [r][i]
    C = torch.zeros(N, K, device='cuda')
    dYd = dYw.cuda()
    hipabi.gemm(dYd[:, off:], X.cuda(), C, N, K, Mr, wide, K, K, a_kc=0, b_kc=0, accum=1, splits=7, prec=prec)
    assert (C.cpu().double() - ref).abs().max().item() < 2e-3 * (1 if prec == 0 else 1)


@pytest.mark.parametrize('prec', [0, 1])
@pytest.mark.parametrize('shift', [-1, 1])
def test_gemm_shifted_rows(prec, shift):
    """Recurrent weight gradient: sum over (b,t) of dG[b,t,:]^T h[b,t+shift,:], zero outside [0,T)."""
    from src import hipabi
    g = torch.Generator().manual_seed(11)
    Bb, T, N, K = 3, 37, 64, 48
    dG = torch.randn(Bb, T, N, generator=g)
    H = torch.randn(Bb, T, K, generator=g)
    Hs = torch.zeros_like(H)
    if shift == -1:
        Hs[:, 1:] = H[:, :-1]
    else:
        Hs[:, :-1] = H[:, 1:]
    ref = _ref(dG.reshape(-1, N), Hs.reshape(-1, K), 0, 0, prec)
    C = torch.zeros(N, K, device='cuda')
    hipabi.gemm(dG.cuda(), H.cuda(), C, N, K, Bb * T, N, K, K, a_kc=0, b_kc=0, accum=1, splits=3,
                seqT=T, bshift=shift, prec=prec)
    assert (C.cpu().double() - ref).abs().max().item() < 1e-3


@pytest.mark.parametrize('prec', [0, 1])
def test_gemm_batched(prec):
    from src import hipabi
    g = torch.Generator().manual_seed(13)
    Bb, L, Tp, D = 4, 19, 75, 130
    attn = torch.rand(Bb, L, Tp, generator=g)
    dctx = torch.randn(Bb, L, D, generator=g)
    ref = _ref(attn, dctx, 0, 0, prec)  # per batch attn^T dctx -> (Tp, D)
    C = torch.zeros(Bb, Tp, D, device='cuda')
    hipabi.gemm(attn.cuda(), dctx.cuda(), C, Tp, D, L, Tp, D, D, a_kc=0, b_kc=0, batch=Bb,
                sA=L * Tp, sB=L * D, sC=Tp * D, prec=prec)
    assert (C.cpu().double() - ref).abs().max().item() < 1e-3


# ---- bf16-storage contractions (asr_gemm16): direct-to-LDS NT kernel (csrc/gemm16.hip) and the generic bf16-operand kernel ----
@pytest.mark.parametrize('M,N,K', [(128, 128, 64), (200, 136, 72), (1, 8, 8), (300, 2560, 160), (1000, 640, 640), (515, 160, 2560),
                                   (129, 132, 200)])
@pytest.mark.parametrize('act', [0, 1, 2])
def test_gemm16_nt_bf16_out(M, N, K, act):
    from src import hipabi as Hh
    g = torch.Generator().manual_seed(M + N + K)
    x = (torch.randn(M, K, generator=g)).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, generator=g)
    ref = x.float() @ w.float().t() + b
    ref = torch.tanh(ref) if act == 1 else (torch.relu(ref) if act == 2 else ref)
    out = torch.full((M, N), 7.0, dtype=torch.bfloat16, device='cuda')
    Hh.gemm16(x.cuda(), w.cuda(), out, M, N, K, K, K, N, 1, 1, bias=b.cuda(), act=act)
    err = (out.float().cpu() - ref).abs().max().item()
    assert err < 2e-2 * max(1.0, ref.abs().max().item()), err          # bf16 rounding of the output
    # the generic bf16-storage kernel must agree: ldc = N + 4 is no multiple of 8 for the six shapes with N % 8 == 0, and the
    # seventh (N = 132) has N % 8 != 0 - either way the direct-to-LDS kernel refuses the call, and the route query says so
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    out2 = torch.full((M, N + 4), 7.0, dtype=torch.bfloat16, device='cuda')
    assert Hh.lib().asr_gemm16_route(Hh.ptr(xd), Hh.ptr(wd), Hh.ptr(out), Hh.ptr(bd), M, N, K, K, K, N, 1, 1, act, 0, 1, 1, 0, 0, 0, 0) == (1 if N % 8 == 0 else 0)
    assert Hh.lib().asr_gemm16_route(Hh.ptr(xd), Hh.ptr(wd), Hh.ptr(out2), Hh.ptr(bd), M, N, K, K, K, N + 4, 1, 1, act, 0, 1, 1, 0, 0, 0, 0) == 0
    Hh.gemm16(xd, wd, out2, M, N, K, K, K, N + 4, 1, 1, bias=bd, act=act)
    assert (out2[:, :N].float().cpu() - ref).abs().max().item() < 2e-2 * max(1.0, ref.abs().max().item())
    assert float(out2[:, N:].float().min()) == 7.0 and float(out2[:, N:].float().max()) == 7.0


def test_gemm16_tn_weight_gradient_permuted_and_shifted():
    from src import hipabi as Hh
    g = torch.Generator().manual_seed(5)
    B, T, Hh_, ND, Din = 3, 17, 8, 2, 24
    G, D = ND * 4 * Hh_, ND * Hh_
    dg = torch.randn(B * T, G, generator=g).to(torch.bfloat16)
    x = torch.randn(B * T, Din, generator=g).to(torch.bfloat16)
    perm = torch.arange(G).view(ND, 4, Hh_).permute(0, 2, 1).reshape(-1)
    want = torch.zeros(G, Din)
    want[perm] = dg.float().t() @ x.float()
    out = torch.zeros(G, Din, device='cuda')
    Hh.gemm16(dg.cuda(), x.cuda(), out, G, Din, B * T, G, Din, Din, 0, 0, accum=1, splits=2, perm_h=Hh_)
    assert (out.cpu() - want).abs().max().item() < 1e-3 * want.abs().max().item() + 1e-4
    # shifted rows of a time-padded operand: dW_hh[d] = sum_{b,t} dg[b,t,d,:]^T y[b,t-1 (d=0) / t+1 (d=1), d*H:(d+1)*H]
    y = torch.zeros(B, T + 2, D)
    y[:, 1:T + 1] = torch.randn(B, T, D, generator=g)
    y16 = y.to(torch.bfloat16)
    for d, sh in ((0, -1), (1, 1)):
        ysh = y16[:, 1 + sh:T + 1 + sh, d * Hh_:(d + 1) * Hh_].float().reshape(B * T, Hh_)
        a = dg.float()[:, d * 4 * Hh_:(d + 1) * 4 * Hh_]
        pr = torch.arange(4 * Hh_).view(4, Hh_).t().reshape(-1)
        want = torch.zeros(4 * Hh_, Hh_)
        want[pr] = a.t() @ ysh
        out = torch.zeros(4 * Hh_, Hh_, device='cuda')
        Hh.gemm16(dg.cuda(), y16.cuda(), out, 4 * Hh_, Hh_, B * T, G, D, Hh_, 0, 0, accum=1, splits=1, perm_h=Hh_, seqT=T,
                  bshift=sh, b_time_padded=1, a_off=d * 4 * Hh_, b_off=d * Hh_)
        assert (out.cpu() - want).abs().max().item() < 1e-3 * want.abs().max().item() + 1e-4
