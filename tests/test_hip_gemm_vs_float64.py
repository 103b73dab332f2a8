"""Every contraction kernel - gemm_kernel behind asr_gemm, its bf16-storage instantiation, gemm16_nt_kernel and
gemm16_tn_kernel behind asr_gemm16 - held element by element to the float64 reference of tests/test_gemm_reference.py at its
tile, k-step and slice edges.

Each case asserts first, through asr_gemm_plan / asr_gemm16_route / asr_gemm16_plan on the REAL device addresses, that it reaches the kernel,
loader pair and tile order its table entry names.  A written C starts as NaN, an accumulated one as its integer C0; the
operands' padding (columns between extent and leading dimension, element offsets, batch gaps) is NaN; C's padding columns,
batch gaps and a guard row above and below hold a sentinel - and the WHOLE buffer is compared, so a store outside the matrix
fails like a wrong element inside.  Exact cases must equal the reference; rounded cases are held to the per-element bound
derived in the reference module's docstring (whose factor 2 and tanh allowance are allowances, not measurements) - the test
prints the largest error / bound ratio it sees.

The switches (ASR_GEMM16_NT=0, ASR_GEMM16_BIG=1, ASR_GEMM16_TN_STAGES=2 / 4, ASR_GEMM_PLAIN_ORDER=1) are read once per
process, so each is tested in ONE fresh child process - this file run as a program - that runs the switch's exact table.
The child asserts per case what the switch must change in the plan (route 0, the 256 x 256 tile, 2 or 4 LDS stages, plain
order), so a variable that is not read fails the test instead of re-running the default kernel.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == '__main__':
    ROOT = os.path.dirname(HERE)
    for p in (HERE, ROOT, os.path.join(ROOT, 'e2e-asr-pytorch_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)

import test_gemm_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu


def run_case(c, override=None):
    """Runs one case on the GPU.  Returns (None or a description of the failure, largest error / bound of a rounded case)."""
    import torch
    from src import hipabi as H
    A, B, bias, C0, ref, tol = R.expected(c)
    io16 = c.api == 'gemm16'
    op_t = torch.bfloat16 if io16 else torch.float32
    c_t = torch.bfloat16 if (io16 and c.c16) else torch.float32
    At = torch.tensor(A, dtype=op_t).cuda()
    Bt = torch.tensor(B, dtype=op_t).cuda()
    Ct = torch.tensor(C0, dtype=c_t).cuda()
    bt = torch.tensor(bias, dtype=torch.float32).cuda() if bias is not None else None
    ptrs = (At.data_ptr(), Bt.data_ptr(), Ct.data_ptr(), bt.data_ptr() if bt is not None else 0)
    bad = R.route_mismatch(c, override, ptrs)
    if bad:
        return 'route ' + bad, 0.0
    args = R.abi_args(c, *ptrs)
    H.call('asr_gemm16' if io16 else 'asr_gemm', *args, H.stream_ptr())
    torch.cuda.synchronize()
    got = Ct.cpu().double().numpy()
    assert np.isfinite(ref).all(), c.name
    if tol is None:
        wrong, ratio = ~(got == ref), 0.0
    else:
        err = np.abs(got - ref)
        wrong = ~(err <= tol)
        ratio = float(np.nanmax(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), 0.0)))
    if not wrong.any():
        return None, ratio
    g = R.geometry(c)
    idx = np.flatnonzero(wrong)
    where = []
    for f in idx[:6]:
        rel = int(f) - g['c_base']
        z, rem = divmod(rel, g['sC']) if g['sC'] else (0, rel)
        where.append('[z %d row %d col %d] got %r want %r%s' % (z, rem // g['ldc'], rem % g['ldc'], float(got[f]), float(ref[f]),
                                                                  '' if tol is None else ' bound %.3g' % tol[f]))
    return '%s: %d wrong of %d (rows/cols relative to C; outside the matrix = padding or guard): %s' % (c.name, idx.size, got.size, '; '.join(where)), ratio


def _check(c, kernel):
    bad, ratio = run_case(c)
    if not c.exact:
        print('ratio %s %s %.4f' % (kernel, c.name, ratio))
    assert bad is None, bad


def _tables(*names):
    cases = [c for n in names for c in R.TABLES[n]]
    return dict(argvalues=cases, ids=[c.name for c in cases])


@pytest.mark.parametrize('c', **_tables('gemm_extents', 'gemm_loaders', 'gemm_slices', 'gemm_shifts', 'gemm_order', 'gemm_rounded'))
def test_asr_gemm(c):
    _check(c, 'gemm_kernel')


@pytest.mark.parametrize('c', **_tables('generic16', 'generic16_rounded'))
def test_generic_bf16_storage_kernel(c):
    assert c.route == R.GENERIC
    _check(c, 'gemm_kernel_io16')


@pytest.mark.parametrize('c', **_tables('nt16', 'nt16_rounded'))
def test_gemm16_nt_kernel(c):
    assert c.route == R.NT128
    _check(c, 'gemm16_nt_kernel')


@pytest.mark.parametrize('c', **_tables('tn16', 'tn16_rounded'))
def test_gemm16_tn_kernel(c):
    assert c.route == R.TN
    _check(c, 'gemm16_tn_kernel')


@pytest.mark.parametrize('setting', list(R.SWITCHES))
def test_switch_in_a_fresh_process(setting):
    """One child per setting, no retry; any non-zero, negative or signal exit status fails as it is."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), setting], env=R._child_env(setting), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    report = json.loads(r.stdout.strip().splitlines()[-1])
    assert report['setting'] == setting and report['ran'] == len(R.SWITCHES[setting][0]) and report['failures'] == []


def _child(setting):
    cases, override = R.SWITCHES[setting]
    k, v = setting.split('=')
    assert os.environ.get(k) == v, 'the child must be started with %s' % setting
    failures, ran = [], 0
    for c in cases:
        assert c.exact
        try:
            bad, _ = run_case(c, override)
        except Exception as e:                   # a refused or failed launch: report it and start nothing more on the GPU
            failures.append('%s: %r' % (c.name, e))
            break
        ran += 1
        if bad:
            failures.append(bad)
    print(json.dumps({'setting': setting, 'ran': ran, 'failures': failures}))
    return 1 if failures else 0


if __name__ == '__main__':
    sys.exit(_child(sys.argv[1]))
