"""bench.py's run modes: a plain run prints the headline line only, `--full` adds the per-kernel figures, `--dump-outputs DIR`
writes what the last timed step computed (float32 / float64 .npy files, the same values from run to run up to the order of
the gradient sums), and `--steps` below 1 is refused."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')
SMALL = ['--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '4', '--frames', '400', '--tokens', '60']
FULL_ONLY = ('roofline', 'roofline_gemm', 'roofline_conv', 'stage_ms_per_step', 'cpu_baseline')


def _env():
    return {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}


def _run(extra):
    r = subprocess.run([sys.executable, BENCH] + SMALL + extra, env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith('.npy')}


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, BENCH, '--dry-run', '--steps', '0'], env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert '--steps must be at least 1' in r.stderr


@pytest.mark.gpu
def test_plain_full_and_dumped_outputs(tmp_path):
    plain_dir, full_dir = str(tmp_path / 'plain'), str(tmp_path / 'full')
    plain = _run(['--dump-outputs', plain_dir])
    for key, kind in (('metric', str), ('value', float), ('unit', str), ('higher_is_better', bool), ('dtype', str), ('ms_per_step', float)):
        assert isinstance(plain[key], kind), (key, plain[key])
    assert plain['steps'] == 2 and plain['ms_per_step'] > 0
    assert not any(k in plain for k in FULL_ONLY), sorted(plain)
    full = _run(['--full', '--no-cpu-baseline', '--dump-outputs', full_dir])
    assert full['roofline'] is not None and full['roofline_gemm'] is not None and full['stage_ms_per_step']
    assert full['cpu_baseline'] is None

    a, b = _load(plain_dir), _load(full_dir)
    assert sorted(a) == sorted(b)
    assert {'total_loss', 'ctc_loss', 'att_loss', 'grad_normsq', 'ctc_output', 'att_output', 'encode_len', 'params', 'grads'} <= set(a)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), (name, a[name].dtype)
        assert a[name].shape == b[name].shape, name
        assert np.isfinite(a[name]).all(), name
    # the last timed step starts from the seeded initial state: its forward results are the same bits in both runs, the
    # gradients and the updated weights differ only by the summation order of the fp32 atomics in the split reductions
    for name in ('total_loss', 'ctc_loss', 'att_loss', 'ctc_output', 'att_output', 'att_align', 'encode_len'):
        assert np.array_equal(a[name], b[name]), name
    for name in ('grad_normsq', 'grads', 'params'):
        err = float(np.abs(a[name].astype(np.float64) - b[name]).max())
        assert err <= 1e-5 * float(np.abs(b[name]).max()), (name, err)
    assert abs(float(a['total_loss']) - plain['loss']) <= 1e-6 * max(1.0, abs(plain['loss']))
