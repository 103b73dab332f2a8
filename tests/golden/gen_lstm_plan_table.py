"""Generates g14_lstm_plan_table.npz: what the host-side queries of the encoder LSTM recurrence answer for a table of shapes
under asr_lstm_set_persistent 0, 1 and 2.  CPU-only; needs the built library.  The committed fixture was written by the build
that preceded the shared host plan of the recurrence (csrc/lstm_plan.h) and is the record of the behaviour that change had to
preserve: regenerate it only when a plan or a workspace size is changed on purpose.

    python tests/golden/gen_lstm_plan_table.py            # writes tests/golden/g14_lstm_plan_table.npz
"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'e2e-asr-pytorch_amd'))

DIM_NAMES = ('B', 'T', 'H', 'ND', 'prec')
MODES = (0, 1, 2)
QUERIES = ('asr_lstm_plan', 'asr_lstm_workspace_bytes', 'asr_lstm16_workspace_bytes_fwd', 'asr_lstm16_workspace_bytes_bwd')
# the shapes of tests/test_hip_kernels.py::test_lstm_recurrence_fwd_bwd
KERNEL_TEST_SHAPES = ((3, 11, 16, 2), (5, 7, 20, 1), (18, 9, 32, 2), (16, 33, 320, 2), (33, 21, 128, 2), (7, 40, 64, 1),
                      (1, 1, 16, 1), (5, 64, 48, 2), (16, 19, 512, 1), (11, 130, 320, 2))


def rows():
    grid = itertools.product((1, 2, 3, 15, 16, 17, 32, 33, 63, 64, 65, 128),
                             (8, 16, 20, 24, 32, 48, 64, 128, 256, 320, 496, 512, 528, 640, 1280), (1, 2), (0, 1))
    out = [dict(B=B, T=50, H=H, ND=ND, prec=prec) for B, H, ND, prec in grid]       # no query depends on T
    return out + [dict(B=B, T=T, H=H, ND=ND, prec=prec) for (B, T, H, ND) in KERNEL_TEST_SHAPES for prec in (0, 1)]


def query(rs):
    """{name: int64 array (len(MODES), len(rs))}; the persistent mode of the process is put back afterwards."""
    from src import hipabi as H
    lib = H.lib()
    out = {q: np.zeros((len(MODES), len(rs)), np.int64) for q in QUERIES}
    old = lib.asr_lstm_set_persistent(MODES[0])
    try:
        for mi, mode in enumerate(MODES):
            lib.asr_lstm_set_persistent(mode)
            for ri, r in enumerate(rs):
                out['asr_lstm_plan'][mi, ri] = lib.asr_lstm_plan(r['B'], r['T'], r['H'], r['ND'], r['prec'])
                out['asr_lstm_workspace_bytes'][mi, ri] = lib.asr_lstm_workspace_bytes(r['B'], r['H'], r['ND'])
                out['asr_lstm16_workspace_bytes_fwd'][mi, ri] = lib.asr_lstm16_workspace_bytes(r['B'], r['H'], r['ND'], 0)
                out['asr_lstm16_workspace_bytes_bwd'][mi, ri] = lib.asr_lstm16_workspace_bytes(r['B'], r['H'], r['ND'], 1)
    finally:
        lib.asr_lstm_set_persistent(old)
    return out


def main():
    rs = rows()
    got = query(rs)
    counts = np.bincount(got['asr_lstm_plan'].ravel(), minlength=3)
    assert counts.min() >= 10, 'plan values 0, 1, 2 occur %s times' % counts.tolist()
    arrays = {'dims': np.array([[r[n] for n in DIM_NAMES] for r in rs], np.int32), 'dim_names': np.array(DIM_NAMES),
              'modes': np.array(MODES, np.int32)}
    arrays.update(got)
    path = os.path.join(HERE, 'g14_lstm_plan_table.npz')
    np.savez_compressed(path, **arrays)
    print('%s: %d rows, %d bytes; plan values: %s' % (path, len(rs), os.path.getsize(path), counts.tolist()))


if __name__ == '__main__':
    main()
