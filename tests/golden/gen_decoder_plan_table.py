"""Generates g13_decoder_plan_table.npz: what the decoder's plan queries answer for a table of dims, under the plan preferences
3 (resident plans preferred) and 15 (streamed plans preferred).  CPU-only; needs the built library.  The committed fixture was
written by the build that preceded the shared host path of the cluster launchers (csrc/decoder_plan.h) and is the record of the
behaviour that change had to preserve: regenerate it only when a plan is changed on purpose.

    python tests/golden/gen_decoder_plan_table.py            # writes tests/golden/g13_decoder_plan_table.npz
"""
import ctypes
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'e2e-asr-pytorch_amd'))

DIM_NAMES = ('B', 'Tp', 'E', 'A', 'Dd', 'NL', 'Kn', 'Ks', 'L')
FLAGS = (3, 15)
QUERIES = ('asr_att_decoder_fwd_plan', 'asr_att_decoder_bwd_plan', 'asr_att_decoder_fwd_work_bytes',
           'asr_att_decoder_bwd_persistent_tiles', 'asr_att_decoder_bwd_status_offset', 'asr_att_decoder_bwd_workspace_bytes')
V = 31                  # vocabulary of corpus/librispeech_char.txt; no plan depends on it
STRIDE = 31             # every STRIDE-th row of the product is kept ...
PER_PAIR = 12           # ... and the first PER_PAIR rows of every (forward kind, backward kind) pair at flags 3


def product_rows():
    grid = itertools.product((1, 2, 8, 9, 16, 17, 32, 64),
                             (1, 7, 40, 150, 300, 400, 640, 641, 750, 850, 1225, 1500, 1700, 3000),
                             (1, 4, 5, 10, 11), (0, 50, 100, 512), (16, 128, 300, 320), (320, 640, 1024), (300, 320, 512, 640))
    return [dict(B=B, Tp=Tp, E=E, A=A, Dd=Dd, NL=1, Kn=Kn, Ks=Ks, L=20) for B, Tp, Kn, Ks, A, E, Dd in grid]


def shipped_rows():
    net = dict(E=640, A=300, Dd=300, NL=1, Kn=10, Ks=100)          # config/librispeech_asr.yaml
    return [dict(net, B=16, Tp=300, L=180),                        # bench.py
            dict(net, B=64, Tp=1500, L=400),                       # BASELINE config 5
            dict(net, B=8, Tp=1700, L=180),                        # the reference's longest batches
            dict(net, B=16, Tp=300, L=180, NL=2)]                  # two decoder layers: no plan


def query(rows):
    """{name: int64 array (len(FLAGS), len(rows))}; the plan preference of the process is put back afterwards."""
    from src import hipabi as H
    lib = H.lib()
    out = {q: np.zeros((len(FLAGS), len(rows)), np.int64) for q in QUERIES}
    old = lib.asr_att_decoder_set_persistent(FLAGS[0])
    try:
        for fi, flags in enumerate(FLAGS):
            lib.asr_att_decoder_set_persistent(flags)
            for ri, r in enumerate(rows):
                d = H.DecDims()
                for n in DIM_NAMES:
                    setattr(d, n, r[n])
                d.Q, d.V, d.temperature = r['Dd'] * r['NL'], V, 1.0
                for q in QUERIES:
                    out[q][fi, ri] = getattr(lib, q)(ctypes.byref(d))
    finally:
        lib.asr_att_decoder_set_persistent(old)
    return out


def main():
    full = product_rows()
    assert len(full) == 107520
    got = query(full)
    pair = got['asr_att_decoder_fwd_plan'][0] * 3 + got['asr_att_decoder_bwd_plan'][0]
    keep = set(range(0, len(full), STRIDE))
    for p in range(9):
        keep.update(np.flatnonzero(pair == p)[:PER_PAIR].tolist())
    keep = sorted(keep)
    for p in range(9):
        n = int((pair[keep] == p).sum())
        assert n >= 10, 'plan pair (%d, %d) occurs %d times in the thinned table' % (p // 3, p % 3, n)
    rows = [full[i] for i in keep] + shipped_rows()
    tail = query(shipped_rows())
    arrays = {'dims': np.array([[r[n] for n in DIM_NAMES] for r in rows], np.int32), 'dim_names': np.array(DIM_NAMES),
              'flags': np.array(FLAGS, np.int32)}
    for q in QUERIES:
        arrays[q] = np.concatenate([got[q][:, keep], tail[q]], axis=1)
    path = os.path.join(HERE, 'g13_decoder_plan_table.npz')
    np.savez_compressed(path, **arrays)
    print('%s: %d rows, %d bytes; pairs at flags 3: %s' % (path, len(rows), os.path.getsize(path),
                                                          np.bincount(pair[keep], minlength=9).tolist()))


if __name__ == '__main__':
    main()
