#!/usr/bin/env python
"""Writes tests/golden/g12_cmvn.npz: the reference's own Delta(2, 2) -> CMVN() -> Postprocess() (its src/audio.py, imported from a
read-only checkout) on three short random mel matrices, F = 8, T = 5, 17, 40, and on one single-frame matrix (T = 1), whose
output shows what the reference makes of one frame: NaN.  CPU only, float32 as the reference runs.

    python tests/golden/gen_cmvn_golden.py <path of the reference checkout>      (or ASR_REFERENCE=<path>)

torchaudio, audiomentations and librosa are not needed by these three classes; they are imported through the inert stand-ins
tests/golden/gen_golden.py uses.  Stored per matrix i: mel{i} (1, F, T) as ExtractAudioFeature returns it, len{i} = T,
delta{i} (3, F, T) what Delta hands to CMVN, out{i} (T, 3 F) what Postprocess makes of CMVN's output."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(8, 5), (8, 17), (8, 40), (8, 1)]


def reference_audio(ref):
    for name in ('torchaudio', 'torchaudio.transforms', 'audiomentations', 'librosa', 'librosa.feature', 'librosa.util'):
        if name not in sys.modules:
            m = types.ModuleType(name)
            if name == 'audiomentations':
                for c in ('Compose', 'AddGaussianNoise', 'TimeStretch', 'PitchShift', 'Shift', 'FrequencyMask', 'TimeMask'):
                    setattr(m, c, object)
            sys.modules[name] = m
            if '.' in name:
                setattr(sys.modules[name.split('.')[0]], name.split('.')[1], m)
    sys.path.insert(0, ref)
    import src.audio as A
    assert os.path.abspath(A.__file__).startswith(os.path.abspath(ref)), A.__file__
    return A


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('ASR_REFERENCE')
    if not ref:
        sys.exit(__doc__)
    A = reference_audio(ref)
    torch.set_num_threads(1)
    g = np.random.Generator(np.random.PCG64(1212))
    delta, cmvn, post = A.Delta(2, 2), A.CMVN(), A.Postprocess()
    arrays = {'n': np.array(len(SHAPES)), 'eps': np.array(cmvn.eps)}
    for i, (F, T) in enumerate(SHAPES):
        mel = g.random((1, F, T), dtype=np.float32)
        d = delta(torch.from_numpy(mel))
        arrays.update({'mel%d' % i: mel, 'len%d' % i: np.array(T, dtype=np.int64), 'delta%d' % i: d.numpy().copy(),
                       'out%d' % i: post(cmvn(d)).numpy().copy()})
    path = os.path.join(HERE, 'g12_cmvn.npz')
    np.savez_compressed(path, **arrays)
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
