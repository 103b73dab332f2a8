#!/usr/bin/env python
"""Writes e2e-asr-pytorch_amd/corpus/librispeech_char_vec.txt: a small SYNTHETIC table of "word vectors" for </s> (<eos>) and the 28
symbols of corpus/librispeech_char.txt, 8 dimensions each, in the fastText text format src/util.load_embedding reads (a `count dim`
header, then `symbol v_1 ... v_dim` per line; the line of the blank symbol begins with a blank).  The values are standard
normal draws of a seeded generator rounded to 4 decimals - plumbing data for config/debug_emb.yaml, not trained vectors.

    python tools/gen_char_vectors.py [--dim 8] [--seed 28]"""
import argparse
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = os.path.join(ROOT, 'e2e-asr-pytorch_amd', 'corpus')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dim', type=int, default=8)
    ap.add_argument('--seed', type=int, default=28)
    a = ap.parse_args()
    with open(os.path.join(CORPUS, 'librispeech_char.txt'), encoding='UTF-8') as f:
        symbols = ['</s>'] + [line.strip('\r\n') for line in f]            # fastText's name of <eos>, then the 28 symbols
    g = np.random.Generator(np.random.PCG64(a.seed))
    vec = np.round(g.standard_normal((len(symbols), a.dim)), 4)
    path = os.path.join(CORPUS, 'librispeech_char_vec.txt')
    with open(path, 'w', encoding='UTF-8') as f:
        f.write('%d %d\n' % (len(symbols), a.dim))
        for s, v in zip(symbols, vec):
            f.write('%s %s\n' % (s, ' '.join('%.4f' % x for x in v)))
    print('wrote %s (%d symbols x %d)' % (path, len(symbols), a.dim))


if __name__ == '__main__':
    main()
