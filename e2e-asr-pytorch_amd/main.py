#!/usr/bin/env python
"""Entry point with the reference's command line (main.py:12-106): `python main.py --config X [--test] ...`.
Under torchrun (WORLD_SIZE > 1) each process drives one GPU and gradients are all-reduced over RCCL."""
import argparse
import random

import numpy as np
import torch
import yaml

parser = argparse.ArgumentParser(description='Training E2E asr (MI355X HIP path).')
parser.add_argument('--config', type=str, help='Path to experiment config.')
parser.add_argument('--name', default=None, type=str)
parser.add_argument('--logdir', default='log/', type=str)
parser.add_argument('--ckpdir', default='ckpt/', type=str)
parser.add_argument('--outdir', default='result/', type=str)
parser.add_argument('--load', default=None, type=str)
parser.add_argument('--seed', default=0, type=int)
parser.add_argument('--cudnn-ctc', action='store_true', help='accepted for compatibility; the HIP CTC kernel is always used')
parser.add_argument('--njobs', default=4, type=int)
parser.add_argument('--cpu', action='store_true', help='not supported: the HIP path has no CPU fallback')
parser.add_argument('--no-pin', action='store_true')
parser.add_argument('--test', action='store_true')
parser.add_argument('--align', action='store_true', help='forced alignment of the transcripts with the CTC head (bin/align_asr.py)')
parser.add_argument('--decode-batch', default=1, type=int,
                    help='--test / --align: utterances per decoder call; N > 1 pads N consecutive utterances to the longest and runs the '
                         'length-aware batched encoder pass (results agree with N = 1 to rounding)')
parser.add_argument('--no-msg', action='store_true')
parser.add_argument('--lm', action='store_true')
parser.add_argument('--amp', action='store_true', help='accepted for compatibility; precision is chosen by hip.prec in the YAML')
parser.add_argument('--cuda', default=0, type=int)
parser.add_argument('--deterministic', action='store_true')
parser.add_argument('--upstream', default=None)


def select_solver(paras):
    """(Solver class, mode) the command line asks for."""
    if paras.lm:
        from bin.train_lm import Solver
        return Solver, 'train'
    if paras.align:
        from bin.align_asr import Solver
        return Solver, 'test'
    if paras.test:
        if paras.decode_batch > 1:
            from bin.batch_asr import Solver
            return Solver, 'test'
        from bin.test_asr import Solver
        return Solver, 'test'
    from bin.train_asr import Solver
    return Solver, 'train'


def main():
    paras = parser.parse_args()
    setattr(paras, 'gpu', not paras.cpu)
    setattr(paras, 'pin_memory', not paras.no_pin)
    setattr(paras, 'verbose', not paras.no_msg)
    config = yaml.load(open(paras.config, 'r'), Loader=yaml.FullLoader)
    from src import dist as D_
    rank, world, local = D_.init_from_env()
    if world > 1:
        paras.cuda = local
        paras.verbose = paras.verbose and rank == 0
    random.seed(paras.seed)
    np.random.seed(paras.seed)
    torch.manual_seed(paras.seed)
    Solver, mode = select_solver(paras)
    if paras.test and not paras.align and not paras.lm:
        from bin.emb_asr import with_emb_decoder      # embedding-fused decoding when the checkpoint's config has a fusing `emb:` block
        Solver = with_emb_decoder(Solver)
    solver = Solver(config, paras, mode)
    solver.load_data()
    solver.set_model()
    solver.exec()


if __name__ == '__main__':
    main()
