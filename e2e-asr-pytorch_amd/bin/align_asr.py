"""Forced-alignment Solver (no reference counterpart): loads the model like bin/test_asr.py, aligns the transcript of every
utterance of each split with the model's CTC head and writes `<name>_<split>_align.tsv`: one line per token with its start
and end in seconds.  --decode-batch N > 1 aligns N consecutive utterances per call through the batched encoder pass."""
import os

import torch

from bin.batch_asr import decode_batch_of, pad_group, utterances
from bin.test_asr import Solver as TestSolver
from src.align import CTCAligner
from src.asr import ASR
from src.ragged import group_consecutive

HEADER = 'idx\ttoken\tstart_s\tend_s\tscore'


def format_alignment(idx, tokens, alignment, seconds_per_frame):
    """TSV lines of one utterance.  `tokens`: the printable form of every token of the transcript; `alignment`: an
    src.align.Alignment; `seconds_per_frame`: duration of one encoder output frame.  A token lasts from the start of its first
    frame to the end of its last one.  An utterance that could not be aligned gets ONE line with empty times."""
    if not alignment.ok:
        return ['\t'.join([idx, '', '', '', '%.4f' % alignment.score])]
    return ['\t'.join([idx, tok, '%.3f' % (s * seconds_per_frame), '%.3f' % ((e + 1) * seconds_per_frame), '%.4f' % sc])
            for tok, s, e, sc in zip(tokens, alignment.start_frame, alignment.end_frame, alignment.token_score)]


class Solver(TestSolver):
    def set_model(self):
        hip = self.src_config.get('hip', {})
        self.model = ASR(self.feat_dim, self.vocab_size, 1, prec=hip.get('prec', 'bf16'), **self.src_config['model']).to(self.device)
        self.load_ckpt()
        self.model.eval()
        self.decode_batch = decode_batch_of(self.paras)
        self.aligner = CTCAligner(self.model, batch_encode=self.decode_batch > 1)      # no `decode` section needed: there is no search
        self.verbose(self.aligner.create_msg())
        self.frame_shift_s = float(self.config['data']['audio'].get('frame_shift', 10)) / 1000.0

    def exec(self):
        for name, ds in (('dev', self.dv_set), ('test', self.tt_set)):
            path = os.path.join(self.paras.outdir, '{}_{}_align.tsv'.format(self.exp_name, name))
            with open(path, 'w') as f:
                f.write(HEADER + '\n')
                for group in group_consecutive(utterances(ds, self.device), self.decode_batch):
                    feat, feat_len = pad_group([g[1] for g in group])
                    txt, _ = pad_group([g[2].to(self.device) for g in group])
                    aligned, rate = self.aligner(feat, feat_len, txt, torch.sum(txt != 0, dim=-1))
                    for (name, _, _), al in zip(group, aligned):
                        toks = [self.tokenizer.decode([t]) or '<%d>' % t for t in al.tokens]      # <1>: the <eos> of the transcript
                        f.write('\n'.join(format_alignment(name, toks, al, rate * self.frame_shift_s)) + '\n')
            self.verbose('Wrote {}'.format(path))
