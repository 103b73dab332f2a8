"""Forced-alignment Solver (no reference counterpart): loads the model like bin/test_asr.py, aligns the transcript of every
utterance of each split with the model's CTC head and writes `<name>_<split>_align.tsv`: one line per token with its start
and end in seconds."""
import os

import torch

from bin.test_asr import Solver as TestSolver
from src.align import CTCAligner
from src.asr import ASR

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
        self.aligner = CTCAligner(self.model)               # no `decode` section needed: there is no search
        self.frame_shift_s = float(self.config['data']['audio'].get('frame_shift', 10)) / 1000.0

    def exec(self):
        for name, ds in (('dev', self.dv_set), ('test', self.tt_set)):
            path = os.path.join(self.paras.outdir, '{}_{}_align.tsv'.format(self.exp_name, name))
            with open(path, 'w') as f:
                f.write(HEADER + '\n')
                for names, feat, feat_len, txt in ds:
                    if feat.dim() == 2:                      # waveform batch: GPU front-end (eval mode: no SpecAugment)
                        with torch.no_grad():
                            feat, feat_len = ds.audio_transform(feat.to(self.device), feat_len.to(self.device))
                    txt = txt.to(self.device)
                    aligned, rate = self.aligner(feat.to(self.device), feat_len.to(self.device), txt, torch.sum(txt != 0, dim=-1))
                    for b, al in enumerate(aligned):
                        toks = [self.tokenizer.decode([t]) or '<%d>' % t for t in al.tokens]      # <1>: the <eos> of the transcript
                        f.write('\n'.join(format_alignment(names[b], toks, al, rate * self.frame_shift_s)) + '\n')
            self.verbose('Wrote {}'.format(path))
