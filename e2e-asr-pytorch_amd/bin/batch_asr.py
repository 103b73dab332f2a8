"""Inference Solver of `--test --decode-batch N`, N > 1 (no reference counterpart): bin/test_asr.py with the decoder called
once per N consecutive utterances.  They are padded to the group's longest and go through the length-aware batched encoder
pass (src/ragged.py) and one search; the TSV rows keep the data set's order.  bin/align_asr.py shares the two helpers."""
import os

import torch

from bin.test_asr import Solver as TestSolver
from src.asr import ASR
from src.decode import BeamDecoder
from src.ragged import group_consecutive


def decode_batch_of(paras):
    """Utterances per decoder call (--decode-batch), at least 1."""
    return max(1, int(getattr(paras, 'decode_batch', 1) or 1))


def pad_group(rows):
    """[(n_i, D) tensors] -> ((U, max n, D) zero-padded, (U) int64 lengths) on the rows' device."""
    lens = [int(r.shape[0]) for r in rows]
    out = torch.zeros((len(rows), max(lens)) + tuple(rows[0].shape[1:]), dtype=rows[0].dtype, device=rows[0].device)
    for u, r in enumerate(rows):
        out[u, :lens[u]] = r
    return out, torch.tensor(lens, dtype=torch.int64, device=rows[0].device)


def utterances(ds, device):
    """Every utterance of a split on its own, in order: (name, features (n,D) on the device, transcript ids)."""
    for names, feat, feat_len, txt in ds:
        if feat.dim() == 2:                      # waveform batch: GPU front-end (eval mode: no SpecAugment)
            with torch.no_grad():
                feat, feat_len = ds.audio_transform(feat.to(device), feat_len.to(device))
        for b in range(feat.shape[0]):
            yield names[b], feat[b, :int(feat_len[b])].to(device), txt[b]


class Solver(TestSolver):
    def set_model(self):
        hip = self.src_config.get('hip', {})
        self.model = ASR(self.feat_dim, self.vocab_size, 1, prec=hip.get('prec', 'bf16'), **self.src_config['model']).to(self.device)
        self.load_ckpt()
        self.model.eval()
        self.decode_batch = decode_batch_of(self.paras)
        self.decoder = BeamDecoder(self.model, None, batch_encode=True, **self.config['decode'])
        self.verbose(self.decoder.create_msg())

    def exec(self):
        for name, ds in (('dev', self.dv_set), ('test', self.tt_set)):
            path = os.path.join(self.paras.outdir, '{}_{}.tsv'.format(self.exp_name, name))
            with open(path, 'w') as f:
                f.write('idx\thyp\ttruth\n')
                for group in group_consecutive(utterances(ds, self.device), self.decode_batch):
                    feat, feat_len = pad_group([g[1] for g in group])
                    out = self.decoder(feat, feat_len)
                    for (idx, _, txt), hyps in zip(group, [out] if len(group) == 1 else out):
                        hyp = self.tokenizer.decode(hyps[0].outIndex) if hyps else ''
                        f.write('\t'.join([idx, hyp, self.tokenizer.decode(txt.tolist())]) + '\n')
            self.verbose('Wrote {}'.format(path))
