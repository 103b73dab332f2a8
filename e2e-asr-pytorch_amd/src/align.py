"""CTC forced alignment of known transcripts with a trained model's CTC head: where in the audio is every token?  The
reference has no counterpart.  CTCAligner encodes every utterance on its own (unpadded, the routine BeamDecoder uses; with
batch_encode=True the whole batch in one length-aware pass, src/ragged.py), runs the CTC head and aligns all utterances in
ONE launch (asr_ctc_align, csrc/ctc_align.hip); the result is read back once."""
import collections

import torch
from torch import nn

from src.ctc import ctc_forced_align
from src.decode import encode_batched, encode_unpadded, encoder_pass_msg

# tokens: the transcript; start_frame / end_frame: first / last encoder output frame of every token (inclusive); token_score:
# sum of the token's log-probs over its frames; score: log-probability of the whole alignment; ok: False when the transcript
# cannot be aligned (more tokens than frames, or only through impossible frames): then the frames are -1 and score is -inf
Alignment = collections.namedtuple('Alignment', 'tokens start_frame end_frame token_score score ok')


class CTCAligner(nn.Module):
    def __init__(self, asr, batch_encode=False):
        super().__init__()
        if not asr.ctc_weight > 0:
            raise ValueError('forced alignment needs a CTC head: this model was trained with ctc_weight = 0')
        self.asr = asr
        self.batch_encode = bool(batch_encode)      # opt-in: the batched pass agrees with the per-utterance one to rounding only
        # feature frames per encoder output frame: what the model applies to feature_len on the way to the encoder length
        self.frames_per_output = int(asr.encoder.sample_rate)

    def create_msg(self):
        return ['Align spec | CTC forced alignment (Viterbi) of the transcripts', encoder_pass_msg(self.asr, self.batch_encode)]

    @torch.no_grad()
    def forward(self, audio_feature, feature_len, text, text_len):
        """audio_feature (U,T,D) zero-padded, feature_len (U), text (U,L) padded token ids, text_len (U) ->
        ([Alignment] * U, frames_per_output).  Feature frame of an output frame f: f * frames_per_output."""
        dev = audio_feature.device
        encode = encode_batched if self.batch_encode else encode_unpadded
        _, _, tlen, ctc_lp = encode(self.asr, audio_feature, feature_len, True)
        U = ctc_lp.shape[0]
        text = text.to(dev, torch.int64).reshape(U, -1)
        L = text.shape[1]
        res = ctc_forced_align(ctc_lp, text, tlen, text_len)
        # the one read-back: everything but the per-frame tables in one tensor (frames and flags are exact in float64)
        packed = torch.cat([res.tok_start.double(), res.tok_end.double(), res.tok_score.double(), res.score.double().unsqueeze(1),
                            res.ok.double().unsqueeze(1), text.double(), text_len.to(dev).double().reshape(U, 1)], dim=1).cpu()
        out = []
        for u in range(U):
            row = packed[u]
            n = max(0, min(int(row[4 * L + 2]), L))
            ok = bool(row[3 * L + 1])
            out.append(Alignment([int(x) for x in row[3 * L + 2:3 * L + 2 + n]], [int(x) for x in row[:n]], [int(x) for x in row[L:L + n]],
                                 [float(x) for x in row[2 * L:2 * L + n]], float(row[3 * L]), ok))
        return out, self.frames_per_output
