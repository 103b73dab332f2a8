"""CTC prefix scorer for joint decoding (reference src/ctc.py:4-108, Watanabe et al. Algo. 2) on the HIP path:
states live on the device as (N,T,2) fp32, `score` evaluates N hypotheses x C candidates in one launch.
`ctc_forced_align` is the Viterbi alignment of known transcripts (asr_ctc_align; no reference counterpart)."""
import collections

import torch

from src import hipabi as H


class CTCPrefixScore(object):
    def __init__(self, x):
        """x: (1,T,V) CTC log-probs of one utterance (device tensor)."""
        self.logzero, self.blank, self.eos = -100000000.0, 0, 1
        self.x = x[0].contiguous().float()
        self.input_length, self.odim = self.x.shape

    def init_state(self):
        r = torch.empty((self.input_length, 2), dtype=torch.float32, device=self.x.device)
        H.call('asr_ctc_prefix_init', H.ptr(self.x), H.ptr(r), self.input_length, self.odim, H.stream_ptr())
        return r

    def score(self, prefix_len, last_token, r_prev, candidates):
        """prefix_len, last_token: (N) ints; r_prev (N,T,2); candidates (N,C) -> psi (N,C), r_new (N,C,T,2)."""
        dev = self.x.device
        N, C = candidates.shape
        cand = candidates.to(dev, torch.int32).contiguous()
        pl = torch.as_tensor(prefix_len, dtype=torch.int32).to(dev)
        lt = torch.as_tensor(last_token, dtype=torch.int32).to(dev)
        r_prev = r_prev.contiguous()
        psi = torch.empty((N, C), dtype=torch.float32, device=dev)
        r_new = torch.empty((N, C, self.input_length, 2), dtype=torch.float32, device=dev)
        H.call('asr_ctc_prefix_score', H.ptr(self.x), H.ptr(r_prev), H.ptr(cand), H.ptr(pl), H.ptr(lt), H.ptr(psi), H.ptr(r_new),
               N, C, self.input_length, self.odim, H.stream_ptr())
        return psi, r_new

    def cheap_compute(self, g, r_prev, candidates):
        """Single-hypothesis form with the reference's signature (returns device tensors)."""
        psi, r = self.score([len(g)], [g[-1] if len(g) > 0 else 0], r_prev.unsqueeze(0),
                            torch.as_tensor(candidates).view(1, -1))
        return psi[0], r[0]


CTCAlignment = collections.namedtuple('CTCAlignment', 'frame_token frame_pos tok_start tok_end tok_score score ok')


def ctc_forced_align(logp, targets, input_len, target_len):
    """Most probable CTC alignment of every row's target, one launch for the batch (asr_ctc_align, csrc/ctc_align.hip).
    logp (B,T,V) fp32 log-probs, targets (B,L), input_len / target_len (B): device tensors.  Returns device tensors, nothing
    is copied to the host: frame_token, frame_pos (B,T) int32; tok_start, tok_end (B,L) int32 (inclusive frames), tok_score
    (B,L); score (B) and ok (B) int32 - the contract of include/asr_hip.h."""
    dev = logp.device
    logp = logp.contiguous().float()
    B, T, V = logp.shape
    targets = targets.to(dev, torch.int64).reshape(B, -1).contiguous()
    L = targets.shape[1]
    input_len = input_len.to(dev, torch.int64).contiguous()
    target_len = target_len.to(dev, torch.int64).contiguous()
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = CTCAlignment(i32(B, T), i32(B, T), i32(B, L), i32(B, L), f32(B, L), f32(B), i32(B))
    nbytes = int(H.lib().asr_ctc_align_workspace_bytes(B, T, L))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    H.call('asr_ctc_align', H.ptr(logp), H.ptr(targets), H.ptr(input_len), H.ptr(target_len), B, T, V, L,
           H.ptr(out.frame_token), H.ptr(out.frame_pos), H.ptr(out.tok_start), H.ptr(out.tok_end), H.ptr(out.tok_score),
           H.ptr(out.score), H.ptr(out.ok), H.ptr(ws), nbytes, H.stream_ptr())
    return out
