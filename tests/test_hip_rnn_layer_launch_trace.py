"""The launch sequence of a training step and of the batched encoder pass is a fixed function of the model, the precision, the
shape and the overlap switches: tests/golden/g16_rnn_layer_launch_trace.json records every entry point they launched, in order,
with its scalar arguments (G, D, Dz, T2, the strides and offsets of the time-padded y, perm_h / seqT / bshift / the splits of the
weight-gradient contractions, the reserved units and launch counters of the recurrences, dropout rate and seed) and the stream
it was issued on (main, rec, side: what was deferred, where it was flushed, what ran in line at the join), before the encoder's
LSTM layer got one loop over a storage object for both storages and for the batched pass; the code must launch the same, entry
by entry.  Pointers are not in the trace: the numeric tests (tests/test_hip_model.py, tests/test_hip_lstm16.py,
tests/test_hip_ragged_encoder.py, tests/test_dp_hooks.py, tests/test_lm_training.py) hold the wiring."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import gen_rnn_layer_launch_trace as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def recorded(golden_dir):
    with open(os.path.join(golden_dir, 'g16_rnn_layer_launch_trace.json')) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases(recorded):
    assert list(recorded) == [G.case_key(c) for c in G.CASES]


@pytest.mark.parametrize('case', G.CASES, ids=G.case_key)
def test_launches_match_the_recorded_trace(case, recorded):
    want, got = recorded[G.case_key(case)], G.trace(case)
    assert list(got) == list(want) == (['train'] if case[2].get('lm') else ['train', 'encode_chunk'])
    for part in want:
        for i, (g, w) in enumerate(zip(got[part], want[part])):
            assert g == w, (part, i, g, w)              # floats too: they are constants
        assert len(got[part]) == len(want[part]), (part, got[part][len(want[part]):], want[part][len(got[part]):])


def test_a_non_contiguous_input_gets_its_gradient():
    """RNNLayerFn reads `requires_grad` off its argument, not off the contiguous copy it makes inside the (no-grad) forward: a
    transposed fp32 input gets the gradient of its contiguous twin.  Same kernels on the same values, so the two agree to the
    last bits: 1e-6 of the largest entry allows for the order of the split reductions only."""
    import torch
    from src import functions as F_hip
    from src import hipabi as H
    layer = G._asr('fp32', {}).encoder.layers[0]
    anchor = torch.zeros(1, device='cuda', requires_grad=True)
    torch.manual_seed(1)
    base = torch.rand(G.B, G.D, G.T, device='cuda')
    grads = []
    for x in (base.transpose(1, 2).requires_grad_(), base.transpose(1, 2).contiguous().requires_grad_()):
        out = F_hip.RNNLayerFn.apply(anchor, x, layer, False, 0, H.F32, F_hip.LayerF32)
        out.sum().backward()
        H.join_side()
        assert x.grad is not None and x.grad.shape == x.shape
        grads.append(x.grad)
    assert float((grads[0] - grads[1]).abs().max()) <= 1e-6 * float(grads[1].abs().max())
    assert float(grads[1].abs().max()) > 0
