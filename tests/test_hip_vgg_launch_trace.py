"""The launch sequence of the VGG front-ends is a fixed function of the extractor, the precision and the shape:
tests/golden/g15_vgg_launch_trace.json records every entry point src/vgg.py launched, in order, with its scalar arguments (the
trims, K1p, the splits of the two weight-gradient paths, eps, the relu flags, the mode arguments), for a training forward +
backward and for forward_lens over a padded batch, before training and batched inference got one conv-stack loop; the code
must launch the same, entry by entry.  Pointers are not in the trace: the numeric tests (tests/test_hip_vgg_kernels.py,
tests/test_hip_ragged_frontend.py) hold the wiring."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import gen_vgg_launch_trace as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def recorded(golden_dir):
    with open(os.path.join(golden_dir, 'g15_vgg_launch_trace.json')) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases(recorded):
    assert list(recorded) == [G.case_key(c) for c in G.CASES]


@pytest.mark.parametrize('case', G.CASES, ids=G.case_key)
def test_launches_match_the_recorded_trace(case, recorded):
    want, got = recorded[G.case_key(case)], G.trace(case)
    assert list(got) == list(want) == ['train', 'forward_lens']
    for part in want:
        for i, (g, w) in enumerate(zip(got[part], want[part])):
            assert g == w, (part, i, g, w)              # floats too: they are constants
        assert len(got[part]) == len(want[part]), (part, got[part][len(want[part]):], want[part][len(got[part]):])
