"""src.hipabi.step_overlaps, the one predicate behind "does this step put work beside its chain?" (src/step.py, bin/train_asr.py,
src/asr.py, src/functions.py layer_backward / prepack16 / AttDecoderFn.backward, and CTCHeadFn.backward through its argument),
against the expression it replaced, written out here.  Nothing here needs a GPU: the predicate reads the environment only."""
import itertools
import os

import pytest

from test_step_streams_reference import _hipabi

SETTINGS = (None, '0', '1')


@pytest.mark.parametrize('overlap,overlap_dp,has_dp', list(itertools.product(SETTINGS, SETTINGS, (False, True))))
def test_step_overlaps_truth_table(overlap, overlap_dp, has_dp, monkeypatch):
    H = _hipabi()
    for name, value in (('ASR_OVERLAP', overlap), ('ASR_OVERLAP_DP', overlap_dp)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    dp = object() if has_dp else None
    # the literal: the overlap is on unless ASR_OVERLAP=0; under data parallelism it also needs ASR_OVERLAP_DP=1
    on = os.environ.get('ASR_OVERLAP', '1') != '0'
    want = on and (dp is None or (on and os.environ.get('ASR_OVERLAP_DP', '0') == '1'))
    got = H.step_overlaps(dp)
    assert got is want, (overlap, overlap_dp, has_dp, got, want)
    # and what the table says in words
    assert want == (overlap != '0' and (not has_dp or overlap_dp == '1'))
