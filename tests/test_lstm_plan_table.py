"""The host-side queries of the encoder LSTM recurrence are a fixed function of the shape and the persistent mode:
tests/golden/g14_lstm_plan_table.npz records what asr_lstm_plan, asr_lstm_workspace_bytes and asr_lstm16_workspace_bytes
answered before the three kernel generations got one shared host plan (csrc/lstm_plan.h), for every (B, H, ND, precision) of a
grid around each generation's shape limits under asr_lstm_set_persistent 0, 1 and 2, and the built library must answer the
same, exactly.  CPU-only: the queries touch no device."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import gen_lstm_plan_table as G  # noqa: E402


def test_lstm_queries_match_the_recorded_table(golden_dir):
    from src import hipabi as H
    fx = np.load(os.path.join(golden_dir, 'g14_lstm_plan_table.npz'))
    assert tuple(fx['dim_names']) == G.DIM_NAMES and tuple(fx['modes']) == G.MODES
    rows = [dict(zip(G.DIM_NAMES, (int(v) for v in r))) for r in fx['dims']]
    assert rows == G.rows()                                      # the whole grid and the kernel test's ten shapes
    assert np.bincount(fx['asr_lstm_plan'].ravel(), minlength=3).min() >= 10      # every plan value is in the table
    before = H.lib().asr_lstm_set_persistent(1)
    H.lib().asr_lstm_set_persistent(before)
    got = G.query(rows)
    after = H.lib().asr_lstm_set_persistent(before)
    assert after == before                                       # the query put the mode back
    for q in G.QUERIES:
        diff = np.argwhere(got[q] != fx[q])
        assert diff.size == 0, (q, [(G.MODES[m], rows[r], int(fx[q][m, r]), int(got[q][m, r])) for m, r in diff[:5]])
