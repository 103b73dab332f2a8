"""The decoder's plan queries are a fixed function of the dims: tests/golden/g13_decoder_plan_table.npz records what they
answered before the cluster launchers got one shared host path (csrc/decoder_plan.h) - plan kinds, work-area bytes, backward
tiles, status offset and workspace bytes for a few thousand dims rows under both plan preferences - and the built library must
answer the same, exactly.  CPU-only: the queries touch no device."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import gen_decoder_plan_table as G  # noqa: E402


def test_plan_queries_match_the_recorded_table(golden_dir):
    from src import hipabi as H
    fx = np.load(os.path.join(golden_dir, 'g13_decoder_plan_table.npz'))
    assert tuple(fx['dim_names']) == G.DIM_NAMES and tuple(fx['flags']) == G.FLAGS
    rows = [dict(zip(G.DIM_NAMES, (int(v) for v in r))) for r in fx['dims']]
    assert len(rows) > 3000 and rows[-len(G.shipped_rows()):] == G.shipped_rows()
    pair = fx['asr_att_decoder_fwd_plan'][0] * 3 + fx['asr_att_decoder_bwd_plan'][0]
    assert np.bincount(pair, minlength=9).min() >= 10            # every (forward kind, backward kind) pair is in the table
    before = H.lib().asr_att_decoder_set_persistent(3)
    H.lib().asr_att_decoder_set_persistent(before)
    got = G.query(rows)
    after = H.lib().asr_att_decoder_set_persistent(before)
    assert after == before                                       # the query put the preference back
    for q in G.QUERIES:
        diff = np.argwhere(got[q] != fx[q])
        assert diff.size == 0, (q, [(G.FLAGS[f], rows[r], int(fx[q][f, r]), int(got[q][f, r])) for f, r in diff[:5]])
