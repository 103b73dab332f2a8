"""The two backward kernels of the bf16-storage LSTM recurrence (csrc/lstm_persist3.hip) behind one forward call: the gather form
(lstm_bwd_g3: dh is exchanged, every workgroup recomputes the cell backward of its whole batch slice; planned for slices of at
most 4 rows and H <= 384) and the reduce-scatter form (lstm_bwd_p3), selected with asr_lstm16_set_bwd_form.  Both are held to
the step-forced float64 reference and the bound of tests/test_lstm_recurrence_reference.py, exactly as
tests/test_hip_lstm_recurrence_vs_float64.py holds lstm_bwd_p3 (guards, abort word, untouched c / dy included: its Run is used
as it is); the launch's status block must name the kernel that ran (64-bit word 34: 1 reduce-scatter, 2 gather).  Every case
prints the ratio of the two kernels' worst dgates error / bound.

Shapes: H = 16 (one workgroup, a quarter of K shorter than one k-step), 48 (three workgroups, padded k-step), 320 (the encoder's
width); T = 1, 2, 3, 5, 9 (every residue of the time loop unrolled by four, and the first step, which has no gather);
(B, ND) = (1, 2) one row and empty slices, (5, 2) two-row slices with a one-row last slice, (16, 2) and (32, 1) four-row slices.
The k-step classes the kernel is instantiated for and those shapes miss (NKS = 4, 6, 8, 12: H = 128, 192, 256, 384, the last two
at the register ceiling) get one four-row case each.
"""
import pytest
import torch

import test_lstm_recurrence_reference as R
import test_hip_lstm_recurrence_vs_float64 as V

gpu = pytest.mark.gpu

HS = (16, 48, 320)
TS = (1, 2, 3, 5, 9)
BND = ((1, 2), (5, 2), (16, 2), (32, 1))
CASES = [R.Case('lstm16', 1, R.BF16, B, T, H, ND, 'plain') for H in HS for (B, ND) in BND for T in TS]
WIDE = [R.Case('lstm16', 1, R.BF16, 16, 5, H, 2, 'plain') for H in (128, 192, 256, 384)]
GATHER, SCATTER = 1, 0
FORM_WORD = 34                               # 64-bit word of the status block: 1 reduce-scatter, 2 gather


def _backward_as(run, form, epoch, saved_act):
    """one backward launch under `form` on the activated gates of the forward call -> (stored gradients, form the launch reports)"""
    lib = run.lib
    run.gates.raw[run.gates.g:run.gates.g + run.gates.nbytes].copy_(saved_act)
    old = lib.asr_lstm16_set_bwd_form(form)
    try:
        planned = lib.asr_lstm16_bwd_form(run.case.B, run.case.H, run.case.ND)
        run.backward(epoch)
    finally:
        lib.asr_lstm16_set_bwd_form(old)
    off = (epoch & 1) * 1024 + FORM_WORD * 8
    ran = int(run.wsb.t[off:off + 8].view(torch.int64).item())
    assert ran == planned + 1, 'planned form %d, the launch reports %d' % (planned, ran)
    return run.stored_gates(), ran


def _forward(run):
    run.forward()
    run._guards('forward')
    return {'act': run.stored_gates(), 'c': run.c.data.cpu().to(R.F64), 'y': run.stored_y()}


def _check_both(case, inp, expect_new):
    from src import hipabi as Hh
    lib = Hh.lib()
    old = lib.asr_lstm_set_persistent(1)
    run = None
    try:
        run = V.Run(Hh, case, inp)
        st = _forward(run)
        act_bits, c_bits, dy_bits = run.gates.bits(), run.c.bits(), run.dy.bits()
        dg_new, ran_new = _backward_as(run, GATHER, 1, act_bits)
        run._guards('backward (gather form)')
        dg_old, ran_old = _backward_as(run, SCATTER, 2, act_bits)
        run._guards('backward (reduce-scatter form)')
        assert torch.equal(run.c.bits(), c_bits) and torch.equal(run.dy.bits(), dy_bits), 'a backward call wrote c or dy'
    finally:
        lib.asr_lstm_set_persistent(old)
        if run is not None:
            run.release()
    assert ran_old == 1 and ran_new == expect_new
    what = R.case_id(case)
    r_new = R.assert_forced(R.S_B16, inp, dict(st, dg=dg_new), what + ' form %d' % ran_new)['dgates'][0]
    r_old = R.assert_forced(R.S_B16, inp, dict(st, dg=dg_old), what + ' form 1')['dgates'][0]
    print('%s: dgates error / bound  new %.4f  old %.4f  ratio %.3f' % (what, r_new, r_old, r_new / r_old if r_old > 0 else float('nan')))


def _inputs(case, seed=None):
    return R.make_inputs(case.B, case.T, case.H, case.ND, True, False, case.variant, seed=seed)


@gpu
@pytest.mark.parametrize('case', CASES, ids=R.case_id)
def test_gather_form_vs_forced_float64(case):
    _check_both(case, _inputs(case), expect_new=2)


@gpu
@pytest.mark.parametrize('case', WIDE, ids=R.case_id)
def test_gather_form_every_k_step_class(case):
    _check_both(case, _inputs(case), expect_new=2)


@gpu
def test_five_row_slices_keep_the_reduce_scatter_form():
    """B = 17, ND = 2: slices of 5 rows.  The plan must name the reduce-scatter kernel whatever the switch says, and it passes."""
    case = R.Case('lstm16', 1, R.BF16, 17, 5, 48, 2, 'plain')
    _check_both(case, _inputs(case), expect_new=1)


@gpu
def test_back_to_back_launches_on_one_workspace():
    """Gather-form launches at epochs 15, 16, 17 on one workspace with different gates and dy.  The exchange region is
    (epoch >> 4) % BWD_REGIONS: 15 -> 16 crosses the rotation (and wraps the 4-bit epoch in the tags), 16 -> 17 reuses one region,
    where the later launch must not accept anything the earlier one left (launch epoch in the tags, the producers' clear before
    the consensus); the status block alternates by launch parity throughout."""
    from src import hipabi as Hh
    lib = Hh.lib()
    case = R.Case('lstm16', 1, R.BF16, 16, 9, 48, 2, 'plain')
    first = _inputs(case)
    other = _inputs(case, seed=77)
    second = first._replace(gates_in=other.gates_in, dy=other.dy)
    launches = ((15, first), (16, second), (17, first))
    old = lib.asr_lstm_set_persistent(1)
    old_form = lib.asr_lstm16_set_bwd_form(GATHER)
    run, got = None, []
    try:
        run = V.Run(Hh, case, first)
        for epoch, inp in launches:
            run.inp = inp
            run.load_gates()
            run.dy.put(inp.dy)
            run.forward(epoch)
            st = {'act': run.stored_gates(), 'c': run.c.data.cpu().to(R.F64), 'y': run.stored_y()}
            run.backward(epoch)
            off = (epoch & 1) * 1024 + FORM_WORD * 8
            assert int(run.wsb.t[off:off + 8].view(torch.int64).item()) == 2
            st['dg'] = run.stored_gates()
            got.append(st)
        run._guards('last backward')
    finally:
        lib.asr_lstm16_set_bwd_form(old_form)
        lib.asr_lstm_set_persistent(old)
        if run is not None:
            run.release()
    for (epoch, inp), st in zip(launches, got):
        R.assert_forced(R.S_B16, inp, st, 'launch at epoch %d' % epoch)
    assert not torch.equal(got[0]['dg'], got[1]['dg']) and not torch.equal(got[1]['dg'], got[2]['dg'])


def _needs(B, H, ND):
    """bytes of the backward workspace each kernel addresses: two status blocks, BWD_REGIONS = 2 exchange regions, each followed
    by the 8 KB per workgroup where the stores of inactive lanes land"""
    BS, P = -(-B // (8 // ND)), H // 16
    dump = 8 * P * 512 * 16
    scatter = 8 * 2 * P * P * BS * 8 * 8
    gather = 8 * 2 * BS * (H // 2) * 8
    return 2 * 1024 + 2 * (scatter + dump), 2 * 1024 + 2 * (gather + dump)


def test_workspace_covers_both_forms():
    """Host only: asr_lstm16_workspace_bytes(.., backward) is enough for either kernel at every shape of this file, and does not
    depend on the switch - a workspace sized before the gather form existed still serves."""
    from src import hipabi as Hh
    lib = Hh.lib()
    old = lib.asr_lstm_set_persistent(1)
    try:
        for H in HS:
            for B, ND in BND + ((17, 2),):
                sizes = []
                for form in (GATHER, SCATTER):
                    was = lib.asr_lstm16_set_bwd_form(form)
                    try:
                        sizes.append(int(lib.asr_lstm16_workspace_bytes(B, H, ND, 1)))
                        assert lib.asr_lstm16_bwd_form(B, H, ND) == (form if -(-B // (8 // ND)) <= 4 else SCATTER)
                    finally:
                        lib.asr_lstm16_set_bwd_form(was)
                assert sizes[0] == sizes[1]
                scatter, gather = _needs(B, H, ND)
                assert sizes[0] >= scatter and sizes[0] >= gather, (B, H, ND, sizes, scatter, gather)
    finally:
        lib.asr_lstm_set_persistent(old)
