"""Step-forced float64 reference of the encoder LSTM recurrence, the case tables of
tests/test_hip_lstm_recurrence_vs_float64.py and the CPU checks of both.  Nothing of the code under test is imported here.

THE FORCED REFERENCE.  A whole bf16 sequence against float64 needs a loose bound, because rounding differences compound over
time.  Here step t is computed in float64 from what THE KERNEL ITSELF stored for the step before, so every element is one step
away from its operands and the bound is that of one step.  Canonical layout of this module: gates (B,T,ND,4,H) in the order
i,f,g,o; c, y, dy (B,T,ND,H); W_hh (ND,4,H,H) = [direction][gate][unit][k]; bias2 (ND,4,H).

Rounding points, read off the kernels (csrc/lstm.hip, lstm_persist.hip, lstm_persist2.hip, lstm_persist3.hip):
  * every conversion is `(__bf16)x` of an fp32 value, round to nearest even (cvt8 / load8_slow of common.h, Frag<true>::set and
    tile_store of lstm_persist.hip, f2bf_bits and the `(__bf16)` casts of the second and third generation);
  * bf16 contraction mode rounds W_hh once (resident fragments of the persistent kernels; the per-step kernels round the same
    fp32 value again at every step, which is the same number); the K tail of a fragment is zero;
  * the forward operand h is the stored y: per step and generations 1, 2 store y as fp32 and contract with its bf16 rounding
    (granule = f2bf_bits(h), the fp32 h goes to y; fp32 mode hands the fp32 value on unrounded); generation 3 stores y as bf16
    (B,T+2,ND*H), frame t at row t+1, and the granule is that same bf16;
  * the cell state is carried in an fp32 register and stored as fp32 unrounded: c_stored[t_prev] IS the carried value;
  * generation 3 reads bf16 gate-minor pre-activations (B,T,ND,H,4), forms the cell from the UNROUNDED fp32 activations and
    stores their bf16 roundings; its backward reads those bf16 values and bf16 dy, and stores bf16 gradients, which are also its
    contraction operand; generations 1, 2 and the per-step kernels store fp32 gradients and contract with their bf16 rounding
    (nothing is rounded in fp32 mode);
  * the backward's dc * f carry lives in an fp32 register and is never stored: the reference carries it in float64 from its own
    forced dh.  An error there is multiplied by f in (0,1) at every step, so it grows as fp32 round-off and not as a rounding
    difference that compounds.
Forward, step t of a direction (t_prev = t-1 forward, t+1 reverse; zero h and c before the first step):
    pre = gates_in[t] + W~ . h~[t_prev] (+ bias2);  i,f,o = sigmoid, g = tanh;  c[t] = f c_stored[t_prev] + i g;  h[t] = o tanh c[t]
  compared per element: activated gates, c[t], y[t].
Backward, step t (t_next = the step the backward walk did just before): dh[t] = dy[t] + W~^T . dg~_stored[t_next], coefficients
  from the activated gates and c the forward call stored, dc[t] = dh o (1 - tanh^2 c) + carry, carry' = dc f; compared per
  element: the four pre-activation gradients.

BOUNDS, derived, applied per element (never a norm):
    fp32-stored:  |got - ref| <= 2e-5 max(1, |ref|)      bf16-stored: that + 2^-8 |ref|
2e-5 is the fp32 bound tests/test_hip_kernels.py already holds this recurrence to.  It covers fp32 accumulation over K <= 2048
(2048 * 2^-24 = 1.2e-4 RELATIVE TO sum|terms| in the worst case, ~sqrt(K) 2^-24 = 2.7e-6 for rounding errors of either sign;
sum|terms| of a row here is below ~10), the ~5e-6 of __expf / rcp in the fast activations and the three tag bits masked out of
the second and third generation's backward partial sums (2^-21 relative, at most 8 partials).  2^-8 |ref| is one rounding to
bf16 of a value that far from the reference (half an ulp is at most 2^-8 relative).

THE STAND-IN.  emulate() is a plain torch fp32 restatement of each storage scheme (f32: fp32 storage and contraction; f32c16:
fp32 storage, bf16 contraction; bf16: bf16 storage) with torch.sigmoid / torch.tanh and the rounding points above, in both
directions.  Fed through the forced check as if it were the kernel it must pass every case of the case tables with 4x headroom:
the proof that the reference alone does not eat the bounds.  For a bf16-STORED quantity 4x headroom under the whole bound is not
there to be had: a correctly rounded bf16 store of a value just above a power of two is off by 2^-8 |value|, the whole of the
2^-8 |ref| term, whatever computed the value (measured: error / bound up to 0.99).  That term is arithmetic, not slack, so the
headroom is asserted on what is left of the error after 2^-8 |ref| has been taken off, against the fp32 term 2e-5 max(1, |ref|)
alone (ratio(..., fp32_part=True)); the whole bound is asserted as well.  Worst ratios over all cases (test_stand_in_headroom
prints them; all on plain cases):
    f32     gates 0.026 (B33 T5 H320 ND1)  c 0.021 (B18 T8 H320 ND2)  y 0.014 (B17 T8 H320 ND2)  dgates 0.024 (B33 T6 H160 ND1)
    f32c16  gates 0.016 (B16 T7 H336 ND2)  c 0.012 (B33 T6 H320 ND1)  y 0.007 (B16 T8 H384 ND2)  dgates 0.019 (B16 T5 H320 ND1)
    bf16    gates 0.003 (B64 T7 H320 ND2)  c 0.013 (B64 T7 H320 ND2)  y 0.001 (B64 T8 H384 ND2)  dgates 0.002 (B64 T8 H192 ND2)

PLANTED DEFECTS (test_planted_defects, schemes f32c16 and bf16): each is planted in emulate() and must fail the forced check;
the marked ones (*) also PASS the criteria the suite had before (|y - float64 run| < 3e-2, every gradient after its
weight-gradient contraction - dx, dW_ih, dW_hh, db - as one relative L2 norm < 4e-2), asserted as well.  All at H = 320, T = 8,
B = 64, ND = 2 (16-row slices of the third generation):
  (a)* batch row 37 of the reverse direction reads h[t-2] instead of h[t-1]       (b)* column H-1 of W_hh dropped (the K tail)
  (c)* the dc carry of row 31 (last row of a slice) zeroed at every fourth step   (d) i and f swapped for one unit
  (e) the reverse direction starts at T-2      (f) c[t_prev] of the first step is 0.25, not 0
  (g) the saved o gates of one direction truncated to bf16 instead of rounded (bf16 storage only)
Figures (forced error / bound of the worst output | old criteria: max |y error|, worst gradient norm), f32c16 scheme:
  (a) 1677 | 7.2e-3, 1.5e-2 pass   (b) 336 | 2.5e-3, 2.3e-2 pass   (c) 25689 | 1.4e-3, 2.3e-2 pass   (d) 42792 | 0.46, 3.2e-2 fail
  (e) 264428 | 0.67, 4.7 fail      (f) 12420 | 0.22, 0.12 fail      (g, bf16) 2.0 | 2.3e-3, 4.1e-3 pass
What it takes for the marked ones to pass the old criteria is part of the finding.  With inputs of unit scale (a) moves y by
0.35 and (b) by 0.067, and the old absolute 3e-2 sees both; that bound does not scale with the signal, so on a quiet input
(x and biases times 1/32, the `scale` argument, used for (a) and (b) only) they pass it while being 300 to 1700 times outside
the forced bound.  (c) with the carry zeroed at EVERY step reaches 4.4e-2 in db at B = 64, just above 4e-2; zeroed at every
fourth step (a lost register at the unroll-by-four boundary) it is 2.3e-2 and passes.  On (g): truncation is off by less than
one ulp, 2^-7 relative at the most, and the bound lies between half an ulp and one ulp, so a single element need not exceed it;
over a whole gate plane some dropped fraction always does (2.0 here): kept, and caught.

CASE TABLES, derived from the dispatch macros (FWD_CASE / BWD_CASE of lstm_persist.hip; FWD2_CASE / BWD2_CASE of
lstm_persist2.hip and FWD3_CASE / BWD3_CASE of lstm_persist3.hip, both expanded over the class lists LSTM_G23_NKS / LSTM_G23_NTO
of lstm_persist_common.h) by the plan arithmetic restated below; test_case_tables_cover
enumerates every (B, H, ND, precision) the plans accept and asserts that every instantiation any shape reaches is launched by
a case, and that the lines below are the tables.  Shape -> instantiation:
  lstm16-bf16-B4-T4-H16-ND2                    fwd fwd3<NKS=1,CH=1>           bwd bwd3<NTO=1>
  lstm16-bf16-B4-T5-H32-ND2                    fwd fwd3<NKS=1,CH=1>           bwd bwd3<NTO=1>
  lstm16-bf16-B4-T6-H48-ND2                    fwd fwd3<NKS=2,CH=1>           bwd bwd3<NTO=1>
  lstm16-bf16-B4-T7-H64-ND2                    fwd fwd3<NKS=2,CH=1>           bwd bwd3<NTO=1>
  lstm16-bf16-B4-T8-H80-ND2                    fwd fwd3<NKS=4,CH=1>           bwd bwd3<NTO=2>
  lstm16-bf16-B4-T4-H128-ND2                   fwd fwd3<NKS=4,CH=1>           bwd bwd3<NTO=2>
  lstm16-bf16-B4-T5-H144-ND2                   fwd fwd3<NKS=6,CH=1>           bwd bwd3<NTO=3>
  lstm16-bf16-B64-T6-H144-ND2                  fwd fwd3<NKS=6,CH=2>           bwd bwd3<NTO=3>
  lstm16-bf16-B4-T7-H192-ND2                   fwd fwd3<NKS=6,CH=1>           bwd bwd3<NTO=3>
  lstm16-bf16-B64-T8-H192-ND2                  fwd fwd3<NKS=6,CH=2>           bwd bwd3<NTO=3>
  lstm16-bf16-B4-T4-H208-ND2                   fwd fwd3<NKS=8,CH=1>           bwd bwd3<NTO=4>
  lstm16-bf16-B64-T5-H208-ND2                  fwd fwd3<NKS=8,CH=2>           bwd bwd3<NTO=4>
  lstm16-bf16-B4-T6-H256-ND2                   fwd fwd3<NKS=8,CH=1>           bwd bwd3<NTO=4>
  lstm16-bf16-B64-T7-H256-ND2                  fwd fwd3<NKS=8,CH=2>           bwd bwd3<NTO=4>
  lstm16-bf16-B4-T8-H272-ND2                   fwd fwd3<NKS=10,CH=1>          bwd bwd3<NTO=5>
  lstm16-bf16-B64-T4-H272-ND2                  fwd fwd3<NKS=10,CH=3>          bwd bwd3<NTO=5>
  lstm16-bf16-B32-T5-H272-ND2                  fwd fwd3<NKS=10,CH=2>          bwd bwd3<NTO=5>
  lstm16-bf16-B4-T6-H320-ND2                   fwd fwd3<NKS=10,CH=1>          bwd bwd3<NTO=5>
  lstm16-bf16-B64-T7-H320-ND2                  fwd fwd3<NKS=10,CH=3>          bwd bwd3<NTO=5>
  lstm16-bf16-B32-T8-H320-ND2                  fwd fwd3<NKS=10,CH=2>          bwd bwd3<NTO=5>
  lstm16-bf16-B4-T4-H336-ND2                   fwd fwd3<NKS=12,CH=1>          bwd bwd3<NTO=6>
  lstm16-bf16-B64-T5-H336-ND2                  fwd fwd3<NKS=12,CH=3>          bwd bwd3<NTO=6>
  lstm16-bf16-B32-T6-H336-ND2                  fwd fwd3<NKS=12,CH=2>          bwd bwd3<NTO=6>
  lstm16-bf16-B4-T7-H384-ND2                   fwd fwd3<NKS=12,CH=1>          bwd bwd3<NTO=6>
  lstm16-bf16-B64-T8-H384-ND2                  fwd fwd3<NKS=12,CH=3>          bwd bwd3<NTO=6>
  lstm16-bf16-B32-T4-H384-ND2                  fwd fwd3<NKS=12,CH=2>          bwd bwd3<NTO=6>
  lstm16-bf16-B4-T5-H400-ND2                   fwd fwd3<NKS=16,CH=1>          bwd bwd3<NTO=8>
  lstm16-bf16-B64-T6-H400-ND2                  fwd fwd3<NKS=16,CH=4>          bwd bwd3<NTO=8>
  lstm16-bf16-B32-T7-H400-ND2                  fwd fwd3<NKS=16,CH=2>          bwd bwd3<NTO=8>
  lstm16-bf16-B4-T8-H512-ND2                   fwd fwd3<NKS=16,CH=1>          bwd bwd3<NTO=8>
  lstm16-bf16-B64-T4-H512-ND2                  fwd fwd3<NKS=16,CH=4>          bwd bwd3<NTO=8>
  lstm16-bf16-B32-T5-H512-ND2                  fwd fwd3<NKS=16,CH=2>          bwd bwd3<NTO=8>
  lstm16-bf16-B9-T6-H64-ND1                    fwd fwd3<NKS=2,CH=1>           bwd bwd3<NTO=1>
  lstm16-bf16-B9-T7-H320-ND1                   fwd fwd3<NKS=10,CH=1>          bwd bwd3<NTO=5>
  lstm16-bf16-B9-T8-H512-ND1                   fwd fwd3<NKS=16,CH=1>          bwd bwd3<NTO=8>
  lstm-m1-bf16-B1-T4-H16-ND2                   fwd fwd2<NKS=1>                bwd bwd2<NTO=1>
  lstm-m1-bf16-B16-T5-H16-ND2                  fwd fwd2<NKS=1>                bwd bwd2<NTO=1>
  lstm-m1-bf16-B1-T5-H32-ND2                   fwd fwd2<NKS=1>                bwd bwd2<NTO=1>
  lstm-m1-bf16-B16-T6-H32-ND2                  fwd fwd2<NKS=1>                bwd bwd2<NTO=1>
  lstm-m1-bf16-B1-T6-H48-ND2                   fwd fwd2<NKS=2>                bwd bwd2<NTO=1>
  lstm-m1-bf16-B16-T7-H48-ND2                  fwd fwd2<NKS=2>                bwd bwd2<NTO=1>
  lstm-m1-bf16-B1-T7-H64-ND2                   fwd fwd2<NKS=2>                bwd bwd2<NTO=1>
  lstm-m1-bf16-B16-T8-H64-ND2                  fwd fwd2<NKS=2>                bwd bwd2<NTO=1>
  lstm-m1-bf16-B1-T8-H80-ND2                   fwd fwd2<NKS=4>                bwd bwd2<NTO=2>
  lstm-m1-bf16-B16-T4-H80-ND2                  fwd fwd2<NKS=4>                bwd bwd2<NTO=2>
  lstm-m1-bf16-B1-T4-H128-ND2                  fwd fwd2<NKS=4>                bwd bwd2<NTO=2>
  lstm-m1-bf16-B16-T5-H128-ND2                 fwd fwd2<NKS=4>                bwd bwd2<NTO=2>
  lstm-m1-bf16-B1-T5-H144-ND2                  fwd fwd2<NKS=6>                bwd bwd2<NTO=3>
  lstm-m1-bf16-B16-T6-H144-ND2                 fwd fwd2<NKS=6>                bwd bwd2<NTO=3>
  lstm-m1-bf16-B1-T6-H192-ND2                  fwd fwd2<NKS=6>                bwd bwd2<NTO=3>
  lstm-m1-bf16-B16-T7-H192-ND2                 fwd fwd2<NKS=6>                bwd bwd2<NTO=3>
  lstm-m1-bf16-B1-T7-H208-ND2                  fwd fwd2<NKS=8>                bwd bwd2<NTO=4>
  lstm-m1-bf16-B16-T8-H208-ND2                 fwd fwd2<NKS=8>                bwd bwd2<NTO=4>
  lstm-m1-bf16-B1-T8-H256-ND2                  fwd fwd2<NKS=8>                bwd bwd2<NTO=4>
  lstm-m1-bf16-B16-T4-H256-ND2                 fwd fwd2<NKS=8>                bwd bwd2<NTO=4>
  lstm-m1-bf16-B1-T4-H272-ND2                  fwd fwd2<NKS=10>               bwd bwd2<NTO=5>
  lstm-m1-bf16-B16-T5-H272-ND2                 fwd fwd2<NKS=10>               bwd bwd2<NTO=5>
  lstm-m1-bf16-B1-T5-H320-ND2                  fwd fwd2<NKS=10>               bwd bwd2<NTO=5>
  lstm-m1-bf16-B16-T6-H320-ND2                 fwd fwd2<NKS=10>               bwd bwd2<NTO=5>
  lstm-m1-bf16-B1-T6-H336-ND2                  fwd fwd2<NKS=12>               bwd bwd2<NTO=6>
  lstm-m1-bf16-B16-T7-H336-ND2                 fwd fwd2<NKS=12>               bwd bwd2<NTO=6>
  lstm-m1-bf16-B1-T7-H384-ND2                  fwd fwd2<NKS=12>               bwd bwd2<NTO=6>
  lstm-m1-bf16-B16-T8-H384-ND2                 fwd fwd2<NKS=12>               bwd bwd2<NTO=6>
  lstm-m1-bf16-B1-T8-H400-ND2                  fwd fwd2<NKS=16>               bwd bwd2<NTO=8>
  lstm-m1-bf16-B16-T4-H400-ND2                 fwd fwd2<NKS=16>               bwd bwd2<NTO=8>
  lstm-m1-bf16-B1-T4-H512-ND2                  fwd fwd2<NKS=16>               bwd bwd2<NTO=8>
  lstm-m1-bf16-B16-T5-H512-ND2                 fwd fwd2<NKS=16>               bwd bwd2<NTO=8>
  lstm-m2-fp32-B5-T4-H20-ND1                   fwd fwd1<fp32,NKS=1,MT=1>      bwd bwd0<fp32,vec>
  lstm-m2-bf16-B5-T5-H20-ND1                   fwd fwd1<bf16,NKS=1,MT=1>      bwd bwd0<bf16,vec>
  lstm-m2-fp32-B18-T6-H20-ND2                  fwd fwd1<fp32,NKS=1,MT=2>      bwd bwd0<fp32,vec>
  lstm-m2-bf16-B18-T7-H20-ND2                  fwd fwd1<bf16,NKS=1,MT=2>      bwd bwd0<bf16,vec>
  lstm-m2-fp32-B33-T8-H20-ND1                  fwd fwd1<fp32,NKS=1,MT=4>      bwd bwd0<fp32,vec>
  lstm-m2-bf16-B33-T4-H20-ND1                  fwd fwd1<bf16,NKS=1,MT=4>      bwd bwd0<bf16,vec>
  lstm-m2-fp32-B5-T7-H32-ND1                   fwd fwd1<fp32,NKS=1,MT=1>      bwd bwd1<fp32,NTO=1,NKS=4,NE=1>
  lstm-m2-bf16-B5-T8-H32-ND1                   fwd fwd1<bf16,NKS=1,MT=1>      bwd bwd1<bf16,NTO=1,NKS=4,NE=1>
  lstm-m2-fp32-B18-T4-H32-ND2                  fwd fwd1<fp32,NKS=1,MT=2>      bwd bwd1<fp32,NTO=1,NKS=4,NE=4>
  lstm-m2-bf16-B18-T5-H32-ND2                  fwd fwd1<bf16,NKS=1,MT=2>      bwd bwd1<bf16,NTO=1,NKS=4,NE=4>
  lstm-m2-fp32-B33-T6-H32-ND1                  fwd fwd1<fp32,NKS=1,MT=4>      bwd bwd1<fp32,NTO=1,NKS=4,NE=8>
  lstm-m2-bf16-B33-T7-H32-ND1                  fwd fwd1<bf16,NKS=1,MT=4>      bwd bwd1<bf16,NTO=1,NKS=4,NE=8>
  lstm-m2-fp32-B5-T5-H64-ND1                   fwd fwd1<fp32,NKS=2,MT=1>      bwd bwd1<fp32,NTO=1,NKS=8,NE=2>
  lstm-m2-bf16-B5-T6-H64-ND1                   fwd fwd1<bf16,NKS=2,MT=1>      bwd bwd1<bf16,NTO=1,NKS=8,NE=2>
  lstm-m2-fp32-B18-T7-H64-ND2                  fwd fwd1<fp32,NKS=2,MT=2>      bwd bwd1<fp32,NTO=1,NKS=8,NE=8>
  lstm-m2-bf16-B18-T8-H64-ND2                  fwd fwd1<bf16,NKS=2,MT=2>      bwd bwd1<bf16,NTO=1,NKS=8,NE=8>
  lstm-m2-fp32-B33-T4-H64-ND1                  fwd fwd1<fp32,NKS=2,MT=4>      bwd bwd0<fp32,vec>
  lstm-m2-bf16-B33-T5-H64-ND1                  fwd fwd1<bf16,NKS=2,MT=4>      bwd bwd0<bf16,vec>
  lstm-m2-fp32-B5-T8-H72-ND1                   fwd fwd1<fp32,NKS=3,MT=1>      bwd bwd0<fp32,vec>
  lstm-m2-bf16-B5-T4-H72-ND1                   fwd fwd1<bf16,NKS=3,MT=1>      bwd bwd0<bf16,vec>
  lstm-m2-fp32-B18-T5-H72-ND2                  fwd fwd1<fp32,NKS=3,MT=2>      bwd bwd0<fp32,vec>
  lstm-m2-bf16-B18-T6-H72-ND2                  fwd fwd1<bf16,NKS=3,MT=2>      bwd bwd0<bf16,vec>
  lstm-m2-fp32-B33-T7-H72-ND1                  fwd fwd1<fp32,NKS=3,MT=4>      bwd bwd0<fp32,vec>
  lstm-m2-bf16-B33-T8-H72-ND1                  fwd fwd1<bf16,NKS=3,MT=4>      bwd bwd0<bf16,vec>
  lstm-m2-fp32-B5-T6-H96-ND1                   fwd fwd1<fp32,NKS=3,MT=1>      bwd bwd1<fp32,NTO=2,NKS=4,NE=1>
  lstm-m2-bf16-B5-T7-H96-ND1                   fwd fwd1<bf16,NKS=3,MT=1>      bwd bwd1<bf16,NTO=2,NKS=4,NE=1>
  lstm-m2-fp32-B18-T8-H96-ND2                  fwd fwd1<fp32,NKS=3,MT=2>      bwd bwd1<fp32,NTO=2,NKS=4,NE=4>
  lstm-m2-bf16-B18-T4-H96-ND2                  fwd fwd1<bf16,NKS=3,MT=2>      bwd bwd1<bf16,NTO=2,NKS=4,NE=4>
  lstm-m2-fp32-B33-T5-H96-ND1                  fwd fwd1<fp32,NKS=3,MT=4>      bwd bwd1<fp32,NTO=2,NKS=4,NE=8>
  lstm-m2-bf16-B33-T6-H96-ND1                  fwd fwd1<bf16,NKS=3,MT=4>      bwd bwd1<bf16,NTO=2,NKS=4,NE=8>
  lstm-m2-fp32-B5-T4-H128-ND1                  fwd fwd1<fp32,NKS=4,MT=1>      bwd bwd1<fp32,NTO=2,NKS=8,NE=2>
  lstm-m2-bf16-B5-T5-H128-ND1                  fwd fwd1<bf16,NKS=4,MT=1>      bwd bwd1<bf16,NTO=2,NKS=8,NE=2>
  lstm-m2-fp32-B18-T6-H128-ND2                 fwd fwd1<fp32,NKS=4,MT=2>      bwd bwd1<fp32,NTO=2,NKS=8,NE=8>
  lstm-m2-bf16-B18-T7-H128-ND2                 fwd fwd1<bf16,NKS=4,MT=2>      bwd bwd1<bf16,NTO=2,NKS=8,NE=8>
  lstm-m2-fp32-B33-T8-H128-ND1                 fwd fwd1<fp32,NKS=4,MT=4>      bwd bwd0<fp32,vec>
  lstm-m2-bf16-B33-T4-H128-ND1                 fwd fwd1<bf16,NKS=4,MT=4>      bwd bwd0<bf16,vec>
  lstm-m2-fp32-B5-T7-H160-ND1                  fwd fwd1<fp32,NKS=5,MT=1>      bwd bwd1<fp32,NTO=3,NKS=4,NE=1>
  lstm-m2-bf16-B5-T8-H160-ND1                  fwd fwd1<bf16,NKS=5,MT=1>      bwd bwd1<bf16,NTO=3,NKS=4,NE=1>
  lstm-m2-fp32-B18-T4-H160-ND2                 fwd fwd1<fp32,NKS=5,MT=2>      bwd bwd1<fp32,NTO=3,NKS=4,NE=4>
  lstm-m2-bf16-B18-T5-H160-ND2                 fwd fwd1<bf16,NKS=5,MT=2>      bwd bwd1<bf16,NTO=3,NKS=4,NE=4>
  lstm-m2-fp32-B33-T6-H160-ND1                 fwd fwd1<fp32,NKS=5,MT=4>      bwd bwd1<fp32,NTO=3,NKS=4,NE=8>
  lstm-m2-bf16-B33-T7-H160-ND1                 fwd fwd1<bf16,NKS=5,MT=4>      bwd bwd1<bf16,NTO=3,NKS=4,NE=8>
  lstm-m2-fp32-B5-T5-H192-ND1                  fwd fwd1<fp32,NKS=6,MT=1>      bwd bwd1<fp32,NTO=3,NKS=4,NE=1>
  lstm-m2-bf16-B5-T6-H192-ND1                  fwd fwd1<bf16,NKS=6,MT=1>      bwd bwd1<bf16,NTO=3,NKS=4,NE=1>
  lstm-m2-fp32-B18-T7-H192-ND2                 fwd fwd1<fp32,NKS=6,MT=2>      bwd bwd1<fp32,NTO=3,NKS=4,NE=4>
  lstm-m2-bf16-B18-T8-H192-ND2                 fwd fwd1<bf16,NKS=6,MT=2>      bwd bwd1<bf16,NTO=3,NKS=4,NE=4>
  lstm-m2-fp32-B33-T4-H192-ND1                 fwd fwd1<fp32,NKS=6,MT=4>      bwd bwd1<fp32,NTO=3,NKS=4,NE=8>
  lstm-m2-bf16-B33-T5-H192-ND1                 fwd fwd1<bf16,NKS=6,MT=4>      bwd bwd1<bf16,NTO=3,NKS=4,NE=8>
  lstm-m2-fp32-B5-T8-H256-ND1                  fwd fwd1<fp32,NKS=8,MT=1>      bwd bwd1<fp32,NTO=4,NKS=4,NE=1>
  lstm-m2-bf16-B5-T4-H256-ND1                  fwd fwd1<bf16,NKS=8,MT=1>      bwd bwd1<bf16,NTO=4,NKS=4,NE=1>
  lstm-m2-fp32-B18-T5-H256-ND2                 fwd fwd1<fp32,NKS=8,MT=2>      bwd bwd1<fp32,NTO=4,NKS=4,NE=4>
  lstm-m2-bf16-B18-T6-H256-ND2                 fwd fwd1<bf16,NKS=8,MT=2>      bwd bwd1<bf16,NTO=4,NKS=4,NE=4>
  lstm-m2-fp32-B33-T7-H256-ND1                 fwd fwd1<fp32,NKS=8,MT=4>      bwd bwd1<fp32,NTO=4,NKS=4,NE=8>
  lstm-m2-bf16-B33-T8-H256-ND1                 fwd fwd1<bf16,NKS=8,MT=4>      bwd bwd1<bf16,NTO=4,NKS=4,NE=8>
  lstm-m2-fp32-B5-T6-H320-ND1                  fwd fwd1<fp32,NKS=10,MT=1>     bwd bwd1<fp32,NTO=5,NKS=4,NE=1>
  lstm-m2-bf16-B5-T7-H320-ND1                  fwd fwd1<bf16,NKS=10,MT=1>     bwd bwd1<bf16,NTO=5,NKS=4,NE=1>
  lstm-m2-fp32-B18-T8-H320-ND2                 fwd fwd1<fp32,NKS=10,MT=2>     bwd bwd1<fp32,NTO=5,NKS=4,NE=4>
  lstm-m2-bf16-B18-T4-H320-ND2                 fwd fwd1<bf16,NKS=10,MT=2>     bwd bwd1<bf16,NTO=5,NKS=4,NE=4>
  lstm-m2-fp32-B33-T5-H320-ND1                 fwd fwd0<fp32,vec>             bwd bwd1<fp32,NTO=5,NKS=4,NE=8>
  lstm-m2-bf16-B33-T6-H320-ND1                 fwd fwd1<bf16,NKS=10,MT=4>     bwd bwd1<bf16,NTO=5,NKS=4,NE=8>
  lstm-m2-fp32-B3-T4-H16-ND1                   fwd fwd1<fp32,NKS=1,MT=1>      bwd bwd1<fp32,NTO=1,NKS=2,NE=1>
  lstm-m2-bf16-B3-T5-H16-ND1                   fwd fwd1<bf16,NKS=1,MT=1>      bwd bwd1<bf16,NTO=1,NKS=2,NE=1>
  lstm-m2-fp32-B24-T5-H16-ND2                  fwd fwd1<fp32,NKS=1,MT=2>      bwd bwd1<fp32,NTO=1,NKS=2,NE=2>
  lstm-m2-bf16-B24-T6-H16-ND2                  fwd fwd1<bf16,NKS=1,MT=2>      bwd bwd1<bf16,NTO=1,NKS=2,NE=2>
  lstm-m2-fp32-B40-T7-H16-ND1                  fwd fwd1<fp32,NKS=1,MT=4>      bwd bwd1<fp32,NTO=1,NKS=2,NE=4>
  lstm-m2-bf16-B40-T8-H16-ND1                  fwd fwd1<bf16,NKS=1,MT=4>      bwd bwd1<bf16,NTO=1,NKS=2,NE=4>
  lstm-m2-fp32-B16-T5-H32-ND1                  fwd fwd1<fp32,NKS=1,MT=1>      bwd bwd1<fp32,NTO=1,NKS=4,NE=2>
  lstm-m2-bf16-B16-T6-H32-ND1                  fwd fwd1<bf16,NKS=1,MT=1>      bwd bwd1<bf16,NTO=1,NKS=4,NE=2>
  lstm-m2-fp32-B3-T8-H64-ND1                   fwd fwd1<fp32,NKS=2,MT=1>      bwd bwd1<fp32,NTO=1,NKS=8,NE=1>
  lstm-m2-bf16-B3-T4-H64-ND1                   fwd fwd1<bf16,NKS=2,MT=1>      bwd bwd1<bf16,NTO=1,NKS=8,NE=1>
  lstm-m2-fp32-B16-T7-H64-ND1                  fwd fwd1<fp32,NKS=2,MT=1>      bwd bwd1<fp32,NTO=1,NKS=8,NE=4>
  lstm-m2-bf16-B16-T8-H64-ND1                  fwd fwd1<bf16,NKS=2,MT=1>      bwd bwd1<bf16,NTO=1,NKS=8,NE=4>
  lstm-m2-fp32-B16-T4-H96-ND1                  fwd fwd1<fp32,NKS=3,MT=1>      bwd bwd1<fp32,NTO=2,NKS=4,NE=2>
  lstm-m2-bf16-B16-T5-H96-ND1                  fwd fwd1<bf16,NKS=3,MT=1>      bwd bwd1<bf16,NTO=2,NKS=4,NE=2>
  lstm-m2-fp32-B3-T7-H128-ND1                  fwd fwd1<fp32,NKS=4,MT=1>      bwd bwd1<fp32,NTO=2,NKS=8,NE=1>
  lstm-m2-bf16-B3-T8-H128-ND1                  fwd fwd1<bf16,NKS=4,MT=1>      bwd bwd1<bf16,NTO=2,NKS=8,NE=1>
  lstm-m2-fp32-B16-T6-H128-ND1                 fwd fwd1<fp32,NKS=4,MT=1>      bwd bwd1<fp32,NTO=2,NKS=8,NE=4>
  lstm-m2-bf16-B16-T7-H128-ND1                 fwd fwd1<bf16,NKS=4,MT=1>      bwd bwd1<bf16,NTO=2,NKS=8,NE=4>
  lstm-m2-fp32-B16-T8-H160-ND1                 fwd fwd1<fp32,NKS=5,MT=1>      bwd bwd1<fp32,NTO=3,NKS=4,NE=2>
  lstm-m2-bf16-B16-T4-H160-ND1                 fwd fwd1<bf16,NKS=5,MT=1>      bwd bwd1<bf16,NTO=3,NKS=4,NE=2>
  lstm-m2-fp32-B16-T5-H224-ND1                 fwd fwd0<fp32,vec>             bwd bwd1<fp32,NTO=4,NKS=4,NE=2>
  lstm-m2-bf16-B16-T6-H224-ND1                 fwd fwd0<bf16,vec>             bwd bwd1<bf16,NTO=4,NKS=4,NE=2>
  lstm-m2-fp32-B16-T4-H320-ND1                 fwd fwd1<fp32,NKS=10,MT=1>     bwd bwd1<fp32,NTO=5,NKS=4,NE=2>
  lstm-m2-bf16-B16-T5-H320-ND1                 fwd fwd1<bf16,NKS=10,MT=1>     bwd bwd1<bf16,NTO=5,NKS=4,NE=2>
  lstm-m0-fp32-B1-T4-H20-ND2                   fwd fwd0<fp32,vec>             bwd bwd0<fp32,vec>
  lstm-m0-bf16-B1-T4-H20-ND2                   fwd fwd0<bf16,vec>             bwd bwd0<bf16,vec>
  lstm-m0-fp32-B17-T5-H20-ND1                  fwd fwd0<fp32,vec>             bwd bwd0<fp32,vec>
  lstm-m0-bf16-B17-T5-H20-ND1                  fwd fwd0<bf16,vec>             bwd bwd0<bf16,vec>
  lstm-m0-fp32-B1-T5-H37-ND1                   fwd fwd0<fp32,scalar>          bwd bwd0<fp32,scalar>
  lstm-m0-bf16-B1-T5-H37-ND1                   fwd fwd0<bf16,scalar>          bwd bwd0<bf16,scalar>
  lstm-m0-fp32-B17-T6-H37-ND2                  fwd fwd0<fp32,scalar>          bwd bwd0<fp32,scalar>
  lstm-m0-bf16-B17-T6-H37-ND2                  fwd fwd0<bf16,scalar>          bwd bwd0<bf16,scalar>
  lstm-m0-fp32-B1-T6-H64-ND2                   fwd fwd0<fp32,vec>             bwd bwd0<fp32,vec>
  lstm-m0-bf16-B1-T6-H64-ND2                   fwd fwd0<bf16,vec>             bwd bwd0<bf16,vec>
  lstm-m0-fp32-B17-T7-H64-ND1                  fwd fwd0<fp32,vec>             bwd bwd0<fp32,vec>
  lstm-m0-bf16-B17-T7-H64-ND1                  fwd fwd0<bf16,vec>             bwd bwd0<bf16,vec>
  lstm-m0-fp32-B1-T7-H320-ND1                  fwd fwd0<fp32,vec>             bwd bwd0<fp32,vec>
  lstm-m0-bf16-B1-T7-H320-ND1                  fwd fwd0<bf16,vec>             bwd bwd0<bf16,vec>
  lstm-m0-fp32-B17-T8-H320-ND2                 fwd fwd0<fp32,vec>             bwd bwd0<fp32,vec>
  lstm-m0-bf16-B17-T8-H320-ND2                 fwd fwd0<bf16,vec>             bwd bwd0<bf16,vec>
Instantiations no shape can reach (recorded, nothing changed):
  fwd1<fp32,NKS=10,MT=4> bwd1<fp32,NTO=1,NKS=1,NE=1> bwd1<fp32,NTO=1,NKS=1,NE=2> bwd1<fp32,NTO=1,NKS=1,NE=4>
  bwd1<fp32,NTO=1,NKS=1,NE=8> bwd1<fp32,NTO=1,NKS=2,NE=8> bwd1<bf16,NTO=1,NKS=1,NE=1> bwd1<bf16,NTO=1,NKS=1,NE=2>
  bwd1<bf16,NTO=1,NKS=1,NE=4> bwd1<bf16,NTO=1,NKS=1,NE=8> bwd1<bf16,NTO=1,NKS=2,NE=8>
"""
import collections
import itertools

import pytest
import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
FP32, BF16 = 0, 1                      # `prec` of the C ABI
DIN = 16

Scheme = collections.namedtuple('Scheme', 'name contract16 store16')
S_F32 = Scheme('f32', False, False)
S_C16 = Scheme('f32c16', True, False)
S_B16 = Scheme('bf16', True, True)
SCHEMES = (S_F32, S_C16, S_B16)


def rbf(x):
    """(__bf16)x of fp32 values held in any float dtype: round to nearest even, returned in the dtype of x."""
    return x.to(F32).to(BF).to(x.dtype)


def trunc_bf(x):
    """fp32 -> bf16 by dropping the low 16 bits (defect g)."""
    return (x.to(F32).contiguous().view(torch.int32) & -65536).view(F32).to(x.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# one step, any leading dims: the ONLY arithmetic of the reference (forced and unforced use the same functions)
# ---------------------------------------------------------------------------------------------------------------------
def cell_fwd(pre, c_prev):
    """pre (..., 4, H), c_prev (..., H) -> activated gates (..., 4, H), c, h."""
    i, f, o = torch.sigmoid(pre[..., 0, :]), torch.sigmoid(pre[..., 1, :]), torch.sigmoid(pre[..., 3, :])
    g = torch.tanh(pre[..., 2, :])
    c = f * c_prev + i * g
    return torch.stack([i, f, g, o], dim=-2), c, o * torch.tanh(c)


def cell_bwd(dh, carry, act, c, c_prev):
    """-> the four pre-activation gradients (..., 4, H) and the carry dc * f for the step before."""
    i, f, g, o = act[..., 0, :], act[..., 1, :], act[..., 2, :], act[..., 3, :]
    tc = torch.tanh(c)
    dc = dh * o * (1 - tc * tc) + carry
    return torch.stack([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], dim=-2), dc * f


def rec_fwd(W, h):
    """W (ND,4,H,H), h (..., ND, H) -> W . h as (..., ND, 4, H)."""
    return torch.einsum('dgjk,...dk->...dgj', W, h)


def rec_bwd(W, dg):
    """W (ND,4,H,H), dg (..., ND, 4, H) -> W^T . dg as (..., ND, H)."""
    return torch.einsum('dgjk,...dgj->...dk', W, dg)


def _shift(x, step0):
    """x (B,T,ND,...) -> out[:, t, d] = x[:, t + step0] for direction 0 and x[:, t - step0] for direction 1; zero outside."""
    out = torch.zeros_like(x)
    for d in range(x.shape[2]):
        st = step0 if d == 0 else -step0
        if x.shape[1] > 1:
            if st < 0:
                out[:, 1:, d] = x[:, :-1, d]
            else:
                out[:, :-1, d] = x[:, 1:, d]
    return out


def prev_step(x):
    """value at the step the FORWARD walk of each direction did just before (zero state before the first)."""
    return _shift(x, -1)


def next_step(x):
    """value at the step the BACKWARD walk of each direction did just before."""
    return _shift(x, +1)


def time_order(T, d, backward=False):
    fwd = range(T) if d == 0 else range(T - 1, -1, -1)
    return list(reversed(fwd)) if backward else list(fwd)


# ---------------------------------------------------------------------------------------------------------------------
# forced reference
# ---------------------------------------------------------------------------------------------------------------------
def forced_forward(scheme, gates_in, whh, bias2, k_y, k_c):
    """float64 activated gates, c, y of EVERY step, each from the kernel's stored y / c of the step before."""
    W = rbf(whh) if scheme.contract16 else whh
    h_op = rbf(k_y) if scheme.contract16 else k_y
    pre = gates_in + rec_fwd(W, prev_step(h_op))
    if bias2 is not None:
        pre = pre + bias2
    return cell_fwd(pre, prev_step(k_c))


def forced_backward(scheme, whh, dy, k_act, k_c, k_dg):
    """float64 pre-activation gradients of every step: dh from the kernel's stored gradients of the step before, coefficients
    from the stored activated gates / c of the forward call, the dc * f carry in float64 from this function's own dh."""
    W = rbf(whh) if scheme.contract16 else whh
    dg_op = rbf(k_dg) if scheme.contract16 else k_dg
    dh = dy + rec_bwd(W, next_step(dg_op))
    c_prev = prev_step(k_c)
    B, T, ND, H = k_c.shape
    out = torch.empty_like(k_act)
    for d in range(ND):
        carry = torch.zeros(B, H, dtype=F64)
        for t in time_order(T, d, backward=True):
            out[:, t, d], carry = cell_bwd(dh[:, t, d], carry, k_act[:, t, d], k_c[:, t, d], c_prev[:, t, d])
    return out


def bound(ref, store16):
    b = 2e-5 * ref.abs().clamp(min=1.0)
    return b + 2.0 ** -8 * ref.abs() if store16 else b


def ratio(got, ref, store16, fp32_part=False):
    """worst |got - ref| / bound and where; NaN / inf in `got` counts as infinite.  fp32_part: the error left after the bf16
    rounding allowance 2^-8 |ref| has been taken off, over the fp32 term 2e-5 max(1, |ref|) alone (the stand-in's headroom)."""
    e = (got - ref).abs()
    if fp32_part:
        r = ((e - 2.0 ** -8 * ref.abs()) if store16 else e).clamp(min=0) / bound(ref, False)
    else:
        r = e / bound(ref, store16)
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float('inf')))
    k = int(r.argmax())
    return float(r.reshape(-1)[k]), tuple(int(v) for v in torch.unravel_index(torch.tensor(k), r.shape))


def forced_ratios(scheme, inp, st, fp32_part=False):
    """inp: Inputs; st: dict of the kernel's stored outputs as float64 canonical tensors: act, c, y after the forward call and
    dg after the backward call.  -> {name: (worst ratio, index)}."""
    s16, fp = scheme.store16, fp32_part
    ra, rc, ry = forced_forward(scheme, inp.gates_in, inp.whh, inp.bias2, st['y'], st['c'])
    out = {'gates': ratio(st['act'], ra, s16, fp), 'c': ratio(st['c'], rc, False, fp), 'y': ratio(st['y'], ry, s16, fp)}
    if 'dg' in st:
        out['dgates'] = ratio(st['dg'], forced_backward(scheme, inp.whh, inp.dy, st['act'], st['c'], st['dg']), s16, fp)
    return out


def assert_forced(scheme, inp, st, what=''):
    rs = forced_ratios(scheme, inp, st)
    print('forced %s %s: %s' % (scheme.name, what, '  '.join('%s %.3f @%s' % (k, v[0], v[1]) for k, v in rs.items())))
    bad = {k: v for k, v in rs.items() if not v[0] <= 1.0}
    assert not bad, 'outside the forced float64 bound (error / bound, index [b,t,d,(gate,)unit]) %s: %s' % (what, bad)
    return rs


# ---------------------------------------------------------------------------------------------------------------------
# unforced float64 (parity with the oracle) - the same step functions, its own values handed on
# ---------------------------------------------------------------------------------------------------------------------
def run_forward(gates_in, whh, bias2):
    B, T, ND, _, H = gates_in.shape
    act, c, y = torch.zeros_like(gates_in), gates_in.new_zeros(B, T, ND, H), gates_in.new_zeros(B, T, ND, H)
    for d in range(ND):
        h, cc = gates_in.new_zeros(B, H), gates_in.new_zeros(B, H)
        for t in time_order(T, d):
            pre = gates_in[:, t, d] + rec_fwd(whh[d:d + 1], h[:, None])[:, 0]
            if bias2 is not None:
                pre = pre + bias2[d]
            act[:, t, d], cc, h = cell_fwd(pre, cc)
            c[:, t, d], y[:, t, d] = cc, h
    return act, c, y


def run_backward(whh, dy, act, c):
    B, T, ND, H = c.shape
    c_prev = prev_step(c)
    dg = torch.zeros_like(act)
    for d in range(ND):
        carry, last = dy.new_zeros(B, H), None
        for t in time_order(T, d, backward=True):
            dh = dy[:, t, d] if last is None else dy[:, t, d] + rec_bwd(whh[d:d + 1], last[:, None])[:, 0]
            last, carry = cell_bwd(dh, carry, act[:, t, d], c[:, t, d], c_prev[:, t, d])
            dg[:, t, d] = last
    return dg


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
Inputs = collections.namedtuple('Inputs', 'x wih b_ih gates_in whh bias2 dy')      # float64 tensors holding fp32 / bf16 values

VARIANTS = ('plain', 'sat', 'zero_in', 'zero_dy')
SAT_SHIFT = (30.0, -30.0, 95.0, -95.0)          # added to all four gates of units 0, 1, 2, 3 (variant 'sat')


def make_inputs(B, T, H, ND, store16, with_bias2, variant='plain', seed=None, scale=1.0):
    """Seeded normals: x ~ N(0,1) (B,T,DIN), W_ih ~ N(0,1)/sqrt(DIN), W_hh ~ N(0,1)/sqrt(H), biases 0.1 N(0,1), dy ~ N(0,1).
    gates_in = x W_ih^T + b_ih in fp32 (+ b_hh where no bias2 is passed); bf16 storage rounds gates_in and dy to bf16.
    scale (the planted defects only): x and both biases times `scale`, a quiet signal."""
    g = torch.Generator().manual_seed(1000003 * B + 10007 * T + 101 * H + ND if seed is None else seed)
    x = torch.randn(B, T, DIN, generator=g) * scale
    wih = torch.randn(ND, 4, H, DIN, generator=g) / DIN ** 0.5
    whh = torch.randn(ND, 4, H, H, generator=g) / H ** 0.5
    b_ih, b_hh = torch.randn(ND, 4, H, generator=g) * 0.1 * scale, torch.randn(ND, 4, H, generator=g) * 0.1 * scale
    dy = torch.randn(B, T, ND, H, generator=g)
    gi = torch.einsum('btk,dgjk->btdgj', x, wih) + b_ih
    bias2 = b_hh if with_bias2 else None
    if not with_bias2:
        gi = gi + b_hh
    if variant == 'sat':
        for u, s in enumerate(SAT_SHIFT):
            gi[..., u] += s
    elif variant == 'zero_in':
        gi, bias2 = torch.zeros_like(gi), None
    elif variant == 'zero_dy':
        dy = torch.zeros_like(dy)
    if store16:
        gi, dy = rbf(gi), rbf(dy)
    d = lambda t: None if t is None else t.to(F64)
    return Inputs(d(x), d(wih), d(b_ih + (0 if with_bias2 else b_hh)), d(gi), d(whh), d(bias2), d(dy))


# ---------------------------------------------------------------------------------------------------------------------
# the stand-in: torch fp32 with the kernels' rounding points
# ---------------------------------------------------------------------------------------------------------------------
def emulate(scheme, inp, defect=None):
    """-> stored outputs {act, c, y, dg} as float64 canonical tensors, computed in fp32.  defect: None or (name, args...)."""
    r = lambda t: t.to(BF).to(F32)
    gates_in, whh, dy = inp.gates_in.to(F32), inp.whh.to(F32), inp.dy.to(F32)
    bias2 = None if inp.bias2 is None else inp.bias2.to(F32)
    B, T, ND, _, H = gates_in.shape
    kind = defect[0] if defect else None
    W = r(whh) if scheme.contract16 else whh
    Wf = W.clone()
    if kind == 'drop_col':
        Wf[..., H - 1] = 0
    act, c, y = gates_in.clone(), torch.zeros(B, T, ND, H), torch.zeros(B, T, ND, H)
    for d in range(ND):
        order = time_order(T, d)
        if kind == 'rev_start' and d == ND - 1:
            order = order[1:]
        h, h2, cc = torch.zeros(B, H), torch.zeros(B, H), torch.zeros(B, H)
        if kind == 'c0_stale' and d == defect[1]:
            cc = torch.full((B, H), 0.25)
        for t in order:
            hop = r(h) if scheme.contract16 else h.clone()
            if kind == 'stale_h' and d == defect[1]:
                hop[defect[2]] = (r(h2) if scheme.contract16 else h2)[defect[2]]
            pre = gates_in[:, t, d] + torch.einsum('gjk,bk->bgj', Wf[d], hop)
            if bias2 is not None:
                pre = pre + bias2[d]
            if kind == 'swap_if' and d == defect[1]:
                pre[:, [0, 1], defect[2]] = pre[:, [1, 0], defect[2]]
            a, cc, hv = cell_fwd(pre, cc)
            h2, h = h, (r(hv) if scheme.store16 else hv)
            act[:, t, d] = r(a) if scheme.store16 else a
            if kind == 'trunc_gate' and d == defect[1]:
                act[:, t, d, 3] = trunc_bf(a[:, 3])
            c[:, t, d], y[:, t, d] = cc, h
    c_prev = prev_step(c)
    dg = torch.zeros_like(act)
    for d in range(ND):
        carry, last = torch.zeros(B, H), None
        for t in time_order(T, d, backward=True):
            dh = dy[:, t, d].clone()
            if last is not None:
                dh = dh + torch.einsum('gjk,bgj->bk', W[d], r(last) if scheme.contract16 else last)
            if kind == 'zero_carry' and d == defect[1] and (T - 1 - t if d == 0 else t) % defect[3] == 0:
                carry[defect[2]] = 0
            v, carry = cell_bwd(dh, carry, act[:, t, d], c[:, t, d], c_prev[:, t, d])
            last = r(v) if scheme.store16 else v
            dg[:, t, d] = last
    return {k: v.to(F64) for k, v in (('act', act), ('c', c), ('y', y), ('dg', dg))}


def old_criteria(inp, st):
    """What the suite checked before: max |y - float64 run| (bound 3e-2) and the relative L2 norm of every gradient AFTER its
    weight-gradient contraction (bound 4e-2): dx, dW_ih, dW_hh, db."""
    act, c, y = run_forward(inp.gates_in, inp.whh, inp.bias2)
    dg = run_backward(inp.whh, inp.dy, act, c)

    def grads(dg_, y_):
        return (torch.einsum('btdgj,dgjk->btk', dg_, inp.wih), torch.einsum('btdgj,btk->dgjk', dg_, inp.x),
                torch.einsum('btdgj,btdk->dgjk', dg_, prev_step(y_)), dg_.sum((0, 1)))
    rel = [float((a - b).norm() / (b.norm() + 1e-300)) for a, b in zip(grads(st['dg'], st['y']), grads(dg, y))]
    return float((st['y'] - y).abs().max()), max(rel)


def passes_old(inp, st):
    ey, rg = old_criteria(inp, st)
    return ey < 3e-2 and rg < 4e-2, (ey, rg)


# ---------------------------------------------------------------------------------------------------------------------
# plan arithmetic of the dispatch tables, restated (csrc/lstm_plan.h and the plan / CASE macros of each generation)
# ---------------------------------------------------------------------------------------------------------------------
G1_FWD_NKS = (1, 2, 3, 4, 5, 6, 8, 10)                                          # FWD_CASE, each x MT {1, 2, 4}
G1_BWD = ((1, 1), (1, 2), (1, 4), (1, 8), (2, 8), (4, 4), (5, 4), (3, 4), (2, 4))   # BWD_CASE (NTO, NKS), each x NE {1, 2, 4, 8}
G23_FWD_NKS = (1, 2, 4, 6, 8, 10, 12, 16)                                       # LSTM_G23_NKS (FWD2_CASE / FWD3_CASE)
G23_BWD_NTO = (1, 2, 3, 4, 5, 6, 8)                                             # LSTM_G23_NTO (BWD2_CASE / BWD3_CASE)


def _cdiv(a, b):
    return (a + b - 1) // b


def _first(classes, n):
    return next((c for c in classes if n <= c), None)


def gen1(B, H, bf16, bwd):
    if not bwd:
        if B > 64 or H > 320:
            return None
        nks, mt = _cdiv(H, 32), _cdiv(B, 16)
        mt = 4 if mt == 3 else mt
        ld = nks * 32 + (8 if bf16 else 4)
        if 2 * mt * 16 * ld * (2 if bf16 else 4) > 150 * 1024 or nks not in G1_FWD_NKS:
            return None
        return 'fwd1<%s,NKS=%d,MT=%d>' % ('bf16' if bf16 else 'fp32', nks, mt)
    if H % 16 or B > 64:
        return None
    nto = _cdiv(H // 16, 4)
    hs = next((c for c in (64, 32, 16, 8) if H % c == 0 and nto * (4 * c // 32) <= 20), 0)
    if not hs:
        return None
    nks, mt, ne, k = 4 * hs // 32, _cdiv(B, 16), _cdiv(B * hs, 256), 4 * hs
    lds = mt * 16 * (k + (8 if bf16 else 4)) * (2 if bf16 else 4) + B * hs * 4
    if lds > 150 * 1024 or (H // hs) * 2 > 200 or B * hs > 256 * 8 or (nto, nks) not in G1_BWD:
        return None
    return 'bwd1<%s,NTO=%d,NKS=%d,NE=%d>' % ('bf16' if bf16 else 'fp32', nto, nks, _first((1, 2, 4, 8), ne))


def gen2(B, H, bf16, bwd):
    if not bf16 or B > 16 or H % 16 or H > 512:
        return None
    if bwd:
        return 'bwd2<NTO=%d>' % _first(G23_BWD_NTO, _cdiv(H // 16, 4))
    return 'fwd2<NKS=%d>' % _first(G23_FWD_NKS, _cdiv(H, 32))


def gen3(B, H, ND, bwd):
    if H % 16 or not 16 <= H <= 512 or not 1 <= B <= 16 * (8 // ND):
        return None
    if bwd:
        return 'bwd3<NTO=%d>' % _first(G23_BWD_NTO, _cdiv(H // 16, 4))
    nks = _first(G23_FWD_NKS, _cdiv(H, 32))
    chmax, ch = (nks + 3) // 4, _cdiv(_cdiv(B, 8 // ND) * (H // 8), 256)
    return 'fwd3<NKS=%d,CH=%d>' % (nks, 1 if ch <= 1 else (min(chmax, 2) if ch <= 2 or chmax <= 2 else chmax))


def route(api, mode, prec, B, H, ND, bwd):
    """the kernel one pass of a case runs: api 'lstm16' (asr_lstm16_*) or 'lstm' (asr_lstm_* under asr_lstm_set_persistent(mode));
    tensors 16-byte aligned, workspace as large as the query asks."""
    if api == 'lstm16':
        return gen3(B, H, ND, bwd)
    r = None
    if mode == 1:
        r = gen2(B, H, prec == BF16, bwd)
    if r is None and mode >= 1:
        r = gen1(B, H, prec == BF16, bwd)
    return r or '%s0<%s,%s>' % ('bwd' if bwd else 'fwd', 'bf16' if prec == BF16 else 'fp32', 'vec' if H % 4 == 0 else 'scalar')


Case = collections.namedtuple('Case', 'api mode prec B T H ND variant')


def case_id(c):
    return '%s%s-%s-B%d-T%d-H%d-ND%d%s' % (c.api, '' if c.api == 'lstm16' else '-m%d' % c.mode, 'bf16' if c.prec else 'fp32', c.B, c.T, c.H, c.ND,
                                           '' if c.variant == 'plain' else '-' + c.variant)


def case_scheme(c):
    return S_B16 if c.api == 'lstm16' else (S_C16 if c.prec == BF16 else S_F32)


def case_routes(c):
    return [route(c.api, c.mode, c.prec, c.B, c.H, c.ND, bwd) for bwd in (False, True)]


H16 = (16, 32, 48, 64, 80, 128, 144, 192, 208, 256, 272, 320, 336, 384, 400, 512)


def _t(k):
    return 4 + k % 5                     # T in 4..8


def _gen3_cases():
    out, k = [], 0
    for H in H16:
        # B = 4: one-row slices; B = 64: full 16-row slices; B = 32 (8 rows) is where NKS >= 10 takes CH = 2
        for B in (4, 64, 32):
            r = gen3(B, H, 2, False)
            if B == 4 or all(gen3(c.B, H, 2, False) != r for c in out if c.H == H):
                out.append(Case('lstm16', 1, BF16, B, _t(k), H, 2, 'plain'))
                k += 1
    for H in (64, 320, 512):
        out.append(Case('lstm16', 1, BF16, 9, _t(k), H, 1, 'plain'))
        k += 1
    return out


def _gen2_cases():
    return [Case('lstm', 1, BF16, B, _t(i + j), H, 2, 'plain') for i, H in enumerate(H16) for j, B in enumerate((1, 16))]


def _reachable_gen1(bwd):
    return sorted({gen1(B, H, bf, bwd) for B in range(1, 65) for H in range(1, 513) for bf in (False, True)} - {None})


def _gen1_cases():
    """greedy: walk the issue's shapes, keep a shape when one of its two passes launches an instantiation not launched yet"""
    fwd_shapes = [(B, H) for H in (20, 32, 64, 72, 96, 128, 160, 192, 256, 320) for B in (5, 18, 33, 64)]
    bwd_shapes = [(B, H) for H in (16, 32, 64, 96, 128, 160, 224, 256, 320) for B in (3, 8, 16, 24, 40, 64)]
    out, seen = [], set()
    for k, ((B, H), prec) in enumerate(itertools.product(fwd_shapes + bwd_shapes, (FP32, BF16))):
        c = Case('lstm', 2, prec, B, _t(k), H, 1 + (k // 2) % 2, 'plain')
        new = {r for r in case_routes(c) if r[3] == '1'} - seen
        if new:
            out.append(c)
            seen |= new
    return out


def _step_cases():
    return [Case('lstm', 0, prec, B, _t(i + j), H, 2 - (i + j) % 2, 'plain')
            for i, H in enumerate((20, 37, 64, 320)) for j, B in enumerate((1, 17)) for prec in (FP32, BF16)]


# one small H per generation (+ H = 320 for the third): (api, mode, prec, B, H)
EDGE_TARGETS = (('lstm16', 1, BF16, 5, 32), ('lstm16', 1, BF16, 5, 320), ('lstm', 1, BF16, 5, 32), ('lstm', 2, FP32, 5, 32),
                ('lstm', 2, BF16, 5, 32), ('lstm', 0, FP32, 5, 20), ('lstm', 0, BF16, 5, 20))


def _edge_cases():
    out = []
    for api, mode, prec, B, H in EDGE_TARGETS:
        out += [Case(api, mode, prec, B, T, H, 2, 'plain') for T in (1, 2, 3, 4, 5, 9)]
        out.append(Case(api, mode, prec, 3, 130, H, 2, 'plain'))
        out += [Case(api, mode, prec, B, 6, H, 2, v) for v in ('sat', 'zero_in', 'zero_dy')]
    for H in (32, 320):
        out += [Case('lstm16', 1, BF16, B, 5, H, ND, 'plain') for B, ND in ((1, 2), (9, 2), (63, 2), (128, 1), (7, 1))]
    return out


GEN3_CASES, GEN2_CASES, GEN1_CASES, STEP_CASES, EDGE_CASES = _gen3_cases(), _gen2_cases(), _gen1_cases(), _step_cases(), _edge_cases()
INST_CASES = GEN3_CASES + GEN2_CASES + GEN1_CASES + STEP_CASES
ALL_CASES = INST_CASES + EDGE_CASES
EPOCH_CASE = Case('lstm16', 1, BF16, 3, 5, 32, 2, 'plain')
EPOCHS = 70


def reachable():
    """every instantiation some accepted shape launches, per entry point"""
    r3 = {gen3(B, H, ND, bwd) for ND in (1, 2) for B in range(1, 129) for H in range(16, 513, 16) for bwd in (False, True)} - {None}
    r2 = {gen2(B, H, True, bwd) for B in range(1, 17) for H in range(16, 513, 16) for bwd in (False, True)}
    return r3, r2, set(_reachable_gen1(False)) | set(_reachable_gen1(True))


def unreachable():
    r3, r2, r1 = reachable()
    out = []
    for bf in ('fp32', 'bf16'):
        out += ['fwd1<%s,NKS=%d,MT=%d>' % (bf, n, m) for n in G1_FWD_NKS for m in (1, 2, 4)]
        out += ['bwd1<%s,NTO=%d,NKS=%d,NE=%d>' % (bf, a, b, e) for a, b in G1_BWD for e in (1, 2, 4, 8)]
    out += ['fwd2<NKS=%d>' % n for n in G23_FWD_NKS] + ['bwd2<NTO=%d>' % n for n in G23_BWD_NTO]
    out += ['fwd3<NKS=%d,CH=%d>' % (n, ch) for n in G23_FWD_NKS for ch in sorted({1, min((n + 3) // 4, 2), (n + 3) // 4})]
    out += ['bwd3<NTO=%d>' % n for n in G23_BWD_NTO]
    return [i for i in out if i not in r3 | r2 | r1]


def table_lines():
    return ['  %-44s fwd %-26s bwd %s' % ((case_id(c),) + tuple(case_routes(c))) for c in INST_CASES]


def unreachable_lines():
    u = unreachable()
    return ['  ' + ' '.join(u[i:i + 4]) for i in range(0, len(u), 4)]


# ---------------------------------------------------------------------------------------------------------------------
# CPU checks
# ---------------------------------------------------------------------------------------------------------------------
def test_unforced_float64_parity_with_oracle_and_autograd():
    from oracle import asr_oracle as O
    for B, T, H, ND, with_b2 in ((3, 5, 20, 2, True), (2, 1, 16, 1, False), (4, 7, 37, 2, False), (1, 2, 16, 2, True)):
        inp = make_inputs(B, T, H, ND, False, with_b2)
        P = {}
        for d, sfx in enumerate(('', '_reverse')[:ND]):
            P['weight_ih_l0' + sfx] = inp.wih[d].reshape(4 * H, DIN)
            P['weight_hh_l0' + sfx] = inp.whh[d].reshape(4 * H, H)
            P['bias_ih_l0' + sfx] = inp.b_ih[d].reshape(4 * H)
            P['bias_hh_l0' + sfx] = (inp.bias2[d].reshape(4 * H) if with_b2 else torch.zeros(4 * H, dtype=F64))
        y_or = O.bilstm(inp.x, P, '', ND == 2).view(B, T, ND, H)
        # the input projection in float64 here (make_inputs forms it in fp32, as the kernels receive it)
        pre = (torch.einsum('btk,dgjk->btdgj', inp.x, inp.wih) + inp.b_ih).requires_grad_(True)
        act, c, y = run_forward(pre, inp.whh, inp.bias2)
        assert float((y.detach() - y_or).abs().max()) < 1e-10
        (y * inp.dy).sum().backward()
        dg = run_backward(inp.whh, inp.dy, act.detach(), c.detach())
        assert float((dg - pre.grad).abs().max()) < 1e-10
        # forced on its own outputs, unrounded: the forced functions are the same map
        st = {'act': act.detach(), 'c': c.detach(), 'y': y.detach(), 'dg': dg}
        ra, rc, ry = forced_forward(S_F32, pre.detach(), inp.whh, inp.bias2, st['y'], st['c'])
        rd = forced_backward(S_F32, inp.whh, inp.dy, st['act'], st['c'], st['dg'])
        assert max(float((a - b).abs().max()) for a, b in ((ra, st['act']), (rc, st['c']), (ry, st['y']), (rd, st['dg']))) < 1e-10


def _cpu_shapes():
    """every (scheme, B, T, H, ND, variant, bias2) of the case tables, each once"""
    seen = {}
    for c in ALL_CASES:
        seen.setdefault((case_scheme(c), c.B, c.T, c.H, c.ND, c.variant, c.api == 'lstm'), c)
    return list(seen)


def test_stand_in_headroom():
    """the fp32 emulation of every storage scheme stays 4x inside the forced bounds on every case of the case tables"""
    worst = {}
    for scheme, B, T, H, ND, variant, b2 in _cpu_shapes():
        inp = make_inputs(B, T, H, ND, scheme.store16, b2, variant)
        st = emulate(scheme, inp)
        assert all(v[0] <= 1.0 for v in forced_ratios(scheme, inp, st).values())
        for k, (v, _) in forced_ratios(scheme, inp, st, fp32_part=True).items():
            w = worst.setdefault(scheme.name, {})
            if v > w.get(k, (0, None))[0]:
                w[k] = (v, (B, T, H, ND, variant))
    for s, w in worst.items():
        print('%-7s %s' % (s, '  '.join('%s %.3f %s' % (k, v[0], v[1]) for k, v in w.items())))
    assert set(worst) == {'f32', 'f32c16', 'bf16'}
    for s, w in worst.items():
        for k, v in w.items():
            assert v[0] <= 0.25, (s, k, v)


# name, defect, marked, (B, T, H, ND), input scale.  B = 64, ND = 2 and B = 128, ND = 1 are 16-row slices of the third generation;
# 319 is the K tail column of H = 320.
DEFECTS = (('a', ('stale_h', 1, 37), True, (64, 8, 320, 2), 1 / 32), ('b', ('drop_col',), True, (64, 8, 320, 2), 1 / 32),
           ('c', ('zero_carry', 0, 31, 4), True, (64, 8, 320, 2), 1.0), ('d', ('swap_if', 1, 5), False, (64, 8, 320, 2), 1.0),
           ('e', ('rev_start',), False, (64, 8, 320, 2), 1.0), ('f', ('c0_stale', 0), False, (64, 8, 320, 2), 1.0),
           ('g', ('trunc_gate', 1), False, (64, 8, 320, 2), 1.0))


@pytest.mark.parametrize('scheme', [S_C16, S_B16], ids=lambda s: s.name)
def test_planted_defects(scheme):
    clean_seen = set()
    for name, defect, marked, (B, T, H, ND), scale in DEFECTS:
        if defect[0] == 'trunc_gate' and not scheme.store16:
            continue
        inp = make_inputs(B, T, H, ND, scheme.store16, not scheme.store16, scale=scale)
        if (B, ND, scale) not in clean_seen:                # the stand-in without a defect passes both sets of criteria on these inputs
            clean_seen.add((B, ND, scale))
            clean = emulate(scheme, inp)
            assert all(v[0] <= 0.25 for v in forced_ratios(scheme, inp, clean, fp32_part=True).values())
            ok, figs = passes_old(inp, clean)
            assert ok, figs
        st = emulate(scheme, inp, defect)
        rs = forced_ratios(scheme, inp, st)
        ok, figs = passes_old(inp, st)
        print('defect (%s) %-10s %s B%d ND%d scale %.3f: forced %s | old criteria: y %.2e grads %.2e -> %s' % (
            name, defect[0], scheme.name, B, ND, scale, '  '.join('%s %.1f' % (k, v[0]) for k, v in rs.items()), figs[0], figs[1],
            'pass' if ok else 'fail'))
        assert max(v[0] for v in rs.values()) > 1.0, 'defect (%s) not caught by the forced check' % name
        if marked:
            assert ok, 'defect (%s) is meant to pass the old criteria: %s' % (name, figs)


def test_case_tables_cover_every_reachable_instantiation():
    r3, r2, r1 = reachable()
    launched = {r for c in ALL_CASES for r in case_routes(c)}
    assert not (r3 | r2 | r1) - launched, sorted((r3 | r2 | r1) - launched)
    assert {'%s0<%s,%s>' % (p, b, v) for p in ('fwd', 'bwd') for b in ('fp32', 'bf16') for v in ('vec', 'scalar')} <= launched
    assert all('bwd1<%s,NTO=1,NKS=1,NE=%d>' % (b, e) in unreachable() for b in ('fp32', 'bf16') for e in (1, 2, 4, 8))
    for line in table_lines() + unreachable_lines():
        assert line in __doc__, line
    assert len({case_id(c) for c in ALL_CASES}) == len(ALL_CASES)
    for c in ALL_CASES:
        assert (c.T in (1, 2, 3, 130) or 4 <= c.T <= 9) and c.variant in VARIANTS


if __name__ == '__main__':
    print('\n'.join(table_lines()))
    print('\n'.join(unreachable_lines()))
