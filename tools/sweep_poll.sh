#!/bin/bash
# Sweep of the polling delays of the persistent kernels on the bench step (ms per step + recurrence / decoder stage times).
# usage: bash tools/sweep_poll.sh > gpurun_out/sweep_poll.txt
run() {
  env "$@" python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline 2>/dev/null | python3 -c "
import sys, json
for l in sys.stdin:
    if l.startswith('{'):
        d = json.loads(l); s = d['stage_ms_per_step']
        print('%-50s %.3f ms  lstm fwd %.3f bwd %.3f  dec fwd %.3f bwd %.3f' % ('$*', d['ms_per_step'], s['asr_lstm16_fwd'], s['asr_lstm16_bwd'], s['asr_att_decoder_fwd'], s['asr_att_decoder_bwd_ex']))
"
}
run ASR_NOP=1
for f in 0 2 4 8 12; do run ASR_LSTM3_POLL_DELAY_FWD=$f; done
for b in 0 2 6 8 12; do run ASR_LSTM3_POLL_DELAY_BWD=$b; done
for d in 1 2 4; do run ASR_DEC_BWD_POLL_DELAY=$d; done
run ASR_NOP=2
