#!/usr/bin/env python3
"""Cost of log-probabilities: tiny in the headline config (bf16 encoder, fp32 decoder and K/V), one fixed-length pass
with and without return_logprobs, same B and steps.  Prints JSON lines and writes them to --out (default profiles/logprobs_cost.jsonl):

  {"what": "pass", "rows": 64, ...}      synchronous pass of B = 64 rows (dec_logits_split_kernel<3,4>), median of --reps
  {"what": "pass", "rows": 128, ...}     two coalesced 64-row submits on the 128-row pair state (dec_logits_split128_kernel<3>),
                                         wall time from the first submit to the second wait

Host-timed whole passes (encoder included), interleaved plain / log-prob so that drift hits both alike.

    python tools/logprobs_cost.py [--max-loop 120] [--reps 7] [--out profiles/logprobs_cost.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-loop", type=int, default=120)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logprobs_cost.jsonl"))
    a = ap.parse_args()
    from whisper_mojo_amd import DT_BF16, DT_F32, GELU_ERF, POS_HF, WhisperConfig, synth
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.tiny()
    w = synth.synth_weights(cfg, 0)
    mels = np.stack([synth.synth_mel(cfg, 100 + b) for b in range(64)])
    kw = dict(prompt=(50258, 50259, 50359), eot=50257, max_loop=a.max_loop, timestamps=(50364, 50363, 50), ignore_eot=True)
    lines = []
    for rows in (64, 128):
        m = Whisper(cfg, compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=64,
                    coalesce=2 if rows == 128 else 0)
        m.load(WeightLoader.from_array(w))

        def run(lp):
            if rows == 64:
                m.transcribe_batch(mels, return_logprobs=lp, **kw)
            else:
                m.transcribe_submit(mels, slot=0, return_logprobs=lp, **kw)
                m.transcribe_submit(mels, slot=1, return_logprobs=lp, **kw)
                m.transcribe_wait(0)
                m.transcribe_wait(1)

        ts = {False: [], True: []}
        for lp in (False, True, False, True):  # warm-up: states, both graphs, code objects
            run(lp)
        for _ in range(a.reps):
            for lp in (False, True):
                t0 = time.perf_counter()
                run(lp)
                ts[lp].append((time.perf_counter() - t0) * 1e3)
        plain, lpm = float(np.median(ts[False])), float(np.median(ts[True]))
        lines.append(json.dumps(dict(what="pass", rows=rows, max_loop=a.max_loop, reps=a.reps, plain_ms=round(plain, 3), lp_ms=round(lpm, 3),
                              plain_minmax=[round(min(ts[False]), 3), round(max(ts[False]), 3)],
                              lp_minmax=[round(min(ts[True]), 3), round(max(ts[True]), 3)], lp_over_plain=round(lpm / plain, 4),
                              per_step_us=round((lpm - plain) / a.max_loop * 1e3, 2))))
        print(lines[-1], flush=True)
        m.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
