#!/usr/bin/env python3
"""Cost of the top-k alternatives: tiny in the headline config (bf16 encoder, fp32 decoder and K/V), fixed-length
synchronous passes of B = 64 rows with return_logprobs alone and with top_k = 1, 5, 8.  Prints JSON lines and writes them to --out
(default profiles/topk_cost.jsonl), one per mode:

  {"top_k": 0 | 1 | 5 | 8, "pass_ms": ..., "pass_minmax": [...], "step_us": ..., "over_logprobs": ..., "step_over_logprobs_us": ...}

pass_ms: host-timed whole pass of --max-loop steps (encoder included), median of --reps, the four modes interleaved so that drift hits
all alike.  step_us: one decode step, as the slope between that pass and one of half the steps (the library brackets no single loop step
of a log-prob pass with events; prefill, encoder and launch ramp cancel in the difference), median of the same reps.

    python tools/topk_cost.py [--max-loop 120] [--reps 5] [--out profiles/topk_cost.jsonl]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_cost.jsonl"))
    a = ap.parse_args()
    from whisper_mojo_amd import DT_BF16, DT_F32, GELU_ERF, POS_HF, WhisperConfig, synth
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.tiny()
    w = synth.synth_weights(cfg, 0)
    mels = np.stack([synth.synth_mel(cfg, 100 + b) for b in range(64)])
    kw = dict(prompt=(50258, 50259, 50359), eot=50257, timestamps=(50364, 50363, 50), ignore_eot=True, return_logprobs=True)
    m = Whisper(cfg, compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=64)
    m.load(WeightLoader.from_array(w))
    modes, half = (0, 1, 5, 8), a.max_loop // 2

    def run(k, steps):
        t0 = time.perf_counter()
        m.transcribe_batch(mels, max_loop=steps, top_k=k or None, **kw)
        return (time.perf_counter() - t0) * 1e3

    for k in modes + modes:  # warm-up: the state, every mode's graph, code objects
        run(k, a.max_loop)
    full, slope = {k: [] for k in modes}, {k: [] for k in modes}
    for _ in range(a.reps):
        for k in modes:
            t_full, t_half = run(k, a.max_loop), run(k, half)
            full[k].append(t_full)
            slope[k].append((t_full - t_half) / (a.max_loop - half) * 1e3)
    base, base_step = float(np.median(full[0])), float(np.median(slope[0]))
    lines = []
    for k in modes:
        p, s = float(np.median(full[k])), float(np.median(slope[k]))
        lines.append(json.dumps(dict(top_k=k, rows=64, max_loop=a.max_loop, reps=a.reps, pass_ms=round(p, 3),
                                     pass_minmax=[round(min(full[k]), 3), round(max(full[k]), 3)], step_us=round(s, 2),
                                     over_logprobs=round(p / base, 4), step_over_logprobs_us=round(s - base_step, 2))))
        print(lines[-1], flush=True)
    m.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
