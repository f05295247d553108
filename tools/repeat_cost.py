#!/usr/bin/env python3
"""Cost of the repetition processors: tiny in the headline config (bf16 encoder, fp32 decoder and K/V), B = 64, one
fixed-length pass with the options off, with repetition_penalty only, with no_repeat_ngram_size only and with both.  Prints JSON lines
and writes them to --out (default profiles/repeat_cost.jsonl), one per setting:

  {"what": "step", "setting": "off" | "p" | "n" | "both", "pass_ms": ..., "step_us": ..., "extra_step_us": ...}

step_us = (median pass at --max-loop steps - median pass at --short steps) / (their difference): the encoder, the prefill and the
init launch cancel, what is left is the replayed step graph.  extra_step_us: over "off".  Host-timed whole passes, the four settings
interleaved so that drift hits them alike.

    python tools/repeat_cost.py [--max-loop 120] [--short 20] [--reps 7] [--out profiles/repeat_cost.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = {"off": {}, "p": dict(repetition_penalty=1.3), "n": dict(no_repeat_ngram_size=3),
            "both": dict(repetition_penalty=1.3, no_repeat_ngram_size=3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-loop", type=int, default=120)
    ap.add_argument("--short", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repeat_cost.jsonl"))
    a = ap.parse_args()
    from whisper_mojo_amd import DT_BF16, DT_F32, GELU_ERF, POS_HF, WhisperConfig, synth
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.tiny()
    w = synth.synth_weights(cfg, 0)
    mels = np.stack([synth.synth_mel(cfg, 100 + b) for b in range(64)])
    kw = dict(prompt=(50258, 50259, 50359), eot=50257, timestamps=(50364, 50363, 50), ignore_eot=True)
    m = Whisper(cfg, compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=64)
    m.load(WeightLoader.from_array(w))
    ts = {(s, L): [] for s in SETTINGS for L in (a.short, a.max_loop)}
    for key in list(ts) * 2:  # warm-up: state, both graphs, code objects
        m.transcribe_batch(mels, max_loop=key[1], **SETTINGS[key[0]], **kw)
    for _ in range(a.reps):
        for key in ts:
            t0 = time.perf_counter()
            m.transcribe_batch(mels, max_loop=key[1], **SETTINGS[key[0]], **kw)
            ts[key].append((time.perf_counter() - t0) * 1e3)
    m.close()
    step = {s: (float(np.median(ts[(s, a.max_loop)])) - float(np.median(ts[(s, a.short)]))) / (a.max_loop - a.short) * 1e3 for s in SETTINGS}
    lines = []
    for s in SETTINGS:
        long_ = ts[(s, a.max_loop)]
        lines.append(json.dumps(dict(what="step", setting=s, options=SETTINGS[s], rows=64, max_loop=a.max_loop, short=a.short, reps=a.reps,
                                     pass_ms=round(float(np.median(long_)), 3), pass_minmax=[round(min(long_), 3), round(max(long_), 3)],
                                     step_us=round(step[s], 2), extra_step_us=round(step[s] - step["off"], 2))))
        print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
