#!/usr/bin/env python3
"""Cost of the phrase-list constraint: tiny in the headline config (bf16 encoder, fp32 decoder and K/V), B = 64, one
fixed-length pass with the option off, with the repetition processors alone (the instantiation the constraint rides on), with a table
of 16 phrases and with one of 4096 phrases whose root has more than 1000 edges.  Prints JSON lines and writes them to --out (default
profiles/constraint_cost.jsonl):

  {"what": "step", "setting": "off" | "rp" | "ct16" | "ct4096", "pass_ms": ..., "step_us": ..., "extra_step_us": ...}

step_us = (median pass at --max-loop steps - median pass at --short steps) / (their difference): the encoder, the prefill and the
init launches cancel, what is left is the replayed step graph — under a table that is the trie walk and the rewrite of the row's
whole ban set (1621 words, 6.5 KB per row) in the argmax launch.  extra_step_us: over "off".  Host-timed whole passes, the settings
interleaved so that drift hits them alike; ignore_eot keeps every row in the loop (a row that has left the trie still rewrites its set).

    python tools/constraint_cost.py [--max-loop 120] [--short 20] [--reps 7] [--out profiles/constraint_cost.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table(n, fan_out, seed=0):
    """n phrases of 1..4 text ids with fan_out distinct first ids"""
    r = np.random.default_rng(seed)
    heads = r.choice(np.arange(1000, 40000), fan_out, replace=False)
    tails = r.choice(np.arange(1000, 40000), 64, replace=False)
    had = []
    seen = set()
    for h in heads[:n]:
        had.append((int(h),))
        seen.add(had[-1])
    while len(had) < n:
        p = (int(r.choice(heads)),) + tuple(int(t) for t in r.choice(tails, int(r.integers(1, 4))))
        if p not in seen:
            seen.add(p)
            had.append(p)
    return dict(constraint=had)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-loop", type=int, default=120)
    ap.add_argument("--short", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constraint_cost.jsonl"))
    a = ap.parse_args()
    from whisper_mojo_amd import DT_BF16, DT_F32, GELU_ERF, POS_HF, WhisperConfig, synth
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    settings = {"off": {}, "rp": dict(repetition_penalty=1.3, no_repeat_ngram_size=3), "ct16": table(16, 8), "ct4096": table(4096, 1100)}
    cfg = WhisperConfig.tiny()
    w = synth.synth_weights(cfg, 0)
    mels = np.stack([synth.synth_mel(cfg, 100 + b) for b in range(64)])
    kw = dict(prompt=(50258, 50259, 50359), eot=50257, timestamps=(50364, 50363, 50), ignore_eot=True)
    m = Whisper(cfg, compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=64)
    m.load(WeightLoader.from_array(w))
    ts = {(s, L): [] for s in settings for L in (a.short, a.max_loop)}
    for key in list(ts) * 2:  # warm-up: state, graphs, code objects
        m.transcribe_batch(mels, max_loop=key[1], **settings[key[0]], **kw)
    for _ in range(a.reps):
        for key in ts:
            t0 = time.perf_counter()
            m.transcribe_batch(mels, max_loop=key[1], **settings[key[0]], **kw)
            ts[key].append((time.perf_counter() - t0) * 1e3)
    m.close()
    step = {s: (float(np.median(ts[(s, a.max_loop)])) - float(np.median(ts[(s, a.short)]))) / (a.max_loop - a.short) * 1e3 for s in settings}
    lines = []
    for s in settings:
        long_ = ts[(s, a.max_loop)]
        lines.append(json.dumps(dict(what="step", setting=s, phrases=len(settings[s].get("constraint", [])), rows=64, max_loop=a.max_loop,
                                     short=a.short, reps=a.reps, pass_ms=round(float(np.median(long_)), 3),
                                     pass_minmax=[round(min(long_), 3), round(max(long_), 3)], step_us=round(step[s], 2),
                                     extra_step_us=round(step[s] - step["off"], 2))))
        print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
