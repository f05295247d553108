#!/usr/bin/env python3
"""Cost of sequence_bias / bad_words_ids: tiny in the headline config (bf16 encoder, fp32 decoder and K/V), B = 64, one
fixed-length pass with the options off, with the repetition processors alone (the instantiation the sequence options ride on), and
with tables of 16 and of 1024 sequences.  Prints JSON lines and writes them to --out (default profiles/seq_bias_cost.jsonl):

  {"what": "step", "setting": "off" | "rp" | "seq16" | "seq1024", "pass_ms": ..., "step_us": ..., "extra_step_us": ...}

step_us = (median pass at --max-loop steps - median pass at --short steps) / (their difference): the encoder, the prefill and the
init launches cancel, what is left is the replayed step graph.  extra_step_us: over "off".  Host-timed whole passes, the settings
interleaved so that drift hits them alike.  A table: a quarter length-1 biases, the rest sequences of 2..4 ids over a few hundred text
ids, every fourth a bad word; small biases, so hits occur and the stream stays a stream.

    python tools/seq_bias_cost.py [--max-loop 120] [--short 20] [--reps 7] [--out profiles/seq_bias_cost.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table(n, seed=0):
    r = np.random.default_rng(seed)
    pool = r.choice(np.arange(1000, 40000), 400, replace=False)
    bias, bad, had = {}, [], set()
    while len(bias) + len(bad) < n:
        m = 1 if len(had) % 4 == 0 else int(r.integers(2, 5))
        s = tuple(int(t) for t in r.choice(pool, m))
        if s in had:
            continue
        had.add(s)
        if len(had) % 4 == 3 and m > 1:
            bad.append(list(s))
        else:
            bias[s] = float(r.uniform(-0.5, 0.5))
    return dict(sequence_bias=bias, bad_words_ids=bad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-loop", type=int, default=120)
    ap.add_argument("--short", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_bias_cost.jsonl"))
    a = ap.parse_args()
    from whisper_mojo_amd import DT_BF16, DT_F32, GELU_ERF, POS_HF, WhisperConfig, synth
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    settings = {"off": {}, "rp": dict(repetition_penalty=1.3, no_repeat_ngram_size=3), "seq16": table(16), "seq1024": table(1024)}
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
        n_seq = len(settings[s].get("sequence_bias", {})) + len(settings[s].get("bad_words_ids", []))
        lines.append(json.dumps(dict(what="step", setting=s, sequences=n_seq, rows=64, max_loop=a.max_loop, short=a.short, reps=a.reps,
                                     pass_ms=round(float(np.median(long_)), 3), pass_minmax=[round(min(long_), 3), round(max(long_), 3)],
                                     step_us=round(step[s], 2), extra_step_us=round(step[s] - step["off"], 2))))
        print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
