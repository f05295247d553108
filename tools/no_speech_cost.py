#!/usr/bin/env python3
"""Cost of the no-speech probe: tiny in the headline config (bf16 encoder, fp32 decoder and K/V).  Prints JSON lines
and writes them to --out (default profiles/no_speech_cost.jsonl):

  {"what": "pass", "rows": 64, ...}    synchronous log-prob pass of B = 64 rows with and without the probe, fixed loop length,
                                       interleaved, median of --reps with min..max
  {"what": "pass", "rows": 128, ...}   two coalesced 64-row submits on the 128-row pair state, first submit to second wait
  {"what": "long", ...}                one long-form run on the same synthetic audio without thresholds, with logprob_threshold
                                       alone, and with both thresholds set between the run's own values

Host-timed whole passes (encoder included), interleaved so that drift hits both alike.  --trace: only a few passes of each kind,
for a kernel trace taken around this tool.

    python tools/no_speech_cost.py [--max-loop 120] [--reps 7] [--trace] [--out profiles/no_speech_cost.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOKEN = 50362  # <|nospeech|>


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-loop", type=int, default=120)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "no_speech_cost.jsonl"))
    a = ap.parse_args()
    from whisper_mojo_amd import DT_BF16, DT_F32, GELU_ERF, POS_HF, WhisperConfig, synth
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.tiny()
    w = synth.synth_weights(cfg, 0)
    mels = np.stack([synth.synth_mel(cfg, 100 + b) for b in range(64)])
    kw = dict(prompt=(50258, 50259, 50359), eot=50257, max_loop=a.max_loop, timestamps=(50364, 50363, 50), ignore_eot=True, return_logprobs=True)
    if a.trace:  # (the kernel tracer has crashed on step graphs that carry the timestamp rules; the probe does not depend on them)
        del kw["timestamps"]
    mk = dict(compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=64)
    lines = []
    for rows in (64, 128):
        m = Whisper(cfg, coalesce=2 if rows == 128 else 0, **mk)
        m.load(WeightLoader.from_array(w))

        def run(ns):
            extra = dict(no_speech_token=TOKEN) if ns else {}
            if rows == 64:
                m.transcribe_batch(mels, **extra, **kw)
            else:
                m.transcribe_submit(mels, slot=0, **extra, **kw)
                m.transcribe_submit(mels, slot=1, **extra, **kw)
                m.transcribe_wait(0)
                m.transcribe_wait(1)

        ts = {False: [], True: []}
        for ns in (False, True, False, True):  # warm-up: states, graph, code objects
            run(ns)
        for _ in range(2 if a.trace else a.reps):
            for ns in (False, True):
                t0 = time.perf_counter()
                run(ns)
                ts[ns].append((time.perf_counter() - t0) * 1e3)
        lp, nsm = float(np.median(ts[False])), float(np.median(ts[True]))
        lines.append(json.dumps(dict(what="pass", rows=rows, max_loop=a.max_loop, reps=len(ts[True]), lp_ms=round(lp, 3), lp_ns_ms=round(nsm, 3),
                                     lp_minmax=[round(min(ts[False]), 3), round(max(ts[False]), 3)],
                                     lp_ns_minmax=[round(min(ts[True]), 3), round(max(ts[True]), 3)], probe_us_per_pass=round((nsm - lp) * 1e3, 1))))
        print(lines[-1], flush=True)
        m.close()
    if not a.trace:
        m = Whisper(cfg, **mk)
        m.load(WeightLoader.from_array(w))
        lengths = [6000 + 1500 * (b % 9) for b in range(32)]
        feats = [synth.synth_long_mel(cfg, 300 + b, n) for b, n in enumerate(lengths)]
        lk = dict(prompt=(50258, 50259, 50359), eot=50257, max_loop=60, timestamps=(50364, 50363, 50))
        probe = m.transcribe_long_form(feats, logprob_threshold=-np.inf, no_speech_token=TOKEN, **lk)
        win = [e for r in probe for e in r["windows"]]
        lt = float(np.median([e["avg_logprob"] for e in win]))
        nt = float(np.median([e["no_speech_prob"] for e in win]))
        forms = dict(plain={}, logprob_only=dict(logprob_threshold=lt, no_speech_token=TOKEN),
                     both=dict(logprob_threshold=lt, no_speech_threshold=nt, no_speech_token=TOKEN))
        ts = {k: [] for k in forms}
        stats = {}
        for rep in range(1 + a.reps):
            for k, extra in forms.items():
                t0 = time.perf_counter()
                _, stats[k] = m.transcribe_long_form(feats, return_stats=True, **extra, **lk)
                if rep:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
        lines.append(json.dumps(dict(what="long", recordings=len(lengths), frames=sum(lengths), reps=a.reps,
                                     **{k + "_ms": round(float(np.median(v)), 2) for k, v in ts.items()},
                                     **{k + "_minmax": [round(min(v), 2), round(max(v), 2)] for k, v in ts.items()},
                                     **{k + "_windows": stats[k]["windows"] for k in forms}, **{k + "_passes": stats[k]["passes"] for k in forms},
                                     skipped=stats["both"]["skipped_windows"])))
        print(lines[-1], flush=True)
        m.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
