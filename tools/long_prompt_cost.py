#!/usr/bin/env python3
"""Cost of per-utterance prompts: tiny in the headline config (bf16 encoder, fp32 decoder and K/V), the recordings
and pass size of tools/long_form_cost.py.  Appends JSON lines to stdout (profiles/long_prompt_cost.jsonl keeps one run):

  {"what": "long_form", ...}  wall time per audio second of PCM-in long-form transcription (long log-mel included) with conditioning off, on,
                              and on with prompt_ids; windows, passes and ids emitted.
  {"what": "prefill", ...}    one synchronous pass of `rows` windows, median of `reps`: a 3-id shared prompt, a 3-id per-row prompt and
                              a 227-id per-row prompt (1 + 223 + 3 ids: the longest a conditioned window carries; one row keeps the
                              3-id prompt, so the pass is ragged), each with max_loop = 0 (encoder + prefill + first id) and with a
                              fixed-length loop of `--max-loop` steps.  From these: the long prefill's time (the max_loop = 0
                              difference), the loop's time at either cache length, and the prefill's share of the window's
                              decode time.  These are HOST-timed differences of whole synchronous passes, not device events
                              round the prefill: the long prefill's figure also holds whatever else differs between the two
                              passes (the larger table upload, init_tokens_rows, the host's enqueue of 15 chunks).  DESIGN §16
                              sets the device-side span of a kernel trace beside it.

    python tools/long_prompt_cost.py [--n 64] [--rows 32] [--max-loop 120] [--reps 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 3) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--max-loop", type=int, default=120)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from oracle import logmel_oracle as lo
    from oracle import oracle
    from whisper_mojo_amd import DT_BF16, DT_F32, GELU_ERF, POS_HF, WhisperConfig, frontend
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.tiny()
    m = Whisper(cfg, compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=a.rows)
    m.load(WeightLoader.from_array(oracle.synth_weights_c(cfg, 0)))
    rng = np.random.default_rng(0)
    secs = rng.uniform(60, 300, a.n)
    audios = [lo.synth_audio(500 + i, int(s * 16000)) for i, s in enumerate(secs)]
    init = (50258, 50259, 50359)
    kw = dict(prompt=init, eot=50257, max_loop=a.max_loop, timestamps=(50364, 50363, 50))
    audio_s = float(secs.sum())
    variants = {"off": {}, "condition_on_prev_tokens": dict(condition_on_prev_tokens=True),
                "condition_and_prompt_ids": dict(condition_on_prev_tokens=True, prompt_ids=[50361, 2425, 11, 1002, 318])}
    short = [x[:16000 * 3] for x in audios]
    frontend.transcribe_audio_long_form(m, short, **kw)  # warm-up: states, graphs, code objects
    base = None
    for name, extra in variants.items():
        frontend.transcribe_audio_long_form(m, short, **kw, **extra)
        t0 = time.perf_counter()
        res, st = frontend.transcribe_audio_long_form(m, audios, return_stats=True, **kw, **extra)
        t = time.perf_counter() - t0
        base = base or t
        print(json.dumps(dict(what="long_form", variant=name, recordings=a.n, audio_s=round(audio_s, 1), rows=a.rows, max_loop=a.max_loop,
                              windows=st["windows"], stalled=st["stalled"], passes=st["passes"], ids=sum(len(r["sequence"]) for r in res),
                              loop_s=round(t, 3), ms_per_audio_s=round(t / audio_s * 1e3, 4), over_off=round(t / base, 4))), flush=True)
    # one pass: what the long prefill costs next to the loop it precedes
    win = frontend.log_mel(m, audios[:a.rows])
    long_prompt = [50361] + rng.integers(1000, 40000, 223).tolist() + list(init)
    rows_long = [long_prompt] * (a.rows - 1) + [list(init)]  # one short row: the pass is ragged, Lmax = 227
    fixed = dict(eot=50257, timestamps=(50364, 50363, 50), ignore_eot=True)
    out = dict(what="prefill", rows=a.rows, prompt_ids=len(long_prompt), max_loop=a.max_loop, reps=a.reps)
    for tag, call in (("shared3", lambda n: m.transcribe_batch(win, prompt=init, max_loop=n, **fixed)),
                      ("rows3", lambda n: m.transcribe_batch(win, prompts=[list(init)] * a.rows, max_loop=n, **fixed)),
                      ("rows227", lambda n: m.transcribe_batch(win, prompts=rows_long, max_loop=n, **fixed))):
        for n in (0, a.max_loop):
            out[f"{tag}_loop{n}_ms"], out[f"{tag}_loop{n}_all"] = median_ms(lambda: call(n), a.reps)
    L = a.max_loop
    out["long_prefill_ms"] = round(out["rows227_loop0_ms"] - out["rows3_loop0_ms"], 3)
    out["loop_ms_short_cache"] = round(out["rows3_loop%d_ms" % L] - out["rows3_loop0_ms"], 3)
    out["loop_ms_long_cache"] = round(out["rows227_loop%d_ms" % L] - out["rows227_loop0_ms"], 3)
    out["per_row_path_over_shared"] = round(out["rows3_loop%d_ms" % L] / out["shared3_loop%d_ms" % L], 4)
    out["prefill_share_of_decode"] = round(out["long_prefill_ms"] / out["loop_ms_long_cache"], 4)
    print(json.dumps(out), flush=True)
    m.close()


if __name__ == "__main__":
    main()
