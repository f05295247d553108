#!/usr/bin/env python3
"""Cost of token timestamps in long-form transcription: tiny at its true dims in the headline precision (bf16 encoder,
fp32 decoder and K/V), synthetic weights, a few 75 s recordings (three windows each), 4 alignment heads.  transcribe_long_form with
and without return_token_timestamps, whole calls host-timed and interleaved in one process, median of --reps with min and max after
two warm-up calls of each (states, buffers, graphs, code objects).  Prints one JSON line and appends it to --out.

No target is set for these numbers: they are recorded, not judged.

    python tools/long_token_times_cost.py [--recordings 8] [--max-loop 60] [--reps 5] [--out profiles/long_token_times_cost.jsonl]"""
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
    ap.add_argument("--recordings", type=int, default=8)
    ap.add_argument("--max-loop", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_token_times_cost.jsonl"))
    a = ap.parse_args()
    import ctypes as C
    from whisper_mojo_amd import DT_BF16, DT_F32, GELU_ERF, POS_HF, WhisperConfig, _lib, synth
    from whisper_mojo_amd.config import ALIGNMENT_HEADS_TINY
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.tiny()
    w = np.empty(cfg.weight_count(), np.float32)
    dims = cfg.dims()
    assert _lib.lib().wm_synth_weights(C.byref(dims), 0, w.ctypes.data_as(C.POINTER(C.c_float))) == w.size  # the C generator
    frames = 7500  # 75 s
    feats = np.stack([synth.synth_long_mel(cfg, 500 + b, frames) for b in range(a.recordings)])
    m = Whisper(cfg, compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=a.recordings)
    m.load(WeightLoader.from_array(w))
    heads = list(ALIGNMENT_HEADS_TINY[:4])
    m.set_alignment_heads(heads)
    kw = dict(prompt=(50258, 50259, 50359), eot=50257, max_loop=a.max_loop, timestamps=(50364, 50363, 50), return_stats=True)
    ts = {False: [], True: []}
    res = {}
    for rep in range(2 + a.reps):
        for tt in (False, True):
            t0 = time.perf_counter()
            res[tt] = m.transcribe_long_form(feats, return_token_timestamps=tt, **kw)
            if rep >= 2:
                ts[tt].append((time.perf_counter() - t0) * 1e3)
    (plain, st0), (timed, st1) = res[False], res[True]
    same = [r["sequence"] for r in plain] == [r["sequence"] for r in timed]
    med = {k: float(np.median(v)) for k, v in ts.items()}
    line = json.dumps(dict(what="long_token_times_cost", model="tiny", precision="bf16 encoder, fp32 decoder + KV", recordings=a.recordings,
                           seconds_each=frames / 100, alignment_heads=heads, max_loop=a.max_loop, reps=a.reps, windows=st1["windows"],
                           passes=st1["passes"], rows=st1["rows"], ids=sum(len(r["sequence"]) for r in timed),
                           plain_ms=round(med[False], 2), plain_min_max=[round(min(ts[False]), 2), round(max(ts[False]), 2)],
                           timestamps_ms=round(med[True], 2), timestamps_min_max=[round(min(ts[True]), 2), round(max(ts[True]), 2)],
                           overhead=round(med[True] / med[False] - 1, 4), same_ids=bool(same)))
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    m.close()
    assert same and st0["windows"] == st1["windows"]


if __name__ == "__main__":
    main()
