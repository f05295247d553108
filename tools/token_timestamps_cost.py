#!/usr/bin/env python3
"""Cost of token-level timestamps on the headline-shaped workload: tiny, bf16 encoder with fp32 decoder (the absorbed
cross-attention path), 64 clips per submit, 8 submits in flight, coalesce = 2, 195 fixed steps — timed with and without
return_token_timestamps (alignment heads: four heads of the last two layers).  Prints one JSON line per variant and the ratio.

    python tools/token_timestamps_cost.py [--reps 5]
Under `rocprofv3 --kernel-trace --stats -- python tools/token_timestamps_cost.py --reps 1` the align_* kernels' share shows up."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whisper_mojo_amd import DT_BF16, DT_F32, WhisperConfig, _lib  # noqa: E402
from whisper_mojo_amd.loader import WeightLoader  # noqa: E402
from whisper_mojo_amd.whisper import Whisper  # noqa: E402

HEADS = [(2, 2), (3, 0), (3, 3), (3, 5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=8)
    a = ap.parse_args()
    L = _lib.lib()
    cfg, B = WhisperConfig.tiny(), 64
    w = np.empty(cfg.weight_count(), np.float32)
    d = cfg.dims()
    L.wm_synth_weights(C.byref(d), 0, w.ctypes.data_as(C.POINTER(C.c_float)))
    mels = np.empty((B, cfg.n_mels, cfg.n_frames), np.float32)
    for i in range(B):
        L.wm_synth_mel_host(1000 + i, cfg.n_mels, cfg.n_frames, mels[i].ctypes.data_as(C.POINTER(C.c_float)))
    mel = torch.from_numpy(mels).cuda()
    m = Whisper(cfg, compute_dtype=DT_BF16, kv_dtype=DT_F32, max_batch=B, decoder_fp32=True, coalesce=2)
    m.load(WeightLoader.from_array(w))
    m.set_alignment_heads(HEADS)
    res = {}
    for tt in (False, True, False, True):  # interleaved: drift affects both variants alike
        kw = dict(max_loop=195, ignore_eot=True, return_token_timestamps=tt)
        for s in range(a.inflight):  # warm-up (graph capture, buffer growth)
            m.transcribe_submit(mel, slot=s, **kw)
        for s in range(a.inflight):
            m.transcribe_wait(s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            for s in range(a.inflight):
                m.transcribe_submit(mel, slot=s, **kw)
            for s in range(a.inflight):
                m.transcribe_wait(s)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / (a.reps * a.inflight)
        res.setdefault(tt, []).append(ms)
    for tt in (False, True):
        print(json.dumps({"timestamps": tt, "ms_per_64_clip_pass": [round(x, 3) for x in res[tt]], "clips": B, "inflight": a.inflight,
                          "coalesce": 2, "steps": 195, "heads": len(HEADS)}))
    print(json.dumps({"overhead_rel": round(min(res[True]) / min(res[False]) - 1, 4)}))
    m.close()


if __name__ == "__main__":
    main()
