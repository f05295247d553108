#!/usr/bin/env python3
"""Cost of wm_resample_pcm beside a plain device copy of the same bytes: B = 64 rows of 30 s and one row of 30 minutes, at
44 100 and 48 000 Hz, float32 in, input and output both on the device.  One JSON line per case.

Timed on the host around the blocking call (median of 9 after a warm-up call, which also builds the rate's table): the call uploads
the B lengths, launches resample_kernel and zero_tails_kernel on the model's stream and waits for them, so the figure holds that fixed
cost as well as the kernels.  The floor is timed the same way: one device copy of the input bytes plus one of the output bytes
(torch copy_, then a synchronize).  Recorded, not judged.

    python tools/resample_cost.py >> profiles/resample_cost.jsonl"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps=9):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def main():
    import torch
    from whisper_mojo_amd import GELU_ERF, POS_HF, WhisperConfig, _lib, synth
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.micro()
    m = Whisper(cfg, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=64)
    m.load(WeightLoader.from_array(synth.synth_weights(cfg, 0)))
    ip = C.POINTER(C.c_int32)
    for sr in (44100, 48000):
        for name, B, seconds in (("64 x 30 s", 64, 30), ("1 x 30 min", 1, 1800)):
            n_in = sr * seconds
            n_out = _lib.resample_len(n_in, sr)
            src = torch.rand((B, n_in), dtype=torch.float32, device="cuda") - 0.5
            dst = torch.empty((B, n_out), dtype=torch.float32, device="cuda")
            src2, dst2 = torch.empty_like(src), torch.empty_like(dst)
            torch.cuda.synchronize()
            lens, got = np.full(B, n_in, np.int32), np.zeros(B, np.int32)

            def run():
                _lib.check(_lib.lib().wm_resample_pcm(m._h, C.c_void_p(src.data_ptr()), _lib.WM_F32, 1, lens.ctypes.data_as(ip), B, n_in, sr,
                                                      C.c_void_p(dst.data_ptr()), 1, n_out, got.ctypes.data_as(ip)))

            def copy():
                src2.copy_(src)
                dst2.copy_(dst)
                torch.cuda.synchronize()

            t, f = timed(run), timed(copy)
            assert got.tolist() == [n_out] * B and bool(torch.isfinite(dst).all())
            print(json.dumps({"case": name, "sr_in": sr, "rows": B, "in_bytes": src.numel() * 4, "out_bytes": dst.numel() * 4,
                              "resample": t, "copy_floor": f, "ratio": round(t["median_ms"] / f["median_ms"], 2)}), flush=True)
            del src, dst, src2, dst2
            torch.cuda.empty_cache()
    m.close()


if __name__ == "__main__":
    main()
