#!/usr/bin/env python3
"""Cost of Whisper-medium: WhisperConfig.medium() at its true dims — 24 + 24 layers, 1500 / 448 contexts, 51 865 ids — in
the headline precision (bf16 encoder, fp32 decoder and K/V), B = 64, synthetic weights.  Prints one JSON line and appends it to --out
(default profiles/medium_cost.jsonl):

  encoder_ms         the encoder of 64 clips, HIP events on the library's stream (wm_bench_kernel KERNEL_ENCODER)
  decode_step_us     one decode step of 64 rows alone, HIP events over a chain of steps (KERNEL_DECODE_STEP)
  pass_ms            a whole synchronous 64-clip pass (encoder + prefill + --max-loop steps), host-timed, median of --reps after
                     two warm-up passes (states, graphs, code objects), as the other tools/*_cost.py do
  ids_in_range, b2_equals_b1   the run doubles as the full-size check: every id inside the vocabulary, rows 0 and 1 decoded as a
                     batch of 2 equal to the same rows of the 64-row pass

No target is set for these numbers: they are recorded, not judged.

    python tools/medium_cost.py [--max-loop 99] [--reps 5] [--out profiles/medium_cost.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-loop", type=int, default=99)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "medium_cost.jsonl"))
    a = ap.parse_args()
    import torch
    from whisper_mojo_amd import DT_BF16, DT_F32, WhisperConfig, _lib, synth
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.medium()
    B = 64
    t0 = time.perf_counter()
    n = cfg.weight_count()
    w = np.empty(n, np.float32)
    dims = cfg.dims()
    assert _lib.lib().wm_synth_weights(C.byref(dims), 0, w.ctypes.data_as(C.POINTER(C.c_float))) == n  # the C generator
    mels = synth.synth_mels(cfg, 100, B)
    t_synth = time.perf_counter() - t0
    m = Whisper(cfg, compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True, max_batch=B)
    m.load(WeightLoader.from_array(w))
    del w
    mel_dev = torch.from_numpy(mels).cuda()
    kw = dict(prompt=(50258, 50259, 50359, 50363), eot=50257, max_loop=a.max_loop, ignore_eot=True)
    ts = []
    ids = None
    for rep in range(2 + a.reps):
        t0 = time.perf_counter()
        ids = m.transcribe_batch(mel_dev, **kw)
        if rep >= 2:
            ts.append((time.perf_counter() - t0) * 1e3)
    in_range = all(0 <= t < cfg.vocab_size for r in ids for t in r) and all(len(r) == 4 + 1 + a.max_loop for r in ids)
    pair = m.transcribe_batch(mel_dev[:2], **kw)
    L = _lib.lib()
    st = C.c_void_p()
    _lib.check(L.wm_state_new(m._h, B, C.byref(st)))
    _lib.check(L.wm_encode(m._h, st, C.c_void_p(mel_dev.data_ptr()), 1, B, None))
    step_us, enc_us = C.c_float(), C.c_float()
    _lib.check(L.wm_bench_kernel(m._h, st, _lib.KERNEL_DECODE_STEP, 50, C.byref(step_us)))
    _lib.check(L.wm_bench_kernel(m._h, st, _lib.KERNEL_ENCODER, 3, C.byref(enc_us)))
    L.wm_state_free(st)
    line = json.dumps(dict(what="medium_cost", dims=[cfg.d_model, cfg.n_heads, cfg.n_layers, cfg.vocab_size, cfg.ffn], rows=B,
                           precision="bf16 encoder, fp32 decoder + KV", max_loop=a.max_loop, reps=a.reps,
                           encoder_ms=round(enc_us.value / 1e3, 3), decode_step_us=round(step_us.value, 1),
                           pass_ms=round(float(np.median(ts)), 2), pass_min_max=[round(min(ts), 2), round(max(ts), 2)],
                           ids_in_range=bool(in_range), b2_equals_b1=bool(pair == ids[:2]), synth_seconds=round(t_synth, 1)))
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    m.close()
    assert in_range and pair == ids[:2]


if __name__ == "__main__":
    main()
