#!/usr/bin/env python3
"""Cost of sequential long-form transcription: tiny in the headline config (bf16 encoder, fp32 decoder and K/V),
64 ragged synthetic recordings of 60-300 s, passes of 32 rows (two in flight).  Prints one JSON line:
audio seconds per wall second, windows decoded, passes the scheduler ran and the share of their rows that were spare, long
log-mel time per audio hour, and the window loop's time against the same number of plain 32-row timestamp passes
(transcribe_submit on two slots, first windows of the recordings).

    python tools/long_form_cost.py [--n 64] [--rows 32]
    python tools/long_form_cost.py --trace <rocprofv3 kernel_trace.csv>   # GPU busy / idle within the window loop"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def trace_idle(path):
    rows = list(csv.DictReader(open(path)))
    iv = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows)
    marks = [i for i, r in enumerate(iv) if "window_gather" in r[2]]
    t0, t1 = iv[marks[0]][0], max(e for _, e, _ in iv[marks[0]:])
    busy, cur_s, cur_e, gaps = 0, None, None, []
    for s, e, _ in iv[marks[0]:]:
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                busy += cur_e - cur_s
                gaps.append(s - cur_e)
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    busy += cur_e - cur_s
    gaps = np.asarray(gaps or [0], np.float64)
    return dict(loop_ms=(t1 - t0) / 1e6, busy_ms=busy / 1e6, idle_ms=(t1 - t0 - busy) / 1e6, idle_frac=round(1 - busy / (t1 - t0), 4),
                gaps_over_50us=int((gaps > 5e4).sum()), longest_gap_ms=float(gaps.max()) / 1e6, windows_gathered=len(marks))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--max-loop", type=int, default=120)
    ap.add_argument("--trace")
    a = ap.parse_args()
    if a.trace:
        print(json.dumps(trace_idle(a.trace)))
        return
    from oracle import logmel_oracle as lo
    from oracle import oracle
    from whisper_mojo_amd import DT_BF16, DT_F32, GELU_ERF, POS_HF, WhisperConfig, _lib, frontend
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.tiny()
    m = Whisper(cfg, compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=a.rows)
    m.load(WeightLoader.from_array(oracle.synth_weights_c(cfg, 0)))
    rng = np.random.default_rng(0)
    secs = rng.uniform(60, 300, a.n)
    audios = [lo.synth_audio(500 + i, int(s * 16000)) for i, s in enumerate(secs)]
    kw = dict(prompt=(50258, 50259, 50359), eot=50257, max_loop=a.max_loop, timestamps=(50364, 50363, 50))
    # warm-up (states, graphs, code objects) with the same batch, so the timed call runs on the same two decode states
    frontend.transcribe_audio_long_form(m, [x[:16000 * 3] for x in audios], **kw)
    buf, n, stride = frontend._pack(audios)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    nf = np.zeros(a.n, np.int32)
    t0 = time.perf_counter()
    _lib.check(_lib.lib().wm_log_mel_long(m._h, buf.ctypes.data_as(fp), n.ctypes.data_as(ip), a.n, stride, None, nf.ctypes.data_as(ip)))
    t_mel = time.perf_counter() - t0
    t0 = time.perf_counter()
    res, stats = frontend.transcribe_audio_long_form(m, audios, return_stats=True, **kw)
    t_all = time.perf_counter() - t0
    passes = stats["passes"]
    # the same number of plain passes of `rows` first windows, two slots in flight, timestamps on
    mels = frontend.log_mel(m, audios[:a.rows])
    t0 = time.perf_counter()
    for p in range(passes):
        if p >= 2:
            m.transcribe_wait(p % 2)
        m.transcribe_submit(mels, slot=p % 2, **kw)
    for p in range(max(0, passes - 2), passes):
        m.transcribe_wait(p % 2)
    t_plain = time.perf_counter() - t0
    audio_s = float(secs.sum())
    print(json.dumps(dict(recordings=a.n, audio_s=round(audio_s, 1), rows=a.rows, max_loop=a.max_loop, windows=stats["windows"],
                          stalled=stats["stalled"], passes=passes, rows_run=stats["rows"],
                          spare_row_share=round(1 - stats["windows"] / stats["rows"], 4), segments=sum(len(r["segments"]) for r in res),
                          long_form_s=round(t_all, 3), audio_s_per_wall_s=round(audio_s / t_all, 1),
                          log_mel_s=round(t_mel, 4), log_mel_s_per_audio_hour=round(t_mel / audio_s * 3600, 4),
                          loop_s=round(t_all - t_mel, 3), plain_passes_s=round(t_plain, 3),
                          loop_over_plain=round((t_all - t_mel) / t_plain, 4))))
    m.close()


if __name__ == "__main__":
    main()
