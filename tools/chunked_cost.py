#!/usr/bin/env python3
"""Cost of chunked long-form transcription beside the sequential algorithm: tiny in the headline config (bf16 encoder,
fp32 decoder and K/V), ONE synthetic recording of 30 minutes.  Prints one JSON line: wall time of transcribe_audio_long_form and of
transcribe_audio_chunked (median of 5 with min / max), the passes each ran, and whether every id is a vocabulary id.

Recorded, not judged: with synthetic weights the two produce different text by construction (the sequential algorithm seeks by the
timestamps it decodes, the chunked one cuts every 25 s), so the ids are not compared.

    python tools/chunked_cost.py [--minutes 30] [--rows 64] [--max-loop 120] >> profiles/chunked_cost.jsonl"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps=5):
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return {"median_s": round(float(np.median(ts)), 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4)}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--max-loop", type=int, default=120)
    a = ap.parse_args()
    from oracle import logmel_oracle as lo
    from oracle import oracle
    from whisper_mojo_amd import DT_BF16, DT_F32, GELU_ERF, POS_HF, WhisperConfig, frontend
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.tiny()
    m = Whisper(cfg, compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=a.rows)
    m.load(WeightLoader.from_array(oracle.synth_weights_c(cfg, 0)))
    audio = lo.synth_audio(730, int(a.minutes * 60 * 16000))
    seq_kw = dict(prompt=(50258, 50259, 50359), eot=50257, max_loop=a.max_loop, timestamps=(50364, 50363, 50))
    chk_kw = dict(prompt=(50258, 50259, 50359, 50363), eot=50257, max_loop=a.max_loop)
    frontend.transcribe_audio_long_form(m, [audio[:16000 * 40]], **seq_kw)  # warm-up: states, graphs, code objects
    frontend.transcribe_audio_chunked(m, audio[:16000 * 40], **chk_kw)
    t_seq, (res, st_seq) = timed(lambda: frontend.transcribe_audio_long_form(m, [audio], return_stats=True, **seq_kw))
    t_chk, (out, st_chk) = timed(lambda: frontend.transcribe_audio_chunked(m, audio, return_stats=True, **chk_kw))
    ok = all(0 <= t < cfg.vocab_size for t in res[0]["sequence"]) and all(0 <= t < 50257 for t in out["sequence"])
    print(json.dumps(dict(model="tiny", operands="bf16 encoder, fp32 decoder and K/V", audio_s=round(len(audio) / 16000, 1), rows=a.rows,
                          max_loop=a.max_loop, sequential=dict(t_seq, passes=st_seq["passes"], windows=st_seq["windows"], ids=len(res[0]["sequence"])),
                          chunked=dict(t_chk, passes=st_chk["passes"], chunks=st_chk["chunks"], ids=len(out["sequence"])),
                          sequential_over_chunked=round(t_seq["median_s"] / t_chk["median_s"], 2), ids_in_range=bool(ok))))
    m.close()


if __name__ == "__main__":
    main()
