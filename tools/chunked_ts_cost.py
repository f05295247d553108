#!/usr/bin/env python3
"""Cost of the timestamp modes of chunked long-form transcription: tiny in the headline config (bf16 encoder, fp32
decoder and K/V), ONE synthetic recording of 30 minutes, the timestamp rule on in all three runs so that they decode the same
ids.  Prints one JSON line: wall time of transcribe_audio_chunked with return_timestamps off, True and "word" (median of 5 with
min / max), the passes, chunks, segments and ids of each.

Recorded, not judged: "word" adds the alignment-head capture and the align chain to every pass.

    python tools/chunked_ts_cost.py [--minutes 30] [--rows 64] [--max-loop 120] >> profiles/chunked_ts_cost.jsonl"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--max-loop", type=int, default=120)
    a = ap.parse_args()
    from chunked_cost import timed
    from oracle import logmel_oracle as lo
    from oracle import oracle
    from whisper_mojo_amd import DT_BF16, DT_F32, GELU_ERF, POS_HF, WhisperConfig, config, frontend
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.tiny()
    m = Whisper(cfg, compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=a.rows)
    m.load(WeightLoader.from_array(oracle.synth_weights_c(cfg, 0)))
    m.set_alignment_heads(config.ALIGNMENT_HEADS_TINY)
    audio = lo.synth_audio(730, int(a.minutes * 60 * 16000))
    kw = dict(prompt=(50258, 50259, 50359), eot=50257, max_loop=a.max_loop, timestamps=(50364, 50363, 50))
    out = dict(model="tiny", operands="bf16 encoder, fp32 decoder and K/V", audio_s=round(len(audio) / 16000, 1), rows=a.rows, max_loop=a.max_loop)
    seqs = {}
    for name, mode in (("off", False), ("segments", True), ("word", "word")):
        frontend.transcribe_audio_chunked(m, audio[:16000 * 40], return_timestamps=mode, **kw)  # warm-up: states, graphs, code objects
        t, (res, st) = timed(lambda: frontend.transcribe_audio_chunked(m, audio, return_stats=True, return_timestamps=mode, **kw))
        seqs[name] = res["sequence"]
        out[name] = dict(t, passes=st["passes"], chunks=st["chunks"], ids=len(res["sequence"]), segments=len(res.get("segments", [])))
    out["segments_over_off"] = round(out["segments"]["median_s"] / out["off"]["median_s"], 2)
    out["word_over_off"] = round(out["word"]["median_s"] / out["off"]["median_s"], 2)
    out["ids_in_range"] = bool(all(0 <= t < 50257 for s in seqs.values() for t in s))
    print(json.dumps(out))
    m.close()


if __name__ == "__main__":
    main()
