#!/usr/bin/env python3
"""Cost of language detection: tiny in the headline config (bf16 encoder, fp32 decoder and K/V), B = 64, fixed loop.
Prints one JSON line and writes it to --out (default profiles/lang_detect_cost.jsonl).  Three legs, host-timed whole passes (encoder
included), interleaved so that drift hits all alike, median of --reps with min..max:

  (a) rows          wm_transcribe_rows with the language given
  (b) lang          wm_transcribe_lang: detection inside the pass
  (c) detect_rows   wm_detect_language, the ids read back, then wm_transcribe_rows with them (the audio is encoded twice)

    python tools/lang_detect_cost.py [--max-loop 120] [--reps 7] [--out profiles/lang_detect_cost.jsonl]"""
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
    ap.add_argument("--max-loop", type=int, default=120)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lang_detect_cost.jsonl"))
    a = ap.parse_args()
    from whisper_mojo_amd import DT_BF16, DT_F32, GELU_ERF, POS_HF, WhisperConfig, synth
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.tokenizer import language_ids
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.tiny()
    B = 64
    mels = np.stack([synth.synth_mel(cfg, 100 + b) for b in range(B)])
    init = [50258, 50259, 50359]
    langs = language_ids()[0]
    kw = dict(eot=50257, max_loop=a.max_loop, timestamps=(50364, 50363, 50), ignore_eot=True)
    m = Whisper(cfg, compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=B)
    m.load(WeightLoader.from_array(synth.synth_weights(cfg, 0)))

    def rows(lang):
        return m.transcribe_batch(mels, prompts=[[init[0], int(lang[b]), init[2]] for b in range(B)], **kw)

    def detect_rows():
        return rows(m.detect_language(mels, langs, sot=init[0])[0])

    fused = lambda: m.transcribe_batch(mels, prompts=[init] * B, n_init=3, detect_language=langs, **kw)
    given = m.detect_language(mels, langs, sot=init[0])[0]
    legs = dict(rows=lambda: rows(given), lang=fused, detect_rows=detect_rows)
    ts = {k: [] for k in legs}
    for rep in range(2 + a.reps):  # two warm-up rounds: states, graph, code objects
        for k, f in legs.items():
            t0 = time.perf_counter()
            f()
            if rep >= 2:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    assert fused()[0] == detect_rows() == rows(given)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    line = json.dumps(dict(what="pass", rows=B, n_lang=len(langs), max_loop=a.max_loop, reps=a.reps,
                           **{k + "_ms": round(v, 3) for k, v in med.items()},
                           **{k + "_minmax": [round(min(v), 3), round(max(v), 3)] for k, v in ts.items()},
                           lang_minus_rows_us=round((med["lang"] - med["rows"]) * 1e3, 1),
                           detect_rows_minus_rows_us=round((med["detect_rows"] - med["rows"]) * 1e3, 1)))
    print(line, flush=True)
    # long form, tools/long_form_cost.py's method: 32 synthetic recordings, whole runs host-timed, interleaved; the pre-pass (one gather,
    # encoder run, [SOT] pass and read-back per group of first windows) is the difference to the run with the languages given
    lengths = [6000 + 1500 * (b % 9) for b in range(32)]
    feats = [synth.synth_long_mel(cfg, 300 + b, n) for b, n in enumerate(lengths)]
    lk = dict(eot=50257, max_loop=60, timestamps=(50364, 50363, 50))
    _, lang = m.transcribe_long_form(feats, prompt=init, detect_language=langs, **lk)
    assert len(set(lang.tolist())) == 1  # (the synthetic model: one language, so the given-language run can share one prompt's slot)
    given_prompt = [init[0], int(lang[0]), init[2]]
    lt = dict(given=[], detect=[])
    stats = {}
    for rep in range(1 + a.reps):
        for k in lt:
            t0 = time.perf_counter()
            if k == "given":
                _, stats[k] = m.transcribe_long_form(feats, prompt=given_prompt, return_stats=True, **lk)
            else:
                _, stats[k], _ = m.transcribe_long_form(feats, prompt=init, detect_language=langs, return_stats=True, **lk)
            if rep:
                lt[k].append((time.perf_counter() - t0) * 1e3)
    lmed = {k: float(np.median(v)) for k, v in lt.items()}
    line2 = json.dumps(dict(what="long", recordings=len(lengths), frames=sum(lengths), reps=a.reps,
                            **{k + "_ms": round(v, 2) for k, v in lmed.items()},
                            **{k + "_minmax": [round(min(v), 2), round(max(v), 2)] for k, v in lt.items()},
                            **{k + "_passes": stats[k]["passes"] for k in lt}, **{k + "_windows": stats[k]["windows"] for k in lt},
                            prepass_ms=round(lmed["detect"] - lmed["given"], 2),
                            prepass_share=round((lmed["detect"] - lmed["given"]) / lmed["detect"], 4)))
    print(line2, flush=True)
    m.close()
    with open(a.out, "w") as f:
        f.write(line + "\n" + line2 + "\n")


if __name__ == "__main__":
    main()
