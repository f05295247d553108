#!/usr/bin/env python3
"""Cost of n-best scoring: tiny in the headline config (bf16 encoder, fp32 decoder and K/V), 4 clips x 16 candidates
(R = 64 rows) of about 20 ids.  Prints one JSON line and appends it to --out (default profiles/nbest_cost.jsonl).

Two legs on two models in the same process, host-timed whole passes (mel upload and encoder included), interleaved so that drift hits
both alike, two warm-up rounds, then median of --reps with min..max:
  (a) nbest   Whisper.score_candidates(mel[4], 4 x 16 candidates)
  (b) score   Whisper.score(mel[utt_of] = 64 repeated mel rows, the same 64 id rows)
and both passes' split by HIP events on the pass's stream (wm_score_phases, median over the same passes): encoder / prefill chunks +
row collection / final LayerNorm / vocabulary sweep / merge + sums (+ the ranking launch in the n-best leg).  The per-row results of
the two legs are compared bit for bit on the way.  Device memory: the drop of free device memory (hipMemGetInfo through torch) over
each model's FIRST pass, which is when its 64-row state is created — both forms allocate a 64-row state, so this shows what the arena
holds, not a saving.

    python tools/nbest_cost.py [--reps 7] [--out profiles/nbest_cost.jsonl]"""
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nbest_cost.jsonl"))
    a = ap.parse_args()
    import torch
    from whisper_mojo_amd import DT_BF16, DT_F32, GELU_ERF, POS_HF, WhisperConfig, synth
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.tiny()
    U, N = 4, 16
    R = U * N
    r = np.random.default_rng(40)
    prompt = [50258, 50259, 50359, 50363]
    cands = [[prompt + r.integers(0, 50257, int(r.integers(14, 19))).tolist() for _ in range(N)] for _ in range(U)]
    flat = [c for g in cands for c in g]
    mels = np.stack([synth.synth_mel(cfg, 100 + u) for u in range(U)])
    rep_mels = np.ascontiguousarray(mels[np.repeat(np.arange(U), N)])
    w = synth.synth_weights(cfg, 0)

    def model():
        m = Whisper(cfg, compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=R)
        m.load(WeightLoader.from_array(w))
        return m

    free = lambda: torch.cuda.mem_get_info()[0]
    ms = {"nbest": model(), "score": model()}
    legs = {"nbest": lambda: ms["nbest"].score_candidates(mels, cands, context_len=len(prompt)),
            "score": lambda: ms["score"].score(rep_mels, flat, context_len=len(prompt))}
    mem, first = {}, {}
    for k, f in legs.items():  # the first pass of each model creates its state
        torch.cuda.synchronize()
        f0 = free()
        out = f()
        mem[k] = f0 - free()
        first[k] = out
    nb, (lps, (sm, avg)) = first["nbest"], first["score"]
    assert [x for d in nb for x in d["token_logprobs"]] == lps
    assert np.array_equal(np.concatenate([d["sum_logprob"] for d in nb]).view(np.uint32), np.asarray(sm).view(np.uint32))
    ts = {k: [] for k in legs}
    ph = {k: [] for k in legs}
    for rep in range(2 + a.reps):
        for k, f in legs.items():
            t0 = time.perf_counter()
            f()  # synchronous: returns after the results are on the host
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= 2:
                ts[k].append(dt)
                ph[k].append(ms[k].score_phases(0))
    med = lambda v: float(np.median(v))
    line = {"what": "nbest_vs_repeated_score", "model": "tiny", "precision": "bf16 encoder, fp32 decoder + K/V", "clips": U, "candidates_per_clip": N,
            "rows": R, "ids_per_row": [min(map(len, flat)), max(map(len, flat))], "reps": a.reps, "per_row_results_identical": True,
            "device": torch.cuda.get_device_name(0)}
    for k in legs:
        line[k] = {"pass_ms": {"median": round(med(ts[k]), 3), "min": round(min(ts[k]), 3), "max": round(max(ts[k]), 3)},
                   "phases_ms": {p: {"median": round(med([x[p] for x in ph[k]]), 3), "min": round(min(x[p] for x in ph[k]), 3),
                                     "max": round(max(x[p] for x in ph[k]), 3)} for p in ph[k][0]},
                   "first_pass_device_memory_mb": round(mem[k] / 2 ** 20, 1)}
    e = {k: line[k]["phases_ms"]["encoder"]["median"] for k in legs}
    p = {k: line[k]["phases_ms"]["prefill"]["median"] for k in legs}
    line["encoder_ratio_nbest_over_score"] = round(e["nbest"] / e["score"], 4)
    line["prefill_ratio_nbest_over_score"] = round(p["nbest"] / p["score"], 4)
    line["pass_ratio_nbest_over_score"] = round(line["nbest"]["pass_ms"]["median"] / line["score"]["pass_ms"]["median"], 4)
    for m in ms.values():
        m.close()
    s = json.dumps(line)
    print(s)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
