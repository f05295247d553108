#!/usr/bin/env python3
"""Cost of forced alignment: tiny in the headline config (bf16 encoder, fp32 decoder and K/V), B = 64, 200 ids per
row, 4 alignment heads.  Prints JSON lines and appends them to --out (default profiles/align_cost.jsonl).

Line "align_cost": four legs in the same process, host-timed whole passes (encoder included), interleaved so that drift hits all
alike, median of --reps with min..max:
  (a) greedy_tt   transcribe_batch(return_token_timestamps=True, ignore_eot=True): 4 prompt ids + 1 + 195 loop steps
  (b) score       Whisper.score of those 200 ids per row (context_len 4)
  (c) align_lp    Whisper.align(..., return_logprobs=True) of the same ids
  (d) align       Whisper.align of the same ids, times only
and the align passes' split by HIP events on their stream (wm_align_phases, medians over the same passes): encoder / prefill chunks /
LayerNorm / sweep / merge + sums / align chain.  times_equal_greedy: the align pass returns the greedy pass's own times.

Line "bench" (with --parent DIR, a built checkout of the parent commit): `bench.py --gpus 1 --steps S --warmup W --no-extras` in
child processes — parent, this commit, parent — with the ids of the last step dumped and compared.

    python tools/align_cost.py [--reps 7] [--parent DIR] [--out profiles/align_cost.jsonl]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit: also run bench.py there and here")
    ap.add_argument("--bench-steps", type=int, default=16)
    ap.add_argument("--bench-warmup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_cost.jsonl"))
    a = ap.parse_args()
    from whisper_mojo_amd import DT_BF16, DT_F32, GELU_ERF, POS_HF, WhisperConfig, synth
    from whisper_mojo_amd.config import ALIGNMENT_HEADS_TINY
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.tiny()
    B, max_loop = 64, 195
    prompt = [50258, 50259, 50359, 50363]
    heads = list(ALIGNMENT_HEADS_TINY)[:4]
    mels = np.stack([synth.synth_mel(cfg, 100 + b) for b in range(B)])
    m = Whisper(cfg, compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=B)
    m.load(WeightLoader.from_array(synth.synth_weights(cfg, 0)))
    m.set_alignment_heads(heads)
    greedy = lambda: m.transcribe_batch(mels, prompt=prompt, eot=50257, max_loop=max_loop, ignore_eot=True, return_token_timestamps=True)
    ids, gtimes = greedy()
    assert all(len(r) == len(prompt) + 1 + max_loop for r in ids)
    legs = dict(greedy_tt=greedy, score=lambda: m.score(mels, ids, context_len=len(prompt)),
                align_lp=lambda: m.align(mels, ids, context_len=len(prompt), return_logprobs=True),
                align=lambda: m.align(mels, ids, context_len=len(prompt)))
    ts = {k: [] for k in legs}
    ph = {"align_lp": [], "align": []}
    for rep in range(2 + a.reps):
        for k, f in legs.items():
            t0 = time.perf_counter()
            f()
            if rep >= 2:
                ts[k].append((time.perf_counter() - t0) * 1e3)
                if k in ph:
                    ph[k].append(m.align_phases(0))
    atimes = legs["align"]()
    same = sum(atimes[b] == gtimes[b] for b in range(B))
    med = {k: float(np.median(v)) for k, v in ts.items()}
    phases = {k: {p: float(np.median([x[p] for x in v])) for p in v[0]} for k, v in ph.items()}
    line = json.dumps(dict(what="align_cost", rows=B, ids_per_row=len(ids[0]), heads=len(heads), reps=a.reps,
                           ms={k: med[k] for k in legs}, min_max={k: [min(ts[k]), max(ts[k])] for k in legs},
                           align_over_greedy_tt=med["align"] / med["greedy_tt"], align_lp_over_score=med["align_lp"] / med["score"],
                           phases_ms=phases, rows_with_greedy_times=int(same)))
    print(line)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    m.close()
    if a.parent:
        runs = []
        with tempfile.TemporaryDirectory() as tmp:
            for i, (tag, root) in enumerate((("parent", a.parent), ("commit", ROOT), ("parent", a.parent))):
                idp = os.path.join(tmp, f"ids{i}.npy")
                out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup),
                                      "--no-extras", "--dump-ids", idp], cwd=root, capture_output=True, text=True, timeout=600, check=True)
                res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
                runs.append(dict(tree=tag, ms_per_step=res["ms_per_step"], value=res["value"], ids=np.load(idp)))
        same = all(np.array_equal(runs[0]["ids"], r["ids"]) for r in runs[1:])
        line = json.dumps(dict(what="bench", steps=a.bench_steps, warmup=a.bench_warmup, ids_identical=bool(same),
                               runs=[{k: v for k, v in r.items() if k != "ids"} for r in runs]))
        print(line)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        assert same


if __name__ == "__main__":
    main()
