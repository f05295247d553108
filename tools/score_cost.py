#!/usr/bin/env python3
"""Cost of scoring a transcript: tiny in the headline config (bf16 encoder, fp32 decoder and K/V), B = 64.
Prints JSON lines and appends them to --out (default profiles/score_cost.jsonl).

Line "score_vs_greedy": two legs in the same process, host-timed whole passes (encoder included), interleaved so that drift hits both
alike, median of --reps with min..max:
  (a) greedy   transcribe_batch(return_logprobs=True, ignore_eot=True): 4 prompt ids + 1 + 195 loop steps = 200 ids per row
  (b) score    Whisper.score of those 200 ids per row (context_len 4): the same decoder positions, teacher-forced
and the score pass's split by HIP events on its stream (wm_score_phases; median over the same passes): encoder / prefill chunks + row
collection / final LayerNorm / vocabulary sweep / merge + sums.  For the sweep: its FLOPs on the split path (six bf16 MFMA products of
2·M·N·K), the achieved FLOP/s, the bytes it requests (the fp32 embedding once per 128-row block, the three operand images once per
vocabulary part, the partials) and their rate, the time the MFMAs alone need at the dense bf16 MFMA peak (--peak-tflops, 16 x the
157.3 TFLOP/s fp32 matrix rate) and the achieved fraction of that bound.

Line "bench" (with --parent DIR, a built checkout of the parent commit): `bench.py --gpus 1 --steps S --warmup W --no-extras` in
child processes — parent, this commit, parent — with the ids of the last step dumped and compared.

    python tools/score_cost.py [--reps 7] [--parent DIR] [--out profiles/score_cost.jsonl]"""
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
    ap.add_argument("--peak-tflops", type=float, default=16 * 157.3)
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit: also run bench.py there and here")
    ap.add_argument("--bench-steps", type=int, default=16)
    ap.add_argument("--bench-warmup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_cost.jsonl"))
    a = ap.parse_args()
    from whisper_mojo_amd import DT_BF16, DT_F32, GELU_ERF, POS_HF, WhisperConfig, synth
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.tiny()
    B, max_loop = 64, 195
    prompt = [50258, 50259, 50359, 50363]
    mels = np.stack([synth.synth_mel(cfg, 100 + b) for b in range(B)])
    m = Whisper(cfg, compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=B)
    m.load(WeightLoader.from_array(synth.synth_weights(cfg, 0)))
    greedy = lambda: m.transcribe_batch(mels, prompt=prompt, eot=50257, max_loop=max_loop, ignore_eot=True, return_logprobs=True)
    ids, (glp, _) = greedy()
    assert all(len(r) == len(prompt) + 1 + max_loop for r in ids)
    score = lambda: m.score(mels, ids, context_len=len(prompt))
    legs = dict(greedy=greedy, score=score)
    ts = {k: [] for k in legs}
    ph = []
    for rep in range(2 + a.reps):
        for k, f in legs.items():
            t0 = time.perf_counter()
            f()
            if rep >= 2:
                ts[k].append((time.perf_counter() - t0) * 1e3)
                if k == "score":
                    ph.append(m.score_phases(0))
    slp, _ = score()
    err = max(float(np.abs(np.asarray(slp[b][len(prompt):]) - np.asarray(glp[b][len(prompt):])).max()) for b in range(B))
    med = {k: float(np.median(v)) for k, v in ts.items()}
    M = B * (len(ids[0]) - 1)
    N, K = cfg.vocab_size, cfg.d_model
    flops = 6 * 2.0 * M * N * K
    phases = {k: float(np.median([p[k] for p in ph])) for k in ph[0]}
    blocks, parts = (M + 127) // 128, 32  # csrc/kernels_score.hip: SCORE_ROWS, score_parts(51865, fp32)
    sweep_bytes = blocks * N * K * 4.0 + parts * M * K * 6.0 + M * parts * 12.0 + M * 8.0
    sweep_s = phases["sweep"] * 1e-3
    bound_ms = flops / (a.peak_tflops * 1e12) * 1e3
    line = json.dumps(dict(what="score_vs_greedy", rows=B, ids_per_row=len(ids[0]), reps=a.reps, M=M,
                           greedy_ms=med["greedy"], greedy_min_max=[min(ts["greedy"]), max(ts["greedy"])],
                           score_ms=med["score"], score_min_max=[min(ts["score"]), max(ts["score"])],
                           score_over_greedy=med["score"] / med["greedy"], phases_ms=phases, phases_sum_ms=sum(phases.values()),
                           sweep_row_blocks=blocks, sweep_parts=parts, sweep_workgroups=blocks * parts,
                           sweep_bf16_mfma_flops=flops, sweep_tflops=flops / sweep_s / 1e12, sweep_bytes=sweep_bytes,
                           sweep_gb_per_s=sweep_bytes / sweep_s / 1e9, sweep_ms_at_mfma_peak=bound_ms, peak_tflops=a.peak_tflops,
                           sweep_fraction_of_mfma_bound=bound_ms / phases["sweep"], max_abs_logprob_diff=err))
    print(line)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    m.close()
    if a.parent:
        runs = []
        with tempfile.TemporaryDirectory() as tmp:
            for i, (tag, root) in enumerate((("parent", a.parent), ("commit", ROOT), ("parent", a.parent))):
                ids = os.path.join(tmp, f"ids{i}.npy")
                out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup),
                                      "--no-extras", "--dump-ids", ids], cwd=root, capture_output=True, text=True, timeout=600, check=True)
                res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
                runs.append(dict(tree=tag, ms_per_step=res["ms_per_step"], value=res["value"], ids=np.load(ids)))
        same = all(np.array_equal(runs[0]["ids"], r["ids"]) for r in runs[1:])
        line = json.dumps(dict(what="bench", steps=a.bench_steps, warmup=a.bench_warmup, ids_identical=bool(same),
                               runs=[{k: v for k, v in r.items() if k != "ids"} for r in runs]))
        print(line)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        assert same


if __name__ == "__main__":
    main()
