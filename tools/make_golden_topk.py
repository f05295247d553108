#!/usr/bin/env python3
"""Generates the top-k fixture on the CPU from HF transformers' own code.

  topk_micro_hf.npz
      HF-mode greedy decoding (fp32) of single synthetic recordings of the micro architecture (the weights and clips of
      tools/make_golden.py, the options and processors of tools/make_golden_logprobs.py, applied in generate's order), with
      (`return_timestamps`: the timestamp rules on) and without them.  Per row: the prompt, prompt + generated ids, every step's RAW
      logits (float32) and, of every step's processed scores — what generate(output_scores=True) hands back —
      scores.log_softmax(-1).topk(8): ids and values.

Every stored row survives three draws of 1e-5 relative noise on every step's processed scores (seeds that do not are skipped), and
at most 2 % of its (position, rank) pairs lie within the project's fp32 margin of 1e-3 of a neighbouring rank's score (the share of
id comparisons the GPU tests may skip; tests/test_topk_ref.py asserts it): a seed over that is skipped too.

Usage: python tools/make_golden_topk.py   (dev container: needs transformers; never at test time)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden import hf_model  # noqa: E402
from make_golden_logprobs import MAX_INIT  # noqa: E402
from make_golden_long_form import N_DRAWS, PERTURB, Perturb, ids_setup  # noqa: E402
from whisper_mojo_amd import WhisperConfig, synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
K = 8
MARGIN, SKIP_CAP = 1e-3, 0.02


@torch.no_grad()
def hf_greedy_topk(m, enc_out, prompt, max_loop, setup, ts_on, sup, bsup, rng=None):
    """-> (ids, raw logits [steps, V], top ids [steps, K], top log-probs [steps, K], (position, rank) pairs within MARGIN of a neighbour)"""
    from types import SimpleNamespace

    from transformers import (SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor,
                              WhisperTimeStampLogitsProcessor)
    from transformers.modeling_outputs import BaseModelOutput
    eo = BaseModelOutput(last_hidden_state=enc_out)
    procs = [SuppressTokensLogitsProcessor(list(sup)), SuppressTokensAtBeginLogitsProcessor(list(bsup), begin_index=len(prompt))]
    if ts_on:
        gc = SimpleNamespace(eos_token_id=setup["eos"], no_timestamps_token_id=setup["no_ts"], max_initial_timestamp_index=MAX_INIT)
        procs.append(WhisperTimeStampLogitsProcessor(gc, begin_index=len(prompt)))
    if rng is not None:
        procs.append(Perturb(rng))
    toks = [int(t) for t in prompt]
    raw, top_i, top_v, close = [], [], [], 0
    out = m(decoder_input_ids=torch.tensor([toks]), encoder_outputs=eo, use_cache=True)
    for _ in range(1 + max_loop):
        scores = out.logits[:, -1].float()
        raw.append(scores[0].numpy().copy())
        ids = torch.tensor([toks])
        for p in procs:
            scores = p(ids, scores.clone())
        nxt = int(scores[0].argmax())
        v, i = scores[0].log_softmax(-1).topk(K)
        g = -np.diff(scores[0].double().topk(K + 1).values.numpy())  # rank r to rank r + 1, r = 0 .. K - 1
        near = np.concatenate([[False], g[:-1] <= MARGIN]) | (g <= MARGIN)
        close += int((near & np.isfinite(v.numpy())).sum())
        top_i.append(i.numpy().astype(np.int32))
        top_v.append(v.numpy().astype(np.float32))
        toks.append(nxt)
        if nxt == setup["eos"]:
            break
        out = m(decoder_input_ids=torch.tensor([[nxt]]), encoder_outputs=eo, past_key_values=out.past_key_values, use_cache=True)
    return np.asarray(toks, np.int32), np.stack(raw), np.stack(top_i), np.stack(top_v), close


def make(max_loop=14, plan=((1, 2), (0, 2))):
    cfg = WhisperConfig.micro()
    m = hf_model(cfg, synth.split_weights(cfg, synth.synth_weights(cfg, 0)), False)
    setup = ids_setup(cfg)
    prompt = setup["prompt"]
    tb = setup["no_ts"] + 1
    rng = np.random.default_rng(41)
    text_hi = min(setup["eos"], 800)
    sup = sorted(set(rng.integers(4, text_hi, 12).tolist()))
    bsup = sorted({setup["eos"], int(rng.integers(4, text_hi))})
    out = dict(prompt=np.asarray(prompt, np.int32), eos=np.int32(setup["eos"]), no_ts=np.int32(setup["no_ts"]), timestamp_begin=np.int32(tb),
               max_loop=np.int32(max_loop), max_init=np.int32(MAX_INIT), suppress=np.asarray(sup, np.int32),
               begin_suppress=np.asarray(bsup, np.int32), perturb_rel=np.float64(PERTURB), k=np.int32(K))
    rows = 0
    for ts_on, n in plan:
        for _ in range(n):
            seed = 7000 + 97 * rows
            while True:
                seed += 1
                enc = m.model.encoder(torch.from_numpy(synth.synth_mel(cfg, seed))[None]).last_hidden_state
                ids, raw, ti, tv, close = hf_greedy_topk(m, enc, prompt, max_loop, setup, ts_on, sup, bsup)
                if close > SKIP_CAP * np.isfinite(tv).sum():
                    print(f"  row {rows} seed {seed}: {close} pairs within the margin, next", flush=True)
                    continue
                if all(np.array_equal(ids, hf_greedy_topk(m, enc, prompt, max_loop, setup, ts_on, sup, bsup, rng)[0]) for _ in range(N_DRAWS)):
                    break
                print(f"  row {rows} seed {seed} unstable under noise, next", flush=True)
            k = f"r{rows}_"
            out[k + "seed"] = np.int64(seed)
            out[k + "ts"] = np.int32(ts_on)
            out[k + "ids"] = ids
            out[k + "raw"] = raw.astype(np.float32)
            out[k + "top_ids"] = ti
            out[k + "top_logprobs"] = tv
            print(f"row {rows} ts={ts_on} seed {seed} -> {len(ti)} generated", flush=True)
            rows += 1
    out["n_rows"] = np.int32(rows)
    path = os.path.join(GOLDEN, "topk_micro_hf.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    torch.manual_seed(0)
    make()
