#!/usr/bin/env python3
"""Generates the log-probability fixtures on the CPU from HF transformers' own code, for wm_transcribe_lp.

  logprobs_{micro,tiny}_hf.npz
      HF-mode greedy decoding (fp32) of single synthetic recordings (the weights and clips of tools/make_golden.py, the options of
      tools/make_golden_prompts.py) through SuppressTokensLogitsProcessor, SuppressTokensAtBeginLogitsProcessor and
      WhisperTimeStampLogitsProcessor, the order generate applies them in.  Cases: "shared" (one prompt, suppress lists and timestamp
      rules on), "off" (suppress lists, rules off), "rows" (a prompt per recording, 1 .. 20 ids, rules on; one recording at a time, as
      the prompt fixtures are).  Per row: the prompt, prompt + generated ids, per generated id log_softmax(processed scores)[id], and
      WhisperGenerationMixin._retrieve_avg_logprobs(scores, ids, 0.0) called as HF's own static method.  micro also stores every
      step's RAW logits (float32) for the CPU restatement (tests/test_logprobs_ref.py); tiny's would not fit a committed file.

Every stored row survives three draws of 1e-5 relative noise on every step's processed scores (seeds that do not are skipped).

Usage: python tools/make_golden_logprobs.py [micro] [tiny]   (dev container: needs transformers; never at test time)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden import hf_model  # noqa: E402
from make_golden_long_form import N_DRAWS, PERTURB, Perturb, ids_setup  # noqa: E402
from whisper_mojo_amd import WhisperConfig, synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MAX_INIT = 50


@torch.no_grad()
def hf_greedy_lp(m, enc_out, prompt, max_loop, setup, ts_on, sup, bsup, rng=None):
    """-> (ids, logprobs of the generated ids, avg_logprob, raw logits [steps, V])"""
    from types import SimpleNamespace

    from transformers import (SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor,
                              WhisperTimeStampLogitsProcessor)
    from transformers.modeling_outputs import BaseModelOutput
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin as G
    eo = BaseModelOutput(last_hidden_state=enc_out)
    procs = []
    if len(sup):
        procs.append(SuppressTokensLogitsProcessor(list(sup)))
    if len(bsup):
        procs.append(SuppressTokensAtBeginLogitsProcessor(list(bsup), begin_index=len(prompt)))
    if ts_on:
        gc = SimpleNamespace(eos_token_id=setup["eos"], no_timestamps_token_id=setup["no_ts"], max_initial_timestamp_index=MAX_INIT)
        procs.append(WhisperTimeStampLogitsProcessor(gc, begin_index=len(prompt)))
    if rng is not None:
        procs.append(Perturb(rng))
    toks = [int(t) for t in prompt]
    raw, scores_all, gen = [], [], []
    out = m(decoder_input_ids=torch.tensor([toks]), encoder_outputs=eo, use_cache=True)
    for _ in range(1 + max_loop):
        scores = out.logits[:, -1].float()
        raw.append(scores[0].numpy().copy())
        ids = torch.tensor([toks])
        for p in procs:
            scores = p(ids, scores.clone())
        nxt = int(scores[0].argmax())
        scores_all.append(scores[0])
        gen.append(nxt)
        toks.append(nxt)
        if nxt == setup["eos"]:
            break
        out = m(decoder_input_ids=torch.tensor([[nxt]]), encoder_outputs=eo, past_key_values=out.past_key_values, use_cache=True)
    lps = np.asarray([float(torch.log_softmax(s, -1)[g]) for s, g in zip(scores_all, gen)], np.float32)
    avg = float(G._retrieve_avg_logprobs(tuple(scores_all), torch.tensor(gen), 0.0))
    return np.asarray(toks, np.int32), lps, np.float32(avg), np.stack(raw)


def make(name, cfg, n_shared, n_off, row_lengths, max_loop, keep_raw):
    m = hf_model(cfg, synth.split_weights(cfg, synth.synth_weights(cfg, 0)), False)
    setup = ids_setup(cfg)
    init = setup["prompt"]
    tb = setup["no_ts"] + 1
    rng = np.random.default_rng(23)
    text_hi = min(setup["eos"], 800 if cfg.vocab_size < 2000 else 50000)
    sup = sorted(set(rng.integers(4, text_hi, 12).tolist()))
    bsup = sorted({setup["eos"], int(rng.integers(4, text_hi))})
    out = dict(init=np.asarray(init, np.int32), eos=np.int32(setup["eos"]), no_ts=np.int32(setup["no_ts"]), timestamp_begin=np.int32(tb),
               max_loop=np.int32(max_loop), max_init=np.int32(MAX_INIT), suppress=np.asarray(sup, np.int32),
               begin_suppress=np.asarray(bsup, np.int32), perturb_rel=np.float64(PERTURB))
    rows = 0
    plan = [("shared", 1, len(init))] * n_shared + [("off", 0, len(init))] * n_off + [("rows", 1, L) for L in row_lengths]
    for case, ts_on, L in plan:
        seed = 5000 + 89 * rows
        while True:
            seed += 1
            text = rng.integers(4, text_hi, max(L - len(init), 0)).tolist()
            prompt = (text + init)[-L:] if L >= len(init) else init[:L]
            enc = m.model.encoder(torch.from_numpy(synth.synth_mel(cfg, seed))[None]).last_hidden_state
            ids, lps, avg, raw = hf_greedy_lp(m, enc, prompt, max_loop, setup, ts_on, sup, bsup)
            if all(np.array_equal(ids, hf_greedy_lp(m, enc, prompt, max_loop, setup, ts_on, sup, bsup, rng)[0]) for _ in range(N_DRAWS)):
                break
            print(f"  {name}: row {rows} seed {seed} unstable under noise, next", flush=True)
        k = f"r{rows}_"
        out[k + "case"] = np.array(case)
        out[k + "seed"] = np.int64(seed)
        out[k + "ts"] = np.int32(ts_on)
        out[k + "prompt"] = np.asarray(prompt, np.int32)
        out[k + "ids"] = ids
        out[k + "logprobs"] = lps
        out[k + "avg_logprob"] = avg
        if keep_raw:
            out[k + "raw"] = raw.astype(np.float32)
        print(f"{name}: row {rows} {case} L={L} -> {len(lps)} generated, avg_logprob {avg:.4f}", flush=True)
        rows += 1
    out["n_rows"] = np.int32(rows)
    path = os.path.join(GOLDEN, f"logprobs_{name}_hf.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["micro", "tiny"]
    torch.manual_seed(0)
    if "micro" in which:
        make("micro", WhisperConfig.micro(), 3, 2, (1, 3, 9, 20), 14, True)
    if "tiny" in which:
        make("tiny", WhisperConfig.tiny(), 3, 2, (1, 3, 20), 24, False)
