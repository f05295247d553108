#!/usr/bin/env python3
"""Generates the transcript-scoring fixtures on the CPU from HF transformers' own forward, for wm_score.

  score_{micro,tiny}_hf.npz
      fp32, HF positions, the synthetic weights (seed 0) and clips (synth.synth_mel) of tools/make_golden.py.  Per row: the clip's
      seed, the ids y (decoder prompt + hypothesis), context_len, and from
      model(input_features, decoder_input_ids=y[:-1]).logits.float().log_softmax(-1): logprobs [len] (0 at t = 0), their sum and mean
      over t >= context_len, neg_loss = -model(..., labels=y[1:] with -100 on the context).loss (HF's own reduction), and top_ids
      [len]: the arg-max at every position that survives three draws of 1e-5 relative noise on the logits (N_DRAWS / PERTURB of
      tools/make_golden_long_form.py), -1 where it does not (and at t = 0).  At most 5 % of a file's positions may be -1: the
      random rows are redrawn until that holds.  micro also stores the RAW logits of its rows of at most RAW_MAX_LEN ids for the CPU
      restatement (tests/test_score_ref.py: greedy rows with a context above 1, random ids, length 2); the long rows' and tiny's would
      make the file larger than the existing fixtures.
      Rows: the greedy ids of the clip (logprobs_*_hf.npz row 0), the greedy ids of ANOTHER clip (row 1's ids on a different seed), a
      uniformly random id sequence, a row of length 2, a row at full context (n_text_ctx ids), and a row with a long previous-text
      context in front of the initial ids (context_len = its length).

Usage: python tools/make_golden_score.py [micro] [tiny]   (dev container: needs transformers; never at test time)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden import hf_model  # noqa: E402
from make_golden_long_form import N_DRAWS, PERTURB, ids_setup  # noqa: E402
from whisper_mojo_amd import WhisperConfig, synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MAX_UNASSERTED = 0.05
RAW_MAX_LEN = 24


@torch.no_grad()
def hf_score(m, cfg, seed, y, ctx, rng):
    """-> (logprobs [len], sum, mean, neg_loss, top_ids [len], raw logits [len - 1, V])"""
    mel = torch.from_numpy(synth.synth_mel(cfg, seed))[None]
    yt = torch.tensor([list(map(int, y))])
    z = m(input_features=mel, decoder_input_ids=yt[:, :-1]).logits[0].float()
    lsm = z.log_softmax(-1)
    lp = np.zeros(len(y), np.float32)
    lp[1:] = lsm[torch.arange(len(y) - 1), yt[0, 1:]].numpy()
    labels = yt[:, 1:].clone()
    labels[:, :ctx - 1] = -100
    loss = float(m(input_features=mel, decoder_input_ids=yt[:, :-1], labels=labels).loss)
    top = np.full(len(y), -1, np.int32)
    base = z.argmax(-1).numpy()
    ok = np.ones(len(y) - 1, bool)
    for _ in range(N_DRAWS):
        noise = torch.from_numpy(rng.standard_normal(tuple(z.shape))).to(z.dtype)
        ok &= (z * (1 + PERTURB * noise)).argmax(-1).numpy() == base
    top[1:] = np.where(ok, base, -1)
    s = float(lp[ctx:].astype(np.float64).sum())
    return lp, np.float32(s), np.float32(s / (len(y) - ctx)), np.float32(-loss), top, z.numpy().astype(np.float32)


def make(name, cfg, keep_raw):
    m = hf_model(cfg, synth.split_weights(cfg, synth.synth_weights(cfg, 0)), False)
    setup = ids_setup(cfg)
    init = list(setup["prompt"])
    lpf = np.load(os.path.join(GOLDEN, f"logprobs_{name}_hf.npz"))
    text_hi = min(setup["eos"], 800 if cfg.vocab_size < 2000 else 50000)
    ctx_n = cfg.n_text_ctx
    attempt = 0
    while True:
        rng = np.random.default_rng(41 + attempt)
        g0, g1 = lpf["r0_ids"].tolist(), lpf["r1_ids"].tolist()
        n_prev = min(ctx_n // 2 - 1, ctx_n - len(g0) - 1)
        prev = rng.integers(4, text_hi, n_prev).tolist()
        rows = [
            ("greedy", int(lpf["r0_seed"]), g0, len(lpf["r0_prompt"])),
            ("other_clip", int(lpf["r0_seed"]) + 1000, g1, len(lpf["r1_prompt"])),
            ("random", 7100 + attempt, rng.integers(0, cfg.vocab_size, 24).tolist(), 1),
            ("len2", 7200 + attempt, init[:1] + [int(rng.integers(4, text_hi))], 1),
            ("full_context", 7300 + attempt, (init + rng.integers(4, text_hi, ctx_n).tolist())[:ctx_n], len(init)),
            ("prev_text", int(lpf["r0_seed"]), prev + g0[len(lpf["r0_prompt"]) - len(init):], n_prev + len(init)),
        ]
        out = dict(n_rows=np.int32(len(rows)), perturb_rel=np.float64(PERTURB), n_text_ctx=np.int32(ctx_n))
        total = unasserted = 0
        for i, (case, seed, y, ctx) in enumerate(rows):
            lp, sm, mean, nl, top, raw = hf_score(m, cfg, seed, y, ctx, rng)
            k = f"r{i}_"
            out[k + "case"] = np.array(case)
            out[k + "seed"] = np.int64(seed)
            out[k + "ids"] = np.asarray(y, np.int32)
            out[k + "context_len"] = np.int32(ctx)
            out[k + "logprobs"] = lp
            out[k + "sum"] = sm
            out[k + "mean"] = mean
            out[k + "neg_loss"] = nl
            out[k + "top_ids"] = top
            if keep_raw and len(y) <= RAW_MAX_LEN:
                out[k + "raw"] = raw
            total += len(y) - 1
            unasserted += int((top[1:] < 0).sum())
            print(f"{name}: row {i} {case} len {len(y)} ctx {ctx} mean {mean:.4f} -loss {nl:.4f} unstable top {int((top[1:] < 0).sum())}", flush=True)
        if unasserted <= MAX_UNASSERTED * total:
            break
        attempt += 1
        print(f"  {name}: {unasserted} of {total} positions unstable under noise, next seeds", flush=True)
    assert unasserted <= MAX_UNASSERTED * total
    path = os.path.join(GOLDEN, f"score_{name}_hf.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["micro", "tiny"]
    torch.manual_seed(0)
    if "micro" in which:
        make("micro", WhisperConfig.micro(), True)
    if "tiny" in which:
        make("tiny", WhisperConfig.tiny(), False)
