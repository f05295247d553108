#!/usr/bin/env python3
"""Generates the forced-alignment fixtures tests/golden/align_{micro,tiny}_hf.npz from HF transformers' own code.

Per case: a synthetic clip (mel seed), an id row y and a context length.  The reference is what the issue of forced alignment
states: model(input_features, decoder_input_ids=y[:, :-1], output_attentions=True), its cross-attentions handed to
WhisperGenerationMixin._extract_token_timestamps with sequences = y, num_input_ids = context_len, time_precision 0.02 and
(second variant) num_frames.  The models are the synthetic ones of tools/make_golden.py in HF semantics.

Cases (every one must be found; the generator walks seeds until a case's times survive a 1e-5 relative perturbation of the
attentions, twice, and records the seed): context_len 1; context_len 4; a previous-text context of 30 ids; another clip's greedy
ids; random ids; len = context_len + 1 (no row) and + 2 (one row); 16, 17 and 33 decoder inputs (rows that cross the 16-position
prefill chunks with different left padding in one batch); on tiny one row of 448 ids (the DTW trace in global memory).
micro also stores the selected heads' probabilities of the rows that count.
Usage: python tools/make_golden_align.py   (needs transformers; never at test time)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden import PROMPT, TanhStemGelu, hf_model  # noqa: E402
from make_golden_token_timestamps import HEADS, PERTURB, _Out, _Self, greedy_with_attn  # noqa: E402
from whisper_mojo_amd import WhisperConfig, synth  # noqa: E402


def hf_times(atts, n_ids, ctx, heads, n_layers, num_frames=None):
    """atts: per layer [1, H, n_ids - 1, T] cross-attentions of the teacher-forced pass -> HF's float32 times of the n_ids ids."""
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin
    out = _Out(cross_attentions=(tuple(torch.as_tensor(a) for a in atts),), sequences=torch.zeros((1, n_ids), dtype=torch.long))
    t = WhisperGenerationMixin._extract_token_timestamps(_Self(n_layers), out, heads, time_precision=0.02,
                                                         num_frames=None if num_frames is None else [int(num_frames)],
                                                         num_input_ids=int(ctx))
    return t[0, :n_ids].numpy().astype(np.float32)


@torch.no_grad()
def forced_attentions(m, enc_out, ids):
    from transformers.modeling_outputs import BaseModelOutput
    out = m(decoder_input_ids=torch.tensor([list(ids[:-1])]), encoder_outputs=BaseModelOutput(last_hidden_state=enc_out),
            output_attentions=True, use_cache=False)
    return [a.numpy().copy() for a in out.cross_attentions]


def perturbed(atts, rng):
    return [(a.astype(np.float64) * (1 + PERTURB * rng.standard_normal(a.shape))).astype(np.float32) for a in atts]


@torch.no_grad()
def make(name, cfg):
    heads = HEADS[name]
    w = synth.split_weights(cfg, synth.synth_weights(cfg, 0))
    m = hf_model(cfg, w, False)
    prompt = list(PROMPT if cfg.vocab_size > 50363 else [1, 2, 3, 4])
    T, V = cfg.n_audio_ctx, cfg.vocab_size

    def encode(seed):
        with TanhStemGelu(False):
            return m.model.encoder(torch.from_numpy(synth.synth_mel(cfg, seed))[None]).last_hidden_state

    def greedy(seed, start, steps):
        ids, _ = greedy_with_attn(m, encode(seed), np.asarray(start, np.int32), steps, False)
        return ids.tolist()

    def rand(rng, n):
        return rng.integers(0, V, n).tolist()

    # (case name, builder(seed, rng) -> (ids, context_len)); the mel of a case is synth_mel(cfg, seed)
    cases = [
        ("ctx1", lambda s, r: (greedy(s, prompt[:1], 12), 1)),
        ("ctx4", lambda s, r: (greedy(s, prompt, 20), 4)),
        ("prev_text", lambda s, r: (greedy(s, rand(r, 26) + prompt, 10), 30)),
        ("other_clip", lambda s, r: (greedy(s + 500, prompt, 18), 4)),
        ("random", lambda s, r: (rand(r, 25), 3)),
        ("rows0", lambda s, r: (prompt + rand(r, 1), 4)),
        ("rows1", lambda s, r: (prompt + rand(r, 2), 4)),
        ("in16", lambda s, r: (greedy(s, prompt, 12), 4)),      # 17 ids = 16 inputs: exactly one chunk
        ("in17", lambda s, r: (greedy(s, prompt[:2], 15), 2)),  # 18 ids = 17 inputs: one position into the second chunk
        ("in33", lambda s, r: (greedy(s, prompt, 29), 4)),      # 34 ids = 33 inputs: three chunks
    ]
    if name == "tiny":
        cases.append(("len448", lambda s, r: (prompt + rand(r, 444), 4)))
    out = dict(heads=np.asarray(heads, np.int32), perturb_rel=np.float64(PERTURB), names=np.array([c[0] for c in cases]))
    seed = 7000 if name == "micro" else 8000
    for cname, build in cases:
        while True:
            seed += 1
            rng = np.random.default_rng(seed)
            ids, ctx = build(seed, rng)
            atts = forced_attentions(m, encode(seed), ids)
            nf = int(rng.integers(T // 2, 2 * T + 1))
            res = {}
            ok = True
            for tag, fr in (("times", None), ("times_nf", nf)):
                base = hf_times(atts, len(ids), ctx, heads, cfg.n_layers, fr)
                for _ in range(2):
                    ok = ok and np.array_equal(hf_times(perturbed(atts, rng), len(ids), ctx, heads, cfg.n_layers, fr), base)
                res[tag] = base
            if ok:
                break
            print(f"{name} {cname}: seed {seed} rejected (DTW path moves under {PERTURB} relative noise)", flush=True)
        assert len(ids) == {"in16": 17, "in17": 18, "in33": 34, "len448": 448}.get(cname, len(ids))
        k = cname + "_"
        out[k + "seed"], out[k + "ids"], out[k + "context_len"] = np.int64(seed), np.asarray(ids, np.int32), np.int32(ctx)
        out[k + "n_frames"], out[k + "times"], out[k + "times_nf"] = np.int32(nf), res["times"], res["times_nf"]
        if name == "micro":  # [n_sel, R, T]: the rows that count
            out[k + "probs"] = np.stack([atts[l][0, h, ctx:] for l, h in heads]).astype(np.float32)
        print(f"{name} {cname}: seed {seed} len {len(ids)} ctx {ctx} n_frames {nf}", flush=True)
    path = os.path.join(ROOT, "tests", "golden", f"align_{name}_hf.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    make("micro", WhisperConfig.micro())
    make("tiny", WhisperConfig.tiny())
