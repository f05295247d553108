#!/usr/bin/env python3
"""Generates the token-level timestamp fixtures (tests/golden/token_timestamps_*.npz) from HF transformers' own code:
WhisperGenerationMixin._extract_token_timestamps (which calls _median_filter and _dynamic_time_warping), with
time_precision 0.02, median_filter_width 7 and num_input_ids = n_prompt — what generate(..., return_token_timestamps=True) runs.

  token_timestamps_tables.npz   attention tensors straight into _extract_token_timestamps: R in {0, 1, 2, 7, 60}, F in {3, 8, 100,
                                1500}, plus tie tables (two-level columns: every z-score is exactly +-1, so the DTW compares equal
                                costs all the time).  Weights are stored as k / 65536 (uint16 k), exact in fp32.
  token_timestamps_{micro,tiny}_{hf,ref}.npz
                                greedy streams of the synthetic models (tools/make_golden.py: same HF architecture, our synthetic
                                weights, HF or REF semantics) with output_attentions=True: per clip the ids of an uncut loop, then
                                the times of the same clip for (a) the uncut loop, (b) the loop cut at a shared `eot` (ragged stop
                                lengths over the clips), each without and with per-clip n_frames.  micro also stores the selected
                                heads' probabilities (the capture known-answer test).

Only inputs whose times are stable are kept: every matrix is also run with its attentions perturbed by 1e-5 relative, and a
table / clip whose DTW path moves is rejected (a new seed is drawn) — an exact-equality bar is only fair on stable inputs.
Usage: python tools/make_golden_token_timestamps.py   (dev container: needs transformers; never at test time)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden import PROMPT, TanhStemGelu, hf_model  # noqa: E402
from whisper_mojo_amd import WhisperConfig, synth  # noqa: E402

N_PROMPT = 4
PERTURB = 1e-5
HEADS = {"micro": [(1, 0), (0, 1), (1, 1)], "tiny": [(3, 1), (1, 4), (2, 2), (3, 5)]}
STEPS = {"micro": 40, "tiny": 40}


class _Out(dict):
    __getattr__ = dict.__getitem__


class _Cfg:
    def __init__(self, n_layers):
        self.decoder_layers = n_layers
        self.median_filter_width = 7


class _Self:
    def __init__(self, n_layers):
        self.config = _Cfg(n_layers)


def hf_times(layers_steps, n_ids, heads, n_layers, num_frames=None):
    """layers_steps: list over generate steps of per-layer [1, H, q, T] attentions (step 0 = prefill with n_prompt rows).
    Returns HF's float32 token times for a sequence of n_ids ids."""
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin
    out = _Out(cross_attentions=tuple(tuple(torch.as_tensor(a) for a in st) for st in layers_steps),
               sequences=torch.zeros((1, n_ids), dtype=torch.long))
    t = WhisperGenerationMixin._extract_token_timestamps(_Self(n_layers), out, heads, time_precision=0.02,
                                                         num_frames=None if num_frames is None else [int(num_frames)],
                                                         num_input_ids=N_PROMPT)
    return t[0, :n_ids].numpy().astype(np.float32)


def table_times(w):
    """w [n_sel, R, F] -> HF times for n_prompt + R + 1 ids (one layer, heads 0..n_sel-1; random prompt rows)."""
    n_sel, R, F = w.shape
    prompt_rows = np.random.default_rng(0).random((1, n_sel, N_PROMPT, F), dtype=np.float32)
    full = np.concatenate([prompt_rows, w[None]], axis=2)
    return hf_times([[full]], N_PROMPT + R + 1, [(0, k) for k in range(n_sel)], 1)


def stable(fn, w, rng):
    base = fn(w)
    for _ in range(2):
        wp = (w.astype(np.float64) * (1 + PERTURB * rng.standard_normal(w.shape))).astype(np.float32)
        if not np.array_equal(fn(wp), base):
            return None
    return base


def make_tables():
    out = {}
    names = []
    seed = 100
    for R in (0, 1, 2, 7, 60):
        for F in (3, 8, 100, 1500):
            n_sel = 1 if R * F > 20000 else 2
            while True:
                seed += 1
                rng = np.random.default_rng(seed)
                q = rng.integers(1, 65536, (n_sel, R, F), dtype=np.uint16)
                w = q.astype(np.float32) / 65536
                t = table_times(w) if R <= 1 else stable(table_times, w, rng)
                if t is not None:
                    break
            name = f"r{R}_f{F}"
            out[name + "_q"], out[name + "_times"] = q, t
            names.append(name)
    for R, F in ((2, 3), (2, 8), (4, 100), (2, 100)):  # ties: two levels per column, every z-score exactly +-1
        seed += 1
        rng = np.random.default_rng(seed)
        lv = np.zeros((1, R, F), np.uint16)
        for j in range(F):
            col = np.array([16384] * (R // 2) + [49152] * (R - R // 2), np.uint16)
            rng.shuffle(col)
            lv[0, :, j] = col
        name = f"tie_r{R}_f{F}"
        out[name + "_q"], out[name + "_times"] = lv, table_times(lv.astype(np.float32) / 65536)
        names.append(name)
    out["names"] = np.array(names)
    out["n_prompt"] = np.int32(N_PROMPT)
    out["perturb_rel"] = np.float64(PERTURB)
    path = os.path.join(ROOT, "tests", "golden", "token_timestamps_tables.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(names), "tables")


@torch.no_grad()
def greedy_with_attn(m, enc_out, prompt, steps, ref_mode):
    """prefill + `steps` greedy steps (no stop): ids and per generate step the per-layer cross-attentions [1, H, q, T]."""
    from transformers.modeling_outputs import BaseModelOutput
    eo = BaseModelOutput(last_hidden_state=enc_out)
    ids = list(prompt)
    out = m(decoder_input_ids=torch.tensor([ids]), encoder_outputs=eo, use_cache=True,
            decoder_position_ids=torch.arange(len(ids))[None], output_attentions=True)
    past, atts = out.past_key_values, [[a.numpy().copy() for a in out.cross_attentions]]
    nxt = int(out.logits[0, -1].argmax())
    cur = len(ids)
    for _ in range(steps):
        ids.append(nxt)
        pos = cur - 1 if ref_mode else cur
        out = m(decoder_input_ids=torch.tensor([[nxt]]), encoder_outputs=eo, past_key_values=past, use_cache=True,
                decoder_position_ids=torch.tensor([[pos]]), output_attentions=True)
        past = out.past_key_values
        atts.append([a.numpy().copy() for a in out.cross_attentions])
        nxt = int(out.logits[0, -1].argmax())
        cur += 1
    ids.append(nxt)
    return np.asarray(ids, np.int32), atts


def perturbed(atts, rng):
    return [[(a.astype(np.float64) * (1 + PERTURB * rng.standard_normal(a.shape))).astype(np.float32) for a in st] for st in atts]


@torch.no_grad()
def make_streams(name, cfg, ref_mode):
    heads = HEADS[name]
    steps = STEPS[name]
    flat = synth.synth_weights(cfg, 0)
    w = synth.split_weights(cfg, flat)
    m = hf_model(cfg, w, ref_mode)
    prompt = np.asarray(PROMPT if cfg.vocab_size > 50363 else [1, 2, 3, 4], np.int32)
    T = cfg.n_audio_ctx
    clips = []
    seed = 2000 if ref_mode else 3000
    rng = np.random.default_rng(seed)
    while len(clips) < 3:
        seed += 1
        mel = synth.synth_mel(cfg, seed)
        with TanhStemGelu(ref_mode):
            enc_out = m.model.encoder(torch.from_numpy(mel)[None]).last_hidden_state
        ids, atts = greedy_with_attn(m, enc_out, prompt, steps, ref_mode)
        clips.append(dict(seed=seed, ids=ids, atts=atts))
    # the shared stop id: clip 0's 12th generated id (clips stop at its first occurrence, or never)
    eot = int(clips[0]["ids"][N_PROMPT + 11])
    nf = [2 * T, int(1.3 * T) + 1, int(0.7 * T)]  # per-clip mel frames of "real audio"
    out = dict(mode=np.array("ref" if ref_mode else "hf"), prompt=prompt, heads=np.asarray(heads, np.int32), eot=np.int32(eot),
               max_loop=np.int32(steps), n_frames=np.asarray(nf, np.int32), perturb_rel=np.float64(PERTURB))
    for c, clip in enumerate(clips):
        ids, atts = clip["ids"], clip["atts"]
        gen = ids[N_PROMPT:]
        hit = np.nonzero(gen == eot)[0]
        n_cut = N_PROMPT + (int(hit[0]) + 1 if len(hit) else len(gen))
        out[f"c{c}_mel_seed"] = np.int64(clip["seed"])
        out[f"c{c}_ids"] = ids
        out[f"c{c}_n_cut"] = np.int32(n_cut)
        for tag, n in (("full", len(ids)), ("cut", n_cut)):
            for fr_tag, fr in (("", None), ("_nf", nf[c])):
                fn = lambda a, n=n, fr=fr: hf_times(a[:max(1, n - N_PROMPT)], n, heads, cfg.n_layers, fr)  # noqa: E731
                base = fn(atts)
                for _ in range(2):
                    if not np.array_equal(fn(perturbed(atts, rng)), base):
                        raise SystemExit(f"{name} clip {c} ({tag}{fr_tag}): DTW path not stable under {PERTURB} relative noise")
                out[f"c{c}_times_{tag}{fr_tag}"] = base
        if name == "micro":  # selected heads' probabilities of the loop rows [n_sel, steps, T]
            out[f"c{c}_probs"] = np.stack([np.concatenate([st[l][0, h] for st in atts[1:]], 0) for l, h in heads])
    path = os.path.join(ROOT, "tests", "golden", f"token_timestamps_{name}_{'ref' if ref_mode else 'hf'}.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; eot", eot, "cut lengths", [int(out[f"c{c}_n_cut"]) for c in range(3)], flush=True)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    make_tables()
    for ref_mode in (False, True):
        make_streams("micro", WhisperConfig.micro(), ref_mode)
        make_streams("tiny", WhisperConfig.tiny(), ref_mode)
