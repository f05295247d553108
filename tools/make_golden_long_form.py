#!/usr/bin/env python3
"""Generates the sequential long-form fixtures (tests/golden/long_form_*.npz) from HF transformers' own code
(WhisperGenerationMixin.generate on its long-form path, and its _retrieve_segment), for wm_transcribe_long / wm_op_long_segments.

  long_form_segments.npz   _retrieve_segment on crafted id sequences: no timestamps, only <|0.00|>, a lone non-zero timestamp,
                           single- and double-timestamp endings, several pairs, an empty sequence, a short tail window and the
                           zero-advance case.  Per case: ids, seek, seek_num_frames, the segments (first, count, start, end as
                           float64) and the seek advance.
  long_form_{micro,tiny}_hf.npz
                           HF generate long-form (greedy, condition_on_prev_tokens=False, return_timestamps=True,
                           return_segments=True) on the synthetic models (tools/make_golden.py:hf_model, HF mode, fp32) over
                           ragged batches of synth.synth_long_mel recordings (seeds and frame counts stored, not the mels).
                           Cases: a plain ragged batch, one with suppress lists, one with a max_new_tokens that windows hit.
                           Only inputs whose segments survive 1e-5 relative noise on every step's processed scores are kept.
  long_form_logmel.npz     WhisperFeatureExtractor(truncation=False, padding="longest", return_attention_mask=True) on
                           oracle/logmel_oracle.synth_audio recordings: sampled columns, per-utterance max and row sums, and the
                           number of ones in the attention mask.

Usage: python tools/make_golden_long_form.py   (dev container: needs transformers; never at test time)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden import hf_model  # noqa: E402
from whisper_mojo_amd import WhisperConfig, synth  # noqa: E402

PERTURB = 1e-5
N_DRAWS = 3


def retrieve(ids, seek, snf, tb, n_prompt=4):
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin
    seq = torch.as_tensor(np.asarray(ids, np.int64))
    time_offset = torch.tensor([seek], dtype=torch.long).to(torch.float64) * 0.02 / 2
    segs, adv = WhisperGenerationMixin._retrieve_segment(
        seek_sequence=seq, seek_outputs=[None], time_offset=time_offset, timestamp_begin=tb,
        seek_num_frames=torch.tensor([snf], dtype=torch.long), time_precision=0.02, time_precision_features=0.01, input_stride=2,
        prev_idx=0, idx=0, return_token_timestamps=False, decoder_input_ids=torch.zeros((1, n_prompt), dtype=torch.long))
    rows = [(s["idxs"][0] - n_prompt, s["idxs"][1] - s["idxs"][0], float(s["start"]), float(s["end"])) for s in segs]
    for (f, c, _, _), s in zip(rows, segs):
        assert np.array_equal(np.asarray(ids[f:f + c]), s["tokens"].numpy())
    return rows, int(adv)


def make_segments():
    tb = 50365
    T = lambda p: tb + p  # noqa: E731
    cases = {
        "no_timestamps": ([11, 12, 13], 0, 3000),
        "only_zero": ([T(0), 11, 12, 13], 6000, 3000),
        "lone_nonzero": ([T(0), 11, 12, T(37), 13], 3000, 3000),
        "single_ending": ([T(0), 11, 12, T(20), T(20), 13, 14, T(55)], 1234, 3000),
        "double_ending": ([T(0), 11, 12, T(20), T(20), 13, 14, T(55), T(55), 15], 4321, 3000),
        "several_pairs": ([T(0), 11, T(12), T(12), 13, 14, T(40), T(41), 15, T(90), T(90), 16, T(130), T(130)], 90000, 3000),
        "empty": ([], 12000, 3000),
        "short_tail": ([T(0), 11, 12, 13], 177000, 1417),
        "short_tail_lone": ([T(0), 11, T(5)], 200, 333),
        "zero_advance": ([T(0), T(0)], 3000, 3000),
        "zero_advance_text": ([T(0), 11, T(0), T(0), 12], 51, 3000),
        "text_first_pair": ([11, 12, T(30), T(31), 13, T(60)], 7, 2999),
        "big_seek": ([T(3), 11, T(1499), T(1499)], 9_000_001, 3000),
    }
    out = dict(timestamp_begin=np.int32(tb))
    names = []
    for name, (ids, seek, snf) in cases.items():
        rows, adv = retrieve(ids, seek, snf, tb)
        out[name + "_ids"] = np.asarray(ids, np.int32)
        out[name + "_seek"] = np.int64(seek)
        out[name + "_snf"] = np.int32(snf)
        out[name + "_first"] = np.asarray([r[0] for r in rows], np.int32)
        out[name + "_count"] = np.asarray([r[1] for r in rows], np.int32)
        out[name + "_start"] = np.asarray([r[2] for r in rows], np.float64)
        out[name + "_end"] = np.asarray([r[3] for r in rows], np.float64)
        out[name + "_advance"] = np.int32(adv)
        names.append(name)
    out["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "long_form_segments.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(names), "cases; zero advance:", int(out["zero_advance_advance"]))


class Perturb:
    """Multiplies every finite processed score by (1 + 1e-5 · N(0, 1)): the stability filter."""

    def __init__(self, rng):
        self.rng = rng

    def __call__(self, input_ids, scores):
        noise = torch.from_numpy(self.rng.standard_normal(tuple(scores.shape))).to(scores.dtype)
        return torch.where(torch.isfinite(scores), scores * (1 + PERTURB * noise), scores)


def ids_setup(cfg):
    if cfg.vocab_size > 50363:  # the multilingual vocabulary
        return dict(prompt=[50258, 50259, 50359], eos=50257, no_ts=50363)
    return dict(prompt=[1, 2, 3], eos=900, no_ts=940)


@torch.no_grad()
def hf_long(m, cfg, mels, lengths, setup, max_new, sup, bsup, max_init, rng=None):
    from transformers import GenerationConfig, LogitsProcessorList
    B = len(lengths)
    Tm = max(lengths)
    feats = np.zeros((B, cfg.n_mels, Tm), np.float32)
    mask = np.zeros((B, Tm), np.int64)
    for b, (mel, n) in enumerate(zip(mels, lengths)):
        feats[b, :, :n] = mel
        mask[b, :n] = 1
    p = setup["prompt"]
    gc = GenerationConfig(decoder_start_token_id=p[0], forced_decoder_ids=[[i, t] for i, t in enumerate(p[1:], 1)],
                          eos_token_id=setup["eos"], pad_token_id=setup["eos"], no_timestamps_token_id=setup["no_ts"],
                          max_initial_timestamp_index=max_init, suppress_tokens=list(sup) or None,
                          begin_suppress_tokens=list(bsup) or None)
    kw = dict(logits_processor=LogitsProcessorList([Perturb(rng)])) if rng is not None else {}
    out = m.generate(torch.from_numpy(feats), attention_mask=torch.from_numpy(mask), generation_config=gc, return_timestamps=True,
                     return_segments=True, condition_on_prev_tokens=False, temperature=0.0, num_beams=1, max_new_tokens=max_new, **kw)
    res = []
    for b in range(B):
        segs = [(s["tokens"].numpy().astype(np.int32), float(s["start"]), float(s["end"])) for s in out["segments"][b]]
        seq = np.concatenate([s[0] for s in segs]) if segs else np.zeros(0, np.int32)
        res.append((seq, segs))
    return res


def same(a, b):
    return all(np.array_equal(x[0], y[0]) and len(x[1]) == len(y[1]) and
               all(np.array_equal(s[0], t[0]) and s[1] == t[1] and s[2] == t[2] for s, t in zip(x[1], y[1])) for x, y in zip(a, b))


@torch.no_grad()
def make_runs(name, cfg, cases):
    flat = synth.synth_weights(cfg, 0)
    m = hf_model(cfg, synth.split_weights(cfg, flat), False)
    setup = ids_setup(cfg)
    W = cfg.n_frames
    out = dict(prompt=np.asarray(setup["prompt"], np.int32), eos=np.int32(setup["eos"]), no_ts=np.int32(setup["no_ts"]),
               timestamp_begin=np.int32(setup["no_ts"] + 1), perturb_rel=np.float64(PERTURB))
    names = []
    for case, (lengths, max_new, sup, bsup, max_init) in cases.items():
        seed = {"micro": 10, "tiny": 50}[name] + 100 * len(names)
        rng = np.random.default_rng(seed)
        while True:
            seed += 1
            seeds = [seed * 10 + b for b in range(len(lengths))]
            mels = [synth.synth_long_mel(cfg, s, n) for s, n in zip(seeds, lengths)]
            base = hf_long(m, cfg, mels, lengths, setup, max_new, sup, bsup, max_init)
            if all(same(base, hf_long(m, cfg, mels, lengths, setup, max_new, sup, bsup, max_init, rng)) for _ in range(N_DRAWS)):
                break
            print(f"  {name}/{case}: seed {seed} unstable under noise, next", flush=True)
        out[case + "_lengths"] = np.asarray(lengths, np.int32)
        out[case + "_seeds"] = np.asarray(seeds, np.int64)
        out[case + "_max_new_tokens"] = np.int32(max_new)
        out[case + "_suppress"] = np.asarray(sup, np.int32)
        out[case + "_begin_suppress"] = np.asarray(bsup, np.int32)
        out[case + "_max_init"] = np.int32(max_init)
        for b, (seq, segs) in enumerate(base):
            out[f"{case}_u{b}_sequence"] = seq
            out[f"{case}_u{b}_count"] = np.asarray([len(s[0]) for s in segs], np.int32)
            out[f"{case}_u{b}_start"] = np.asarray([s[1] for s in segs], np.float64)
            out[f"{case}_u{b}_end"] = np.asarray([s[2] for s in segs], np.float64)
        names.append(case)
        print(f"{name}/{case}: lengths {lengths} ({[-(-n // W) for n in lengths]} windows min), segments",
              [len(s) for _, s in base], flush=True)
    out["cases"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", f"long_form_{name}_hf.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", flush=True)


def make_logmel():
    from transformers import WhisperFeatureExtractor
    from oracle import logmel_oracle as lo
    seconds = [70.3, 41.0, 3.01]
    seeds = [31, 32, 33]
    audios = [lo.synth_audio(s, int(round(t * 16000))) for s, t in zip(seeds, seconds)]
    fe = WhisperFeatureExtractor(feature_size=80)
    r = fe(audios, sampling_rate=16000, truncation=False, padding="longest", return_attention_mask=True, return_tensors="np")
    f, mask = r["input_features"].astype(np.float32), r["attention_mask"]
    N = max(len(a) for a in audios)
    assert f.shape[2] == N // 160, (f.shape, N)
    n_frames = mask.sum(-1).astype(np.int32)
    assert [int(v) for v in n_frames] == [min(-(-len(a) // 160), N // 160) for a in audios], (n_frames, [len(a) for a in audios])
    rng = np.random.default_rng(5)
    cols = np.unique(np.concatenate([[0, 1, 2999, 3000, 3001, N // 160 - 1], rng.integers(0, N // 160, 120)])).astype(np.int32)
    out = dict(seeds=np.asarray(seeds, np.int64), n_samples=np.asarray([len(a) for a in audios], np.int32), n_frames=n_frames,
               cols=cols, mel_cols=f[:, :, cols], mel_max=f.max(axis=(1, 2)), mel_rowsum=f.astype(np.float64).sum(2))
    path = os.path.join(ROOT, "tests", "golden", "long_form_logmel.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; n_frames", n_frames.tolist(), "of", N // 160)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    what = sys.argv[1:] or ["segments", "logmel", "micro", "tiny"]
    if "segments" in what:
        make_segments()
    if "logmel" in what:
        make_logmel()
    if "micro" in what:
        make_runs("micro", WhisperConfig.micro(), {
            "ragged": ([700, 455, 150, 1130], 40, (), (), 50),
            "suppress": ([610, 1000, 90], 40, (5, 17, 300, 899), (7, 941), 50),
            "max_new": ([900, 380], 12, (), (), 50),
        })
    if "tiny" in what:
        make_runs("tiny", WhisperConfig.tiny(), {
            "ragged": ([9000, 4400, 2100], 40, (), (), 50),
            "max_new": ([7000, 2500], 10, (), (), 50),
            "suppress": ([8000, 5200, 1500], 40, (8084, 28445, 39474, 36974, 220), (220, 50257), 50),
        })
