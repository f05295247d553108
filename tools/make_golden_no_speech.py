#!/usr/bin/env python3
"""Generates the no-speech fixtures on the CPU from HF transformers' own code, for wm_transcribe_lp_ns and the
logprob_threshold / no_speech_threshold options of wm_transcribe_long_ex.

  no_speech_{micro,tiny}_hf.npz

  Short form ("s{i}_" keys; the weights and clips of tools/make_golden.py, the decoding of tools/make_golden_logprobs.py with the
  timestamp rules and suppress lists on): a shared-prompt batch (case "shared": the initial ids) and a per-row batch (case "rows":
  random previous-text ids + the initial ids, lengths 3 .. 33, so that with 16-position prefill chunks the <|startoftranscript|>
  slot of the longest row is not in the last chunk).  Per row: prompt, ids, token log-probs, avg_logprob and no_speech_prob — the
  value HF's WhisperNoSpeechDetection computes, called as HF's own class on the model's logits (begin_index = the prompt length,
  start_of_trans_offset = n_init); micro also stores the raw logits row of that position.

  Long form (tiny; one block of keys per case; micro has none: its avg_logprob moves by at most 0.08 over a run whatever the input,
  correlated with log no_speech_prob, so the conditions below cannot hold for it): real generate(..., logprob_threshold=, no_speech_threshold=, temperature=0.0,
  return_segments=True) runs, every recording ALONE (as the conditioned fixtures of tools/make_golden_prompts.py are), with
  WhisperGenerationMixin._need_fallback wrapped to record per window (utterance, seek, avg_logprob, no_speech_prob, should_skip) and
  the ids it saw.  Two things spread
  the values, which on the plain synthetic inputs move by less than 1 % from window to window:
    * the fixture model's token embedding is multiplied by emb_scale (sharper logits) and its <|nospeech|> row replaced by
      default_rng(ns_row_seed).standard_normal(d_model) * ns_row_scale (the three numbers are stored, not the weights; the id is in
      suppress_tokens, as in HF's released configs, so it is never fed back);
    * every block of n_frames frames of a recording is faded towards silence and tilted over the mel bins: x -> g·x - (1 - g) +
      t·linspace(-1, 1, n_mels), with a stored gain g in [0, 1] and tilt t in [-1, 1] per block (-1 is the synthetic mels' floor).
  The thresholds are plain float32 values taken from a first run that records the values without skipping: the middles of gaps
  of the sorted values for which the conditions below hold on that run; the real run is then made with them and checked again.

  Conditions checked here per model, over its cases (an input set that misses one is dropped, the seed moves on):
    * at least two skipped and two kept windows; a skipped window followed by a kept one in the same recording;
    * a window with no_speech_prob > threshold but avg_logprob >= logprob_threshold, and one the reverse (both kept);
    * the conditioned case skips a window after history exists;
    * every window's margin is >= 1e-2 in avg_logprob and in log(no_speech_prob);
    * no window fails to advance seek; segments unchanged under three draws of 1e-5 relative noise on every step's processed scores.

Usage: python tools/make_golden_no_speech.py [micro] [tiny]   (dev container: needs transformers; never at test time)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden import hf_model  # noqa: E402
from make_golden_logprobs import MAX_INIT, hf_greedy_lp  # noqa: E402
from make_golden_long_form import N_DRAWS, PERTURB, Perturb, ids_setup, same  # noqa: E402
from make_golden_prompts import prev_sot_of  # noqa: E402
from whisper_mojo_amd import WhisperConfig, synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MARGIN = 1e-2


# ---- short form ------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def hf_no_speech(m, enc_out, prompt, n_init, token):
    """HF's WhisperNoSpeechDetection on one row -> (no_speech_prob, raw logits row of the <|startoftranscript|> position)"""
    from types import SimpleNamespace

    from transformers.generation.logits_process import WhisperNoSpeechDetection
    from transformers.modeling_outputs import BaseModelOutput
    ids = torch.tensor([[int(t) for t in prompt]])
    logits = m(decoder_input_ids=ids, encoder_outputs=BaseModelOutput(last_hidden_state=enc_out)).logits
    det = WhisperNoSpeechDetection(no_speech_token=token, begin_index=n_init)
    det.set_begin_index(ids.shape[1])
    det.model = lambda **kw: SimpleNamespace(logits=logits)
    det.inputs = {}
    det(ids, logits[:, -1])
    assert n_init > 1  # (with one initial id HF reads the processed scores of the first step instead)
    return np.float32(det.no_speech_prob[0]), logits[0, ids.shape[1] - n_init].float().numpy().copy()


def make_short(name, cfg, m, out, keep_raw, max_loop):
    setup = ids_setup(cfg)
    init = setup["prompt"]
    token = setup["no_ts"] - 1
    rng = np.random.default_rng(29)
    text_hi = min(setup["eos"], 800 if cfg.vocab_size < 2000 else 50000)
    sup = sorted(set(rng.integers(4, text_hi, 12).tolist()))
    bsup = sorted({setup["eos"], int(rng.integers(4, text_hi))})
    out.update(s_suppress=np.asarray(sup, np.int32), s_begin_suppress=np.asarray(bsup, np.int32), s_max_loop=np.int32(max_loop),
               s_max_init=np.int32(MAX_INIT))
    rows = 0
    for case, L in [("shared", len(init))] * 3 + [("rows", L) for L in (3, 7, 18, 33)]:
        seed = 7000 + 61 * rows
        while True:
            seed += 1
            prompt = rng.integers(4, text_hi, L - len(init)).tolist() + init
            enc = m.model.encoder(torch.from_numpy(synth.synth_mel(cfg, seed))[None]).last_hidden_state
            ids, lps, avg, _ = hf_greedy_lp(m, enc, prompt, max_loop, setup, 1, sup, bsup)
            if all(np.array_equal(ids, hf_greedy_lp(m, enc, prompt, max_loop, setup, 1, sup, bsup, rng)[0]) for _ in range(N_DRAWS)):
                break
            print(f"  {name}: short row {rows} seed {seed} unstable under noise, next", flush=True)
        nsp, raw = hf_no_speech(m, enc, prompt, len(init), token)
        k = f"s{rows}_"
        out[k + "case"] = np.array(case)
        out[k + "seed"] = np.int64(seed)
        out[k + "prompt"] = np.asarray(prompt, np.int32)
        out[k + "ids"] = ids
        out[k + "logprobs"] = lps
        out[k + "avg_logprob"] = avg
        out[k + "no_speech_prob"] = nsp
        if keep_raw:
            out[k + "sot_logits"] = raw.astype(np.float32)
        print(f"{name}: short row {rows} {case} L={L}: {len(lps)} generated, avg_logprob {avg:.4f}, no_speech_prob {nsp:.3e}", flush=True)
        rows += 1
    out["s_rows"] = np.int32(rows)


# ---- long form -------------------------------------------------------------------------------------------------------------
def biased_weights(cfg, token, seed, scale, emb_scale):
    """the synthetic weights with the token embedding scaled and the <|nospeech|> row replaced (the tests rebuild them from the numbers)"""
    flat = synth.synth_weights(cfg, 0)
    synth.split_weights(cfg, flat)["dec.tok_emb"][:] *= np.float32(emb_scale)
    synth.split_weights(cfg, flat)["dec.tok_emb"][token] = (np.random.default_rng(seed).standard_normal(cfg.d_model) * scale).astype(np.float32)
    return flat


def faded_mel(cfg, seed, n, gains, tilts):
    """synth_long_mel with block k of n_frames frames faded towards the floor and tilted over the mel bins:
    x -> g·x - (1 - g) + t·linspace(-1, 1, n_mels)"""
    mel = synth.synth_long_mel(cfg, seed, n)
    W = cfg.n_frames
    ramp = np.linspace(-1, 1, cfg.n_mels, dtype=np.float32)[:, None]
    for k, (g, t) in enumerate(zip(gains, tilts)):
        g, t = np.float32(g), np.float32(t)
        mel[:, k * W:(k + 1) * W] = g * mel[:, k * W:(k + 1) * W] - (np.float32(1) - g) + t * ramp
    return mel


class Recorder:
    """Wraps WhisperGenerationMixin._need_fallback / generate_with_fallback while a generate call runs: per window
    [utterance, seek, avg_logprob, no_speech_prob, should_skip, ids as _need_fallback saw them, raw SOT logits or None]."""

    def __init__(self, keep_raw):
        self.log = []
        self.keep_raw = keep_raw

    def __enter__(self):
        from transformers.generation.logits_process import WhisperNoSpeechDetection
        from transformers.models.whisper import generation_whisper as gw
        G = gw.WhisperGenerationMixin
        self.G, self.orig_nf, self.orig_gf = G, G._need_fallback, G.generate_with_fallback
        rec = self

        def need_fallback(self_, seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size, temperature):
            res = rec.orig_nf(self_, seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size, temperature)
            avg = float(self_._retrieve_avg_logprobs(seek_outputs[index]["scores"], seek_sequence, temperature))
            det = next(p for p in logits_processor if isinstance(p, WhisperNoSpeechDetection))
            raw = None
            if rec.keep_raw:
                with torch.no_grad():
                    lg = det.model(**det.inputs).logits
                raw = lg[index, det.begin_index - det.start_of_trans_offset].float().numpy().copy()
            rec.log.append([index, None, avg, float(det.no_speech_prob[index]), bool(res[1]), seek_sequence.numpy().astype(np.int32), raw])
            return res

        def with_fallback(self_, *a, **kw):
            seek = (kw["seek"] if "seek" in kw else a[3]).clone()
            bim = list(kw["batch_idx_map"] if "batch_idx_map" in kw else a[4])
            n0 = len(rec.log)
            res = rec.orig_gf(self_, *a, **kw)
            for e in rec.log[n0:]:
                e[0], e[1] = bim[e[0]], int(seek[bim[e[0]]])
            return res

        G._need_fallback, G.generate_with_fallback = need_fallback, with_fallback
        return self

    def __exit__(self, *exc):
        self.G._need_fallback, self.G.generate_with_fallback = self.orig_nf, self.orig_gf


@torch.no_grad()
def hf_long_ns(m, cfg, mel, n, setup, max_new, lt, nt, cond, rng=None, keep_raw=False):
    """One recording alone -> ((sequence, segments), window log)"""
    from transformers import GenerationConfig, LogitsProcessorList
    p = setup["prompt"]
    gc = GenerationConfig(decoder_start_token_id=p[0], forced_decoder_ids=[[i, t] for i, t in enumerate(p[1:], 1)],
                          eos_token_id=setup["eos"], pad_token_id=setup["eos"], no_timestamps_token_id=setup["no_ts"],
                          max_initial_timestamp_index=MAX_INIT, prev_sot_token_id=prev_sot_of(cfg), suppress_tokens=[setup["no_ts"] - 1])
    kw = dict(logits_processor=LogitsProcessorList([Perturb(rng)])) if rng is not None else {}
    with Recorder(keep_raw) as rec:
        out = m.generate(torch.from_numpy(mel[None, :, :n].copy()), attention_mask=torch.ones((1, n), dtype=torch.long), generation_config=gc,
                         return_timestamps=True, return_segments=True, condition_on_prev_tokens=bool(cond), temperature=0.0, num_beams=1,
                         max_new_tokens=max_new, logprob_threshold=lt, no_speech_threshold=nt, **kw)
    segs = [(s["tokens"].numpy().astype(np.int32), float(s["start"]), float(s["end"])) for s in out["segments"][0]]
    return (np.concatenate([s[0] for s in segs]) if segs else np.zeros(0, np.int32), segs), rec.log


def quadrants(w, lt, nt):
    """windows of a log by decision: (skipped, no-speech alone, log-prob alone, neither)"""
    return (sum(e[2] < lt and e[3] > nt for e in w), sum(e[2] >= lt and e[3] > nt for e in w), sum(e[2] < lt and e[3] <= nt for e in w),
            sum(e[2] >= lt and e[3] <= nt for e in w))


def pick_thresholds(w, full):
    """float32 gap middles (gaps >= 2.5 margins) of avg_logprob and log no_speech_prob with every quadrant of the log populated (full;
    else: a skipped and a kept window), the pair whose rarest quadrant is largest; None when there is none"""
    def mids(v):
        v = np.sort(np.asarray(v, np.float64))
        return [0.5 * (a + b) for a, b in zip(v[:-1], v[1:]) if b - a >= 2.5 * MARGIN]
    best = None
    for lt in mids([e[2] for e in w]):
        for lnt in mids([np.log(e[3]) for e in w]):
            lt32, nt32 = float(np.float32(lt)), float(np.float32(np.exp(lnt)))
            q = quadrants(w, lt32, nt32)
            ok = (min(q) >= 1 and q[0] >= 2) if full else (q[0] >= 1 and sum(q[1:]) >= 1)
            score = min(q) if full else min(q[0], sum(q[1:]))
            if ok and (best is None or score > best[0]):
                best = (score, lt32, nt32)
    return None if best is None else best[1:]


def conditions(logs, lt, nt, cond):
    """logs: per recording its window log of the real run -> None or the reason the case fails"""
    w = [e for lg in logs for e in lg]
    if any(abs(e[2] - lt) < MARGIN or abs(np.log(e[3]) - np.log(nt)) < MARGIN for e in w):
        return "a margin below 1e-2"
    q = quadrants(w, lt, nt)
    if q[0] != sum(e[4] for e in w):
        return "HF's flags are not the rule's"
    if not cond and (q[0] < 2 or q[1] < 1 or q[2] < 1 or q[1] + q[2] + q[3] < 2):  # (the per-model counts are met by the unconditioned case)
        return f"quadrants {q}"
    if not cond and not any(lg[i][4] and any(not e[4] for e in lg[i + 1:]) for lg in logs for i in range(len(lg))):
        return "no skipped window followed by a kept one"
    if cond and not any(lg[i][4] and any(not e[4] for e in lg[:i]) for lg in logs for i in range(len(lg))):
        return "no window skipped after history"
    return None


def make_long(name, cfg, out, keep_raw, cases, max_new, row_seed, row_scale, emb_scale):
    setup = ids_setup(cfg)
    token = setup["no_ts"] - 1
    m = hf_model(cfg, synth.split_weights(cfg, biased_weights(cfg, token, row_seed, row_scale, emb_scale)), False)
    out.update(prompt=np.asarray(setup["prompt"], np.int32), prev_sot=np.int32(prev_sot_of(cfg)), max_new_tokens=np.int32(max_new),
               max_init=np.int32(MAX_INIT), ns_row_seed=np.int64(row_seed), ns_row_scale=np.float32(row_scale), emb_scale=np.float32(emb_scale), cases=np.array(list(cases)))
    rng = np.random.default_rng(41)
    W = cfg.n_frames
    for ci, (case, (cond, lengths)) in enumerate(cases.items()):
        seed = {"micro": 300, "tiny": 700}[name] + 40 * ci
        while True:
            seed += 1
            seeds = [seed * 100 + b for b in range(len(lengths))]
            gains = [rng.uniform(0, 1, -(-n // W)).astype(np.float32) for n in lengths]
            tilts = [rng.uniform(-1, 1, -(-n // W)).astype(np.float32) for n in lengths]
            mels = [faded_mel(cfg, s, n, g, t) for s, n, g, t in zip(seeds, lengths, gains, tilts)]
            probe = [hf_long_ns(m, cfg, mel, n, setup, max_new, -1e9, 2.0, cond)[1] for mel, n in zip(mels, lengths)]
            th = pick_thresholds([e for lg in probe for e in lg], not cond)
            why = "no thresholds split the first run" if th is None else None
            if why is None:
                lt, nt = th
                runs = [hf_long_ns(m, cfg, mel, n, setup, max_new, lt, nt, cond, keep_raw=keep_raw) for mel, n in zip(mels, lengths)]
                why = conditions([r[1] for r in runs], lt, nt, cond)
            if why is None and any(lg[i + 1][1] <= lg[i][1] for _, lg in runs for i in range(len(lg) - 1)):
                why = "a window does not advance seek"
            if why is None and not all(same([r[0]], [hf_long_ns(m, cfg, mel, n, setup, max_new, lt, nt, cond, rng)[0]])
                                       for r, mel, n in zip(runs, mels, lengths) for _ in range(N_DRAWS)):
                why = "unstable under noise"
            if why is None:
                break
            print(f"  {name}/{case}: seed {seed}: {why}; first run avg {[round(e[2], 3) for lg in probe for e in lg]}, log nsp "
                  f"{[round(float(np.log(e[3])), 3) for lg in probe for e in lg]}", flush=True)
        out[case + "_cond"] = np.int32(cond)
        out[case + "_lengths"] = np.asarray(lengths, np.int32)
        out[case + "_seeds"] = np.asarray(seeds, np.int64)
        out[case + "_logprob_threshold"] = np.float32(lt)
        out[case + "_no_speech_threshold"] = np.float32(nt)
        for b, ((seq, segs), log) in enumerate(runs):
            k = f"{case}_u{b}_"
            out[k + "gains"] = gains[b]
            out[k + "tilts"] = tilts[b]
            out[k + "sequence"] = seq
            out[k + "count"] = np.asarray([len(s[0]) for s in segs], np.int32)
            out[k + "start"] = np.asarray([s[1] for s in segs], np.float64)
            out[k + "end"] = np.asarray([s[2] for s in segs], np.float64)
            out[k + "w_seek"] = np.asarray([e[1] for e in log], np.int64)
            out[k + "w_avg_logprob"] = np.asarray([e[2] for e in log], np.float32)
            out[k + "w_no_speech_prob"] = np.asarray([e[3] for e in log], np.float32)
            out[k + "w_skipped"] = np.asarray([e[4] for e in log], np.int32)
            out[k + "w_count"] = np.asarray([len(e[5]) for e in log], np.int32)
            out[k + "w_ids"] = np.concatenate([e[5] for e in log]) if log else np.zeros(0, np.int32)
            if keep_raw:
                out[k + "w_sot_logits"] = np.stack([e[6] for e in log]).astype(np.float32)
            print(f"{name}/{case} u{b}: {lengths[b]} frames, thresholds {lt:.4f} / {nt:.4e}, windows (seek, avg, nsp, skip):",
                  [(e[1], round(e[2], 3), float(f"{e[3]:.3g}"), int(e[4])) for e in log], flush=True)


def make(name, cfg, keep_raw, max_loop, cases, max_new, row_seed, row_scale, emb_scale):
    m = hf_model(cfg, synth.split_weights(cfg, synth.synth_weights(cfg, 0)), False)
    setup = ids_setup(cfg)
    out = dict(init=np.asarray(setup["prompt"], np.int32), eos=np.int32(setup["eos"]), no_ts=np.int32(setup["no_ts"]),
               timestamp_begin=np.int32(setup["no_ts"] + 1), no_speech_token=np.int32(setup["no_ts"] - 1), perturb_rel=np.float64(PERTURB))
    make_short(name, cfg, m, out, keep_raw, max_loop)
    make_long(name, cfg, out, keep_raw, cases, max_new, row_seed, row_scale, emb_scale)
    path = os.path.join(GOLDEN, f"no_speech_{name}_hf.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["micro", "tiny"]
    torch.manual_seed(0)
    torch.set_num_threads(16)
    if "micro" in which:
        make("micro", WhisperConfig.micro(), True, 14, {}, 24, 5, 0.3, 1.0)
    if "tiny" in which:
        make("tiny", WhisperConfig.tiny(), False, 24, {"ragged": (0, [11000, 9000, 7000, 4400]), "cond": (1, [12000])}, 24, 5, 0.3, 1.0)
