#!/usr/bin/env python3
"""Generates the language-detection fixtures on the CPU from HF transformers' own code, for wm_detect_language and
wm_transcribe_lang.

  lang_detect_{micro,tiny}_hf.npz

  The weights, clips and decoding of tools/make_golden.py / make_golden_logprobs.py / make_golden_no_speech.py (timestamp rules and
  suppress lists on).  With synthetic weights and inputs the language logits barely move from clip to clip, so
    * the language rows of the token embedding are replaced by default_rng(lang_row_seed).standard_normal((n_lang, d_model)) *
      lang_row_scale, in list order (the numbers are stored, not the weights);
    * every clip is faded towards silence and tilted over the mel bins, x -> g·x - (1 - g) + t·linspace(-1, 1, n_mels), with a
      stored gain g and tilt t per row.
  Language lists: micro a stored, unsorted, non-contiguous list of 12 ids outside the initial ids, eos, no_ts and the suppress
  lists; tiny the ids 50259 … 50357.

  Per row ("s{i}_" keys): HF model.detect_language(encoder_outputs=…, generation_config=gc) with gc.lang_to_id set and
  gc.decoder_start_token_id = the first initial id; the float64 softmax over the candidates of HF's raw logits row of a
  [<|startoftranscript|>] pass (that row's candidate logits are stored too); then the prompt with the detected language at the
  language slot and the ids, token log-probs, avg_logprob and no_speech_prob of hf_greedy_lp / hf_no_speech on it.  Cases: a
  shared-prompt batch and a per-row batch with previous text of the no-speech fixture's lengths (3 … 33: with 16-position prefill
  chunks the 33-id row's <|startoftranscript|> slot is not in the last chunk).

  Conditions checked here (a row that misses one is dropped, the seed moves on; the set as a whole is checked at the end):
    * at least three different detected languages among the rows;
    * every row's top-2 gap in the language logits is >= 1e-2; the smallest gap is stored;
    * ids unchanged under three draws of 1e-5 relative noise on every step's processed scores.

  micro: as its weights stand, the hidden row of the [<|startoftranscript|>] pass barely depends on the audio (every clip detects the
  same language at row scales 0.02 … 0.3), so the micro fixture model also has its decoder cross-attention output projections
  multiplied by a stored cross_o_scale = 7 and its tilts drawn from ±16 (tiny: 1 and ±1).

  Cross-check, once per model: a real generate(input_features, language=None, task="transcribe", return_timestamps=True) on the model
  with its generation config marked multilingual, detect_language wrapped to record what generate detected; it must reproduce the
  first shared row's stored language and generated ids (generate_checked = 1; 0 and the printed reason if HF refuses the config).

  Long form (tiny; "{case}_u{b}_" keys): real generate(..., language=None, return_segments=True) runs, every recording alone, a plain
  case and one with condition_on_prev_tokens=True; a recording is faded / tilted as a whole.  Stored: the language generate itself
  detected (on the first 3000 frames), sequence and segments.  Checked: at least two languages among the recordings, the first
  window's top-2 language gap >= 1e-2, sequences unchanged under the three noise draws.

Usage: python tools/make_golden_lang.py [micro] [tiny]   (dev container: needs transformers; never at test time)"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden import hf_model  # noqa: E402
from make_golden_logprobs import MAX_INIT, hf_greedy_lp  # noqa: E402
from make_golden_long_form import N_DRAWS, PERTURB, Perturb, ids_setup  # noqa: E402
from make_golden_prompts import prev_sot_of  # noqa: E402
from make_golden_no_speech import MARGIN, hf_no_speech  # noqa: E402
from whisper_mojo_amd import WhisperConfig, synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def lang_weights(cfg, lang_ids, seed, scale, cross_o_scale=1.0):
    """the synthetic weights with the language rows of the token embedding replaced and the decoder's cross-attention output
    projections multiplied by cross_o_scale (the tests rebuild them from the numbers)"""
    flat = synth.synth_weights(cfg, 0)
    if cross_o_scale != 1.0:
        for l in range(cfg.n_layers):
            synth.split_weights(cfg, flat)[f"dec.{l}.cross.o.w"][:] *= np.float32(cross_o_scale)
    rows = (np.random.default_rng(seed).standard_normal((len(lang_ids), cfg.d_model)) * scale).astype(np.float32)
    emb = synth.split_weights(cfg, flat)["dec.tok_emb"]
    for i, t in enumerate(lang_ids):
        emb[int(t)] = rows[i]
    return flat


def lang_mel(cfg, seed, gain, tilt):
    g, t = np.float32(gain), np.float32(tilt)
    ramp = np.linspace(-1, 1, cfg.n_mels, dtype=np.float32)[:, None]
    return (g * synth.synth_mel(cfg, seed) - (np.float32(1) - g) + t * ramp).astype(np.float32)


@torch.no_grad()
def hf_detect(m, enc, sot, lang_ids):
    """-> (HF detect_language's id, raw candidate logits of the [sot] pass in list order)"""
    from transformers.modeling_outputs import BaseModelOutput
    gc = SimpleNamespace(decoder_start_token_id=int(sot), lang_to_id={f"<|l{i}|>": int(t) for i, t in enumerate(lang_ids)})
    eo = BaseModelOutput(last_hidden_state=enc)
    got = int(m.detect_language(encoder_outputs=eo, generation_config=gc)[0])
    raw = m(decoder_input_ids=torch.tensor([[int(sot)]]), encoder_outputs=eo, use_cache=False).logits[0, -1].double().numpy()
    return got, raw[np.asarray(lang_ids)]


@torch.no_grad()
def hf_generate_default(m, mel, setup, lang_ids, sup, bsup, max_loop):
    """a real generate(..., language=None) on the model with its generation config marked multilingual -> (the language ids its
    own detect_language call returned, the ids generate returns for the clip: the generated ones, without the initial ids)"""
    gc = m.generation_config
    init = setup["prompt"]
    gc.is_multilingual = True
    gc.lang_to_id = {f"<|l{i}|>": int(t) for i, t in enumerate(lang_ids)}
    gc.task_to_id = {"transcribe": int(init[2])}
    gc.decoder_start_token_id = int(init[0])
    gc.eos_token_id = gc.pad_token_id = int(setup["eos"])
    gc.no_timestamps_token_id = int(setup["no_ts"])
    gc.max_initial_timestamp_index = MAX_INIT
    gc.suppress_tokens = [int(t) for t in sup]
    gc.begin_suppress_tokens = [int(t) for t in bsup]
    gc.forced_decoder_ids = None
    seen, orig = [], m.detect_language

    def spy(*a, **k):
        seen.append(orig(*a, **k))
        return seen[-1]

    m.detect_language = spy
    try:
        out = m.generate(input_features=torch.from_numpy(mel)[None], language=None, task="transcribe", return_timestamps=True, do_sample=False,
                         num_beams=1, max_new_tokens=max_loop + 1)
    finally:
        del m.detect_language
    seq = out["sequences"] if isinstance(out, dict) else out
    assert len(seen) == 1, "generate(language=None) did not call detect_language once"
    return int(seen[0][0]), seq[0].numpy().astype(np.int32)


def mark_multilingual(m, cfg, setup, lang_ids, sup, bsup):
    gc = m.generation_config
    init = setup["prompt"]
    gc.is_multilingual = True
    gc.lang_to_id = {f"<|l{i}|>": int(t) for i, t in enumerate(lang_ids)}
    gc.task_to_id = {"transcribe": int(init[2])}
    gc.decoder_start_token_id = int(init[0])
    gc.eos_token_id = gc.pad_token_id = int(setup["eos"])
    gc.no_timestamps_token_id = int(setup["no_ts"])
    gc.prev_sot_token_id = int(prev_sot_of(cfg))
    gc.max_initial_timestamp_index = MAX_INIT
    gc.suppress_tokens = [int(t) for t in sup]
    gc.begin_suppress_tokens = [int(t) for t in bsup]
    gc.forced_decoder_ids = None


@torch.no_grad()
def hf_long_default(m, mel, cond, max_new, rng=None):
    """a real long-form generate(..., language=None, return_segments=True) on ONE recording -> (the language generate detected,
    sequence, [(ids, start, end)])"""
    from transformers import LogitsProcessorList
    seen, orig = [], m.detect_language

    def spy(*a, **k):
        seen.append(orig(*a, **k))
        return seen[-1]

    kw = dict(logits_processor=LogitsProcessorList([Perturb(rng)])) if rng is not None else {}
    m.detect_language = spy
    try:
        out = m.generate(torch.from_numpy(mel)[None], attention_mask=torch.ones((1, mel.shape[1]), dtype=torch.long), language=None,
                         task="transcribe", return_timestamps=True, return_segments=True, condition_on_prev_tokens=bool(cond), temperature=0.0,
                         num_beams=1, max_new_tokens=max_new, **kw)
    finally:
        del m.detect_language
    assert len(seen) == 1 and len(seen[0]) == 1, "generate(language=None) did not detect once per recording"
    segs = [(sg["tokens"].numpy().astype(np.int32), float(sg["start"]), float(sg["end"])) for sg in out["segments"][0]]
    return int(seen[0][0]), (np.concatenate([t[0] for t in segs]) if segs else np.zeros(0, np.int32)), segs


def make_long(name, cfg, m, out, lang_ids, cases, max_new, tilt_max):
    """long form ("{case}_" keys): every recording alone, a plain case and one with condition_on_prev_tokens"""
    setup = ids_setup(cfg)
    rng = np.random.default_rng(37)
    ramp = np.linspace(-1, 1, cfg.n_mels, dtype=np.float32)[:, None]
    langs_all = []
    out["l_cases"] = np.array(list(cases))
    out["l_max_new"] = np.int32(max_new)
    for case, (cond, lengths) in cases.items():
        out[f"{case}_cond"] = np.int32(cond)
        out[f"{case}_lengths"] = np.asarray(lengths, np.int32)
        for b, n in enumerate(lengths):
            seed, tries = 9500 + 53 * len(langs_all), 0
            while True:
                seed += 1
                tries += 1
                assert tries < 40, "no usable recording found"
                gain, tilt = np.float32(rng.uniform(0.2, 1.0)), np.float32(rng.uniform(-tilt_max, tilt_max))
                mel = (gain * synth.synth_long_mel(cfg, seed, n) - (np.float32(1) - gain) + tilt * ramp).astype(np.float32)
                enc = m.model.encoder(torch.from_numpy(np.ascontiguousarray(mel[:, :cfg.n_frames]))[None]).last_hidden_state
                lang0, cand = hf_detect(m, enc, setup["prompt"][0], lang_ids)
                srt = np.sort(cand)
                if srt[-1] - srt[-2] < MARGIN or (len(set(langs_all)) < 2 and lang0 in langs_all and tries < 20):
                    continue
                lang, seq, segs = hf_long_default(m, mel, cond, max_new)
                assert lang == lang0, (lang, lang0)
                if all(np.array_equal(seq, hf_long_default(m, mel, cond, max_new, rng)[1]) for _ in range(N_DRAWS)):
                    break
                print(f"  {name}/{case} u{b} seed {seed} unstable under noise, next", flush=True)
            k = f"{case}_u{b}_"
            out[k + "seed"] = np.int64(seed)
            out[k + "gain"] = gain
            out[k + "tilt"] = tilt
            out[k + "lang"] = np.int32(lang)
            out[k + "gap"] = np.float64(srt[-1] - srt[-2])
            out[k + "sequence"] = seq
            out[k + "count"] = np.asarray([len(t[0]) for t in segs], np.int32)
            out[k + "start"] = np.asarray([t[1] for t in segs], np.float64)
            out[k + "end"] = np.asarray([t[2] for t in segs], np.float64)
            langs_all.append(lang)
            print(f"{name}/{case} u{b}: {n} frames seed {seed}: language {lang} (gap {srt[-1] - srt[-2]:.3f}), {len(segs)} segments, {len(seq)} ids",
                  flush=True)
    assert len(set(langs_all)) >= 2, langs_all


def make(name, cfg, max_loop, lang_row_seed, lang_row_scale, cross_o_scale=1.0, tilt_max=1.0, long_cases=None):
    setup = ids_setup(cfg)
    init = setup["prompt"]
    token = setup["no_ts"] - 1
    rng = np.random.default_rng(31)
    text_hi = min(setup["eos"], 800 if cfg.vocab_size < 2000 else 50000)
    sup = sorted(set(rng.integers(4, text_hi, 12).tolist()))
    bsup = sorted({setup["eos"], int(rng.integers(4, text_hi))})
    if cfg.vocab_size > 50363:
        lang_ids = list(range(50259, 50358))
    else:
        pool = [t for t in range(4, text_hi) if t not in sup and t not in bsup]
        lang_ids = [int(t) for t in rng.choice(pool, 12, replace=False)]
        if lang_ids == sorted(lang_ids):
            lang_ids = lang_ids[::-1]
    m = hf_model(cfg, synth.split_weights(cfg, lang_weights(cfg, lang_ids, lang_row_seed, lang_row_scale, cross_o_scale)), False)
    out = dict(init=np.asarray(init, np.int32), eos=np.int32(setup["eos"]), no_ts=np.int32(setup["no_ts"]),
               timestamp_begin=np.int32(setup["no_ts"] + 1), no_speech_token=np.int32(token), perturb_rel=np.float64(PERTURB),
               lang_ids=np.asarray(lang_ids, np.int32), lang_row_seed=np.int64(lang_row_seed), lang_row_scale=np.float64(lang_row_scale), cross_o_scale=np.float64(cross_o_scale),
               s_suppress=np.asarray(sup, np.int32), s_begin_suppress=np.asarray(bsup, np.int32), s_max_loop=np.int32(max_loop),
               s_max_init=np.int32(MAX_INIT))
    rows, gaps, langs = 0, [], []
    for case, L in [("shared", len(init))] * 3 + [("rows", L) for L in (3, 7, 18, 33)]:
        seed, tries = 9000 + 67 * rows, 0
        while True:
            seed += 1
            gain, tilt = float(np.float32(rng.uniform(0.2, 1.0))), float(np.float32(rng.uniform(-tilt_max, tilt_max)))
            enc = m.model.encoder(torch.from_numpy(lang_mel(cfg, seed, gain, tilt))[None]).last_hidden_state
            lang, cand = hf_detect(m, enc, init[0], lang_ids)
            srt = np.sort(cand)
            gap = float(srt[-1] - srt[-2])
            if gap < MARGIN:
                print(f"  {name}: row {rows} seed {seed}: language gap {gap:.2e} below {MARGIN}, next", flush=True)
                continue
            tries += 1
            assert tries < 200, "no usable clip found"
            if len(set(langs)) < 3 and lang in langs and tries < 60:  # spread the languages over the rows
                continue
            ini = list(init)
            ini[1] = lang
            prompt = rng.integers(4, text_hi, L - len(init)).tolist() + ini
            ids, lps, avg, _ = hf_greedy_lp(m, enc, prompt, max_loop, setup, 1, sup, bsup)
            if all(np.array_equal(ids, hf_greedy_lp(m, enc, prompt, max_loop, setup, 1, sup, bsup, rng)[0]) for _ in range(N_DRAWS)):
                break
            print(f"  {name}: row {rows} seed {seed} unstable under noise, next", flush=True)
        assert lang == lang_ids[int(np.argmax(cand))], "HF detect_language is not the arg-max of the candidates' raw logits"
        e = np.exp(cand - cand.max())
        nsp, _ = hf_no_speech(m, enc, prompt, len(init), token)
        k = f"s{rows}_"
        out[k + "case"] = np.array(case)
        out[k + "seed"] = np.int64(seed)
        out[k + "gain"] = np.float32(gain)
        out[k + "tilt"] = np.float32(tilt)
        out[k + "lang"] = np.int32(lang)
        out[k + "lang_probs"] = (e / e.sum()).astype(np.float64)
        out[k + "prompt"] = np.asarray(prompt, np.int32)
        out[k + "ids"] = ids
        out[k + "logprobs"] = lps
        out[k + "avg_logprob"] = avg
        out[k + "no_speech_prob"] = nsp
        out[k + "lang_logits"] = cand.astype(np.float64)  # HF's raw fp32 logits of the candidates, widened
        if case == "shared" and rows == 0:  # once per model: generate's own default route gives the stored language and ids
            try:
                glang, gen = hf_generate_default(m, lang_mel(cfg, seed, gain, tilt), setup, lang_ids, sup, bsup, max_loop)
            except Exception as ex:  # HF refuses the synthetic configuration: the reason goes to DESIGN §19
                print(f"{name}: generate(language=None) refused: {type(ex).__name__}: {ex}", flush=True)
                out["generate_checked"] = np.int32(0)
            else:
                assert glang == lang, (glang, lang)
                assert np.array_equal(gen, ids[len(prompt):]), (gen, ids)
                out["generate_checked"] = np.int32(1)
                print(f"{name}: generate(language=None) reproduces language {lang} and the {len(gen)} ids", flush=True)
        gaps.append(gap)
        langs.append(lang)
        print(f"{name}: row {rows} {case} L={L} seed {seed}: language {lang} (p {e.max() / e.sum():.3f}, gap {gap:.3f}), {len(lps)} generated, "
              f"avg_logprob {avg:.4f}, no_speech_prob {nsp:.3e}", flush=True)
        rows += 1
    assert len(set(langs)) >= 3, langs
    if long_cases:
        mark_multilingual(m, cfg, setup, lang_ids, sup, bsup)
        make_long(name, cfg, m, out, lang_ids, long_cases, max_loop, tilt_max)
    out["s_rows"] = np.int32(rows)
    out["s_min_gap"] = np.float64(min(gaps))
    path = os.path.join(GOLDEN, f"lang_detect_{name}_hf.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; smallest language gap", min(gaps), "languages", langs, flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["micro", "tiny"]
    torch.manual_seed(0)
    torch.set_num_threads(16)
    if "micro" in which:
        make("micro", WhisperConfig.micro(), 14, 11, 0.3, 7.0, 16.0)
    if "tiny" in which:
        make("tiny", WhisperConfig.tiny(), 24, 11, 0.3, long_cases={"plain": (0, [7000, 5200, 8400]), "cond": (1, [9000, 6100])})
