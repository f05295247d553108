#!/usr/bin/env python3
"""Generates the per-utterance prompt fixtures from HF transformers' own code, for wm_op_long_prompt,
wm_transcribe_rows and wm_transcribe_long_ex.

  long_prompt_rows.npz       WhisperGenerationMixin._prepare_decoder_input_ids on crafted segment lists, one utterance each: no
                             segments, one short segment, a double-timestamp ending (last id dropped), a two-id segment (kept),
                             history longer than cut_off_length, prompt_ids first-segment before / after the first window,
                             all-segments, prompt_ids without conditioning; n_text_ctx 64 and 448.
  prompt_rows_{micro,tiny}_hf.npz
                             HF-mode greedy decoding (fp32) of single recordings whose decoder input starts with a prompt of
                             1 .. 31 (micro) / 1 .. 228 (tiny) ids, with HF's WhisperTimeStampLogitsProcessor (begin_index = the
                             prompt length) on and off.  One row per (length, rules); ids stored per row.
  long_form_prompt_{micro,tiny}_hf.npz
                             HF generate long-form (greedy, return_timestamps, return_segments) with condition_on_prev_tokens /
                             prompt_ids / prompt_condition_type on ragged batches of synth.synth_long_mel recordings, the storage
                             scheme of long_form_*_hf.npz plus the options.  Every recording is ALSO run alone; the batched result
                             must equal the single ones (inputs on which it does not are skipped), the single ones are stored.

Every stored case survives three draws of 1e-5 relative noise on every step's processed scores (seeds that do not are skipped).

Usage: python tools/make_golden_prompts.py [rows] [micro] [tiny]   (dev container: needs transformers; never at test time)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden import hf_model  # noqa: E402
from make_golden_long_form import N_DRAWS, PERTURB, Perturb, ids_setup, same  # noqa: E402
from whisper_mojo_amd import WhisperConfig, synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
COND_TYPES = ("first-segment", "all-segments")


def prev_sot_of(cfg):
    return 50361 if cfg.vocab_size > 50363 else 939


# ---- _prepare_decoder_input_ids on crafted segment lists --------------------------------------------------------------------
def hf_prompt(segments, init, n_text_ctx, tb, prev_sot, prompt_ids, cond, cond_type):
    """One utterance through HF's own code; segments = its real segments so far (lists of ids)."""
    from types import SimpleNamespace

    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin as G
    gc = SimpleNamespace(prev_sot_token_id=prev_sot, prompt_condition_type=cond_type, pad_token_id=0, cache_implementation=None)
    pid = None if prompt_ids is None else torch.tensor(prompt_ids, dtype=torch.long)
    cur = G._prepare_segments(prompt_ids=pid, batch_size=1, generation_config=gc)
    cur[0] = cur[0] + [{"tokens": torch.tensor(s, dtype=torch.long)} for s in segments]
    ids, _ = G._prepare_decoder_input_ids(
        cur_bsz=1, init_tokens=torch.tensor([init], dtype=torch.long), current_segments=cur, batch_idx_map=[0],
        do_condition_on_prev_tokens=[bool(cond)], prompt_ids=pid, generation_config=gc,
        config=SimpleNamespace(max_target_positions=n_text_ctx), device="cpu", suppress_tokens=None, timestamp_begin=tb, kwargs={})
    return ids[0].numpy().astype(np.int32)


def make_rows():
    out, names = {}, []
    rng = np.random.default_rng(3)
    for ctx, tb, prev_sot, init in ((64, 941, 939, [1, 2, 3]), (448, 50364, 50361, [50258, 50259, 50359])):
        T = lambda p: tb + p  # noqa: E731
        txt = lambda n: rng.integers(4, 800, n).tolist()  # noqa: E731
        pids = [prev_sot] + txt(5)
        cut = ctx // 2 - 1
        cases = {
            "no_segments": ([], None, 1, 0),
            "one_short": ([[T(0)] + txt(3) + [T(10)]], None, 1, 0),
            "double_ts_end": ([[T(0)] + txt(4) + [T(20), T(20)]], None, 1, 0),
            "two_ids": ([[T(7), T(7)]], None, 1, 0),
            "three_ids_ts": ([[11, T(7), T(9)]], None, 1, 0),
            "several": ([[T(0)] + txt(2) + [T(9), T(9)], txt(2), [T(9), 5, T(30), T(30)]], None, 1, 0),
            "long_history": ([[T(0)] + txt(cut // 2) + [T(50)], [T(50)] + txt(cut) + [T(90), T(90)]], None, 1, 0),
            "exact_cut": ([txt(cut)], None, 1, 0),
            "cond_off": ([[T(0)] + txt(3) + [T(10)]], None, 0, 0),
            "first_seg_before": ([], pids, 1, 0),
            "first_seg_after": ([[T(0)] + txt(3) + [T(10), T(10)]], pids, 1, 0),
            "first_seg_no_sot": ([txt(3)], pids[1:], 1, 0),
            "first_seg_long": ([txt(cut - 3)], pids, 1, 0),
            "all_seg_before": ([], pids, 1, 1),
            "all_seg_after": ([[T(0)] + txt(3) + [T(10), T(10)], txt(4)], pids, 1, 1),
            "all_seg_long": ([txt(cut + 9)], pids, 1, 1),
            "prompt_no_cond": ([[T(0)] + txt(3) + [T(10)]], pids, 0, 0),
            "prompt_no_cond_before": ([], pids, 0, 0),
        }
        for name, (segs, p, cond, ct) in cases.items():
            key = f"c{ctx}_{name}"
            ids = hf_prompt(segs, init, ctx, tb, prev_sot, p, cond, COND_TYPES[ct])
            out[key + "_seq"] = np.asarray([t for s in segs for t in s], np.int32)
            out[key + "_count"] = np.asarray([len(s) for s in segs], np.int32)
            out[key + "_prompt_ids"] = np.asarray([] if p is None else p, np.int32)
            out[key + "_opts"] = np.asarray([cond, ct, ctx, tb, prev_sot], np.int32)
            out[key + "_init"] = np.asarray(init, np.int32)
            out[key + "_expect"] = ids
            names.append(key)
    out["names"] = np.array(names)
    path = os.path.join(GOLDEN, "long_prompt_rows.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(names), "cases", flush=True)


# ---- short-form rows with long prompts ---------------------------------------------------------------------------------------
@torch.no_grad()
def hf_greedy(m, enc_out, prompt, max_loop, setup, ts_on, max_init, rng=None):
    """Greedy HF-mode decoding from decoder ids `prompt`: at most 1 + max_loop generated ids, stops after eos."""
    from types import SimpleNamespace

    from transformers import WhisperTimeStampLogitsProcessor
    from transformers.modeling_outputs import BaseModelOutput
    eo = BaseModelOutput(last_hidden_state=enc_out)
    proc = None
    if ts_on:
        gc = SimpleNamespace(eos_token_id=setup["eos"], no_timestamps_token_id=setup["no_ts"], max_initial_timestamp_index=max_init)
        proc = WhisperTimeStampLogitsProcessor(gc, begin_index=len(prompt))
    noise = Perturb(rng) if rng is not None else None
    toks = list(int(t) for t in prompt)
    out = m(decoder_input_ids=torch.tensor([toks]), encoder_outputs=eo, use_cache=True)
    for _ in range(1 + max_loop):
        scores = out.logits[:, -1].float()
        ids = torch.tensor([toks])
        if proc is not None:
            scores = proc(ids, scores)
        if noise is not None:
            scores = noise(ids, scores)
        nxt = int(scores[0].argmax())
        toks.append(nxt)
        if nxt == setup["eos"]:
            break
        out = m(decoder_input_ids=torch.tensor([[nxt]]), encoder_outputs=eo, past_key_values=out.past_key_values, use_cache=True)
    return np.asarray(toks, np.int32)


@torch.no_grad()
def make_short(name, cfg, lengths, max_loop):
    m = hf_model(cfg, synth.split_weights(cfg, synth.synth_weights(cfg, 0)), False)
    setup = ids_setup(cfg)
    init = setup["prompt"]
    assert max(lengths) + 1 + max_loop <= cfg.n_text_ctx
    out = dict(init=np.asarray(init, np.int32), eos=np.int32(setup["eos"]), no_ts=np.int32(setup["no_ts"]),
               timestamp_begin=np.int32(setup["no_ts"] + 1), max_loop=np.int32(max_loop), max_init=np.int32(50),
               perturb_rel=np.float64(PERTURB))
    rng = np.random.default_rng(17)
    rows = 0
    for ts_on in (0, 1):
        for L in lengths:
            seed = 3000 + 97 * rows
            while True:
                seed += 1
                text = rng.integers(4, min(setup["eos"], 800 if cfg.vocab_size < 2000 else 50000), max(L - len(init), 0)).tolist()
                prompt = (text + init)[-L:] if L >= len(init) else init[:L]
                enc = m.model.encoder(torch.from_numpy(synth.synth_mel(cfg, seed))[None]).last_hidden_state
                base = hf_greedy(m, enc, prompt, max_loop, setup, ts_on, 50)
                if all(np.array_equal(base, hf_greedy(m, enc, prompt, max_loop, setup, ts_on, 50, rng)) for _ in range(N_DRAWS)):
                    break
                print(f"  {name}: row {rows} seed {seed} unstable under noise, next", flush=True)
            out[f"r{rows}_seed"] = np.int64(seed)
            out[f"r{rows}_ts"] = np.int32(ts_on)
            out[f"r{rows}_prompt"] = np.asarray(prompt, np.int32)
            out[f"r{rows}_ids"] = base
            print(f"{name}: row {rows} L={L} ts={ts_on} -> {len(base) - L} generated", flush=True)
            rows += 1
    out["n_rows"] = np.int32(rows)
    path = os.path.join(GOLDEN, f"prompt_rows_{name}_hf.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", flush=True)


# ---- long-form with conditioning / prompt_ids ------------------------------------------------------------------------------------
@torch.no_grad()
def hf_long_ex(m, cfg, mels, lengths, setup, max_new, opt, rng=None):
    from transformers import GenerationConfig, LogitsProcessorList
    B, Tm = len(lengths), max(lengths)
    feats = np.zeros((B, cfg.n_mels, Tm), np.float32)
    mask = np.zeros((B, Tm), np.int64)
    for b, (mel, n) in enumerate(zip(mels, lengths)):
        feats[b, :, :n] = mel
        mask[b, :n] = 1
    p = setup["prompt"]
    gc = GenerationConfig(decoder_start_token_id=p[0], forced_decoder_ids=[[i, t] for i, t in enumerate(p[1:], 1)],
                          eos_token_id=setup["eos"], pad_token_id=setup["eos"], no_timestamps_token_id=setup["no_ts"],
                          max_initial_timestamp_index=50, prev_sot_token_id=prev_sot_of(cfg))
    kw = dict(logits_processor=LogitsProcessorList([Perturb(rng)])) if rng is not None else {}
    if opt["prompt_ids"] is not None:
        kw.update(prompt_ids=torch.tensor(opt["prompt_ids"], dtype=torch.long), prompt_condition_type=COND_TYPES[opt["cond_type"]])
    out = m.generate(torch.from_numpy(feats), attention_mask=torch.from_numpy(mask), generation_config=gc, return_timestamps=True,
                     return_segments=True, condition_on_prev_tokens=bool(opt["cond"]), temperature=0.0, num_beams=1,
                     max_new_tokens=max_new, **kw)
    res = []
    for b in range(B):
        segs = [(s["tokens"].numpy().astype(np.int32), float(s["start"]), float(s["end"])) for s in out["segments"][b]]
        res.append((np.concatenate([s[0] for s in segs]) if segs else np.zeros(0, np.int32), segs))
    return res


@torch.no_grad()
def history_bound(segs, max_new, tb):
    """A lower bound of the previous ids in front of an utterance's LAST window: its segments' ids as _pad_to_max_length counts them
    (a segment of more than two ids ending in a timestamp pair loses one), without the trailing segments that hold the last
    max_new ids (a window generates at most that many)."""
    kept = [len(t) - (1 if len(t) > 2 and t[-2] >= tb else 0) for t, _, _ in segs]
    tail = 0
    while kept and tail < max_new:
        tail += len(segs[len(kept) - 1][0])
        kept.pop()
    return sum(kept)


def make_long(name, cfg, cases, only=None):
    """only: regenerate that case alone and keep the others of the existing file"""
    m = hf_model(cfg, synth.split_weights(cfg, synth.synth_weights(cfg, 0)), False)
    setup = ids_setup(cfg)
    out = dict(prompt=np.asarray(setup["prompt"], np.int32), eos=np.int32(setup["eos"]), no_ts=np.int32(setup["no_ts"]),
               timestamp_begin=np.int32(setup["no_ts"] + 1), prev_sot=np.int32(prev_sot_of(cfg)), perturb_rel=np.float64(PERTURB))
    path = os.path.join(GOLDEN, f"long_form_prompt_{name}_hf.npz")
    if only:
        old = np.load(path)
        out = {k: old[k] for k in old.files if not k.startswith(only + "_")}
    names = []
    for case, (lengths, max_new, opt) in cases.items():
        seed = {"micro": 7000, "tiny": 9000}[name] + 100 * len(names)
        if only and case != only:
            names.append(case)
            continue
        rng = np.random.default_rng(seed)
        while True:
            seed += 1
            seeds = [seed * 10 + b for b in range(len(lengths))]
            mels = [synth.synth_long_mel(cfg, s, n) for s, n in zip(seeds, lengths)]
            singles = [hf_long_ex(m, cfg, [mel], [n], setup, max_new, opt)[0] for mel, n in zip(mels, lengths)]
            if not all(same([sg], hf_long_ex(m, cfg, [mel], [n], setup, max_new, opt, rng)) for sg, mel, n in zip(singles, mels, lengths)
                       for _ in range(N_DRAWS)):
                print(f"  {name}/{case}: seed {seed} unstable under noise, next", flush=True)
                continue
            # the target semantics are per utterance; only inputs on which HF's batched run agrees with its single runs are kept
            if len(lengths) == 1 or same(hf_long_ex(m, cfg, mels, lengths, setup, max_new, opt), singles):  # (a batch of one IS the single run)
                break
            print(f"  {name}/{case}: seed {seed}: the batched HF run differs from the recordings run alone, next", flush=True)
        out[case + "_lengths"] = np.asarray(lengths, np.int32)
        out[case + "_seeds"] = np.asarray(seeds, np.int64)
        out[case + "_max_new_tokens"] = np.int32(max_new)
        out[case + "_cond"] = np.int32(opt["cond"])
        out[case + "_cond_type"] = np.int32(opt["cond_type"])
        out[case + "_prompt_ids"] = np.asarray([] if opt["prompt_ids"] is None else opt["prompt_ids"], np.int32)
        for b, (seq, segs) in enumerate(singles):
            out[f"{case}_u{b}_sequence"] = seq
            out[f"{case}_u{b}_count"] = np.asarray([len(s[0]) for s in segs], np.int32)
            out[f"{case}_u{b}_start"] = np.asarray([s[1] for s in segs], np.float64)
            out[f"{case}_u{b}_end"] = np.asarray([s[2] for s in segs], np.float64)
        if case == "long_history":  # some window must carry the whole cut: a lower bound of the history in front of the last window
            cut = cfg.n_text_ctx // 2 - 1
            hist = max(history_bound(segs, max_new, int(out["timestamp_begin"])) for _, segs in singles)
            assert hist > cut, f"{name}/{case}: history {hist} stays below {cut} ids"
        names.append(case)
        print(f"{name}/{case}: lengths {lengths}, ids", [len(s) for s, _ in singles], "segments", [len(s) for _, s in singles], flush=True)
    out["cases"] = np.array(names)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", flush=True)


def opt(cond, prompt_ids=None, cond_type=0):
    return dict(cond=cond, prompt_ids=prompt_ids, cond_type=cond_type)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    what = sys.argv[1:] or ["rows", "micro", "tiny"]  # micro / tiny: both parts; micro_short, micro_long, ...: one part
    only = next((w.split(":", 1)[1] for w in what if w.startswith("only:")), None)  # e.g. tiny_long only:long_history
    for n in ("micro", "tiny"):
        if n in what:
            what += [n + "_short", n + "_long"]
    if "rows" in what:
        make_rows()
    if "micro_short" in what:
        make_short("micro", WhisperConfig.micro(), [1, 4, 5, 16, 17, 31], 24)
    if "micro_long" in what:
        cfg = WhisperConfig.micro()
        pid = [prev_sot_of(cfg), 77, 301, 12]
        make_long("micro", cfg, {
            "cond": ([700, 455, 150, 1130], 20, opt(1)),
            "first_segment": ([610, 1000, 90], 20, opt(1, pid, 0)),
            "all_segments": ([900, 380, 640], 20, opt(1, pid, 1)),
            "prompt_no_cond": ([520, 1010], 20, opt(0, pid, 0)),
            "long_history": ([2400, 800], 24, opt(1)),
            "max_new": ([900, 380], 8, opt(1)),
        })
    if "tiny_short" in what:
        make_short("tiny", WhisperConfig.tiny(), [1, 4, 17, 100, 228], 40)
    if "tiny_long" in what:
        cfg = WhisperConfig.tiny()
        pid = [prev_sot_of(cfg), 2425, 11, 1002, 318]
        make_long("tiny", cfg, {
            "cond": ([9000, 4400, 2100], 40, opt(1)),
            "first_segment": ([7000, 2500], 40, opt(1, pid, 0)),
            "all_segments": ([6500, 3100], 40, opt(1, pid, 1)),
            "prompt_no_cond": ([6100, 2000], 40, opt(0, pid, 0)),
            "long_history": ([100000], 40, opt(1)),  # history beyond cut_off_length = 223 ids (asserted in make_long)
            "max_new": ([7000, 2500], 10, opt(1)),
        }, only)
