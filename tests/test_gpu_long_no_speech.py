"""Long-form tests (-m gpu) of logprob_threshold / no_speech_threshold: the window scheduler's skip rule, seek advance,
window log and per-segment quality values against a host restatement of HF's loop — window by window over the library's own
transcribe_batch(..., no_speech_token=) (whose values tests/test_gpu_no_speech.py holds to HF's), HF's _need_fallback rule at the
single temperature 0, wm_op_long_segments and wm_op_long_prompt.  Batch invariance is bitwise, so everything is compared exactly.

The thresholds of those restated runs are inputs taken between the values of a first run without skipping, so that the decisions split.

test_tiny_matches_hf_generate compares with HF itself: the long-form fixture of tools/make_golden_no_speech.py (real generate() runs
with both thresholds, tiny, a ragged unconditioned case and a conditioned one): sequences, segment boundaries and times, seeks and
skipped flags exactly; avg_logprob and log no_speech_prob within 1e-4."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()
    import whisper_mojo_amd as pkg
    return pkg


def _model(cfg, max_batch):
    from whisper_mojo_amd import GELU_ERF, POS_HF, synth
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=max_batch)
    m.load(WeightLoader.from_array(synth.synth_weights(cfg, 0)))
    return m


def _ids(cfg):
    if cfg.vocab_size > 50363:
        return dict(prompt=(50258, 50259, 50359), eot=50257, timestamps=(50364, 50363, 50)), 50362, 50361
    return dict(prompt=(1, 2, 3), eot=900, timestamps=(941, 940, 50)), 939, 938


def restate(m, cfg, mel, n, kw, token, prev_sot, lt, nt, cond):
    """One recording through HF's loop on the host -> (result in the library's form, window log)"""
    from whisper_mojo_amd import _lib
    W, tb, init = cfg.n_frames, kw["timestamps"][0], list(kw["prompt"])
    seek, segs, log = 0, [], []
    while seek < n:
        snf = min(n - seek, W)
        win = np.zeros((1, cfg.n_mels, W), np.float32)
        win[0, :, :snf] = mel[:, seek:seek + snf]
        prompt = _lib.long_prompt([s["tokens"] for s in segs], init, tb, cfg.n_text_ctx, None, cond, "first-segment", prev_sot) if cond else init
        kw1 = {k: v for k, v in kw.items() if k != "prompt"}
        pk = dict(prompt=init) if prompt == init else dict(prompts=[prompt])  # (a pass whose rows all carry the initial ids goes out shared)
        ids, (_, avg, nsp) = m.transcribe_batch(win, return_logprobs=True, no_speech_token=token, n_init=len(init), **pk, **kw1)
        gen = ids[0][len(prompt):]
        if gen and gen[-1] == kw["eot"]:
            gen = gen[:-1]
        skip = nt is not None and float(avg[0]) < lt and float(nsp[0]) > nt
        log.append(dict(seek=seek, avg_logprob=float(avg[0]), no_speech_prob=float(nsp[0]), skipped=bool(skip)))
        if skip:
            seek += snf
            continue
        rows, adv = _lib.long_segments(gen, tb, seek, snf)
        for first, count, start, end in rows:
            segs.append(dict(start=start, end=end, tokens=gen[first:first + count], avg_logprob=float(avg[0]), no_speech_prob=float(nsp[0])))
        seek += adv if adv else snf
    return dict(sequence=[t for s in segs for t in s["tokens"]], segments=segs, windows=log), log


def between(values):
    """a float32 strictly between the two middle values of the sorted list"""
    v = np.sort(np.asarray(values, np.float64))
    k = len(v) // 2
    assert v[k - 1] < v[k]
    t = float(np.float32(0.5 * (v[k - 1] + v[k])))
    assert v[k - 1] < t < v[k]
    return t


def _run_case(name, cond, lengths, max_batch, seed0):
    from whisper_mojo_amd import WhisperConfig, synth
    cfg = WhisperConfig.micro() if name == "micro" else WhisperConfig.tiny()
    kw, token, prev_sot = _ids(cfg)
    kw = dict(kw, max_loop=23)
    m = _model(cfg, max_batch)
    mels = [synth.synth_long_mel(cfg, seed0 + b, n) for b, n in enumerate(lengths)]
    lo = dict(condition_on_prev_tokens=cond, prev_sot_token=prev_sot)
    plain = m.transcribe_long_form(mels, **kw, **lo)
    # thresholds that can never trigger: the plain run's sequences, plus the quality values of the restated loop
    never, st = m.transcribe_long_form(mels, return_stats=True, logprob_threshold=-np.inf, no_speech_threshold=0.5, no_speech_token=token, **kw, **lo)
    assert st["skipped_windows"] == 0
    base = [restate(m, cfg, mel, n, kw, token, prev_sot, -np.inf, 0.5, cond)[0] for mel, n in zip(mels, lengths)]
    for b in range(len(lengths)):
        assert never[b]["sequence"] == plain[b]["sequence"] == base[b]["sequence"]
        assert [(s["start"], s["end"], s["tokens"]) for s in never[b]["segments"]] == [(s["start"], s["end"], s["tokens"]) for s in plain[b]["segments"]]
        assert never[b] == base[b], (b, never[b]["windows"], base[b]["windows"])
    # logprob_threshold alone: same ids, quality values available
    only_lp = m.transcribe_long_form(mels, logprob_threshold=0.0, no_speech_token=token, **kw, **lo)
    assert only_lp == never
    # thresholds between the observed values: the decisions split
    w = [e for r in base for e in r["windows"]]
    lt, nt = between([e["avg_logprob"] for e in w]), between([e["no_speech_prob"] for e in w])
    got, st = m.transcribe_long_form(mels, return_stats=True, logprob_threshold=lt, no_speech_threshold=nt, no_speech_token=token, **kw, **lo)
    want = [restate(m, cfg, mel, n, kw, token, prev_sot, lt, nt, cond)[0] for mel, n in zip(mels, lengths)]
    ww = [e for r in want for e in r["windows"]]
    print(f"{name} cond {cond}: thresholds {lt:.5f} / {nt:.4e}; windows (seek, avg, nsp, skipped):",
          [[(e["seek"], round(e["avg_logprob"], 4), float(f"{e['no_speech_prob']:.4g}"), int(e["skipped"])) for e in r["windows"]] for r in want])
    for b in range(len(lengths)):
        assert got[b]["windows"] == want[b]["windows"], b  # seeks and flags exact, values bitwise (batch invariance)
        assert got[b] == want[b], b
    assert st["skipped_windows"] == sum(e["skipped"] for e in ww)
    assert st["windows"] == len(ww)
    m.close()
    return want, lt, nt


def test_micro_skip_rule_matches_restated_loop(hip):
    want, lt, nt = _run_case("micro", False, [1130, 900, 700, 455], 4, 500)
    ww = [e for r in want for e in r["windows"]]
    assert any(e["skipped"] for e in ww) and sum(not e["skipped"] for e in ww) >= 2
    assert any(r["windows"][i]["skipped"] and any(not e["skipped"] for e in r["windows"][i + 1:]) for r in want for i in range(len(r["windows"])))
    # a skipped window leaves no segment: every segment's values are a kept window's
    kept = {(e["avg_logprob"], e["no_speech_prob"]) for e in ww if not e["skipped"]}
    assert all((s["avg_logprob"], s["no_speech_prob"]) in kept for r in want for s in r["segments"])


def test_micro_conditioned_skip_leaves_history_without_the_window(hip):
    want, lt, nt = _run_case("micro", True, [1200, 1000], 2, 520)
    assert any(r["windows"][i]["skipped"] and any(not e["skipped"] for e in r["windows"][:i]) for r in want for i in range(len(r["windows"])))


def test_tiny_ragged_batch(hip):
    want, lt, nt = _run_case("tiny", False, [9000, 7000, 4400], 2, 540)
    assert any(e["skipped"] for r in want for e in r["windows"])


def test_quality_needs_thresholds_and_c_refusals(hip):
    from whisper_mojo_amd import WhisperConfig, _lib, synth
    cfg = WhisperConfig.micro()
    kw, token, prev_sot = _ids(cfg)
    m = _model(cfg, 2)
    mel = np.ascontiguousarray(synth.synth_long_mel(cfg, 560, 450)[None])
    L = _lib.lib()
    opts, _keep = m._opts(kw["prompt"], kw["eot"], 20, False, (), (), kw["timestamps"])
    args = (m._h, C.c_void_p(mel.ctypes.data), 0, 1, 450, None, C.byref(opts))
    h = C.c_void_p()
    _lib.check(L.wm_transcribe_long_ex(*args, C.byref(_lib.WmLongOpts(0, prev_sot, None, 0, 0)), C.byref(h)))
    n, f = C.c_int32(), (C.c_float * 64)()
    assert L.wm_long_result_quality(h, 0, f, f) == -5      # WM_E_STATE: a run without thresholds
    assert L.wm_long_result_windows(h, 0, C.byref(n), None, None, None, None) == -5
    sk = C.c_int32(7)
    _lib.check(L.wm_long_result_skip_stats(h, C.byref(sk)))
    assert sk.value == 0
    L.wm_long_result_free(h)
    bad = [_lib.WmLongOpts(0, prev_sot, None, 0, 0, 0, 0.0, 1, 0.5, token),              # no_speech_threshold without logprob_threshold
           _lib.WmLongOpts(0, prev_sot, None, 0, 0, 1, -1.0, 1, 0.5, -1),                # ... without a vocabulary id
           _lib.WmLongOpts(0, prev_sot, None, 0, 0, 1, -1.0, 1, 0.5, cfg.vocab_size)]
    for lo in bad:
        h = C.c_void_p()
        assert L.wm_transcribe_long_ex(*args, C.byref(lo), C.byref(h)) == -1 and not h.value
    m.close()


def _fixture_model(z, cfg, max_batch):
    """the fixture's model: token embedding scaled, <|nospeech|> row replaced (the numbers are in the fixture), HF mode"""
    from whisper_mojo_amd import GELU_ERF, POS_HF, synth
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    flat = synth.synth_weights(cfg, 0)
    emb = synth.split_weights(cfg, flat)["dec.tok_emb"]
    emb[:] *= np.float32(z["emb_scale"])
    emb[int(z["no_speech_token"])] = (np.random.default_rng(int(z["ns_row_seed"])).standard_normal(cfg.d_model) * float(z["ns_row_scale"])).astype(np.float32)
    m = Whisper(cfg, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=max_batch)
    m.load(WeightLoader.from_array(flat))
    return m


def _faded_mel(cfg, seed, n, gains, tilts):
    """tools/make_golden_no_speech.py faded_mel: block k of n_frames frames becomes g·x - (1 - g) + t·linspace(-1, 1, n_mels)"""
    from whisper_mojo_amd import synth
    mel = synth.synth_long_mel(cfg, seed, n)
    W = cfg.n_frames
    ramp = np.linspace(-1, 1, cfg.n_mels, dtype=np.float32)[:, None]
    for k, (g, t) in enumerate(zip(gains, tilts)):
        g, t = np.float32(g), np.float32(t)
        mel[:, k * W:(k + 1) * W] = g * mel[:, k * W:(k + 1) * W] - (np.float32(1) - g) + t * ramp
    return mel


def test_tiny_matches_hf_generate(hip):
    from whisper_mojo_amd import WhisperConfig
    cfg = WhisperConfig.tiny()
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "no_speech_tiny_hf.npz"))
    tok = int(z["no_speech_token"])
    m = _fixture_model(z, cfg, 2)
    seen = dict(skipped=0, kept=0, ns_only=0, lp_only=0, after_history=0)
    for case in z["cases"]:
        case = str(case)
        lengths = [int(v) for v in z[case + "_lengths"]]
        cond = bool(z[case + "_cond"])
        lt, nt = float(z[case + "_logprob_threshold"]), float(z[case + "_no_speech_threshold"])
        mels = [_faded_mel(cfg, int(sd), n, z[f"{case}_u{b}_gains"], z[f"{case}_u{b}_tilts"]) for b, (sd, n) in enumerate(zip(z[case + "_seeds"], lengths))]
        got, st = m.transcribe_long_form(mels, prompt=tuple(int(v) for v in z["prompt"]), eot=int(z["eos"]), max_loop=int(z["max_new_tokens"]) - 1,
                                         suppress_tokens=[tok], timestamps=(int(z["timestamp_begin"]), int(z["no_ts"]), int(z["max_init"])),
                                         condition_on_prev_tokens=cond, prev_sot_token=int(z["prev_sot"]), logprob_threshold=lt,
                                         no_speech_threshold=nt, no_speech_token=tok, return_stats=True)
        assert st["stalled"] == 0
        for b in range(len(lengths)):
            k = f"{case}_u{b}_"
            wl = got[b]["windows"]
            avg, nsp = np.asarray([e["avg_logprob"] for e in wl], np.float64), np.asarray([e["no_speech_prob"] for e in wl], np.float64)
            print(f"tiny {case} u{b}: seeks {[e['seek'] for e in wl]} skipped {[int(e['skipped']) for e in wl]} (HF {z[k + 'w_skipped'].tolist()}); "
                  f"max |avg - HF| {np.abs(avg - z[k + 'w_avg_logprob']).max() if len(wl) == len(z[k + 'w_seek']) else None}, "
                  f"max |Δ log nsp| {np.abs(np.log(nsp) - np.log(z[k + 'w_no_speech_prob'].astype(np.float64))).max() if len(wl) == len(z[k + 'w_seek']) else None}")
            assert [e["seek"] for e in wl] == z[k + "w_seek"].tolist(), (case, b)
            assert [int(e["skipped"]) for e in wl] == z[k + "w_skipped"].tolist(), (case, b)
            assert np.abs(avg - z[k + "w_avg_logprob"]).max() <= 1e-4, (case, b)
            assert np.abs(np.log(nsp) - np.log(z[k + "w_no_speech_prob"].astype(np.float64))).max() <= 1e-4, (case, b)
            assert got[b]["sequence"] == z[k + "sequence"].tolist(), (case, b)
            assert [len(s["tokens"]) for s in got[b]["segments"]] == z[k + "count"].tolist(), (case, b)
            assert [s["start"] for s in got[b]["segments"]] == z[k + "start"].tolist(), (case, b)  # float64, bit for bit
            assert [s["end"] for s in got[b]["segments"]] == z[k + "end"].tolist(), (case, b)
            kept_before = False
            for e in wl:
                seen["skipped"] += e["skipped"]
                seen["kept"] += not e["skipped"]
                seen["ns_only"] += (not e["skipped"]) and e["no_speech_prob"] > nt   # one threshold crossed, the window kept
                seen["lp_only"] += (not e["skipped"]) and e["avg_logprob"] < lt
                seen["after_history"] += bool(cond and e["skipped"] and kept_before)
                kept_before = kept_before or not e["skipped"]
        assert st["skipped_windows"] == sum(int(v) for b in range(len(lengths)) for v in z[f"{case}_u{b}_w_skipped"])
    assert seen["skipped"] >= 2 and seen["kept"] >= 2 and seen["ns_only"] >= 1 and seen["lp_only"] >= 1 and seen["after_history"] >= 1, seen
    m.close()
