"""CPU tests of the no-speech probe's definition and host interface.

  * A float64 restatement — softmax over the whole vocabulary of the fixture's raw logits at the <|startoftranscript|> position,
    read at no_speech_token — reproduces the value HF's WhisperNoSpeechDetection recorded (tools/make_golden_no_speech.py) to 1e-5.
  * A replay of HF's recorded long-form window log (tiny) — the skip rule, the seek advance of skipped and kept windows through
    wm_op_long_segments — reproduces HF's should_skip flags, seeks, segments and sequences.
  * The new symbols are exported and the ABI version is 5.
  * The host-side refusals that need no GPU."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_float64_softmax_reproduces_hf_no_speech_prob():
    z = np.load(os.path.join(GOLDEN, "no_speech_micro_hf.npz"))
    token = int(z["no_speech_token"])
    assert token == int(z["no_ts"]) - 1  # HF: no_timestamps_token_id - 1
    n = int(z["s_rows"])
    assert n >= 6
    lens = set()
    for i in range(n):
        raw = z[f"s{i}_sot_logits"].astype(np.float64)
        p = np.exp(raw - raw.max())
        p /= p.sum()
        want = float(z[f"s{i}_no_speech_prob"])
        assert 0 < want < 1
        assert abs(np.log(p[token]) - np.log(want)) <= 1e-5, (i, p[token], want)
        prompt = z[f"s{i}_prompt"].tolist()
        assert prompt[-len(z["init"]):] == z["init"].tolist()  # the probed position is len(prompt) - n_init
        lens.add(len(prompt))
    assert max(lens) > 16 + len(z["init"])  # a prefix longer than one prefill chunk


def test_replay_of_hf_window_log_reproduces_decisions_seeks_and_sequences():
    """HF's recorded long-form runs (generate with both thresholds, one recording at a time): the skip rule on the recorded
    avg_logprob / no_speech_prob gives HF's should_skip flags; seek moves by the window's own frames after a skip and by
    _retrieve_segment's advance (wm_op_long_segments) otherwise, which gives HF's next seek; the kept windows' segments are HF's
    segments and sequence."""
    from whisper_mojo_amd import WhisperConfig, _lib
    z = np.load(os.path.join(GOLDEN, "no_speech_tiny_hf.npz"))
    W, tb, eos = WhisperConfig.tiny().n_frames, int(z["timestamp_begin"]), int(z["eos"])
    n_skip = n_keep = mixed_ns = mixed_lp = after_history = 0
    for case in z["cases"]:
        case = str(case)
        lt, nt = float(z[case + "_logprob_threshold"]), float(z[case + "_no_speech_threshold"])
        for u, n in enumerate(int(v) for v in z[case + "_lengths"]):
            k = f"{case}_u{u}_"
            ids_all, cnt = z[k + "w_ids"].tolist(), z[k + "w_count"].tolist()
            seek, off, seq, segs = 0, 0, [], []
            for i in range(len(cnt)):
                assert seek == int(z[k + "w_seek"][i]) < n, (case, u, i)
                snf = min(n - seek, W)
                avg, nsp = float(z[k + "w_avg_logprob"][i]), float(z[k + "w_no_speech_prob"][i])
                assert abs(avg - lt) >= 1e-2 and abs(np.log(nsp) - np.log(nt)) >= 1e-2  # the fixture's margins
                skip = avg < lt and nsp > nt
                assert skip == bool(z[k + "w_skipped"][i]), (case, u, i)
                ids = ids_all[off:off + cnt[i]]
                off += cnt[i]
                if ids and ids[-1] == eos:
                    ids = ids[:-1]
                n_skip, n_keep = n_skip + skip, n_keep + (not skip)
                mixed_ns += (not skip) and nsp > nt
                mixed_lp += (not skip) and avg < lt
                after_history += bool(skip and int(z[case + "_cond"]) and segs)
                if skip:
                    seek += snf
                    continue
                rows, adv = _lib.long_segments(ids, tb, seek, snf)
                assert adv > 0
                for first, count, start, end in rows:
                    segs.append((count, start, end))
                    seq += ids[first:first + count]
                seek += adv
            assert seek >= n
            assert seq == z[k + "sequence"].tolist(), (case, u)
            assert [c for c, _, _ in segs] == z[k + "count"].tolist()
            assert [t for _, t, _ in segs] == z[k + "start"].tolist() and [t for _, _, t in segs] == z[k + "end"].tolist()
    assert n_skip >= 2 and n_keep >= 2 and mixed_ns >= 1 and mixed_lp >= 1 and after_history >= 1


def test_symbols_and_abi_version():
    from whisper_mojo_amd import _lib
    L = _lib.lib()
    assert L.wm_abi_version() == 5 == _lib.ABI_VERSION
    for s in ("wm_transcribe_lp_ns", "wm_transcribe_submit_lp_ns", "wm_transcribe_wait_lp_ns", "wm_op_no_speech", "wm_long_result_quality",
              "wm_long_result_windows", "wm_long_result_skip_stats"):
        assert hasattr(L, s) and s in _lib.SYMBOLS, s
    import ctypes as C
    o = _lib.WmLongOpts(1, 939, None, 0, 0)  # a zero tail keeps the thresholds off
    assert (o.use_logprob_threshold, o.use_no_speech_threshold, o.no_speech_token) == (0, 0, 0)
    assert C.sizeof(_lib.WmLongOpts) == 48


def test_host_side_refusals_need_no_gpu():
    from whisper_mojo_amd import WhisperConfig, _lib
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.micro()
    m = Whisper(cfg)  # not loaded: every refusal below comes before the model is touched
    mel = np.zeros((1, cfg.n_mels, cfg.n_frames), np.float32)
    feats = np.zeros((1, cfg.n_mels, 500), np.float32)
    ts = (941, 940, 50)
    with pytest.raises(ValueError):  # HF dereferences logprob_threshold whenever no_speech_threshold is set
        m.transcribe_long_form(feats, prompt=(1, 2, 3), eot=900, timestamps=ts, no_speech_threshold=0.6, no_speech_token=939)
    with pytest.raises(ValueError):  # no token
        m.transcribe_long_form(feats, prompt=(1, 2, 3), eot=900, timestamps=ts, logprob_threshold=-1.0, no_speech_threshold=0.6)
    for tok in (-1, cfg.vocab_size):  # not a vocabulary id
        with pytest.raises(ValueError):
            m.transcribe_long_form(feats, prompt=(1, 2, 3), eot=900, timestamps=ts, logprob_threshold=-1.0, no_speech_threshold=0.6,
                                   no_speech_token=tok)
        with pytest.raises(ValueError):
            m.transcribe_batch(mel, prompt=(1, 2, 3), return_logprobs=True, no_speech_token=tok)
    with pytest.raises(ValueError):  # n_init larger than the prompt
        m.transcribe_batch(mel, prompt=(1, 2, 3), return_logprobs=True, no_speech_token=939, n_init=4)
    with pytest.raises(ValueError):  # ... than the shortest row's
        m.transcribe_batch(mel, prompts=[(5, 1, 2, 3), (2, 3)], return_logprobs=True, no_speech_token=939, n_init=3)
    with pytest.raises(ValueError):  # required with per-row prompts
        m.transcribe_batch(mel, prompts=[(5, 1, 2, 3)], return_logprobs=True, no_speech_token=939)
    with pytest.raises(ValueError):  # needs return_logprobs
        m.transcribe_submit(mel, prompt=(1, 2, 3), no_speech_token=939)
    with pytest.raises(ValueError):
        m.transcribe_batch(mel, prompt=(1, 2, 3), return_logprobs=True, no_speech_token=939, n_init=0)
    # accepted arguments reach the model check
    with pytest.raises(_lib.WhisperMiError):
        m.transcribe_batch(mel, prompt=(1, 2, 3), return_logprobs=True, no_speech_token=939)
    with pytest.raises(_lib.WhisperMiError):
        m.transcribe_long_form(feats, prompt=(1, 2, 3), eot=900, timestamps=ts, logprob_threshold=-1.0)
    assert _lib.no_speech_args(939, None, 3, 1000) == (939, 3)
    assert _lib.no_speech_args(939, 3, [4, 30], 1000) == (939, 3)
