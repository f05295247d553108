"""CPU tests of language detection: the rule restated in float64 on the fixture's raw logits, the new C-ABI names, the
host-side refusals and the tokenizer helper.  Fixtures: tests/golden/lang_detect_{micro,tiny}_hf.npz (tools/make_golden_lang.py)."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "whisper_mi.h")
NEW = ["wm_detect_language", "wm_transcribe_lang", "wm_transcribe_submit_lang", "wm_transcribe_wait_lang", "wm_op_lang_detect"]


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_float64_rule_reproduces_hf_ids_and_probabilities(name):
    """arg-max over the candidates (ties: the smaller id) and softmax with the maximum subtracted, terms added in list order"""
    z = np.load(os.path.join(GOLDEN, f"lang_detect_{name}_hf.npz"))
    assert int(z["generate_checked"]) == 1  # the tool's generate(language=None) run reproduced the stored language and ids
    ids = z["lang_ids"]
    langs = []
    for i in range(int(z["s_rows"])):
        s = z[f"s{i}_lang_logits"].astype(np.float64)
        best = min(int(t) for t, v in zip(ids, s) if v == s.max())
        assert best == int(z[f"s{i}_lang"]), i
        t = np.exp(s - s.max())
        S = 0.0
        for v in t:
            S += v
        np.testing.assert_allclose(t / S, z[f"s{i}_lang_probs"], rtol=0, atol=1e-6)
        srt = np.sort(s)
        assert srt[-1] - srt[-2] >= float(z["s_min_gap"]) >= 1e-2
        assert int(z[f"s{i}_prompt"][-len(z["init"]) + 1]) == best  # the stored prompt carries the detected language
        langs.append(best)
    assert len(set(langs)) >= 3


def test_new_symbols_are_declared_and_abi_is_5():
    from whisper_mojo_amd import _lib
    text = open(HEADER, encoding="utf-8").read()
    for name in NEW:
        assert name in _lib.SYMBOLS and f"int {name}(" in text, name
    assert _lib.ABI_VERSION == 5 and "#define WM_ABI_VERSION 5" in text
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        assert L.wm_abi_version() == 5
        for name in NEW:
            assert hasattr(L, name), name


def test_host_side_refusals_do_not_touch_the_library(monkeypatch):
    from whisper_mojo_amd import WhisperConfig, _lib
    from whisper_mojo_amd import whisper_tensor as wt
    from whisper_mojo_amd.whisper import Whisper
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    for bad in ([], list(range(129)), [3, 1000], [-1], [5, 9, 5]):
        with pytest.raises(ValueError):
            _lib.lang_args(bad, 1000)
    assert _lib.lang_args([9, 0, 999], 1000).tolist() == [9, 0, 999]
    cfg = WhisperConfig.micro()
    m = Whisper(cfg, max_batch=2)
    mel = np.zeros((2, cfg.n_mels, cfg.n_frames), np.float32)
    with pytest.raises(ValueError):
        m.detect_language(mel, [])
    with pytest.raises(ValueError):
        m.detect_language(mel, [5, 5])
    with pytest.raises(ValueError):
        m.detect_language(mel, [5], sot=cfg.vocab_size)
    with pytest.raises(ValueError):
        m.transcribe_batch(mel, prompt=(1, 2, 3), detect_language=[5, 6], return_token_timestamps=True)
    with pytest.raises(ValueError):
        m.transcribe_batch(mel, prompt=(1, 2, 3), detect_language=[5, 6], n_init=1)
    with pytest.raises(ValueError):
        m.transcribe_batch(mel, prompt=(1, 2, 3), detect_language=[5, 6], n_init=4)
    with pytest.raises(ValueError):
        m.transcribe_batch(mel, prompts=[[1, 2, 3], [7, 1, 2, 3]], detect_language=[5, 6])  # n_init required
    with pytest.raises(ValueError):
        m.transcribe_batch(mel, prompt=(1, 2, 3), detect_language=[5, 6], no_speech_token=939)  # needs return_logprobs
    with pytest.raises(ValueError):
        m.transcribe_submit(mel, prompt=(1, 2, 3), detect_language=[cfg.vocab_size])
    x = np.zeros((2, 128), np.float32)
    with pytest.raises(ValueError):
        wt.lang_detect(x, np.ones(128), np.zeros(128), np.zeros((100, 64), np.float32), [1])
    with pytest.raises(ValueError):
        wt.lang_detect(x[:, :64], np.ones(64), np.zeros(64), np.zeros((100, 64), np.float32), [1])
    with pytest.raises(ValueError):
        wt.lang_detect(x, np.ones(128), np.zeros(128), np.zeros((100, 128), np.float32), [1, 100])


def test_tokenizer_language_helper():
    from whisper_mojo_amd.tokenizer import Tokenizer, language_code, language_ids
    ids, codes, from_vocab = language_ids()
    assert ids == list(range(50259, 50358)) and not from_vocab
    assert codes[50259] == "en" and codes[50261] == "de" and codes[50357] == "su" and len(set(codes.values())) == 99
    assert language_code(50265) == "fr"
    with pytest.raises(KeyError):
        language_code(50358)
    vocab = {50258: "<|startoftranscript|>", 50259: "<|en|>", 50260: "<|zh|>", 50261: "<|haw|>", 50262: "<|translate|>"}
    ids, codes, from_vocab = language_ids(Tokenizer(vocab))
    assert from_vocab and ids == [50259, 50260, 50261] and codes[50261] == "haw"
    ids, codes, from_vocab = language_ids(Tokenizer({5: "a"}))  # a vocabulary without the entries: the published range, said so
    assert not from_vocab and ids[0] == 50259 and len(ids) == 99
