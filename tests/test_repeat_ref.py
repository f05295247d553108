"""CPU tests of the repetition processors: a numpy reference of HF's RepetitionPenaltyLogitsProcessor and
NoRepeatNGramLogitsProcessor written from their definitions, checked on hand-made cases; the Python layer's argument checks; the new
C-ABI names in the header and in _lib.SYMBOLS.  The GPU tests (tests/test_gpu_repeat_op.py, tests/test_gpu_repeat.py) import the
reference from here.

Definitions, for one row with history hist (prompt + generated ids) and fp32 logits z, in this order:
  1. penalty p: every id t that occurs in hist, once: z[t] = z[t] * p if z[t] < 0 else z[t] / p   (fp32 arithmetic)
  2. n-gram size n >= 1: if len(hist) + 1 >= n, every i with i + n - 1 < len(hist) and hist[i : i + n - 1] == hist[len(hist) - (n - 1):]
     bans hist[i + n - 1] (z = -inf); n = 1 bans every id of hist."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def banned_ids(hist, n):
    """The ids NoRepeatNGramLogitsProcessor(n) bans for the next step, as a sorted list."""
    hist = [int(t) for t in hist]
    L = len(hist)
    if not n or L + 1 < n:
        return []
    suffix = hist[L - (n - 1):] if n > 1 else []
    return sorted({hist[i + n - 1] for i in range(L - n + 1) if hist[i:i + n - 1] == suffix})


def process(z, hist, p=None, n=None):
    """One row of logits through both processors -> a float32 copy."""
    z = np.array(z, np.float32)
    if p is not None and p != 1.0:
        ids = np.unique(np.asarray(list(hist), np.int64))
        v = z[ids]
        z[ids] = np.where(v < 0, v * np.float32(p), v / np.float32(p)).astype(np.float32)
    for t in banned_ids(hist, n):
        z[t] = -np.inf
    return z


def bit_set(ids, vocab):
    """ids -> the kernels' bit set: id t is bit (t & 31) of word t >> 5"""
    w = np.zeros((vocab + 31) // 32, np.uint32)
    for t in ids:
        w[int(t) >> 5] |= np.uint32(1) << np.uint32(int(t) & 31)
    return w


def set_ids(words):
    w = np.ascontiguousarray(words, "<u4")
    return np.flatnonzero(np.unpackbits(w.view(np.uint8), bitorder="little")).tolist()


# history with two occurrences of the suffix (7, 8): positions 1-2 and 5-6 (the suffix itself); 8 occurs three times
HIST = [5, 7, 8, 9, 8, 7, 8]


def test_ngram_1_bans_every_id_of_the_history():
    assert banned_ids(HIST, 1) == [5, 7, 8, 9]
    assert banned_ids([], 1) == []


def test_ngram_2_bans_what_followed_the_last_id():
    # the last id 8 occurred at 2 and 4 (and 6, the suffix itself: nothing follows): followed by 9 and 7
    assert banned_ids(HIST, 2) == [7, 9]


def test_ngram_3_bans_what_followed_the_last_two_ids():
    # (7, 8) at positions 1-2 is followed by 9; the occurrence at 5-6 is the suffix
    assert banned_ids(HIST, 3) == [9]
    # two earlier occurrences of the suffix with different followers
    assert banned_ids([1, 2, 3, 1, 2, 4, 1, 2], 3) == [3, 4]


def test_history_shorter_than_the_ngram():
    assert banned_ids([4], 3) == []       # len + 1 = 2 < 3
    assert banned_ids([4, 4], 3) == []    # len + 1 = 3 >= 3 but no complete trigram yet
    assert banned_ids([4, 4, 4], 3) == [4]
    assert banned_ids([4], 2) == []       # one id: no bigram yet
    assert banned_ids([4, 4], 2) == [4]
    assert banned_ids(HIST, 0) == [] and banned_ids(HIST, None) == []


def test_penalty_signs_and_once_per_id():
    z = np.array([2.0, -2.0, 0.0, 3.0, -1.0, 0.5, 6.5, -6.5, 1.0, 4.0], np.float32)
    hist = [0, 1, 2, 8, 8, 8, 7]  # id 8 three times: penalised once
    out = process(z, hist, p=1.3)
    f = np.float32
    assert out[0] == f(2.0) / f(1.3) and out[1] == f(-2.0) * f(1.3) and out[2] == 0.0
    assert out[8] == f(1.0) / f(1.3)  # not / 1.3³
    assert out[7] == f(-6.5) * f(1.3)
    np.testing.assert_array_equal(out[[3, 4, 5, 6, 9]], z[[3, 4, 5, 6, 9]])
    np.testing.assert_array_equal(process(z, hist, p=1.0), z)
    np.testing.assert_array_equal(process(z, hist, p=None, n=None), z)


def test_penalty_then_ban():
    z = np.arange(10, dtype=np.float32) - 4
    out = process(z, HIST, p=2.0, n=2)
    assert out[7] == -np.inf and out[9] == -np.inf          # banned after the penalty
    assert out[8] == np.float32(4.0) / 2 and out[5] == np.float32(1.0) / 2
    assert out[0] == z[0]


def test_bit_sets_round_trip():
    ids = [0, 31, 32, 63, 999]
    w = bit_set(ids, 1000)
    assert w.size == 32 and set_ids(w) == ids
    assert bit_set([51864], 51865).size == 1621  # 51 865 = 32·1620 + 25: the last word is partial


@pytest.mark.parametrize("kw,name", [
    ({"repetition_penalty": 0.0}, "repetition_penalty"),
    ({"repetition_penalty": -1.5}, "repetition_penalty"),
    ({"repetition_penalty": float("nan")}, "repetition_penalty"),
    ({"no_repeat_ngram_size": -1}, "no_repeat_ngram_size"),
    ({"no_repeat_ngram_size": 65}, "no_repeat_ngram_size"),
    ({"no_repeat_ngram_size": 2.5}, "no_repeat_ngram_size"),
])
def test_python_argument_checks(kw, name):
    """Refused on the host, before a model is needed, naming the argument — by every entry point that takes the options."""
    from whisper_mojo_amd import WhisperConfig, frontend
    from whisper_mojo_amd.whisper import Whisper
    model = Whisper(WhisperConfig.micro(), max_batch=1)  # never loaded: the checks come first
    cfg = model.config
    mel = np.zeros((1, cfg.n_mels, 2 * cfg.n_audio_ctx), np.float32)
    for call in (lambda: model.transcribe_batch(mel, **kw), lambda: model.transcribe_submit(mel, **kw),
                 lambda: model.transcribe_long_form(mel, **kw),
                 lambda: frontend.transcribe_audio(model, [np.zeros(1600, np.float32)], **kw),
                 lambda: frontend.transcribe_audio_long_form(model, [np.zeros(1600, np.float32)], **kw)):
        with pytest.raises(ValueError, match=name):
            call()


def test_python_argument_defaults():
    from whisper_mojo_amd import _lib
    assert _lib.repeat_args(None, None) == (1.0, 0)
    assert _lib.repeat_args(1.3, 3) == (1.3, 3)
    assert _lib.repeat_args(1, 64) == (1.0, 64)


def test_header_and_symbols_agree():
    from whisper_mojo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "whisper_mi.h")).read()
    for name in ("wm_set_repeat_options", "wm_op_logits_processed", "wm_op_repeat_sets"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _lib.SYMBOLS, name
    assert "#define WM_ABI_VERSION 5" in hdr  # existing signatures and structs are untouched


def test_reference_equals_hf_processors():
    """Where transformers is installed: generate builds the penalty before the n-gram processor, and process() equals the two HF
    classes applied in that order, bit for bit, on random rows."""
    tf = pytest.importorskip("transformers")
    import inspect
    import torch
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor
    src = inspect.getsource(tf.generation.utils.GenerationMixin._get_logits_processor)
    assert src.index("RepetitionPenaltyLogitsProcessor(") < src.index("NoRepeatNGramLogitsProcessor(")
    r = np.random.default_rng(0)
    for _ in range(200):
        V, L, n = 50, int(r.integers(1, 30)), int(r.integers(1, 6))
        p = float(r.choice([0.7, 1.3, 2.0]))
        hist = r.integers(0, 6, L).tolist()
        z = r.standard_normal(V).astype(np.float32)
        ids, s = torch.tensor([hist]), torch.from_numpy(z.copy())[None]
        s = NoRepeatNGramLogitsProcessor(n)(ids, RepetitionPenaltyLogitsProcessor(p)(ids, s))
        np.testing.assert_array_equal(s[0].numpy(), process(z, hist, p, n))
