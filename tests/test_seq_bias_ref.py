"""CPU tests of sequence_bias / bad_words_ids: a numpy reference of HF's SequenceBiasLogitsProcessor and
NoBadWordsLogitsProcessor in generate's order around the repetition processors, written from their definitions and — where
transformers is installed — checked against the HF classes bit for bit; the reference of the device's per-row hit state (slots and
bits); the Python layer's argument checks; the new C-ABI names.  The GPU tests import the references from here.

One row, history hist, fp32 logits z:
  1. bias = 0; every length-1 sequence sets bias[id]; in the dictionary's order every s with 2 <= len(s) <= len(hist) and
     hist[-(len(s) - 1):] == s[:-1] adds its bias to bias[s[-1]]; z = z + bias (fp32)
  2. repetition_penalty, no_repeat_ngram_size (tests/test_repeat_ref.py)
  3. bad_words_ids: the same with bias -inf, [eot] dropped first."""
import os
import re

import numpy as np
import pytest

from test_repeat_ref import bit_set, process as repeat_process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _items(sequence_bias):
    if not sequence_bias:
        return []
    it = sequence_bias.items() if isinstance(sequence_bias, dict) else [(s[0], s[1]) for s in sequence_bias]
    return [(tuple(int(i) for i in s), np.float32(b)) for s, b in it]


def matches(s, hist):
    """HF's test for one sequence of two ids or more: len(s) <= len(hist), not len(s) - 1 <= len(hist)"""
    return len(s) <= len(hist) and list(hist[len(hist) - (len(s) - 1):]) == list(s[:-1])


def bias_vector(items, hist, vocab):
    bias = np.zeros(vocab, np.float32)
    for s, b in items:
        if len(s) == 1:
            bias[s[0]] = b
    for s, b in items:
        if len(s) >= 2 and matches(s, hist):
            bias[s[-1]] = np.float32(bias[s[-1]] + b)
    return bias


def process(z, hist, sequence_bias=None, bad_words_ids=None, p=None, n=None, eot=None):
    """One row of logits through the four processors in generate's order -> a float32 copy."""
    z = np.array(z, np.float32)
    items = _items(sequence_bias)
    if items:
        z = (z + bias_vector(items, hist, z.size)).astype(np.float32)
    z = repeat_process(z, hist, p, n)
    bad = [(tuple(s), np.float32(-np.inf)) for s in (bad_words_ids or []) if list(s) != [eot]]
    if bad:
        z = (z + bias_vector(bad, hist, z.size)).astype(np.float32)
    return z


def hit_state(hist, sequence_bias, bad_words_ids, vocab, eot=-1):
    """The device's state of one row for its next step: (slot_id ascending, bias [S] float32, flags [S], hit words).  A slot = one
    distinct last id; on (flag 1) when a sequence of it matches, a length-1 one always; ban: flag 2; bias: HF's fp32 sum."""
    items = _items(sequence_bias)
    bad = [tuple(int(i) for i in s) for s in (bad_words_ids or [])]
    slot_id = sorted({s[-1] for s, _ in items} | {s[-1] for s in bad})
    bias, flags = np.zeros(len(slot_id), np.float32), np.zeros(len(slot_id), np.int32)
    for k, t in enumerate(slot_id):
        mine = [(s, b) for s, b in items if s[-1] == t]
        for s, b in [x for x in mine if len(x[0]) == 1] + [x for x in mine if len(x[0]) > 1]:
            if len(s) == 1 or matches(s, hist):
                bias[k] = np.float32(bias[k] + b)
                flags[k] |= 1
        for s in bad:
            if s[-1] == t and ((len(s) == 1 and s[0] != eot) or (len(s) > 1 and matches(s, hist))):
                flags[k] |= 3
    return np.asarray(slot_id, np.int32), bias, flags, bit_set([t for k, t in enumerate(slot_id) if flags[k] & 1], vocab)


def test_length_1_always_and_longer_on_a_matching_tail():
    z = np.zeros(10, np.float32)
    sb = {(3,): 2.0, (1, 2, 4): 1.5, (2, 4): 0.25, (9, 5): -1.0}
    out = process(z, [7, 1, 2], sb)
    assert out[3] == 2.0 and out[4] == 1.5 + 0.25 and out[5] == 0.0
    out = process(z, [7, 1, 9], sb)
    assert out[3] == 2.0 and out[4] == 0.0 and out[5] == -1.0


def test_hfs_length_test_is_len_s_not_len_s_minus_1():
    z = np.zeros(10, np.float32)
    assert process(z, [1, 2], {(1, 2, 4): 1.0})[4] == 0.0      # len(s) = 3 > len(hist) = 2 although the prefix (1, 2) is the whole history
    assert process(z, [0, 1, 2], {(1, 2, 4): 1.0})[4] == 1.0   # len(s) = len(hist)
    assert process(z, [1], {(1, 4): 1.0})[4] == 0.0 and process(z, [0, 1], {(1, 4): 1.0})[4] == 1.0


def test_sum_order_is_the_dictionarys():
    a, b, c = np.float32(1e8), np.float32(-1e8), np.float32(1.0)
    z = np.zeros(4, np.float32)
    assert process(z, [5, 0, 1], {(1, 2): a, (0, 1, 2): b, (2,): c})[2] == np.float32(np.float32(c + a) + b) == 0.0  # the length-1 value first
    assert process(z, [9, 3, 0, 1], {(1, 2): a, (0, 1, 2): c, (3, 0, 1, 2): b})[2] == np.float32(np.float32(a + c) + b) == 0.0
    assert process(z, [9, 3, 0, 1], {(1, 2): a, (3, 0, 1, 2): b, (0, 1, 2): c})[2] == 1.0


def test_bad_words_after_the_repetition_processors_and_eot_dropped():
    z = np.arange(8, dtype=np.float32) - 3
    out = process(z, [5, 6], {(6, 7): 3.0}, [[6, 7], [2], [4]], p=2.0, n=None, eot=4)
    assert out[7] == -np.inf and out[2] == -np.inf and out[4] == z[4]
    assert out[5] == np.float32(2.0) / 2 and out[6] == np.float32(3.0) / 2
    st = hit_state([5, 6], {(6, 7): 3.0}, [[6, 7], [2], [4]], 8, eot=4)
    assert st[0].tolist() == [2, 4, 7] and st[2].tolist() == [3, 0, 3] and st[1].tolist() == [0.0, 0.0, 3.0]


@pytest.mark.parametrize("kw,name", [
    ({"sequence_bias": {(999999,): 1.0}}, "sequence_bias"),
    ({"sequence_bias": {(-1, 2): 1.0}}, "sequence_bias"),
    ({"sequence_bias": {(): 1.0}}, "sequence_bias"),
    ({"sequence_bias": {tuple(range(33)): 1.0}}, "sequence_bias"),
    ({"sequence_bias": [[[1, 2], 1.0], [[1, 2], 2.0]]}, "sequence_bias"),
    ({"sequence_bias": {(1,): float("inf")}}, "sequence_bias"),
    ({"sequence_bias": {(1,): float("nan")}}, "sequence_bias"),
    ({"bad_words_ids": [[1, 2], [1, 2]]}, "bad_words_ids"),
    ({"bad_words_ids": [[]]}, "bad_words_ids"),
    ({"bad_words_ids": [[1.5]]}, "bad_words_ids"),
    ({"bad_words_ids": [list(range(33))]}, "bad_words_ids"),
    ({"sequence_bias": {(i,): 1.0 for i in range(600)}, "bad_words_ids": [[i] for i in range(425)]}, "1024"),
])
def test_python_argument_checks(kw, name):
    """Refused on the host, before a model is needed, naming the argument — by every entry point that takes the options."""
    from whisper_mojo_amd import WhisperConfig, frontend
    from whisper_mojo_amd.whisper import Whisper
    model = Whisper(WhisperConfig.tiny(), max_batch=1)  # never loaded: the checks come first
    cfg = model.config
    mel = np.zeros((1, cfg.n_mels, 2 * cfg.n_audio_ctx), np.float32)
    pcm = [np.zeros(1600, np.float32)]
    for call in (lambda: model.transcribe_batch(mel, **kw), lambda: model.transcribe_submit(mel, **kw),
                 lambda: model.transcribe_long_form(mel, **kw), lambda: model.transcribe_chunked(pcm, **kw),
                 lambda: frontend.transcribe_audio(model, pcm, **kw), lambda: frontend.transcribe_audio_long_form(model, pcm, **kw),
                 lambda: frontend.transcribe_audio_chunked(model, pcm, **kw)):
        with pytest.raises(ValueError, match=name):
            call()


def test_python_argument_packing():
    from whisper_mojo_amd import _lib
    assert _lib.seq_bias_args(None, None, 100) is None and _lib.seq_bias_args({}, [], 100) is None
    key, a = _lib.seq_bias_args({(1, 2): 1.5, (3,): float("-inf")}, [[4, 5, 6]], 100)
    assert a[0].tolist() == [1, 2, 3] and a[1].tolist() == [0, 2, 3] and a[2].tolist() == [1.5, -np.inf] and a[3] == 2
    assert a[4].tolist() == [4, 5, 6] and a[5].tolist() == [0, 3] and a[6] == 1
    assert key == _lib.seq_bias_args([[[1, 2], 1.5], [[3], float("-inf")]], [(4, 5, 6)], 100)[0]
    assert key != _lib.seq_bias_args({(3,): float("-inf"), (1, 2): 1.5}, [[4, 5, 6]], 100)[0]  # the order is part of the table
    assert _lib.seq_bias_args({(i,): 1.0 for i in range(1024)}, None, 2000)[1][3] == 1024


def test_header_and_symbols_agree():
    from whisper_mojo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "whisper_mi.h")).read()
    for name in ("wm_set_sequence_bias", "wm_op_logits_seq_bias", "wm_op_seq_bias_hits"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _lib.SYMBOLS, name
    assert "#define WM_ABI_VERSION 5" in hdr  # existing signatures and structs are untouched
    assert "set_sequence_bias" in open(os.path.join(ROOT, "include", "whisper_mi.hpp")).read()


def _draw(r, V, hist, eot):
    """A table that exercises: shared last ids, sequences of len(hist) and len(hist) + 1, an [eot] bad word, -inf biases"""
    L = len(hist)
    sb = {}
    last = int(r.integers(0, V))
    for m in (1, 2, 3, L, L + 1):
        if m < 1 or m > 32:
            continue
        s = tuple(hist[L - (m - 1):]) + (last,) if m - 1 <= L and r.random() < 0.8 else tuple(r.integers(0, 6, m - 1).tolist()) + (last,)
        sb[s] = float(r.choice([-np.inf, 1e8, -1e8, 0.37, 2.5, -3.25]))
    for _ in range(int(r.integers(0, 5))):
        m = int(r.integers(1, 5))
        sb[tuple(r.integers(0, 6, m - 1).tolist()) + (int(r.integers(0, V)),)] = float(r.standard_normal() * 4)
    bad = {(eot,)}
    for _ in range(int(r.integers(0, 4))):
        m = int(r.integers(1, 4))
        bad.add(tuple(r.integers(0, 6, m - 1).tolist()) + (int(r.integers(0, V)),))
    if L >= 2:
        bad.add(tuple(hist[-2:]) + (int(r.integers(0, V)),))
    return sb, [list(s) for s in sorted(bad)]


def test_reference_equals_hf_processors():
    """Where transformers is installed: generate appends sequence bias, penalty, n-gram, bad words in this order, and process()
    equals the four HF classes applied in it, bit for bit, on 200 random rows."""
    tf = pytest.importorskip("transformers")
    import inspect
    import torch
    from transformers.generation.logits_process import (NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor, SequenceBiasLogitsProcessor)
    src = inspect.getsource(tf.generation.utils.GenerationMixin._get_logits_processor)
    order = [src.index(c + "(") for c in ("SequenceBiasLogitsProcessor", "RepetitionPenaltyLogitsProcessor", "NoRepeatNGramLogitsProcessor",
                                          "NoBadWordsLogitsProcessor")]
    assert order == sorted(order)
    r = np.random.default_rng(0)
    seen_shared = seen_eq = seen_rp = 0
    for _ in range(200):
        V, L, n, eot = 50, int(r.integers(1, 12)), int(r.integers(0, 5)), 7
        p = float(r.choice([1.0, 0.7, 1.3, 2.0]))
        hist = r.integers(0, 6, L).tolist()
        z = r.standard_normal(V).astype(np.float32)
        sb, bad = _draw(r, V, hist, eot)
        lasts = [s[-1] for s in sb if len(s) == 1 or matches(s, hist)]
        seen_shared += len(lasts) != len(set(lasts))
        seen_eq += any(len(s) == L and L >= 2 and matches(s, hist) for s in sb)
        seen_rp += p != 1.0 and n > 0 and len(lasts) > 0
        assert [eot] in bad
        ids, s = torch.tensor([hist]), torch.from_numpy(z.copy())[None]
        s = SequenceBiasLogitsProcessor(dict(sb))(ids, s)
        s = RepetitionPenaltyLogitsProcessor(p)(ids, s) if p != 1.0 else s
        s = NoRepeatNGramLogitsProcessor(n)(ids, s) if n else s
        s = NoBadWordsLogitsProcessor(bad, eos_token_id=eot)(ids, s)
        want = s[0].numpy()
        got = process(z, hist, sb, bad, p, n, eot)
        np.testing.assert_array_equal(got, want)
        # the device's hit state gives the same row: bias where a slot is on, -inf under a ban
        sid, bias, flags, _ = hit_state(hist, sb, bad, V, eot)
        zz = z.copy()
        on = (flags & 1) != 0
        zz[sid[on]] = zz[sid[on]] + bias[on]
        zz = repeat_process(zz, hist, p, n)
        zz[sid[(flags & 2) != 0]] = -np.inf
        np.testing.assert_array_equal(zz, want)
    assert seen_shared > 20 and seen_eq > 20 and seen_rp > 20
