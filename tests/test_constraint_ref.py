"""CPU tests of the phrase-list constraint: a numpy restatement of its semantics, written from the rules below and — where
transformers is installed — checked bit for bit against HF's PrefixConstrainedLogitsProcessor with the function written from the same
rules; the host trie builder against a brute-force prefix scan; the Python layer's refusals through every entry point; the new C-ABI
names.  The GPU tests import the references from here.

One row, gen = the ids it generated behind its own prompt, fp32 scores z:
  1. walk = gen without the ids >= free_from;
  2. node = where walk leads from the root of the phrases' trie, dead if it leaves the trie;
  3. allowed = the ids that continue a phrase from the node, eot if a phrase ends there, every id >= free_from (dead: eot + free ids);
  4. z = -inf outside allowed — where bad_words_ids acts: behind sequence_bias, repetition_penalty, no_repeat_ngram_size."""
import os
import re

import numpy as np
import pytest

from test_seq_bias_ref import process as seq_process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Table:
    """phrases (id tuples), the pass's eot, free_from (None = no free ids) over a vocabulary"""

    def __init__(self, phrases, eot, free_from, vocab):
        self.phrases = [tuple(int(i) for i in p) for p in phrases]
        self.eot, self.vocab = int(eot), int(vocab)
        self.free_from = vocab if free_from is None or free_from < 0 or free_from > vocab else int(free_from)


def walk_of(gen, table):
    return tuple(int(t) for t in gen if t < table.free_from)


def allowed_ids(gen, table):
    """Rules 1-3 by brute force over the phrase list (no trie) -> (sorted allowed ids, match): match = the index of the phrase that
    equals the walk, -1 if none — what constraint_match reports for a row that emits eot here."""
    w = walk_of(gen, table)
    ok = set(range(table.free_from, table.vocab))
    match = -1
    alive = False
    for q, p in enumerate(table.phrases):
        if p[:len(w)] == w:
            alive = True
            if len(p) > len(w):
                ok.add(p[len(w)])
            else:
                match = q
    if match >= 0 or not alive:
        ok.add(table.eot)
    return sorted(ok), match


def constraint_ref(z, gen, table):
    """One row of scores under the constraint -> a float32 copy"""
    z = np.array(z, np.float32)
    keep = np.zeros(z.size, bool)
    keep[allowed_ids(gen, table)[0]] = True
    z[~keep] = -np.inf
    return z


def process_all(z, hist, n_prompt, table, sequence_bias=None, bad_words_ids=None, p=None, n=None):
    """sequence bias, penalty, n-gram, bad words (tests/test_seq_bias_ref.py), then the constraint: HF's order"""
    z = seq_process(z, hist, sequence_bias, bad_words_ids, p, n, table.eot)
    return constraint_ref(z, hist[n_prompt:], table)


def node_of(gen, table, trie=None):
    """the trie node the walk reaches, numbered as _lib.constraint_trie numbers them"""
    from whisper_mojo_amd import _lib
    off, eid, enx, term = trie if trie is not None else _lib.constraint_trie(table.phrases)
    v = 0
    for t in walk_of(gen, table):
        e = [k for k in range(off[v], off[v + 1]) if eid[k] == t]
        v = int(enx[e[0]]) if e else len(term) - 1
    return v


def mask_words(gen, table, banned=()):
    """the row's ban words: the complement of the allowed set below the vocabulary with `banned` (the n-gram bans) on top"""
    bits = np.zeros((table.vocab + 31) // 32 * 32, np.uint8)
    bits[:table.vocab] = 1
    bits[allowed_ids(gen, table)[0]] = 0
    bits[list(banned)] = 1
    return np.packbits(bits, bitorder="little").view(np.uint32)


# ---- the restatement itself -------------------------------------------------------------------------------------------------
def test_rules_on_a_small_list():
    t = Table([(1, 2), (1, 2, 3), (4,)], eot=9, free_from=10, vocab=12)
    assert allowed_ids([], t) == ([1, 4, 10, 11], -1)                      # the root
    assert allowed_ids([1], t) == ([2, 10, 11], -1)                        # an inner node, fan-out 1
    assert allowed_ids([10, 1, 11, 2], t) == ([3, 9, 10, 11], 0)           # a phrase ends here and another goes on; free ids in between
    assert allowed_ids([1, 2, 3], t) == ([9, 10, 11], 1)                   # a leaf
    assert allowed_ids([4, 4], t) == ([9, 10, 11], -1)                     # dead: eot and the free ids
    assert allowed_ids([4, 4, 1], t) == ([9, 10, 11], -1)                  # and it stays dead
    z = constraint_ref(np.arange(12, dtype=np.float32), [1], t)
    assert np.isneginf(z[[0, 1, 3, 4, 5, 6, 7, 8, 9]]).all() and z[[2, 10, 11]].tolist() == [2.0, 10.0, 11.0]
    assert allowed_ids([1], Table([(1, 2)], 9, None, 12))[0] == [2]        # no free ids at all


def _draw(r, V, free_from, eot):
    """a phrase list over a small alphabet with shared prefixes and phrases that are prefixes of others"""
    alpha = [a for a in r.permutation(min(free_from, V))[:6].tolist() if a != eot]
    had = set()
    for _ in range(int(r.integers(1, 9))):
        p = tuple(int(a) for a in r.choice(alpha, int(r.integers(1, 5))))
        had.add(p)
        if r.random() < 0.5 and len(p) > 1:
            had.add(p[:int(r.integers(1, len(p)))])
    return sorted(had, key=lambda p: r.random())


def test_reference_equals_hf_prefix_constrained():
    """Where transformers is installed: generate places PrefixConstrainedLogitsProcessor behind NoBadWordsLogitsProcessor, and
    constraint_ref equals it (num_beams = 1, the function written from rules 1-3) bit for bit on 200 random rows; chained behind
    tests/test_seq_bias_ref.py's reference it equals the five HF classes in generate's order."""
    tf = pytest.importorskip("transformers")
    import inspect
    import torch
    from transformers.generation.logits_process import (NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor, PrefixConstrainedLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor, SequenceBiasLogitsProcessor)
    src = inspect.getsource(tf.generation.utils.GenerationMixin._get_logits_processor)
    order = [src.index(c + "(") for c in ("SequenceBiasLogitsProcessor", "RepetitionPenaltyLogitsProcessor", "NoRepeatNGramLogitsProcessor",
                                          "NoBadWordsLogitsProcessor", "PrefixConstrainedLogitsProcessor")]
    assert order == sorted(order)
    r = np.random.default_rng(0)
    seen = dict(free=0, both=0, root=0, leaf=0, dead=0)
    for _ in range(200):
        V, eot, n_prompt = 40, 7, int(r.integers(1, 4))
        free_from = int(r.choice([30, 36, V]))
        table = Table(_draw(r, V, free_from, eot), eot, free_from, V)
        kind = r.integers(0, 4)
        p = table.phrases[int(r.integers(0, len(table.phrases)))]
        gen = list(p[:int(r.integers(0, len(p) + 1))]) if kind < 3 else r.integers(0, 30, int(r.integers(1, 5))).tolist()
        if kind == 2:
            gen = gen + [int(r.integers(0, 30))]
        for _k in range(int(r.integers(0, 3))):  # free ids anywhere in the history
            if free_from < V:
                gen.insert(int(r.integers(0, len(gen) + 1)), int(r.integers(free_from, V)))
        ok, match = allowed_ids(gen, table)
        w = walk_of(gen, table)
        alive = any(q[:len(w)] == w for q in table.phrases)
        seen["free"] += len(w) < len(gen)
        seen["both"] += match >= 0 and any(len(q) > len(w) and q[:len(w)] == w for q in table.phrases)
        seen["root"] += len(w) == 0
        seen["leaf"] += match >= 0 and not any(len(q) > len(w) and q[:len(w)] == w for q in table.phrases)
        seen["dead"] += not alive
        hist = r.integers(0, 6, n_prompt).tolist() + gen
        z = r.standard_normal(V).astype(np.float32)
        fn = lambda batch_id, sent: allowed_ids(sent.tolist()[n_prompt:], table)[0]  # noqa: E731
        ids, s = torch.tensor([hist]), torch.from_numpy(z.copy())[None]
        want = PrefixConstrainedLogitsProcessor(fn, num_beams=1)(ids, s)[0].numpy()
        np.testing.assert_array_equal(constraint_ref(z, gen, table), want)
        # behind the other four processors, in generate's order
        sb = {(int(hist[-1]), int(r.integers(0, V))): 1.5, (int(r.integers(0, V)),): -0.75}
        bad = [[int(r.integers(0, V))], [int(hist[-1]), int(r.integers(0, V))]]
        pen, n = float(r.choice([1.0, 1.3])), int(r.integers(0, 3))
        s = SequenceBiasLogitsProcessor(dict(sb))(ids, torch.from_numpy(z.copy())[None])
        s = RepetitionPenaltyLogitsProcessor(pen)(ids, s) if pen != 1.0 else s
        s = NoRepeatNGramLogitsProcessor(n)(ids, s) if n else s
        s = NoBadWordsLogitsProcessor(bad, eos_token_id=eot)(ids, s)
        s = PrefixConstrainedLogitsProcessor(fn, num_beams=1)(ids, s)
        np.testing.assert_array_equal(process_all(z, hist, n_prompt, table, sb, bad, pen, n), s[0].numpy())
    assert min(seen.values()) > 10, seen


# ---- the host trie builder -----------------------------------------------------------------------------------------------------
def _check_trie(phrases):
    from whisper_mojo_amd import _lib
    off, eid, enx, term = _lib.constraint_trie(phrases)
    n = len(term)
    assert off[0] == 0 and len(off) == n + 1 and off[-1] == len(eid) == len(enx)
    assert off[n] == off[n - 1] and term[n - 1] == -1          # the dead node: no edges, no phrase
    prefixes = {()}
    for p in phrases:
        prefixes |= {tuple(p[:k]) for k in range(1, len(p) + 1)}
    assert n == len(prefixes) + 1                                # one node per distinct prefix, and the dead node
    path = {0: ()}
    for v in range(n):
        e = eid[off[v]:off[v + 1]]
        assert (np.diff(e) > 0).all()                            # ascending, so distinct
        w = path.get(v)
        assert w is not None or v == n - 1
        if w is None:
            continue
        # brute force: the ids that continue a phrase from the prefix w, and the phrase that ends there
        assert e.tolist() == sorted({p[len(w)] for p in phrases if len(p) > len(w) and tuple(p[:len(w)]) == w})
        assert term[v] == next((q for q, p in enumerate(phrases) if tuple(p) == w), -1)
        for k in range(off[v], off[v + 1]):
            assert 0 < enx[k] < n - 1 and enx[k] not in path
            path[int(enx[k])] = w + (int(eid[k]),)
    assert len(path) == n - 1 and sorted(path.values()) == sorted(prefixes)
    return off, eid, enx, term


def test_trie_builder_against_a_prefix_scan():
    off, *_ = _check_trie([(5, 6, 7), (5, 6, 8), (5, 9), (5,), (1, 2, 3, 4), (1, 2)])   # shared prefixes, prefixes of others
    assert off[1] - off[0] == 2
    _check_trie([(3, 3, 3, 3, 3, 3)])                                                      # fan-out 1 all the way
    off, *_ = _check_trie([(i, i % 3) for i in range(700)] + [(5,), (699, 0, 1)])          # a root fan-out above 600
    assert off[1] - off[0] == 700
    r = np.random.default_rng(1)
    for _ in range(20):
        _check_trie(_draw(r, 40, 40, 7))
    # node numbering: in the order the phrases first reach the nodes
    off, eid, enx, term = _check_trie([(9, 1), (2,), (9, 0)])
    assert eid.tolist() == [2, 9, 0, 1] and enx.tolist() == [3, 1, 4, 2] and term.tolist() == [-1, -1, 0, 1, 2, -1]


# ---- refusals -------------------------------------------------------------------------------------------------------------------
VOCAB, EOT_ID = 51865, 50257  # tiny's vocabulary, the calls' default eot


@pytest.mark.parametrize("kw,name", [
    ({"constraint": []}, "empty list"),
    ({"constraint": [[1, 2], []]}, "1..64 ids"),
    ({"constraint": [[1, VOCAB]]}, "vocabulary"),
    ({"constraint": [[-1]]}, "vocabulary"),
    ({"constraint": [[1.5]]}, "vocabulary"),
    ({"constraint": [[1, EOT_ID]]}, "eot"),
    ({"constraint": [[1, 600]], "free_from": 600}, "free id"),
    ({"constraint": [[1, 2], [3], [1, 2]]}, "twice"),
    ({"constraint": [[i] for i in range(4097)]}, "4096"),
    ({"constraint": [list(range(65))]}, "1..64 ids"),
    ({"constraint": [[1 + q] + [q + k for k in range(63)] for q in range(1100)]}, "65536"),
    ({"free_from": 5}, "free_from without constraint"),
])
def test_python_refusals_through_every_entry_point(kw, name):
    """Refused on the host, before a model is needed, naming the argument — by every entry point that takes the option."""
    from whisper_mojo_amd import WhisperConfig, frontend
    from whisper_mojo_amd.whisper import Whisper
    model = Whisper(WhisperConfig.tiny(), max_batch=1)  # never loaded: the checks come first
    cfg = model.config
    assert cfg.vocab_size == VOCAB
    mel = np.zeros((1, cfg.n_mels, 2 * cfg.n_audio_ctx), np.float32)
    pcm = [np.zeros(1600, np.float32)]
    for call in (lambda: model.transcribe_batch(mel, **kw), lambda: model.transcribe_submit(mel, **kw),
                 lambda: frontend.transcribe_audio(model, pcm, **kw)):
        with pytest.raises(ValueError, match=name):
            call()


def test_timestamp_ids_are_free_by_default_and_refused_inside_a_phrase():
    from whisper_mojo_amd import _lib
    ts = (50364, 50363, 50)
    with pytest.raises(ValueError, match="free id"):
        _lib.constraint_args([[1, 50364]], None, VOCAB, EOT_ID, ts)
    assert _lib.constraint_args([[1, 50364]], None, VOCAB, EOT_ID, None)[1][3] == VOCAB  # rules off: no free ids
    key, a = _lib.constraint_args([(1, 2), [3]], None, VOCAB, EOT_ID, ts)
    assert a[0].tolist() == [1, 2, 3] and a[1].tolist() == [0, 2, 3] and a[2] == 2 and a[3] == 50364
    assert key == _lib.constraint_args([[1, 2], (3,)], 50364, VOCAB, EOT_ID)[0]
    assert key != _lib.constraint_args([[3], [1, 2]], 50364, VOCAB, EOT_ID)[0]   # the order names the phrases: part of the table
    assert key != _lib.constraint_args([[1, 2], [3]], 50000, VOCAB, EOT_ID)[0]
    assert _lib.constraint_args(None, None, VOCAB, EOT_ID, ts) is None
    assert len(_lib.constraint_args([[i] for i in range(4096)], None, VOCAB, EOT_ID)[1][0]) == 4096


def test_long_form_and_chunked_refuse_the_option():
    from whisper_mojo_amd import WhisperConfig, frontend
    from whisper_mojo_amd.whisper import Whisper
    model = Whisper(WhisperConfig.tiny(), max_batch=1)
    cfg = model.config
    mel = np.zeros((1, cfg.n_mels, 2 * cfg.n_audio_ctx), np.float32)
    pcm = [np.zeros(1600, np.float32)]
    for call in (lambda: model.transcribe_long_form(mel, constraint=[[1, 2]]), lambda: model.transcribe_chunked(pcm, constraint=[[1, 2]]),
                 lambda: frontend.transcribe_audio_long_form(model, pcm, constraint=[[1, 2]]),
                 lambda: frontend.transcribe_audio_chunked(model, pcm, constraint=[[1, 2]]),
                 lambda: model.transcribe_long_form(mel, free_from=3)):
        with pytest.raises(ValueError, match="constraint"):
            call()


def test_header_and_symbols_agree():
    from whisper_mojo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "whisper_mi.h")).read()
    for name in ("wm_set_constraint", "wm_transcribe_constraint_match", "wm_op_constraint_states"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _lib.SYMBOLS, name
    assert "#define WM_ABI_VERSION 5" in hdr  # existing signatures and structs are untouched
    hpp = open(os.path.join(ROOT, "include", "whisper_mi.hpp")).read()
    assert "set_constraint" in hpp and "constraint_match" in hpp and "constraint_trie" in hpp
