"""CPU tests of the n-best scoring interface: the host-side argument table of _lib.nbest_args and its refusals through
every Python entry, the float64 reference of the ranking and posterior that the GPU tests use (rank_reference), and the header /
symbol-list bookkeeping.  Nothing here needs a GPU or the built library."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["wm_score_nbest", "wm_score_nbest_submit", "wm_score_nbest_wait", "wm_score_nbest_pcm", "wm_op_attention_cached_map",
               "wm_op_xattn_map", "wm_op_score_rank"]


def rank_reference(key, n_cand):
    """The documented ranking in float64 on the keys as given (fp32 values): per clip, candidate indices by key descending, equal keys
    lower index first; best = the first of them; posterior = exp(key - M) / sum exp(key - M) with M the clip's largest key.
    -> (order [R] int64, best [U] int64, posterior [R] float64)"""
    key = np.asarray(key, np.float64).reshape(-1)
    n_cand = np.asarray(n_cand, np.int64).reshape(-1)
    assert n_cand.min() >= 1 and n_cand.sum() == key.size
    order, best, post = np.zeros(key.size, np.int64), np.zeros(n_cand.size, np.int64), np.zeros(key.size, np.float64)
    r0 = 0
    for u, n in enumerate(n_cand.tolist()):
        k = key[r0:r0 + n]
        o = sorted(range(n), key=lambda c: (-k[c], c))
        order[r0:r0 + n] = o
        best[u] = o[0]
        e = np.exp(k - k.max())
        post[r0:r0 + n] = e / e.sum()
        r0 += n
    return order, best, post


def _args(cands, ctx=None, U=None, vocab=100, n_text_ctx=32, max_batch=8):
    from whisper_mojo_amd import _lib
    return _lib.nbest_args(cands, ctx, len(cands) if U is None else U, vocab, n_text_ctx, max_batch)


def test_nbest_args_builds_the_flat_table():
    cands = [[[1, 2, 3]], [[4, 5], [6, 7, 8, 9], [1, 1]], [[2, 3, 4, 5, 6], [9, 8]]]
    tab, lens, ctx, n_cand, utt_of, row0 = _args(cands)
    assert tab.dtype == np.int32 and tab.shape == (6, 5)
    flat = [r for c in cands for r in c]
    for r, ids in enumerate(flat):
        assert tab[r, :len(ids)].tolist() == ids and not tab[r, len(ids):].any()
    assert lens.tolist() == [3, 2, 4, 2, 5, 2]
    assert ctx.tolist() == [1] * 6
    assert n_cand.tolist() == [1, 3, 2] and n_cand.dtype == np.int32
    assert utt_of.tolist() == [0, 1, 1, 1, 2, 2] and utt_of.dtype == np.int32
    assert row0.tolist() == [0, 1, 4] and row0.dtype == np.int32


def test_nbest_args_context_len_forms():
    cands = [[[1, 2, 3], [4, 5, 6, 7]], [[1, 2, 3, 4, 5]]]
    assert _args(cands, 2)[2].tolist() == [2, 2, 2]
    assert _args(cands, [1, 3, 4])[2].tolist() == [1, 3, 4]
    assert _args(cands, [[2, 1], [3]])[2].tolist() == [2, 1, 3]
    for bad in ([1, 2], [[1], [2]], [[1, 2, 3], [1]]):
        with pytest.raises(ValueError):
            _args(cands, bad)


BAD = [
    ("no clip", dict(cands=[])),
    ("clip count", dict(cands=[[[1, 2]]], U=2)),
    ("empty clip", dict(cands=[[[1, 2]], []])),
    ("over max_batch", dict(cands=[[[1, 2]] * 5, [[1, 2]] * 4])),
    ("short row", dict(cands=[[[1, 2], [3]]])),
    ("long row", dict(cands=[[list(range(33))]])),
    ("id out of range", dict(cands=[[[1, 100]]])),
    ("negative id", dict(cands=[[[1, -1]]])),
    ("context 0", dict(cands=[[[1, 2, 3]]], ctx=0)),
    ("context = len", dict(cands=[[[1, 2, 3]]], ctx=3)),
]


@pytest.mark.parametrize("what,kw", BAD, ids=[b[0] for b in BAD])
def test_nbest_args_refuses(what, kw):
    with pytest.raises(ValueError):
        _args(**kw)


def _unloaded(max_batch=4):
    from whisper_mojo_amd import WhisperConfig
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.micro()
    return cfg, Whisper(cfg, max_batch=max_batch)


ENTRY_BAD = [
    [[[1, 2]], []],                      # a clip without candidates
    [[[1, 2]] * 3, [[1, 2]] * 2],        # R = 5 over max_batch = 4
    [[[1]], [[1, 2]]],                   # a row of one id
    [[[1, 10 ** 6]], [[1, 2]]],          # an id outside the vocabulary
    [[[1, 2]]],                          # one candidate list for two clips
]


@pytest.mark.parametrize("cands", ENTRY_BAD)
def test_entries_refuse_before_the_library(cands):
    """score_candidates, score_candidates_submit and score_audio_candidates raise ValueError on an UNLOADED model: the refusal comes
    before any library call (a loaded model is not needed, so nothing can have been launched)."""
    from whisper_mojo_amd import frontend
    cfg, m = _unloaded()
    mel = np.zeros((2, cfg.n_mels, cfg.n_frames), np.float32)
    with pytest.raises(ValueError):
        m.score_candidates(mel, cands)
    with pytest.raises(ValueError):
        m.score_candidates_submit(mel, cands, slot=1)
    with pytest.raises(ValueError):
        frontend.score_audio_candidates(m, [np.zeros(1600, np.float32)] * 2, cands)
    with pytest.raises(ValueError):
        m.score_candidates(mel, [[[1, 2, 3]], [[1, 2, 3]]], context_len=3)
    assert m._nbest_pending == {}


def test_reference_tie_order_and_posterior():
    key = np.asarray([-1.0, -0.5, -1.0, -0.5, -3.0,   -2.0,   -7.0, -7.0, -7.0], np.float32)
    # the clip split as the feature's own table builder gives it for 5, 1 and 3 candidates
    n_cand, _, row0 = _args([[[1, 2]] * 5, [[1, 2]], [[1, 2]] * 3], max_batch=9)[3:]
    assert row0.tolist() == [0, 5, 6]
    order, best, post = rank_reference(key, n_cand)
    assert order.tolist() == [1, 3, 0, 2, 4,   0,   0, 1, 2]  # equal keys: lower index first
    assert best.tolist() == [1, 0, 0]
    np.testing.assert_allclose(post[5:], [1.0, 1 / 3, 1 / 3, 1 / 3], rtol=1e-15)
    e = np.exp(np.asarray([-0.5, 0, -0.5, 0, -2.5]))
    np.testing.assert_allclose(post[:5], e / e.sum(), rtol=1e-15)
    for lo, hi in ((0, 5), (5, 6), (6, 9)):
        assert abs(post[lo:hi].sum() - 1) < 1e-15
    # spread keys: a posterior may underflow to exactly 0 in float64 only far beyond -700; at -200 it is tiny but positive
    _, _, p = rank_reference(np.asarray([0.0, -200.0], np.float32), [2])
    assert 0 < p[1] < 1e-80 and p[0] == 1.0


def test_header_and_symbol_list():
    from whisper_mojo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "whisper_mi.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", hdr), s
        assert _lib.SYMBOLS.count(s) == 1, s
    assert "WM_ABI_VERSION 5" in hdr or re.search(r"WM_ABI_VERSION\s+5\b", hdr)
