"""Op-level tests (-m gpu) of the timestamp rules' state machine: wm_op_ts_states runs the pass's real init launch and then
one argmax launch per step that is handed the row's next id as its only candidate, so the kernel's own history update (pen_ts, last_ts,
n_gen, t_last, ts_next_ranges) runs on histories of our choosing.  At every prefix of every row the id set the returned ranges admit
equals the numpy restatement of HF's rules 1-4 in tests/test_ts_states_ref.py (itself checked against the oracle and HF's own table).
Everything is integers: no tolerance."""
import numpy as np
import pytest

from test_gpu_decode_ops import DT_BF16, DT_F32, _decoder_like, _ts_decision, hip  # noqa: F401
from test_ts_states_ref import (ENUM_DEPTH, ENUM_ROWS, OFF_POLICY, SMALL, admissible, enumerate_histories, history_fields, named_cases,
                                ragged_prompts, table_rows)

pytestmark = pytest.mark.gpu

SHARED_PROMPT = [1, 2, 3]
WM_E_ARG = -1


def _replay(histories, vocab, tb, eos, max_initial, row_prompts):
    from whisper_mojo_amd import whisper_tensor as wt
    B = len(histories)
    prompts = ragged_prompts(B, min(vocab, tb)) if row_prompts else [SHARED_PROMPT] * B
    steps = max(len(h) for h in histories)
    tok, plen, nids = table_rows(prompts, histories)
    return wt.ts_states(tok, plen, nids, vocab, tb, eos, max_initial, steps, row_prompts), tok, plen, nids, steps


def _check(r, histories, tok, plen, nids, steps, vocab, tb, eos, max_initial, row_prompts):
    """Every prefix of every row: ranges as sets against the reference, the history fields, the picks; then the final buffers."""
    B = len(histories)
    st = r["states"]
    ids = np.arange(vocab)
    got = ((ids >= st[..., 4:5]) & (ids < st[..., 5:6])) | ((ids >= st[..., 6:7]) & (ids < st[..., 7:8]))  # [steps + 1, B, vocab]
    assert (st[..., 4:] >= 0).all() and (st[..., 4:] <= vocab).all()
    cache = {}
    for b, h in enumerate(histories):
        for s in range(len(h) + 1):
            p = tuple(h[:s])
            if p not in cache:
                cache[p] = (admissible(p, vocab, tb, eos, max_initial), history_fields(p, tb))
            ok, fields = cache[p]
            assert np.array_equal(got[s, b], ok), (b, p, st[s, b].tolist(), np.flatnonzero(ok).tolist())
            assert tuple(st[s, b, :4]) == fields, (b, p, st[s, b].tolist(), fields)
            if s:
                assert r["picks"][s - 1, b] == h[s - 1], (b, p)
    want_tok = np.zeros_like(tok)
    for b in range(B):
        want_tok[b, :nids[b]] = tok[b, :nids[b]]
    np.testing.assert_array_equal(r["out_tokens"], want_tok)  # grew by exactly the forced ids, nothing behind a row's end
    np.testing.assert_array_equal(r["n_tokens"], nids)
    Lmax = int(plen.max())
    np.testing.assert_array_equal(r["ctl"], [Lmax + steps, 0, 0, 0])
    np.testing.assert_array_equal(r["pos"], (plen if row_prompts else Lmax) + steps)
    if row_prompts:
        np.testing.assert_array_equal(r["key_lo"], Lmax - plen)
        for b in range(B):
            pad = Lmax - plen[b]
            assert r["tok_rows"][:, b].tolist() == [tok[b, 0]] * pad + tok[b, :plen[b]].tolist()
            assert r["pos_rows"][:, b].tolist() == [0] * pad + list(range(plen[b]))


@pytest.mark.parametrize("row_prompts", [False, True])
@pytest.mark.parametrize("eos", [SMALL["eos"], SMALL["tb"]])
@pytest.mark.parametrize("max_initial", [None, 0, 1, 3, 50])
def test_exhaustive_small_vocabulary(hip, max_initial, eos, row_prompts):
    """vocab 12 (text 0-4, specials 5-7, timestamps 8-11): every history of depth 4 in which each id was admissible at its step — 2656
    rows with eos 5 and no max_initial (depth 3 has 304, depth 5 has 23136; the other settings walk the same depth: 752 .. 2656
    rows) — plus the off-policy rows no admissible walk reaches (two timestamps as the first two ids: after the first generated
    timestamp the rules refuse every timestamp, so such a history can only be forced), as one replay.  max_initial 3 meets the clamp
    (tb + 3 + 1 = vocab), 50 passes it; eos = timestamp_begin is what wm_op_logits hard-codes; both init forms, ragged prompts of
    1 .. 5 ids in the rows form."""
    V, tb = SMALL["vocab"], SMALL["tb"]
    leaves = enumerate_histories(V, tb, eos, max_initial, ENUM_DEPTH)
    if max_initial is None and eos == SMALL["eos"]:
        assert len(leaves) == ENUM_ROWS
    assert 700 <= len(leaves) <= 4096
    hist = leaves + OFF_POLICY
    found = named_cases(hist, V, tb, eos, max_initial)
    assert all(found.values()), found
    r, tok, plen, nids, steps = _replay(hist, V, tb, eos, max_initial, row_prompts)
    assert steps == ENUM_DEPTH and (not row_prompts or sorted(set(plen.tolist())) == [1, 2, 3, 4, 5])
    _check(r, hist, tok, plen, nids, steps, V, tb, eos, max_initial, row_prompts)


TINY = dict(vocab=51865, tb=50364, eos=50257)


def _tiny_rows():
    tb, last, eos = TINY["tb"], TINY["vocab"] - 1, TINY["eos"]
    rows = [(last,), (last, 7), (last, last), (last, last, 9), (tb, 7, last), (tb, 7, last, last, 9), (tb + 50, eos), (tb,), (tb, 5), (tb, 5, tb),
            (tb, 5, tb, tb), (tb, 5, tb, tb, 0), (tb, tb), (tb, tb, tb - 1), (tb + 50, tb - 1, tb + 50, tb + 51), (tb + 1, eos - 1, eos, eos + 1, tb + 1),
            (tb + 51,), (tb + 3, 50363, tb + 2), (tb, 0, last - 1, last - 1, 1, last, last, 2)]
    for k, text in enumerate((0, 1, eos - 1, eos, 50258, 50363, tb - 1, 31, 32, 4097, 220, 50257)):  # 40 steps of alternating pairs
        h, t = [tb + k], tb + k
        while len(h) < 40:
            t += 1 + k % 3
            h += [text, t, t]
        rows.append(tuple(h[:40]))
    rows += [tuple(h[:n]) for h, n in zip(rows[-12:], (39, 38, 37, 5, 4, 3, 2, 1, 17, 18, 19, 20))]
    return rows


@pytest.mark.parametrize("row_prompts", [False, True])
def test_whisper_tiny_layout(hip, row_prompts):
    """eos 50257, timestamp_begin 50364, vocab 51865, max_initial 50 (the tiny config's): 43 hand-built rows that reach t_last = 51864 (the
    timestamp range is empty from then on), t_last = 50364, a first id on the max-initial bound, and 40 steps of alternating pairs."""
    V, tb, eos = TINY["vocab"], TINY["tb"], TINY["eos"]
    hist = _tiny_rows()
    assert 24 <= len(hist) <= 60 and max(len(h) for h in hist) == 40
    st = [history_fields(h[:k], tb) for h in hist for k in range(len(h) + 1)]
    assert any(f[3] == V - 1 for f in st) and any(f[3] == tb for f in st) and any(h[0] == tb + 50 for h in hist)
    r, tok, plen, nids, steps = _replay(hist, V, tb, eos, 50, row_prompts)
    _check(r, hist, tok, plen, nids, steps, V, tb, eos, 50, row_prompts)
    np.testing.assert_array_equal(r["states"][0, :, 4:], np.tile([0, 0, tb, tb + 51], (len(hist), 1)))


@pytest.mark.parametrize("dt", [DT_F32, DT_BF16])
def test_ranges_feed_the_decision(hip, dt):
    """States of the exhaustive replay whose text range starts above 0 (the first timestamp of a pair: no id below eos), handed to the
    logits launch as its four ranges at (K, N) = (128, 12): the pick is _ts_decision's on the kernel's own logits wherever the margin
    exceeds its bound, and always inside the ranges.  The first op-level run of the logits kernel with text_lo = eos > 0."""
    from whisper_mojo_amd import whisper_tensor as wt
    V, tb, eos = SMALL["vocab"], SMALL["tb"], SMALL["eos"]
    hist = enumerate_histories(V, tb, eos, None, ENUM_DEPTH)
    r, *_ = _replay(hist, V, tb, eos, None, False)
    st = r["states"].reshape(-1, 8)
    sel = st[st[:, 4] > 0]
    assert (sel[:, 4] == eos).all() and len(sel) > 100
    uniq = np.unique(sel[:, 4:], axis=0)  # the distinct range quadruples: an open pair's t_last = 9 .. 11 (8 can only open the first pair)
    assert uniq.tolist() == [[eos, tb, t, V] for t in (9, 10, 11)]
    ranges = np.ascontiguousarray(np.tile(uniq, (6, 1))[:16], np.int32)
    rng = np.random.default_rng(12 + dt)
    x, g, b, emb = _decoder_like(rng, 16, 128, V, dt, scale=0.15)
    logits, ids = wt.logits_argmax(x, g, b, emb, dtype=dt, ranges=ranges, timestamp_begin=tb)
    plain, _ = wt.logits_argmax(x, g, b, emb, dtype=dt)
    np.testing.assert_array_equal(logits, plain)
    checked = below = 0
    for row, (pick, margin, bnd) in enumerate(_ts_decision(logits, None, ranges)):
        tlo, thi, qlo, qhi = ranges[row]
        assert tlo <= ids[row] < thi or qlo <= ids[row] < qhi, (row, ids[row], ranges[row])
        if abs(margin) > bnd:
            assert ids[row] == pick, (row, ids[row], pick, margin, bnd, ranges[row])
            checked += 1
        below += int(np.argmax(logits[row, :tb]) < tlo)
    assert checked >= 12 and below >= 2  # rows whose best text id lies below text_lo: the range's lower end decided


def test_ts_states_refusals(hip):
    """Every refusal returns WM_E_ARG before any launch and leaves the outputs as they were."""
    import ctypes as C
    from whisper_mojo_amd import _lib
    L = _lib.lib()
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    tok = np.array([[1, 2, 8, 3], [1, 2, 9, 0]], np.int32)
    plen, nids = np.array([2, 2], np.int32), np.array([4, 3], np.int32)

    def call(vocab=12, tb=8, eos=5, rows=0, tok=tok, plen=plen, nids=nids, with_rows=None):
        with_rows = rows if with_rows is None else with_rows
        out = [np.full(s, -7, np.int32) for s in ((3, 2, 8), (2, 2), (2, 4), (2,), (2,), (4,), (2,), (2, 2), (2, 2))]
        a = [ip(o) for o in out[:6]] + [ip(o) if with_rows else None for o in out[6:]]
        rc = L.wm_op_ts_states(*a, ip(tok), ip(plen), ip(nids), 2, 4, vocab, tb, eos, -1, 2, rows)
        return rc, all((o == -7).all() for o in out)

    assert call() == (0, False) and call(rows=1) == (0, False)
    bad = [dict(tb=0), dict(tb=-3), dict(tb=12), dict(tb=13), dict(eos=9), dict(eos=-1), dict(plen=np.array([0, 2], np.int32)),
           dict(plen=np.array([2, 4], np.int32)), dict(nids=np.array([5, 3], np.int32)), dict(tok=np.array([[1, 2, 12, 3], [1, 2, 9, 0]], np.int32)),
           dict(tok=np.array([[1, 2, 8, 3], [1, -1, 9, 0]], np.int32)), dict(tok=np.array([[1, 2, 8, 3], [1, 3, 9, 0]], np.int32)),  # prompts differ
           dict(plen=np.array([2, 1], np.int32)), dict(rows=1, with_rows=0), dict(rows=0, with_rows=1)]
    for kw in bad:
        assert call(**kw) == (WM_E_ARG, True), kw
    assert call(rows=1, tok=np.array([[1, 2, 8, 3], [1, 3, 9, 0]], np.int32))[0] == 0  # ragged rows may differ
    assert call(eos=8)[0] == 0 and call(eos=0)[0] == 0
