"""CPU tests of the top-k contract: a numpy float64 restatement — every logits processor in the library's order
(sequence_bias, repetition_penalty, no_repeat_ngram_size, bad_words_ids, the suppress lists, the timestamp rules' admissible ranges
and forced-timestamp decision, as tests/test_logprobs_ref.py and tests/test_seq_bias_ref.py restate them), then log-softmax over the
candidates that are left, then a stable top-k (value descending, lowest id first) — applied to the RAW logits of
tests/golden/topk_micro_hf.npz reproduces HF's greedy ids and scores.log_softmax(-1).topk(8) of every step, with and without the
timestamp rules.  The GPU tests (tests/test_gpu_topk.py) compare the library with this restatement."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN_TOL = 1e-3  # the project's fp32 margin: an id comparison is skipped where the reference's gap to a neighbouring rank is below it
SKIP_CAP = 0.02    # ... for at most this share of all (position, rank) pairs


def _ends_with(hist, seq):
    n = len(seq) - 1
    return n == 0 or (len(seq) <= len(hist) and list(hist[len(hist) - n:]) == list(seq[:-1]))


def restate_topk(raw, prompt, k, sup=(), bsup=(), ts=None, penalty=1.0, ngram=0, sequence_bias=(), bad_words=(), eos=-1, steps=None):
    """raw [steps, V] logits along a greedy path; ts = (timestamp_begin, eos, no_ts, max_init) or None.
    -> (ids, top_ids [steps, k], top_lps [steps, k], gaps [steps, k]): the greedy ids by the library's rule, per step the k best
    candidates (id -1 / -inf where fewer are finite) and each rank's distance to the NEXT rank's score (inf where there is none).
    The raw logits belong to one path: with processors that change the path only the steps up to the first changed id are meaningful
    (steps= limits the walk)."""
    V = raw.shape[1]
    hist = [int(t) for t in prompt]
    ids, top_ids, top_lps, gaps = [], [], [], []
    n_gen, last_ts, pen_ts, t_last = 0, 0, 1, -1
    for step in range(raw.shape[0] if steps is None else steps):
        s = raw[step].astype(np.float64).copy()
        for seq, bias in sequence_bias:
            if _ends_with(hist, seq):
                s[seq[-1]] += bias
        if penalty != 1.0:
            for t in set(hist):
                s[t] = s[t] * penalty if s[t] < 0 else s[t] / penalty
        if ngram >= 1 and len(hist) + 1 >= ngram:
            tail = hist[len(hist) - (ngram - 1):] if ngram > 1 else []
            for i in range(len(hist) - ngram + 1):
                if hist[i:i + ngram - 1] == tail:
                    s[hist[i + ngram - 1]] = -np.inf
        for seq in bad_words:
            if not (len(seq) == 1 and seq[0] == eos) and _ends_with(hist, seq):
                s[seq[-1]] = -np.inf
        s[list(sup)] = -np.inf
        if step == 0:
            s[list(bsup)] = -np.inf
        ok = np.ones(V, bool)
        if ts is not None:
            tb, ts_eos, no_ts, max_init = ts
            s[no_ts] = -np.inf
            text_lo, text_hi, ts_lo, ts_hi = 0, tb, tb, V  # ts_next_ranges (wm_kernels.h)
            if n_gen == 0:
                text_hi = 0
                if max_init >= 0:
                    ts_hi = min(ts_hi, tb + max_init + 1)
            else:
                if last_ts:
                    if pen_ts:
                        ts_hi = ts_lo
                    else:
                        text_lo = ts_eos
                if t_last >= 0:
                    ts_lo = max(ts_lo, t_last if (last_ts and not pen_ts) else t_last + 1)
            j = np.arange(V)
            is_text, is_ts = (j >= text_lo) & (j < text_hi), (j >= ts_lo) & (j < ts_hi)
            tss = s[is_ts & np.isfinite(s)]
            best = s[is_text].max() if is_text.any() else -np.inf
            lse_ts = tss.max() + np.log(np.exp(tss - tss.max()).sum()) if tss.size else -np.inf
            forced = lse_ts > -np.inf and (best == -np.inf or lse_ts > best)
            ok = is_ts if forced else (is_text | is_ts)
        c = np.flatnonzero(ok & np.isfinite(s))
        order = c[np.lexsort((c, -s[c]))]
        if order.size:
            M = s[order[0]]
            lse = M + np.log(np.exp(s[c] - M).sum())
            pick = int(order[0])
        else:
            lse, pick = np.inf, 0
        ti, tl, tg = np.full(k, -1, np.int64), np.full(k, -np.inf), np.full(k, np.inf)
        n = min(k, order.size)
        ti[:n] = order[:n]
        tl[:n] = s[order[:n]] - lse
        nxt = s[order[1:n + 1]]
        tg[:nxt.size] = s[order[:nxt.size]] - nxt
        ids.append(pick)
        top_ids.append(ti)
        top_lps.append(tl)
        gaps.append(tg)
        hist.append(pick)
        if ts is not None:
            is_t = pick >= ts[0]
            pen_ts = 1 if n_gen + 1 < 2 else last_ts
            last_ts = int(is_t)
            n_gen += 1
            if is_t:
                t_last = pick
    return ids, np.stack(top_ids), np.stack(top_lps), np.stack(gaps)


def decidable(gaps, tol):
    """[steps, k] bool: rank r's id is compared where its score is more than tol away from both neighbouring ranks'"""
    up = np.concatenate([np.full((gaps.shape[0], 1), np.inf), gaps[:, :-1]], 1)
    return (gaps > tol) & (up > tol)


def load_fixture():
    z = np.load(os.path.join(GOLDEN, "topk_micro_hf.npz"))
    rows = []
    for i in range(int(z["n_rows"])):
        q = f"r{i}_"
        rows.append(dict(seed=int(z[q + "seed"]), ts=int(z[q + "ts"]), ids=z[q + "ids"].tolist(), raw=z[q + "raw"], top_ids=z[q + "top_ids"],
                         top_lps=z[q + "top_logprobs"]))
    return z, rows


def fixture_ts(z, on):
    return (int(z["timestamp_begin"]), int(z["eos"]), int(z["no_ts"]), int(z["max_init"])) if on else None


def test_restatement_reproduces_hf_topk():
    z, rows = load_fixture()
    prompt, K = z["prompt"].tolist(), int(z["k"])
    assert {r["ts"] for r in rows} == {0, 1}
    worst, pairs, skipped = 0.0, 0, 0
    for i, r in enumerate(rows):
        ids, ti, tl, tg = restate_topk(r["raw"], prompt, K, z["suppress"].tolist(), z["begin_suppress"].tolist(), fixture_ts(z, r["ts"]))
        assert ids == r["ids"][len(prompt):], i
        np.testing.assert_array_equal(ti[:, 0], ids)
        fin = np.isfinite(r["top_lps"])
        np.testing.assert_array_equal(np.isfinite(tl), fin)  # the same number of finite candidates at every step
        worst = max(worst, np.abs(tl[fin] - r["top_lps"][fin].astype(np.float64)).max())
        d = decidable(tg, 1e-5) & fin  # (torch.topk names no order among equals; the fixture has none this close)
        np.testing.assert_array_equal(ti[d], r["top_ids"][d])
        # the cap the GPU tests rely on, from the reference alone: few ranks sit within MARGIN_TOL of a neighbour
        pairs += int(fin.sum())
        skipped += int((fin & ~decidable(tg, MARGIN_TOL)).sum())
    print(f"worst |restatement - HF| {worst:.2e}; {skipped} of {pairs} (position, rank) pairs within MARGIN_TOL of a neighbouring rank")
    assert worst <= 1e-5
    assert skipped <= SKIP_CAP * pairs


def test_restatement_fill_ties_and_processors():
    """The contract's corners on a hand-made row: ties by lowest id, -1 / -inf fill, a banned id at no rank, a bias moving a rank."""
    raw = np.full((1, 12), -np.inf)
    raw[0, [2, 5, 9]] = [1.0, 1.0, 0.5]
    ids, ti, tl, _ = restate_topk(raw, [0], 5)
    assert ids == [2] and ti[0].tolist() == [2, 5, 9, -1, -1]
    assert tl[0, 0] == tl[0, 1] and (tl[0, 3:] == -np.inf).all() and abs(np.exp(tl[0, :3]).sum() - 1) < 1e-12
    raw = np.arange(12, dtype=np.float64)[None]
    assert restate_topk(raw, [0], 3, bad_words=[[11]])[1][0].tolist() == [10, 9, 8]
    assert restate_topk(raw, [3, 0], 3, sequence_bias=[((0, 4), 6.5)])[1][0].tolist() == [11, 4, 10]
    assert restate_topk(raw, [3, 1], 3, sequence_bias=[((0, 4), 6.5)])[1][0].tolist() == [11, 10, 9]
    assert restate_topk(raw, [0], 3, sequence_bias=[((0, 4), 6.5)])[1][0].tolist() == [11, 10, 9]  # (HF: a sequence longer than the history is skipped)
    assert restate_topk(raw, [11], 2, penalty=2.0)[1][0].tolist() == [10, 9]
    assert restate_topk(raw, [11, 10, 3, 11], 2, ngram=2)[1][0].tolist() == [11, 9]


def test_host_refusals():
    """top_k is checked on the host before any library call: range, type, and the log-prob requirement."""
    from whisper_mojo_amd import _lib
    from whisper_mojo_amd.whisper import Whisper
    assert _lib.top_k_arg(None, False) == 0 and _lib.top_k_arg(8, True) == 8
    for bad in (0, 9, -1, True, 2.5):
        with pytest.raises(ValueError):
            _lib.top_k_arg(bad, True)
    with pytest.raises(ValueError, match="return_logprobs"):
        _lib.top_k_arg(3, False)
    m = Whisper()
    mel = np.zeros((1, m.config.n_mels, m.config.n_frames), np.float32)
    with pytest.raises(ValueError, match="return_logprobs"):
        m.transcribe_batch(mel, top_k=3)
    with pytest.raises(ValueError, match="top_k"):
        m.transcribe_batch(mel, return_logprobs=True, top_k=9)
    with pytest.raises(ValueError, match="long-form"):
        m.transcribe_long_form(mel, top_k=3)
    from whisper_mojo_amd import frontend
    with pytest.raises(ValueError, match="chunked"):
        frontend.transcribe_audio_chunked(m, np.zeros(16000, np.float32), top_k=3)
    with pytest.raises(ValueError, match="long-form"):
        frontend.transcribe_audio_long_form(m, [np.zeros(16000, np.float32)], top_k=3)


def test_library_exports_the_new_symbols():
    """wm_set_top_k, wm_transcribe_top_k and wm_op_logits_topk are declared in the header, listed in the binding and exported."""
    import ctypes
    import re
    from whisper_mojo_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "whisper_mi.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("wm_set_top_k", "wm_transcribe_top_k", "wm_op_logits_topk"):
        assert re.search(r"\b%s\s*\(" % s, txt) and s in _lib.SYMBOLS and hasattr(lib, s), s
