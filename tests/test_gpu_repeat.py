"""Model-level tests (-m gpu) of repetition_penalty / no_repeat_ngram_size on the micro model with synthetic weights.

Reference: a Python loop over the CPU oracle.  At each step the oracle's teacher-forced logits for the ids so far go through the numpy
processors of tests/test_repeat_ref.py, then through the oracle's timestamp rules where they are on, then arg-max; the log-prob is
the float64 log-softmax of that processed row at the chosen id.  Tokens follow tests/test_gpu_parity.py's rule (a mismatch only where
the reference's top-1 margin is below MARGIN_TOL); log-probs the 1e-4 bar of tests/test_gpu_logprobs.py.

The mel seeds are chosen with the oracle alone, before any GPU run: the unprocessed greedy stream must hold a repeated bigram and an
id that occurs three times (so each option changes the output) and no processed position may have a top-1 margin below 4·MARGIN_TOL."""
import numpy as np
import pytest

from test_gpu_parity import MARGIN_TOL, hip, make_model  # noqa: F401
from test_repeat_ref import process

pytestmark = pytest.mark.gpu

PROMPT = (1, 2, 3, 4)
MAX_LOOP = 12
TS = (900, 899, 50)  # timestamp_begin, <|notimestamps|>, max_initial_timestamp_index on the micro vocabulary (1000 ids)
EOT = 890
CASES = [dict(no_repeat_ngram_size=2), dict(repetition_penalty=1.3), dict(repetition_penalty=1.3, no_repeat_ngram_size=2)]


def _ref_stream(orc, model, enc, prompt, p=None, n=None, ts=None, eot=-1, max_loop=MAX_LOOP):
    """-> (ids, log-probs of the generated ids, smallest top-1 margin) of the processed greedy loop on the oracle"""
    ids, lps, margin = list(prompt), [], np.inf
    for _ in range(max_loop + 1):
        z = model.teacher_forced(enc, ids, n_prompt=len(prompt), pos_mode=0)[-1]  # (positions as the greedy loop's own)
        z = process(z, ids, p, n)
        if ts is not None:
            z[ts[1]] = -np.inf
            z = orc.timestamp_rules(z, ids[len(prompt):], ts[0], ts[1], eot, ts[2])
        s = np.sort(z[np.isfinite(z)])
        margin = min(margin, s[-1] - s[-2])
        t = int(np.flatnonzero(z == z.max())[0])
        z64 = z.astype(np.float64)
        fin = z64[np.isfinite(z64)]
        lps.append(float(z64[t] - (fin.max() + np.log(np.exp(fin - fin.max()).sum()))))
        ids.append(t)
        if t == eot:
            break
    return ids, lps, margin


def _repeats(ids):
    grams = list(zip(ids, ids[1:]))
    return len(set(grams)) < len(grams) and max(np.bincount(ids)) >= 3


@pytest.fixture(scope="module")
def setup(hip):
    """(cfg, weights, oracle module, oracle model, seeds, mels, encoder outputs, reference streams) — chosen and checked on the CPU"""
    from oracle import oracle as orc
    from whisper_mojo_amd import WhisperConfig, synth
    cfg = WhisperConfig.micro()
    w = synth.synth_weights(cfg, 0)
    om = orc.OracleModel(cfg, w)
    picked = []
    for seed in range(1001, 1065):
        mel = synth.synth_mels(cfg, seed, 1)[0]
        enc = om.encode(mel)
        plain, _, _ = _ref_stream(orc, om, enc, PROMPT)
        if not _repeats(plain):
            continue
        refs, ok = {}, True
        for ci, kw in enumerate(CASES):
            for ts in (None, TS):
                r = _ref_stream(orc, om, enc, PROMPT, kw.get("repetition_penalty"), kw.get("no_repeat_ngram_size"), ts, EOT if ts else -1)
                ok = ok and r[2] >= 4 * MARGIN_TOL
                refs[(ci, ts is not None)] = r
        if ok:
            picked.append((seed, mel, enc, plain, refs))
        if len(picked) == 3:
            break
    assert len(picked) == 3, f"only {len(picked)} of the seeds 1001..1064 repeat and keep every processed margin above {4 * MARGIN_TOL}"
    return cfg, w, orc, om, picked


def _kw(ts):
    return dict(prompt=PROMPT, eot=EOT if ts else -1, max_loop=MAX_LOOP, **({"timestamps": TS} if ts else {}))


def _mels(setup):
    return np.stack([p[1] for p in setup[4]])


def test_no_repeat_ngram_changes_the_stream(hip, setup):
    """The oracle-chosen streams do repeat a bigram; with no_repeat_ngram_size=2 none does, and the ids are the reference loop's."""
    cfg, w, orc, om, picked = setup
    m = make_model(cfg, w, max_batch=3)
    plain = m.transcribe_batch(_mels(setup), **_kw(False))
    got = m.transcribe_batch(_mels(setup), no_repeat_ngram_size=2, **_kw(False))
    for b, (seed, mel, enc, ref_plain, refs) in enumerate(picked):
        assert plain[b] == ref_plain and _repeats(plain[b])
        assert got[b] != plain[b]
        assert got[b] == refs[(0, False)][0], (seed, got[b], refs[(0, False)][0])
        grams = list(zip(got[b], got[b][1:]))
        assert len(set(grams)) == len(grams)
    m.close()


def _headline(cfg, w, max_batch, coalesce=0):
    """The benchmark's precision: bf16 encoder GEMMs, fp32 decoder and K/V"""
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, compute_dtype=1, kv_dtype=0, decoder_fp32=True, max_batch=max_batch, coalesce=coalesce)
    m.load(WeightLoader.from_array(w))
    return m


def _dev_stream(orc, m, mel, prompt, p=None, n=None, ts=None, eot=-1, max_loop=MAX_LOOP):
    """The processed greedy loop on the MODEL'S OWN raw logits (wm_decode_step: no processors, no mask), the numpy processors and the
    oracle's timestamp rules applied on the host -> (ids, log-probs, top-1 margin per generated position).  The reference for a
    precision the fp32 oracle cannot stand for: same operands, so the parity rule and the 1e-4 bar apply as they do for fp32."""
    from whisper_mojo_amd.whisper import KVCache
    cache = KVCache(m, 1)
    m.encoder.forward(mel, cache)
    z = m.decoder.forward(list(prompt), None, cache, start_pos=0)
    ids, lps, margins = list(prompt), [], []
    for step in range(max_loop + 1):
        z = process(z, ids, p, n)
        if ts is not None:
            z[ts[1]] = -np.inf
            z = orc.timestamp_rules(z, ids[len(prompt):], ts[0], ts[1], eot, ts[2])
        srt = np.sort(z[np.isfinite(z)])
        margins.append(float(srt[-1] - srt[-2]))
        t = int(np.flatnonzero(z == z.max())[0])
        fin = z.astype(np.float64)[np.isfinite(z)]
        lps.append(float(np.float64(z[t]) - (fin.max() + np.log(np.exp(fin - fin.max()).sum()))))
        ids.append(t)
        if t == eot or step == max_loop:
            break
        z = m.decoder.forward([t], None, cache, start_pos=cache.current_len - 1)
    return ids, lps, margins


def _assert_stream(tag, got, glp, want, wlp, margins):
    """tests/test_gpu_parity.py's rule, position by position: the ids part only where the reference's top-1 margin is below
    MARGIN_TOL (behind that position the streams are different streams); log-probs within 1e-4 up to there."""
    k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
    if k is None:
        assert len(got) == len(want), (tag, got, want)
        k = len(want)
    else:
        assert margins[k - len(PROMPT)] < MARGIN_TOL, (tag, k, got, want, margins[k - len(PROMPT)])
    err = np.abs(np.asarray(glp[len(PROMPT):k], np.float64) - np.asarray(wlp[:k - len(PROMPT)]))
    print(f"{tag}: {k - len(PROMPT)} positions compared, max |log-prob error| {err.max() if err.size else 0:.3g}")
    assert (err <= 1e-4).all(), (tag, err.max())
    return k


@pytest.mark.parametrize("prec", ["fp32", "headline"])
@pytest.mark.parametrize("ts", [False, True], ids=["plain", "timestamps"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=["n2", "p1.3", "both"])
def test_matches_the_processed_oracle_loop(hip, setup, ci, ts, prec):
    """fp32: against the processed loop over the CPU oracle (the fixture holds every margin at 4·MARGIN_TOL or more, so the ids are
    exact).  Headline precision: the bf16 encoder moves the logits by about 1e-2, a hundred times the log-prob bar, so the fp32 oracle
    cannot be the reference; the same loop runs on the model's own raw logits instead (_dev_stream) and everything the options add is
    compared as for fp32 — ids by the parity rule at every position, log-probs within 1e-4.  Against the CPU oracle the headline ids
    must still agree wherever the oracle's margin exceeds 0.12, the bar tests/test_gpu_parity.py sets for this precision."""
    cfg, w, orc, om, picked = setup
    m = make_model(cfg, w, max_batch=3) if prec == "fp32" else _headline(cfg, w, 3)
    kw = CASES[ci]
    ids, (lps, avg) = m.transcribe_batch(_mels(setup), return_logprobs=True, **kw, **_kw(ts))
    for b, (seed, mel, enc, _, refs) in enumerate(picked):
        want, wlp, _ = refs[(ci, ts)]
        got = ids[b]
        if prec == "fp32":
            assert got == want, (seed, got, want)
            k = _assert_stream(f"fp32 seed {seed}", got, lps[b], want, wlp, [np.inf] * len(wlp))
            assert abs(avg[b] - np.mean(wlp)) <= 1e-4
        else:
            dwant, dlp, dm = _dev_stream(orc, m, mel, PROMPT, kw.get("repetition_penalty"), kw.get("no_repeat_ngram_size"),
                                         TS if ts else None, EOT if ts else -1)
            k = _assert_stream(f"headline seed {seed}", got, lps[b], dwant, dlp, dm)
            assert k > len(PROMPT) + 1  # more than the first generated id was compared
            if k == len(dwant):
                assert abs(avg[b] - np.mean(dlp)) <= 1e-4
            j = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
            if j is not None:  # first divergence from the fp32 oracle: only at a margin this precision may cross
                zs = process(om.teacher_forced(enc, want[:j], n_prompt=len(PROMPT), pos_mode=0)[-1], want[:j],
                             kw.get("repetition_penalty"), kw.get("no_repeat_ngram_size"))
                if ts:
                    zs[TS[1]] = -np.inf
                    zs = orc.timestamp_rules(zs, want[len(PROMPT):j], TS[0], TS[1], EOT, TS[2])
                srt = np.sort(zs[np.isfinite(zs)])
                assert srt[-1] - srt[-2] < 0.12, (seed, j, got, want, srt[-1] - srt[-2])
        n = kw.get("no_repeat_ngram_size")
        if n and not ts:
            grams = list(zip(got, got[1:]))
            assert len(set(grams)) == len(grams)
    m.close()


def test_identities_bit_for_bit(hip, setup):
    """Off equals absent; B = 3 equals three B = 1 runs; per-row prompts equal each row alone; a second call on the same state with
    other audio equals a fresh model (stale sets would show)."""
    cfg, w, orc, om, picked = setup
    mels = _mels(setup)
    on = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    m = make_model(cfg, w, max_batch=3)
    base = m.transcribe_batch(mels, return_logprobs=True, **_kw(True))
    off = m.transcribe_batch(mels, return_logprobs=True, repetition_penalty=1.0, no_repeat_ngram_size=0, **_kw(True))
    assert off[0] == base[0] and off[1][0] == base[1][0]
    np.testing.assert_array_equal(np.asarray(off[1][1]).view(np.uint32), np.asarray(base[1][1]).view(np.uint32))
    both = m.transcribe_batch(mels, return_logprobs=True, **on, **_kw(True))
    assert both[0] != base[0]
    for b in range(3):
        one = m.transcribe_batch(mels[b:b + 1], return_logprobs=True, **on, **_kw(True))
        assert one[0][0] == both[0][b] and one[1][0][0] == both[1][0][b]
    # per-row prompts of 1 / 5 / 17 ids
    rows = [[1], [1, 2, 3, 4, 5], list(range(1, 18))]
    kw = dict(eot=EOT, max_loop=MAX_LOOP, timestamps=TS)
    together = m.transcribe_batch(mels, prompts=rows, **on, **kw)
    for b in range(3):
        assert m.transcribe_batch(mels[b:b + 1], prompts=[rows[b]], **on, **kw)[0] == together[b]
    # same state, other audio (rows rotated), against a fresh model
    again = m.transcribe_batch(mels[[1, 2, 0]], **on, **_kw(True))
    m.close()
    fresh = make_model(cfg, w, max_batch=3)
    assert fresh.transcribe_batch(mels[[1, 2, 0]], **on, **_kw(True)) == again
    assert again == [both[0][1], both[0][2], both[0][0]]
    # four pipelined submits equal the synchronous results
    for s in range(4):
        fresh.transcribe_submit(mels[[s % 3]], slot=s, **on, **_kw(True))
    for s in range(4):
        assert fresh.transcribe_wait(s)[0] == both[0][s % 3]
    fresh.close()


@pytest.mark.parametrize("k", [1, 2, 3])
def test_no_kgram_repeats(hip, setup, k):
    cfg, w, orc, om, picked = setup
    m = make_model(cfg, w, max_batch=3)
    out = m.transcribe_batch(_mels(setup), no_repeat_ngram_size=k, **_kw(False))
    m.close()
    for ids in out:
        grams = [tuple(ids[i:i + k]) for i in range(len(ids) - k + 1)]
        assert len(set(grams)) == len(grams), (k, ids)


def test_coalesced_pairs(hip, setup):
    """coalesce = 2: two submits under equal (p, n) share one 2·B-row state, each row with its own sets, and return the synchronous
    results; submits under unequal (p, n) are not paired — each returns what it returns alone, under its own values."""
    cfg, w, orc, om, picked = setup
    mels = _mels(setup)
    rot = mels[[1, 2, 0]].copy()
    on = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    other = dict(repetition_penalty=1.3, no_repeat_ngram_size=3)
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, max_batch=3, coalesce=2)
    m.load(WeightLoader.from_array(w))
    kw = dict(return_logprobs=True, **_kw(True))
    want_a, want_b = m.transcribe_batch(mels, **on, **kw), m.transcribe_batch(rot, **on, **kw)
    want_c, plain = m.transcribe_batch(rot, **other, **kw), m.transcribe_batch(rot, **kw)
    assert want_b[0] != want_c[0] and want_b[0] != plain[0]  # the three settings are told apart by their ids

    def same(x, y):
        assert x[0] == y[0] and x[1][0] == y[1][0]
        np.testing.assert_array_equal(np.asarray(x[1][1]).view(np.uint32), np.asarray(y[1][1]).view(np.uint32))

    m.transcribe_submit(mels, slot=0, **on, **kw)
    m.transcribe_submit(rot, slot=1, **on, **kw)  # the partner: one pass of 6 rows
    same(m.transcribe_wait(0), want_a)
    same(m.transcribe_wait(1), want_b)
    for second, want in ((other, want_c), ({}, plain)):  # unequal values, and options against none: no pair
        m.transcribe_submit(mels, slot=2, **on, **kw)
        m.transcribe_submit(rot, slot=3, **second, **kw)
        same(m.transcribe_wait(2), want_a)
        same(m.transcribe_wait(3), want)
    m.close()


def test_probe_and_language_read_raw_logits(hip, setup):
    """no_speech_prob and the detected language (ids and distribution) are bit for bit what they are without the options."""
    cfg, w, orc, om, picked = setup
    mels = _mels(setup)
    on = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    m = make_model(cfg, w, max_batch=3)
    kw = dict(return_logprobs=True, no_speech_token=7, **_kw(True))
    a, b = m.transcribe_batch(mels, **kw), m.transcribe_batch(mels, **on, **kw)
    assert a[0] != b[0]
    np.testing.assert_array_equal(np.asarray(a[1][2]).view(np.uint32), np.asarray(b[1][2]).view(np.uint32))
    langs = [10, 11, 12, 13, 14]
    c, d = m.transcribe_batch(mels, detect_language=langs, **_kw(True)), m.transcribe_batch(mels, detect_language=langs, **on, **_kw(True))
    np.testing.assert_array_equal(c[1][0], d[1][0])
    np.testing.assert_array_equal(np.asarray(c[1][1]).view(np.uint32), np.asarray(d[1][1]).view(np.uint32))
    assert all(x[1] == int(l) for x, l in zip(d[0], d[1][0]))  # the detected id sits in the prompt and counts as history
    m.close()


def test_long_form_with_conditioning(hip, setup):
    """A 2.5-window recording with no_repeat_ngram_size=3 and condition_on_prev_tokens: the library's scheduler equals the numpy
    window loop over transcribe_batch with the same options — every window's pass sees its own prompt, carried text included."""
    from whisper_mojo_amd import _lib, synth
    cfg, w, orc, om, picked = setup
    W, T, PREV = cfg.n_frames, 5 * cfg.n_frames // 2, 880
    mel = synth.synth_long_mel(cfg, 1001, T)
    m = make_model(cfg, w, max_batch=3)
    kw = dict(eot=EOT, max_loop=MAX_LOOP, timestamps=TS)
    lf = dict(prompt=PROMPT, condition_on_prev_tokens=True, prev_sot_token=PREV, **kw)
    got = m.transcribe_long_form(mel[None], **lf, no_repeat_ngram_size=3)[0]
    without = m.transcribe_long_form(mel[None], **lf)[0]
    assert got["sequence"] != without["sequence"]
    seek, segs, seq = 0, [], []
    while seek < T:
        snf = min(T - seek, W)
        win = np.zeros((1, cfg.n_mels, W), np.float32)
        win[0, :, :snf] = mel[:, seek:seek + snf]
        prompt = _lib.long_prompt(segs, PROMPT, TS[0], cfg.n_text_ctx, condition_on_prev_tokens=True, prev_sot_token=PREV)
        ids = m.transcribe_batch(win, prompts=[prompt], no_repeat_ngram_size=3, **kw)[0][len(prompt):]
        if ids and ids[-1] == EOT:
            ids = ids[:-1]
        sg, adv = _lib.long_segments(ids, TS[0], seek, snf)
        for first, count, _s, _e in sg:
            segs.append(ids[first:first + count])
            seq += ids[first:first + count]
        seek += adv if adv else snf
    assert len(segs) >= 2 and got["sequence"] == seq
    assert [s["tokens"] for s in got["segments"]] == segs
    m.close()
