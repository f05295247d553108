"""Model-level tests (-m gpu) of sequence_bias / bad_words_ids on the micro model with synthetic weights.

Reference: the processed greedy loop of tests/test_gpu_repeat.py with the numpy processors of tests/test_seq_bias_ref.py — over the CPU
oracle for the fp32 model, over the model's own raw logits (wm_decode_step) for the headline precision, whose bf16 encoder moves the
logits by a hundred times the log-prob bar.  Bars as there: ids by tests/test_gpu_parity.py's rule, log-probs within 1e-4.  The
tables are built from the oracle's unprocessed streams alone, before any GPU run."""
import numpy as np
import pytest

from test_gpu_parity import MARGIN_TOL, hip, make_model  # noqa: F401
from test_gpu_repeat import EOT, MAX_LOOP, PROMPT, TS, _assert_stream, _headline
from test_seq_bias_ref import process

pytestmark = pytest.mark.gpu

NP = len(PROMPT)
# The micro model's unprocessed streams repeat one id for many steps, so a 2-gram of such a stream already occurs before positions
# 3-4.  The two stream tests therefore run both sides under no_repeat_ngram_size=1, which makes every id of a stream distinct: the
# banned 2-gram then occurs once, and the sequence options are exercised together with the repetition processors.
BASE = dict(no_repeat_ngram_size=1)


def _step(orc, z, ids, prompt, opt, ts, eot):
    z = process(z, ids, opt.get("sequence_bias"), opt.get("bad_words_ids"), opt.get("repetition_penalty"), opt.get("no_repeat_ngram_size"), eot)
    if ts is not None:
        z[ts[1]] = -np.inf
        z = orc.timestamp_rules(z, ids[len(prompt):], ts[0], ts[1], eot, ts[2])
    srt = np.sort(z[np.isfinite(z)])
    t = int(np.flatnonzero(z == z.max())[0])
    fin = z.astype(np.float64)[np.isfinite(z)]
    return t, float(np.float64(z[t]) - (fin.max() + np.log(np.exp(fin - fin.max()).sum()))), float(srt[-1] - srt[-2])


def _ref_stream(orc, om, enc, prompt, opt, ts=None, eot=-1, max_loop=MAX_LOOP):
    """-> (ids, log-probs, margins) of the processed greedy loop on the CPU oracle"""
    ids, lps, margins = list(prompt), [], []
    for _ in range(max_loop + 1):
        t, lp, mg = _step(orc, om.teacher_forced(enc, ids, n_prompt=len(prompt), pos_mode=0)[-1], ids, prompt, opt, ts, eot)
        ids.append(t), lps.append(lp), margins.append(mg)
        if t == eot:
            break
    return ids, lps, margins


def _dev_stream(orc, m, mel, prompt, opt, ts=None, eot=-1, max_loop=MAX_LOOP):
    """The same loop on the model's own raw logits (no processors, no mask on the device)"""
    from whisper_mojo_amd.whisper import KVCache
    cache = KVCache(m, 1)
    m.encoder.forward(mel, cache)
    z = m.decoder.forward(list(prompt), None, cache, start_pos=0)
    ids, lps, margins = list(prompt), [], []
    for step in range(max_loop + 1):
        t, lp, mg = _step(orc, z, ids, prompt, opt, ts, eot)
        ids.append(t), lps.append(lp), margins.append(mg)
        if t == eot or step == max_loop:
            break
        z = m.decoder.forward([t], None, cache, start_pos=cache.current_len - 1)
    return ids, lps, margins


@pytest.fixture(scope="module")
def setup(hip):
    """Three recordings with their oracle streams, unprocessed and under BASE, every margin of both at 4·MARGIN_TOL or more, and one
    table made from recording 0's streams: a banned 4-gram of the unprocessed stream, an [eot] bad word, two sequences ending in one
    id, length-1 biases and a -inf bias."""
    from oracle import oracle as orc
    from whisper_mojo_amd import WhisperConfig, synth
    cfg = WhisperConfig.micro()
    w = synth.synth_weights(cfg, 0)
    om = orc.OracleModel(cfg, w)
    picked = []
    for seed in range(1001, 1040):
        mel = synth.synth_mels(cfg, seed, 1)[0]
        enc = om.encode(mel)
        plain, _, pm = _ref_stream(orc, om, enc, PROMPT, {})
        div, _, dm = _ref_stream(orc, om, enc, PROMPT, BASE)
        if min(pm) < 4 * MARGIN_TOL or min(dm) < 4 * MARGIN_TOL:
            continue
        picked.append((seed, mel, enc, plain, div))
        if len(picked) == 3:
            break
    assert len(picked) == 3
    g, d = picked[0][3][NP:], picked[0][4][NP:]
    t = _ref_stream(orc, om, picked[0][2], PROMPT, {}, TS, EOT)[0][NP:]  # under the timestamp rules the stream is another one
    assert t[4] == t[5] and t[1] < TS[0]
    opt = dict(bad_words_ids=[[g[0], g[1], g[2], g[3]], [EOT], [d[1], d[2]], [t[4], t[5]]],
               sequence_bias={(g[0], g[1]): 0.5, (PROMPT[-1], g[0], g[1]): 0.25, (11,): -2.0, (g[1], 12): float("-inf"), (13,): 1.5, (d[2], 13): 0.75})
    refs = {"ts_stream": t}
    for ts in (None, TS):
        for b, (seed, mel, enc, plain, div) in enumerate(picked):
            refs[(b, ts is not None)] = _ref_stream(orc, om, enc, PROMPT, opt, ts, EOT if ts else -1)
    return cfg, w, orc, om, picked, opt, refs


def _kw(ts):
    return dict(prompt=PROMPT, eot=EOT if ts else -1, max_loop=MAX_LOOP, **({"timestamps": TS} if ts else {}))


def _mels(setup):
    return np.stack([p[1] for p in setup[4]])


def test_bad_words_change_the_stream(hip, setup):
    """The 2-gram at generated positions 3-4 of each stream (under BASE, see there) is banned: the ids before position 4 stay,
    position 4 differs and is not the banned id."""
    cfg, w, orc, om, picked, _, _ = setup
    m = make_model(cfg, w, max_batch=1)
    for seed, mel, enc, _, plain in picked:
        g = plain[NP:]
        assert m.transcribe_batch(mel[None], **BASE, **_kw(False))[0] == plain
        got = m.transcribe_batch(mel[None], bad_words_ids=[[g[3], g[4]]], **BASE, **_kw(False))[0]
        assert got[:NP + 4] == plain[:NP + 4], (seed, got, plain)
        assert got[NP + 4] != g[4]
        want, _, margins = _ref_stream(orc, om, enc, PROMPT, dict(bad_words_ids=[[g[3], g[4]]], **BASE))
        k = next((i for i in range(len(want)) if got[i] != want[i]), None)
        assert k is None or margins[k - NP] < MARGIN_TOL, (seed, k, got, want)
    m.close()


def test_bias_pulls_a_runner_up_in(hip, setup):
    """At generated position 2 the oracle's runner-up, biased by the margin there plus 1 on the condition of the two ids before it,
    takes the place; the ids before it stay."""
    cfg, w, orc, om, picked, _, _ = setup
    m = make_model(cfg, w, max_batch=1)
    for seed, mel, enc, _, plain in picked:
        z = process(om.teacher_forced(enc, plain[:NP + 2], n_prompt=NP, pos_mode=0)[-1], plain[:NP + 2], n=1)
        order = np.argsort(-z, kind="stable")
        assert int(order[0]) == plain[NP + 2]
        runner, margin = int(order[1]), float(z[order[0]] - z[order[1]])
        got = m.transcribe_batch(mel[None], sequence_bias={(plain[NP], plain[NP + 1], runner): margin + 1.0}, **BASE, **_kw(False))[0]
        assert got[:NP + 2] == plain[:NP + 2] and got[NP + 2] == runner, (seed, got, plain, runner, margin)
        less = m.transcribe_batch(mel[None], sequence_bias={(plain[NP], plain[NP + 1], runner): margin - 4 * MARGIN_TOL}, **BASE, **_kw(False))[0]
        assert less[NP + 2] == plain[NP + 2]
    m.close()


@pytest.mark.parametrize("prec", ["fp32", "headline"])
@pytest.mark.parametrize("ts", [False, True], ids=["plain", "timestamps"])
@pytest.mark.parametrize("rp", [False, True], ids=["alone", "with_p_n"])
def test_matches_the_processed_loop(hip, setup, rp, ts, prec):
    cfg, w, orc, om, picked, opt, refs = setup
    opt = dict(opt, **(dict(repetition_penalty=1.3, no_repeat_ngram_size=3) if rp else {}))
    m = make_model(cfg, w, max_batch=3) if prec == "fp32" else _headline(cfg, w, 3)
    ids, (lps, avg) = m.transcribe_batch(_mels(setup), return_logprobs=True, **opt, **_kw(ts))
    for b, (seed, mel, enc, plain, div) in enumerate(picked):
        if prec == "fp32":
            want, wlp, margins = refs[(b, ts)] if not rp else _ref_stream(orc, om, enc, PROMPT, opt, TS if ts else None, EOT if ts else -1)
        else:
            want, wlp, margins = _dev_stream(orc, m, mel, PROMPT, opt, TS if ts else None, EOT if ts else -1)
        k = _assert_stream(f"{prec} seed {seed}", ids[b], lps[b], want, wlp, margins)
        assert k > NP + 1
    assert ids[0] != picked[0][3]  # the table does change row 0's stream
    m.close()


def test_identities_bit_for_bit(hip, setup):
    """Off equals absent; B = 3 equals three B = 1 runs; per-row prompts equal each row alone; a second call on the same state with
    other audio equals a fresh model (stale hits would show); four pipelined submits equal the synchronous results."""
    cfg, w, orc, om, picked, opt, refs = setup
    mels = _mels(setup)
    m = make_model(cfg, w, max_batch=3)
    base = m.transcribe_batch(mels, return_logprobs=True, **_kw(True))
    off = m.transcribe_batch(mels, return_logprobs=True, sequence_bias={}, bad_words_ids=[], **_kw(True))
    assert off[0] == base[0] and off[1][0] == base[1][0]
    np.testing.assert_array_equal(np.asarray(off[1][1]).view(np.uint32), np.asarray(base[1][1]).view(np.uint32))
    both = m.transcribe_batch(mels, return_logprobs=True, **opt, **_kw(True))
    assert both[0] != base[0]
    for b in range(3):
        one = m.transcribe_batch(mels[b:b + 1], return_logprobs=True, **opt, **_kw(True))
        assert one[0][0] == both[0][b] and one[1][0][0] == both[1][0][b]
    assert m.transcribe_batch(mels, return_logprobs=True, **_kw(True))[0] == base[0]  # and off again after on
    g = picked[0][3][NP:]
    rows = [[1], [1, 2, 3, g[0], g[1]], list(range(1, 18))]  # row 1's prompt ends in a biased prefix
    kw = dict(eot=EOT, max_loop=MAX_LOOP, timestamps=TS)
    together = m.transcribe_batch(mels, prompts=rows, **opt, **kw)
    for b in range(3):
        assert m.transcribe_batch(mels[b:b + 1], prompts=[rows[b]], **opt, **kw)[0] == together[b]
    again = m.transcribe_batch(mels[[1, 2, 0]], **opt, **_kw(True))
    m.close()
    fresh = make_model(cfg, w, max_batch=3)
    assert fresh.transcribe_batch(mels[[1, 2, 0]], **opt, **_kw(True)) == again
    assert again == [both[0][1], both[0][2], both[0][0]]
    for s in range(4):
        fresh.transcribe_submit(mels[[s % 3]], slot=s, **opt, **_kw(True))
    for s in range(4):
        assert fresh.transcribe_wait(s)[0] == both[0][s % 3]
    fresh.close()


def test_coalesced_pairs(hip, setup):
    """coalesce = 2: two submits under the same table share one 2·B-row state and return the synchronous results; submits under
    unequal tables are not paired, and replacing the table while a submit is held does not change that submit."""
    cfg, w, orc, om, picked, opt, refs = setup
    mels = _mels(setup)
    rot = mels[[1, 2, 0]].copy()
    g = picked[1][3][NP:]
    other = dict(bad_words_ids=[[g[0], g[1], g[2]], [g[8]], [refs["ts_stream"][1]]])
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, max_batch=3, coalesce=2)
    m.load(WeightLoader.from_array(w))
    kw = dict(return_logprobs=True, **_kw(True))
    want_a, want_b = m.transcribe_batch(mels, **opt, **kw), m.transcribe_batch(rot, **opt, **kw)
    want_c, plain = m.transcribe_batch(rot, **other, **kw), m.transcribe_batch(rot, **kw)
    assert want_b[0] != want_c[0] and want_b[0] != plain[0] and want_c[0] != plain[0]

    def same(x, y):
        assert x[0] == y[0] and x[1][0] == y[1][0]
        np.testing.assert_array_equal(np.asarray(x[1][1]).view(np.uint32), np.asarray(y[1][1]).view(np.uint32))

    m.transcribe_submit(mels, slot=0, **opt, **kw)
    m.transcribe_submit(rot, slot=1, **opt, **kw)  # the partner: one pass of 6 rows
    same(m.transcribe_wait(0), want_a)
    same(m.transcribe_wait(1), want_b)
    for second, want in ((other, want_c), ({}, plain)):  # another table, and a table against none: no pair, the held one keeps its own
        m.transcribe_submit(mels, slot=2, **opt, **kw)
        m.transcribe_submit(rot, slot=3, **second, **kw)
        same(m.transcribe_wait(2), want_a)
        same(m.transcribe_wait(3), want)
    m.close()


def test_probe_language_and_score_read_raw_logits(hip, setup):
    cfg, w, orc, om, picked, opt, refs = setup
    mels = _mels(setup)
    m = make_model(cfg, w, max_batch=3)
    kw = dict(return_logprobs=True, no_speech_token=7, **_kw(True))
    a, b = m.transcribe_batch(mels, **kw), m.transcribe_batch(mels, **opt, **kw)
    assert a[0] != b[0]
    np.testing.assert_array_equal(np.asarray(a[1][2]).view(np.uint32), np.asarray(b[1][2]).view(np.uint32))
    langs = [10, 11, 12, 13, 14]
    c, d = m.transcribe_batch(mels, detect_language=langs, **_kw(True)), m.transcribe_batch(mels, detect_language=langs, **opt, **_kw(True))
    np.testing.assert_array_equal(c[1][0], d[1][0])
    np.testing.assert_array_equal(np.asarray(c[1][1]).view(np.uint32), np.asarray(d[1][1]).view(np.uint32))
    # score after a pass with the table (the model-wide setting is still in force in the library): unprocessed
    ids = [p[3] for p in picked]
    s0 = make_model(cfg, w, max_batch=3)
    want = s0.score(mels, ids)
    s0.close()
    got = m.score(mels, ids)
    for x, y in zip(got[0], want[0]):
        np.testing.assert_array_equal(np.asarray(x, np.float32).view(np.uint32), np.asarray(y, np.float32).view(np.uint32))
    m.close()


def test_align_reads_raw_logits(hip, setup):
    """align (times and teacher-forced log-probs) after a pass with the table, the model-wide setting still in force in the library,
    equals a fresh model's bit for bit."""
    cfg, w, orc, om, picked, opt, refs = setup
    mels = _mels(setup)
    ids = [p[3] for p in picked]
    heads = [(cfg.n_layers - 1, 0), (0, cfg.n_heads - 1)]
    fresh = make_model(cfg, w, max_batch=3)
    fresh.set_alignment_heads(heads)
    want_t, (want_lp, _) = fresh.align(mels, ids, context_len=NP, return_logprobs=True)
    fresh.close()
    m = make_model(cfg, w, max_batch=3)
    m.set_alignment_heads(heads)
    assert m.transcribe_batch(mels, **opt, **_kw(False))[0] == refs[(0, False)][0]
    got_t, (got_lp, _) = m.align(mels, ids, context_len=NP, return_logprobs=True)
    m.close()
    for a, b in zip(list(got_t) + list(got_lp), list(want_t) + list(want_lp)):
        np.testing.assert_array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_a_reloaded_model_gets_the_table_again(hip, setup):
    """load() makes a new library model without a table: the same lists as the call before the reload must be set again, not taken
    for set already; after close() + load() likewise."""
    from whisper_mojo_amd.loader import WeightLoader
    cfg, w, orc, om, picked, opt, refs = setup
    mels = _mels(setup)
    m = make_model(cfg, w, max_batch=3)
    want = m.transcribe_batch(mels, **opt, **_kw(False))
    plain = m.transcribe_batch(mels, **_kw(False))
    assert want != plain and want[0] == refs[(0, False)][0]
    assert m.transcribe_batch(mels, **opt, **_kw(False)) == want
    m.load(WeightLoader.from_array(w))
    assert m.transcribe_batch(mels, **opt, **_kw(False)) == want
    m.close()
    m.load(WeightLoader.from_array(w))
    assert m.transcribe_batch(mels, **opt, **_kw(False)) == want
    assert m.transcribe_batch(mels, **_kw(False)) == plain
    m.close()


def test_long_form_with_conditioning(hip, setup):
    """A 2.5-window recording with the table and condition_on_prev_tokens: the library's scheduler equals the numpy window loop over
    transcribe_batch with the same options — every window's pass sees its own prompt, carried text included."""
    from whisper_mojo_amd import _lib, synth
    cfg, w, orc, om, picked, opt, refs = setup
    W, T, PREV = cfg.n_frames, 5 * cfg.n_frames // 2, 880
    mel = synth.synth_long_mel(cfg, 1001, T)
    m = make_model(cfg, w, max_batch=3)
    kw = dict(eot=EOT, max_loop=MAX_LOOP, timestamps=TS)
    lf = dict(prompt=PROMPT, condition_on_prev_tokens=True, prev_sot_token=PREV, **kw)
    without = m.transcribe_long_form(mel[None], **lf)[0]
    s = [t for t in without["sequence"] if t < TS[0]]
    tab = dict(bad_words_ids=[[s[1], s[2]], [s[5]]], sequence_bias={(s[0], s[3]): 1.0})
    got = m.transcribe_long_form(mel[None], **lf, **tab)[0]
    assert got["sequence"] != without["sequence"]
    seek, segs, seq = 0, [], []
    while seek < T:
        snf = min(T - seek, W)
        win = np.zeros((1, cfg.n_mels, W), np.float32)
        win[0, :, :snf] = mel[:, seek:seek + snf]
        prompt = _lib.long_prompt(segs, PROMPT, TS[0], cfg.n_text_ctx, condition_on_prev_tokens=True, prev_sot_token=PREV)
        ids = m.transcribe_batch(win, prompts=[prompt], **tab, **kw)[0][len(prompt):]
        if ids and ids[-1] == EOT:
            ids = ids[:-1]
        sg, adv = _lib.long_segments(ids, TS[0], seek, snf)
        for first, count, _s, _e in sg:
            segs.append(ids[first:first + count])
            seq += ids[first:first + count]
        seek += adv if adv else snf
    assert len(segs) >= 2 and got["sequence"] == seq
    assert [x["tokens"] for x in got["segments"]] == segs
    m.close()
