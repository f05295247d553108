"""Model-level tests (-m gpu) of Whisper-medium's shape (d_model 1024, 16 heads, ffn 4096) on a reduced context and vocabulary and
two layers, as tests/test_gpu_small_model.py does for small.  Tolerances are the ones the corresponding tiny / base tests use
(F32_TOL, MARGIN_TOL, the 16-bit bars of test_tiny_16bit_modes_within_tolerance and test_tiny_bf16_encoder_fp32_decoder).  The
rounding error of a K-deep product of rounded operands grows as sqrt(K), so a 16-bit bar could at most have become the tiny bar x
sqrt(1024 / 384) at this width; the tiny bars hold unwidened (see test_medium_16bit_modes_within_tolerance).  The true dims (24 + 24 layers, 51 865 ids) run in tools/medium_cost.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32_TOL = 5e-5      # tests/test_gpu_parity.py
MARGIN_TOL = 1e-3   # tests/test_gpu_parity.py: a token may differ from the oracle's only below this oracle margin
PROMPT = (1, 2, 3, 4)
STEPS = 16


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()  # raises if the HIP library is missing: no fallback
    return True


@pytest.fixture(scope="module")
def medium():
    """(cfg, weights, mels [4], oracle, per-mel (tokens, logits)) — computed once, shared, never modified.  Mel seeds 1006, 1007, 1010
    and 1013: chosen with the oracle alone, on the CPU, among seeds 1001 .. 1024: 0 of their 4 x 17 greedy positions have a top-1
    margin below 0.24 (4x the widest 16-bit bar; the smallest margin is 0.256).  The cap of 1 is checked here, before any GPU run."""
    from oracle import oracle
    from whisper_mojo_amd import WhisperConfig, synth
    cfg = WhisperConfig(1024, 16, 2, 3000, 4096, 80, 200, 64)
    w = synth.synth_weights(cfg, 3)
    mels = np.stack([synth.synth_mel(cfg, s) for s in (1006, 1007, 1010, 1013)])
    ref = oracle.OracleModel(cfg, w)
    runs = [ref.transcribe(mel=mels[i], prompt=PROMPT, eot=-1, max_loop=STEPS, want_logits=True) for i in range(4)]
    low = 0
    for _, logits in runs:
        s = np.sort(logits, 1)
        assert len(s) == STEPS + 1
        low += int(((s[:, -1] - s[:, -2]) < 0.24).sum())
    assert low <= 1, f"{low} of the 68 greedy positions have a margin below 0.24: choose other mels"
    return cfg, w, mels, ref, runs


def _model(cfg, w, **kw):
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, **kw)
    m.load(WeightLoader.from_array(w))
    return m


def _assert_tokens(got, want, logits_ref, n_prompt):
    """tests/test_gpu_parity.py's rule: token-exact unless the oracle itself was at a near-tie where the streams part"""
    got, want = list(got), list(want)
    for i in range(min(len(got), len(want))):
        if got[i] != want[i]:
            s = np.sort(logits_ref[i - n_prompt])
            assert s[-1] - s[-2] < MARGIN_TOL, f"token {i}: HIP {got[i]} vs oracle {want[i]} with oracle margin {s[-1] - s[-2]}"
            return
    assert len(got) == len(want)


def test_medium_fp32_against_oracle(hip, medium):
    """fp32: encoder rows within F32_TOL, 16 greedy steps token-exact where the oracle's margin is clear, and B = 3 equals three
    B = 1 runs bit for bit (16 heads on the K/V-cache cross-attention, fc2 on the K = 4096 linear, 8-panel logits)."""
    cfg, w, mels, ref, runs = medium
    m = _model(cfg, w, max_batch=3)
    err = np.abs(m.encoder.forward(mels[0]) - ref.encode(mels[0])).max()
    print(f"medium dims fp32: encoder max |err| {err:.3g}")
    assert err < F32_TOL
    batch = m.transcribe_batch(mels[:3], prompt=PROMPT, eot=-1, max_loop=STEPS)
    for i in range(3):
        _assert_tokens(batch[i], runs[i][0], runs[i][1], len(PROMPT))
        alone = m.transcribe_batch(mels[i], prompt=PROMPT, eot=-1, max_loop=STEPS)[0]
        assert alone == batch[i]
    m.close()


def _forced_logits(m, mel, tokens):
    from whisper_mojo_amd.whisper import KVCache
    cache = KVCache(m, 1)
    m.encoder.forward(mel, cache)
    n = len(PROMPT)
    lg = [m.decoder.forward(list(tokens[:n]), None, cache, start_pos=0)]
    for i in range(n, len(tokens) - 1):
        lg.append(m.decoder.forward([int(tokens[i])], None, cache, start_pos=cache.current_len - 1))
    return np.stack([np.asarray(v).reshape(-1) for v in lg])


@pytest.mark.parametrize("name,kw,tol", [
    ("bf16 encoder + fp32 decoder", dict(compute_dtype=1, kv_dtype=0, decoder_fp32=True), 0.03),
    ("all bf16", dict(compute_dtype=1, kv_dtype=1), 0.06),
    ("all f16", dict(compute_dtype=2, kv_dtype=2), 0.008),
])
def test_medium_16bit_modes_within_tolerance(hip, medium, name, kw, tol):
    """Teacher-forced along the oracle's own greedy ids: every logit within the bar the tiny tests use for the same mode, top-1 equal
    where the oracle margin exceeds 4x that bar; at most 5 % of the positions may be left unasserted for a small margin."""
    cfg, w, mels, ref, runs = medium
    m = _model(cfg, w, max_batch=1, **kw)
    worst, clear_n, total = 0.0, 0, 0
    for i in range(4):
        tokens, logits = runs[i]
        lg = _forced_logits(m, mels[i], tokens)
        k = min(len(lg), len(logits))
        err = np.abs(lg[:k] - logits[:k]).max()
        worst = max(worst, err)
        s = np.sort(logits[:k], 1)
        clear = (s[:, -1] - s[:, -2]) > 4 * tol
        clear_n += int(clear.sum())
        total += k
        assert np.array_equal(lg[:k].argmax(1)[clear], logits[:k].argmax(1)[clear])
    print(f"medium dims {name}: max |logit error| {worst:.4f} (bar {tol}), top-1 asserted on {clear_n} of {total} positions")
    assert worst < tol
    assert clear_n >= 0.95 * total
    m.close()


def test_medium_score_reproduces_oracle_logprobs(hip, medium):
    """score() of the oracle's greedy ids: log p of every generated id within BAR = 1e-4 of log_softmax of the oracle's logits (the
    logit tolerance moves the target logit and the log-sum-exp by F32_TOL each: the bar return_logprobs is held to), and the arg-max
    ids are the ids themselves where the margin is clear.  Measured on MI355X: 6.1e-6."""
    cfg, w, mels, ref, runs = medium
    m = _model(cfg, w, max_batch=3)
    ids = [list(map(int, runs[i][0])) for i in range(3)]
    lps, (sums, avgs), tops = m.score(mels[:3], ids, context_len=len(PROMPT), return_top_ids=True)
    n = len(PROMPT)
    worst = 0.0
    for i in range(3):
        logits = runs[i][1].astype(np.float64)
        for t in range(n, len(ids[i])):
            z = logits[t - n]
            want = z[ids[i][t]] - (z.max() + np.log(np.exp(z - z.max()).sum()))
            worst = max(worst, abs(lps[i][t] - want))
            s = np.sort(z)
            if s[-1] - s[-2] > MARGIN_TOL:
                assert tops[i][t] == ids[i][t]
    print(f"medium dims score: max |log-prob error| {worst:.3g}")
    assert worst <= BAR
    m.close()


# ---- one pass of each kind at d = 1024, each held to the identity the project pins on micro / tiny -------------------------------

BAR = 1e-4  # tests/test_gpu_logprobs.py, test_gpu_no_speech.py, test_gpu_lang_detect.py: a log-prob is a logit minus a log-sum-exp,
            # each within the 5e-5 fp32 logits bar


def _log_softmax64(z):
    z = np.asarray(z, np.float64)
    return z - (z.max() + np.log(np.exp(z - z.max()).sum()))


def test_medium_per_row_prompts_equal_each_row_alone(hip, medium):
    """Per-row prompts of lengths 1 / 5 / 17 in one pass give, row by row, the ids of that row decoded alone with its own prompt."""
    cfg, w, mels, ref, runs = medium
    m = _model(cfg, w, max_batch=3)
    rng = np.random.default_rng(5)
    prompts = [rng.integers(1, cfg.vocab_size, n).tolist() for n in (1, 5, 17)]
    kw = dict(eot=-1, max_loop=12)
    both = m.transcribe_batch(mels[:3], prompts=prompts, **kw)
    for b in range(3):
        assert both[b][:len(prompts[b])] == prompts[b] and len(both[b]) == len(prompts[b]) + 13
        assert m.transcribe_batch(mels[b:b + 1], prompts=[prompts[b]], **kw)[0] == both[b], b
    m.close()


def test_medium_return_logprobs_against_oracle(hip, medium):
    """return_logprobs: ids equal the plain pass's; every generated id's log-prob within BAR of log_softmax of the oracle's logits
    wherever the streams agree; 0 on the prompt positions; avg_logprob is their mean."""
    cfg, w, mels, ref, runs = medium
    m = _model(cfg, w, max_batch=3)
    kw = dict(prompt=PROMPT, eot=-1, max_loop=STEPS)
    plain = m.transcribe_batch(mels[:3], **kw)
    ids, (lps, avg) = m.transcribe_batch(mels[:3], return_logprobs=True, **kw)
    assert ids == plain
    n, worst, checked = len(PROMPT), 0.0, 0
    for b in range(3):
        want, logits = runs[b]
        got = np.asarray(lps[b], np.float64)
        assert (got[:n] == 0).all()
        for t in range(n, len(ids[b])):
            if list(ids[b][:t + 1]) != list(want[:t + 1]):  # past a near-tie the oracle's logits belong to another stream
                break
            worst = max(worst, abs(got[t] - _log_softmax64(logits[t - n])[ids[b][t]]))
            checked += 1
        assert abs(float(avg[b]) - got[n:].mean()) <= 1e-6
    print(f"medium dims return_logprobs: max |logprob - oracle| {worst:.2e} over {checked} positions")
    assert checked >= 3 * STEPS and worst <= BAR
    m.close()


def test_medium_align_returns_the_timestamp_pass_own_times(hip, medium):
    """16 heads, cross-attention on the K/V cache: aligning a greedy timestamp pass's own ids with context_len = its prompt length
    returns that pass's own token times (tests/test_gpu_align.py's identity), heads from both layers, the last head included."""
    cfg, w, mels, ref, runs = medium
    for kwm in (dict(), dict(compute_dtype=1, kv_dtype=0, decoder_fp32=True)):
        m = _model(cfg, w, max_batch=3, **kwm)
        m.set_alignment_heads([(1, 0), (0, 15), (1, 9), (1, 15)])
        nf = np.asarray([2 * cfg.n_audio_ctx, 333, 200], np.int32)
        ids, times = m.transcribe_batch(mels[:3], prompt=PROMPT, eot=-1, max_loop=12, return_token_timestamps=True, n_frames=nf)
        assert all(len(t) == len(i) for t, i in zip(times, ids))
        assert any(x > 0 for t in times for x in t)
        own = m.align(mels[:3], ids, len(PROMPT), n_frames=nf)
        assert own == times
        again, (alps, (asm, aavg)) = m.align(mels[:3], ids, len(PROMPT), n_frames=nf, return_logprobs=True)  # rides the score sweep
        lps, (sm, avg) = m.score(mels[:3], ids, context_len=len(PROMPT))
        assert again == times and alps == lps
        np.testing.assert_array_equal(asm, sm)
        np.testing.assert_array_equal(aavg, avg)
        m.close()


def _sot_logits(ref, mel):
    return ref.teacher_forced(ref.encode(mel), [PROMPT[0], PROMPT[1]], n_prompt=1)[0].astype(np.float64)


def test_medium_no_speech_prob_against_oracle(hip, medium):
    """no_speech_prob = softmax of the oracle's raw logits at the [sot] position, read at the token: |Δ log| <= BAR."""
    cfg, w, mels, ref, runs = medium
    m = _model(cfg, w, max_batch=3)
    tok = 2500
    ids, (lps, avg, nsp) = m.transcribe_batch(mels[:3], prompt=PROMPT, eot=-1, max_loop=6, return_logprobs=True, no_speech_token=tok, n_init=len(PROMPT))
    assert ids == m.transcribe_batch(mels[:3], prompt=PROMPT, eot=-1, max_loop=6)
    for b in range(3):
        err = abs(np.log(float(nsp[b])) - _log_softmax64(_sot_logits(ref, mels[b]))[tok])
        print(f"medium dims no_speech row {b}: prob {nsp[b]:.4e}, |Δ log| {err:.2e}")
        assert err <= BAR
    m.close()


def test_medium_detect_language_against_oracle(hip, medium):
    """detect_language: the arg-max over the language ids of the oracle's logits at [sot] and their softmax within BAR; the
    in-pass form (transcribe_batch(detect_language=...)) returns the same ids and probabilities bit for bit."""
    cfg, w, mels, ref, runs = medium
    m = _model(cfg, w, max_batch=3)
    lang_ids = list(range(2600, 2699))
    lang, probs = m.detect_language(mels[:3], lang_ids, sot=PROMPT[0])
    for b in range(3):
        z = _sot_logits(ref, mels[b])[lang_ids]
        p = np.exp(z - z.max())
        p /= p.sum()
        s = np.sort(z)
        if s[-1] - s[-2] > MARGIN_TOL:
            assert lang[b] == lang_ids[int(np.argmax(z))]
        err = np.abs(probs[b] - p).max()
        print(f"medium dims detect_language row {b}: id {lang[b]}, max |prob - oracle| {err:.2e}")
        assert err <= BAR
    out, (lang2, probs2) = m.transcribe_batch(mels[:3], prompt=PROMPT, detect_language=lang_ids, eot=-1, max_loop=6)
    np.testing.assert_array_equal(lang2, lang)
    np.testing.assert_array_equal(probs2, probs)
    m.close()


def test_medium_long_form_equals_the_window_loop(hip, medium):
    """Utterances of 3, 2 and 1 windows (1000 / 500 / 150 frames, windows of 400): the library's loop equals the numpy window loop
    (tests/test_long_form.py's restate_long_form) over transcribe_batch, sequences and segment times alike."""
    from test_long_form import restate_long_form
    from whisper_mojo_amd import synth
    cfg, w, mels, ref, runs = medium
    m = _model(cfg, w, max_batch=3)
    W = cfg.n_frames
    lengths = [1000, 500, 150]
    longs = [synth.synth_long_mel(cfg, 70 + i, n) for i, n in enumerate(lengths)]
    tb, eot = 2790, 2789
    kw = dict(prompt=(1, 2, 3), eot=eot, max_loop=20, timestamps=(tb, 2788, 50))
    got = m.transcribe_long_form(longs, **kw)

    def decode(items):
        win = np.zeros((len(items), cfg.n_mels, W), np.float32)
        for r, (b, s, snf) in enumerate(items):
            win[r, :, :snf] = longs[b][:, s:s + snf]
        return [x[len(kw["prompt"]):] for x in m.transcribe_batch(win, **kw)]

    want, _ = restate_long_form(decode, lengths, W, tb, eot)
    assert len(got) == len(want)
    for b, (x, y) in enumerate(zip(got, want)):
        assert x["sequence"] == y["sequence"], b
        assert [(s["tokens"], s["start"], s["end"]) for s in x["segments"]] == [(s["tokens"], s["start"], s["end"]) for s in y["segments"]], b
    assert sum(len(r["sequence"]) for r in got) > 0
    m.close()


@pytest.mark.parametrize("kwm", [dict(), dict(compute_dtype=1, kv_dtype=0, decoder_fp32=True)], ids=["fp32", "headline"])
def test_medium_coalesced_pair_and_pipelined_submits(hip, medium, kwm):
    """coalesce = 2: two submits ride one state of twice the rows (the 32-row logits tiling in more row blocks) and return,
    bit for bit, the ids and log-probs of two uncoalesced submits; four pipelined submits return the synchronous call's ids, per-token
    log-probs and averages bit for bit."""
    cfg, w, mels, ref, runs = medium
    kw = dict(prompt=PROMPT, eot=-1, max_loop=STEPS, return_logprobs=True)
    batches = [mels[:2], mels[2:4]]
    m0 = _model(cfg, w, max_batch=2, **kwm)
    want = []
    for mb in batches:
        ids, (lps, avg) = m0.transcribe_batch(mb, **kw)
        want.append((ids, m0.last_logprobs.copy(), avg.copy()))
    for s in range(4):  # pipelined, uncoalesced
        m0.transcribe_submit(batches[s % 2], slot=s, **kw)
    for s in range(4):
        ids, (lps, avg) = m0.transcribe_wait(s)
        assert ids == want[s % 2][0]
        np.testing.assert_array_equal(m0.last_logprobs.view(np.uint32), want[s % 2][1].view(np.uint32))
        np.testing.assert_array_equal(avg.view(np.uint32), want[s % 2][2].view(np.uint32))
    m0.close()
    mc = _model(cfg, w, max_batch=2, coalesce=2, **kwm)
    for s in range(2):
        mc.transcribe_submit(batches[s], slot=s, **kw)
    for s in range(2):
        ids, (lps, avg) = mc.transcribe_wait(s)
        assert ids == want[s][0]
        np.testing.assert_array_equal(mc.last_logprobs.view(np.uint32), want[s][1].view(np.uint32))
        np.testing.assert_array_equal(avg.view(np.uint32), want[s][2].view(np.uint32))
    mc.close()


@pytest.mark.parametrize("dims,field", [((1024, 16, 3072), "ffn"), ((1024, 8, 4096), "n_heads"), ((1280, 20, 5120), "n_heads"),
                                        ((896, 14, 3584), "n_heads"), ((1024, 16, 2048), "ffn"), ((768, 16, 3072), "n_heads")])
def test_medium_neighbouring_shapes_stay_refused(hip, dims, field):
    """check_cfg accepts d_model 1024 with 16 heads and ffn 4096 and nothing near it: another ffn at 1024, 16 heads at another
    width, 8 heads at 1024, large (1280, 20) and 896 are refused at load, with the field named in the message."""
    from whisper_mojo_amd import WhisperConfig, _lib, synth
    d, h, ffn = dims
    cfg = WhisperConfig(d, h, 1, 1000, ffn, 16, 100, 64)
    with pytest.raises(_lib.WhisperMiError, match=field):
        _model(cfg, np.zeros(cfg.weight_count(), np.float32), max_batch=1)
