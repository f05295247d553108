"""GPU: token timestamps in long-form transcription (wm_transcribe_long_tt).  The definition under test: a kept id's time
is its window-relative float32 time, as the align chain of a 30 s timestamp pass produces it with num_input_ids = the row's own
decoder prompt length and num_frames = the window's real frames, plus float64(seek) * 0.02 / 2, summed in float64."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TS = (941, 940, 50)  # micro: timestamp_begin, <|notimestamps|>, max_initial_timestamp_index
KW = dict(prompt=(1, 2, 3), eot=900, max_loop=30, timestamps=TS)
HEADS = [(0, 1), (1, 0), (1, 1)]  # both layers
LENGTHS = [450, 300, 40]  # micro windows are 200 frames: 200 + 200 + 50, 200 + 100, one sub-window recording


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()
    return True


def make_model(cfg, weights, heads=HEADS, **kw):
    from whisper_mojo_amd import GELU_ERF, POS_HF
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, gelu_mode=GELU_ERF, pos_mode=POS_HF, **kw)
    m.load(WeightLoader.from_array(weights))
    if heads:
        m.set_alignment_heads(heads)
    return m


def precision(name):
    from whisper_mojo_amd import DT_BF16, DT_F32
    return {"fp32": dict(), "headline": dict(compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True), "bf16": dict(compute_dtype=DT_BF16)}[name]


def mels_of(cfg, lengths, seed0):
    from whisper_mojo_amd import synth
    return [synth.synth_long_mel(cfg, seed0 + b, n) for b, n in enumerate(lengths)]


def offset(seek):
    return np.float64(seek) * np.float64(0.02) / np.float64(2)


def window_loop(cfg, mels, lengths, kw, decode, lo=None):
    """The scheduler's loop on the host, one recording at a time.  decode(win [n_mels, W], snf, prompt) -> (generated ids with the eot
    when hit, their window-relative float32 times).  lo: prompt_ids / condition_on_prev_tokens options for wm_op_long_prompt.
    -> (results shaped like transcribe_long_form(return_token_timestamps=True), the decoded windows (b, seek, snf, prompt, ids))."""
    from whisper_mojo_amd import _lib as L
    W, tb, eot = cfg.n_frames, kw["timestamps"][0], kw["eot"]
    out, log = [], []
    for b, (mel, nf) in enumerate(zip(mels, lengths)):
        seq, segments, tt, seek = [], [], [], 0
        while seek < nf:
            snf = min(nf - seek, W)
            win = np.zeros((cfg.n_mels, W), np.float32)
            win[:, :snf] = mel[:, seek:seek + snf]
            prompt = list(kw["prompt"]) if lo is None else L.long_prompt([s["tokens"] for s in segments], kw["prompt"], tb, cfg.n_text_ctx, **lo)
            ids, rel = decode(win, snf, prompt)
            log.append((b, seek, snf, prompt, list(ids)))
            ids, rel = list(ids), np.asarray(rel, np.float32)
            if ids and ids[-1] == eot:
                ids = ids[:-1]
            segs, adv = L.long_segments(ids, tb, seek, snf)
            for first, count, start, end in segs:
                t = rel[first:first + count].astype(np.float64) + offset(seek)
                segments.append({"start": start, "end": end, "tokens": ids[first:first + count], "token_timestamps": t})
                seq += ids[first:first + count]
                tt.append(t)
            seek += adv if adv else snf
        out.append({"sequence": seq, "segments": segments, "token_times": np.concatenate(tt) if tt else np.zeros(0, np.float64)})
    return out, log


def batch_decoder(m, kw):
    """decode through the existing 30 s timestamp pass with the shared prompt"""
    def decode(win, snf, prompt):
        assert tuple(prompt) == tuple(kw["prompt"])
        ids, times = m.transcribe_batch(win[None], return_token_timestamps=True, n_frames=[snf], **kw)
        return ids[0][len(prompt):], times[0][len(prompt):]
    return decode


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def assert_same_tt(got, want, what=""):
    assert len(got) == len(want)
    for b, (x, y) in enumerate(zip(got, want)):
        assert sorted(x) == ["segments", "sequence", "token_times"], (what, b)
        assert x["sequence"] == y["sequence"], (what, b)
        assert isinstance(x["token_times"], np.ndarray) and x["token_times"].dtype == np.float64
        assert len(x["token_times"]) == len(x["sequence"]), (what, b)
        assert same_bits(x["token_times"], y["token_times"]), (what, b, x["token_times"], y["token_times"])
        assert len(x["segments"]) == len(y["segments"]), (what, b)
        first = 0
        for s, t in zip(x["segments"], y["segments"]):
            assert s["tokens"] == t["tokens"] and s["start"] == t["start"] and s["end"] == t["end"], (what, b)
            assert same_bits(s["token_timestamps"], t["token_timestamps"]), (what, b)
            assert same_bits(s["token_timestamps"], x["token_times"][first:first + len(s["tokens"])]), (what, b)
            first += len(s["tokens"])


def assert_times_sane(res, lengths):
    """not a table of zeros: some id of a later window lies behind its window's offset, and no time leaves its recording"""
    for r, n in zip(res, lengths):
        tt = r["token_times"]
        assert (tt >= 0).all() and (tt <= n * 0.01 + 1e-9).all()
    assert any((r["token_times"] > 2.0).any() for r in res)  # micro windows are 2 s long
    assert any(len(np.unique(r["token_times"])) > 2 for r in res)


# ---- 1 / 3: composition with the 30 s timestamp pass, shared prompt, both key kinds ---------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "headline", "bf16"])
def test_composition_shared_prompt_micro(hip, prec, micro_cfg, micro_weights):
    """fp32 and bf16 read the keys from the K/V cache (fp32 / bf16 key kinds), headline (bf16 encoder, fp32 decoder) runs the absorbed
    cross-attention and forms the keys with align_kh."""
    m = make_model(micro_cfg, micro_weights, max_batch=4, **precision(prec))
    mels = mels_of(micro_cfg, LENGTHS, 300)
    got, stats = m.transcribe_long_form(mels, return_token_timestamps=True, return_stats=True, **KW)
    want, log = window_loop(micro_cfg, mels, LENGTHS, KW, batch_decoder(m, KW))
    assert_same_tt(got, want, prec)
    assert stats["windows"] == len(log) == 6 and stats["row_passes"] == 0
    assert_times_sane(got, LENGTHS)
    plain = m.transcribe_long_form(mels, **KW)  # the flag changes no id and no segment
    assert [r["sequence"] for r in got] == [r["sequence"] for r in plain]
    assert [[(g["start"], g["end"], g["tokens"]) for g in r["segments"]] for r in got] == [[(g["start"], g["end"], g["tokens"]) for g in r["segments"]] for r in plain]
    m.close()


def test_composition_shared_prompt_tiny_two_layers(hip):
    """headline precision at d 384 (6 heads, absorbed path), 3000-frame windows that seek at timestamp pairs: ids behind the last pair
    of a window get no entry."""
    from oracle import oracle
    from whisper_mojo_amd import WhisperConfig
    cfg = WhisperConfig(384, 6, 2, 51865, 1536, 80, 1500, 448)
    w = oracle.synth_weights_c(cfg, 0)
    kw = dict(prompt=(50258, 50259, 50359), eot=50257, max_loop=24, timestamps=(50364, 50363, 50))
    lengths = [6700, 4400, 600]
    m = make_model(cfg, w, heads=[(0, 5), (1, 0), (1, 3)], max_batch=4, **precision("headline"))
    mels = mels_of(cfg, lengths, 310)
    got = m.transcribe_long_form(mels, return_token_timestamps=True, **kw)
    want, log = window_loop(cfg, mels, lengths, kw, batch_decoder(m, kw))
    assert_same_tt(got, want)
    m.close()


def test_kv_cache_kinds_at_twelve_heads(hip):
    """d 768, 12 heads, 1 layer, reduced context and vocabulary: the K/V-cache key kinds past 8 heads, head 11 selected."""
    from whisper_mojo_amd import WhisperConfig, synth
    cfg = WhisperConfig(768, 12, 1, 3000, 3072, 80, 200, 64)
    w = synth.synth_weights(cfg, 3)
    kw = dict(prompt=(1, 2, 3), eot=2900, max_loop=20, timestamps=(2941, 2940, 50))
    lengths = [900, 130]
    mels = mels_of(cfg, lengths, 320)
    for prec in ("fp32", "bf16"):  # the fp32 and the bf16 key kind (12 heads never take the absorbed path)
        m = make_model(cfg, w, heads=[(0, 11), (0, 0), (0, 5)], max_batch=2, **precision(prec))
        got = m.transcribe_long_form(mels, return_token_timestamps=True, **kw)
        want, log = window_loop(cfg, mels, lengths, kw, batch_decoder(m, kw))
        assert_same_tt(got, want, prec)
        m.close()


# ---- 2: per-row prompts against forced alignment of every window's own ids ------------------------------------------------------------
LO = dict(prompt_ids=[938, 11, 12, 13, 14], condition_on_prev_tokens=True, prev_sot_token=938)


@pytest.mark.parametrize("prec", ["fp32", "headline"])
def test_per_row_prompts_equal_align_of_each_window(hip, prec, micro_cfg, micro_weights):
    """condition_on_prev_tokens + 5 prompt ids: the rows of a pass carry prompts of different lengths.  Every window is decoded again
    alone with its own prompt (transcribe_batch(prompts=...): the ids must be the scheduler's) and its ids are aligned by the
    teacher-forced pass with context_len = the prompt's length: the same window-relative times, so the same token_times.
    Share of ids whose time differs: 0.
    Five recordings on passes of two rows: the fifth waits for a row, so it rides its first window (a prompt of 8 ids) beside another
    recording's second window (previous text in front), and from then on the rows of a pass are at different windows of their
    recordings.  A finishing launch that takes row 0's prompt length for every row fails here (mutation checks).  Known
    gap: with BOTH launches of the kernel mutated that way the tables and the read-back agree with each other, and since every
    window of the synthetic micro model runs to max_loop the row count clamps to max_loop either way, so that mutant passes."""
    kw = dict(KW, max_loop=24)
    lengths = [450, 300, 40, 610, 420]
    m = make_model(micro_cfg, micro_weights, max_batch=2, **precision(prec))
    mels = mels_of(micro_cfg, lengths, 330)
    got, stats = m.transcribe_long_form(mels, return_token_timestamps=True, return_stats=True, **LO, **kw)
    assert stats["row_passes"] >= 2

    def decode(win, snf, prompt):
        ids = m.transcribe_batch(win[None], prompts=[prompt], **{k: v for k, v in kw.items() if k != "prompt"})[0]
        assert ids[:len(prompt)] == prompt and len(ids) > len(prompt)
        times = m.align(win[None], [ids], context_len=len(prompt), n_frames=[snf])[0]
        assert all(t == 0 for t in times[:len(prompt)])
        return ids[len(prompt):], times[len(prompt):]

    want, log = window_loop(micro_cfg, mels, lengths, kw, decode, LO)
    assert len({len(p) for _b, _s, _n, p, _i in log}) >= 3  # prompts of several lengths were in play
    assert_same_tt(got, want, prec)
    assert_times_sane(got, lengths)
    m.close()


# ---- 4: two passes in flight, spare rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cond", [False, True])
def test_schedule_invariance_with_spare_rows(hip, cond, micro_cfg, micro_weights):
    """B = 5 on max_batch = 2: passes of 2 rows on two states in flight, an odd item count, spare rows that repeat a real item.
    Every recording must come back as it does alone, bit for bit."""
    kw = dict(KW, max_loop=24, **(LO if cond else {}))
    lengths = [450, 300, 40, 620, 210]
    m = make_model(micro_cfg, micro_weights, max_batch=2)
    mels = mels_of(micro_cfg, lengths, 340)
    got, stats = m.transcribe_long_form(mels, return_token_timestamps=True, return_stats=True, **kw)
    assert stats["rows"] == 2 * stats["passes"] and stats["rows"] > stats["windows"]  # spare rows were decoded
    alone = [m.transcribe_long_form([x], return_token_timestamps=True, **kw)[0] for x in mels]
    assert_same_tt(got, alone, cond)
    assert_times_sane(got, lengths)
    m.close()


# ---- 5: dropped ids, empty recordings, nothing from another window ---------------------------------------------------------------------
def test_empty_rows_and_no_value_from_an_earlier_call(hip, micro_cfg, micro_weights):
    """A first call with other audio leaves every buffer of both states full of its own times; the second call (a recording of 0
    frames, a 2-frame one, and suppress lists under which every window is one timestamp and the eot: one row of the chain, the least
    the timestamp rules allow a window to generate) must equal the window loop on a fresh model."""
    text_ids = [i for i in range(TS[0]) if i != KW["eot"]]
    kw2 = dict(KW, suppress_tokens=text_ids)
    lengths = [450, 0, 2, 300]
    mels = mels_of(micro_cfg, [450, 1, 2, 300], 350)
    m = make_model(micro_cfg, micro_weights, max_batch=2)
    first = m.transcribe_long_form(mels_of(micro_cfg, [600, 600, 600, 600], 360), return_token_timestamps=True, **KW)
    assert all((r["token_times"] > 0).any() for r in first)
    fresh = make_model(micro_cfg, micro_weights, max_batch=2)
    for kw in (KW, kw2):
        feats = np.zeros((4, micro_cfg.n_mels, 450), np.float32)
        for b, x in enumerate(mels):
            feats[b, :, :lengths[b]] = x[:, :lengths[b]]
        got = m.transcribe_long_form(feats, n_frames=lengths, return_token_timestamps=True, **kw)
        want, log = window_loop(micro_cfg, [feats[b] for b in range(4)], lengths, kw, batch_decoder(fresh, kw))
        assert_same_tt(got, want)
        assert got[1]["sequence"] == [] and got[1]["token_times"].shape == (0,) and got[1]["segments"] == []
        if kw is kw2:
            assert all(len(ids) == 2 and ids[1] == KW["eot"] for _b, _s, _n, _p, ids in log)
            assert [len(r["sequence"]) for r in got] == [3, 0, 1, 2]  # one kept id per window, the eot dropped
    m.close()
    fresh.close()


# ---- 6: language detection --------------------------------------------------------------------------------------------------------------
def test_detect_language_composes(hip, micro_cfg, micro_weights):
    lang_ids = [20, 7, 33, 12]
    m = make_model(micro_cfg, micro_weights, max_batch=2)
    mels = mels_of(micro_cfg, LENGTHS, 370)
    got, lang = m.transcribe_long_form(mels, return_token_timestamps=True, detect_language=lang_ids, **KW)
    plain, lang2 = m.transcribe_long_form(mels, detect_language=lang_ids, **KW)
    assert lang.tolist() == lang2.tolist() and all(int(v) in lang_ids for v in lang)
    assert [r["sequence"] for r in got] == [r["sequence"] for r in plain]
    for b, x in enumerate(mels):
        kw = dict(KW, prompt=(KW["prompt"][0], int(lang[b]), KW["prompt"][2]))
        want = m.transcribe_long_form([x], return_token_timestamps=True, **kw)
        assert_same_tt([got[b]], want, b)
    m.close()


# ---- 7: refusals and unchanged defaults -----------------------------------------------------------------------------------------------
def test_refusals_and_unchanged_defaults(hip, micro_cfg, micro_weights):
    from whisper_mojo_amd import _lib
    L = _lib.lib()
    m = make_model(micro_cfg, micro_weights, max_batch=2)
    mels = mels_of(micro_cfg, [450, 300], 380)
    win = np.stack([x[:, :200] for x in mels])
    before = m.transcribe_batch(win, **KW)
    steps = m.loop_steps()
    for th in (dict(logprob_threshold=-1.0), dict(logprob_threshold=-1.0, no_speech_threshold=0.6, no_speech_token=939)):
        with pytest.raises(ValueError):
            m.transcribe_long_form(mels, return_token_timestamps=True, **th, **KW)
        assert m.loop_steps() == steps
    # the library refuses the same combination itself (WM_E_ARG), and a result made without the flag has no times (WM_E_STATE)
    feats = np.zeros((2, micro_cfg.n_mels, 450), np.float32)
    feats[0], feats[1, :, :300] = mels[0], mels[1]
    nf = np.asarray([450, 300], np.int32)
    opts, _keep = m._opts(KW["prompt"], KW["eot"], KW["max_loop"], False, timestamps=TS)
    lo, _keep2 = _lib.long_opts(logprob_threshold=-1.0)
    ip = C.POINTER(C.c_int32)
    h = C.c_void_p()
    args = (m._h, C.c_void_p(feats.ctypes.data), 0, 2, 450, nf.ctypes.data_as(ip), C.byref(opts))
    assert L.wm_transcribe_long_tt(*args, C.byref(lo), None, 0, None, 1, C.byref(h)) == -1 and not h.value
    assert m.loop_steps() == steps
    lo0, _keep3 = _lib.long_opts()
    assert L.wm_transcribe_long_tt(*args, C.byref(lo0), None, 0, None, 0, C.byref(h)) == 0  # flag off: a plain run
    tt = np.zeros(64, np.float64)
    assert L.wm_long_result_token_times(h, 0, tt.ctypes.data_as(C.POINTER(C.c_double))) == -5
    plain_c, _st = _lib.long_result(h, 2)
    # the default returns exactly today's dicts
    plain = m.transcribe_long_form(mels, **KW)
    assert plain == plain_c and all(sorted(r) == ["segments", "sequence"] for r in plain)
    assert all(sorted(s) == ["end", "start", "tokens"] for r in plain for s in r["segments"])
    got = m.transcribe_long_form(mels, return_token_timestamps=True, **KW)
    assert all(sorted(s) == ["end", "start", "token_timestamps", "tokens"] for r in got for s in r["segments"])
    # a plain pass after timestamp long-form calls returns what it returned before
    assert m.transcribe_batch(win, **KW) == before
    assert m.transcribe_long_form(mels, **KW) == plain
    # no alignment heads: WM_E_STATE, from both layers
    m.set_alignment_heads([])
    with pytest.raises(_lib.WhisperMiError, match="error -5"):
        m.transcribe_long_form(mels, return_token_timestamps=True, **KW)
    assert L.wm_transcribe_long_tt(*args, C.byref(lo0), None, 0, None, 1, C.byref(h)) == -5
    assert m.transcribe_long_form(mels, **KW) == plain
    m.close()
