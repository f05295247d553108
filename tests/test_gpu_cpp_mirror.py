"""GPU: every public entry of the C++ host mirror (include/whisper_mi.hpp, class Whisper) against the Python host, bit for bit
(DESIGN §43).  tests/cpp/host_mirror_check.cpp runs one mode per child process on the micro model with the synthetic weights and
prints every result field as text — integers in decimal, floats and doubles as their bit patterns; each test here computes the same
thing in this process with whisper_mojo_amd.whisper.Whisper (or, where the Python host has no method of that shape, with the C
function through _lib.lib()), renders it with the same format and compares the lines.  Both hosts call the same library, the same
kernels and the same inputs, so there is no tolerance: ints equal, float patterns equal.

Each test also asserts, on the Python side, that its case is not vacuous.  Inputs: the ids the features' own micro tests use (prompt
1 2 3, eot 900, timestamps from 941, <|nospeech|> 939, <|startofprev|> 938, languages 20 7 33 12; the chunked vocabulary of
tests/test_gpu_chunked_ts.py: specials from 890, timestamps from 899) on the raw synthetic model (no suppress lists, the mirror has
none), mels of seeds 1000 + b.

A child that ends in any way other than a clean non-zero exit with a message (a signal, a time limit) stops the module: the tests
after it fail from the flag below without starting anything."""
import ctypes as C
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whisper.mojo_amd", "csrc")
_STOP = {"why": None}  # set once a child process died or hung: nothing further is launched

KW = dict(prompt=(1, 2, 3), eot=900)
TS = (941, 940, 50)
NO_SPEECH, PREV_SOT = 939, 938
HEADS = [(0, 1), (1, 0)]
LANGS = [20, 7, 33, 12]


@pytest.fixture(scope="module")
def exe():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not os.path.exists(os.path.join(CSRC, "libwhispermi.so")):
        pytest.skip("libwhispermi.so not built")
    out = os.path.join(ROOT, "tests", "cpp", "host_mirror_check")
    subprocess.check_call([shutil.which("g++") or shutil.which("c++"), "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_mirror_check.cpp"), "-o", out, "-L", CSRC, "-lwhispermi", "-Wl,-rpath," + CSRC])
    return out


def child(exe, mode):
    """the C++ program's lines for one mode"""
    if _STOP["why"]:
        pytest.fail("not started: " + _STOP["why"])
    try:
        r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _STOP["why"] = f"mode {mode} ran into its time limit"
        pytest.fail(_STOP["why"])
    if r.returncode != 0 and not (r.returncode in (1, 2) and r.stderr.strip()):
        _STOP["why"] = f"mode {mode} ended with status {r.returncode}: {r.stderr[-400:]}"
        pytest.fail(_STOP["why"])
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def model(max_batch):
    from whisper_mojo_amd import WhisperConfig, synth
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.micro()
    m = Whisper(cfg, max_batch=max_batch)
    m.load(WeightLoader.from_array(synth.synth_weights(cfg, 0)))
    return cfg, m


def mels(cfg, n, first=0):
    from whisper_mojo_amd import synth
    return np.stack([synth.synth_mel(cfg, 1000 + first + b) for b in range(n)])


def pcm_rows(B, stride):
    """[B, stride]: row b is the synthetic mel generator's stream of seed 1000 + b, scaled by 1 / 4"""
    from whisper_mojo_amd import synth
    shape = types.SimpleNamespace(n_mels=1, n_frames=stride)
    return np.stack([synth.synth_mel(shape, 1000 + b)[0] for b in range(B)]) * np.float32(0.25)


# ---- the program's line format ------------------------------------------------------------------------------------------------
def _line(name, toks):
    return f"{name} {len(toks)}" + "".join(" " + t for t in toks)


def I(name, v):
    return [_line(name, [str(int(x)) for x in np.asarray(v).ravel()])]


def F(name, v):
    a = np.ascontiguousarray(np.asarray(v, np.float32).ravel())
    return [_line(name, ["nan" if x != x else f"{b:08x}" for x, b in zip(a.tolist(), a.view(np.uint32).tolist())])]


def D(name, v):
    a = np.ascontiguousarray(np.asarray(v, np.float64).ravel())
    return [_line(name, ["nan" if x != x else f"{b:016x}" for x, b in zip(a.tolist(), a.view(np.uint64).tolist())])]


def rows(fmt, name, v):
    return [ln for r in v for ln in fmt(name, r)]


def same(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i}:\n  C++    {g}\n  Python {w}"
    assert len(got) == len(want), (len(got), len(want), (got + want)[min(len(got), len(want))])


def score_lines(tag, lps, sm, avg, top=()):
    return rows(F, tag + ".lp", lps) + F(tag + ".sum", sm) + F(tag + ".avg", avg) + rows(I, tag + ".top", top)


def lang_lines(tag, res):
    if len(res) == 2:
        ids, (lang, probs) = res
        lps, avg, nsp = [], [], []
    else:
        ids, (lps, avg, nsp), (lang, probs) = res
    return (rows(I, tag + ".ids", ids) + I(tag + ".lang", lang) + F(tag + ".probs", probs) + rows(F, tag + ".lp", lps) + F(tag + ".avg", avg) +
            F(tag + ".nsp", nsp))


def long_lines(tag, res):
    out = []
    for b, u in enumerate(res):
        p = f"{tag}.u{b}"
        out += I(p + ".seq", u["sequence"]) + I(p + ".nseg", [len(u["segments"])])
        for sg in u["segments"]:
            out += D(p + ".seg.span", [sg["start"], sg["end"]]) + I(p + ".seg.tokens", sg["tokens"])
            out += F(p + ".seg.quality", [sg.get("avg_logprob", 0.0), sg.get("no_speech_prob", 0.0)]) + D(p + ".seg.tt", sg.get("token_timestamps", []))
        wins = u.get("windows", [])
        out += I(p + ".nwin", [len(wins)])
        for w in wins:
            out += I(p + ".win.seek", [w["seek"], int(w["skipped"])]) + F(p + ".win.quality", [w["avg_logprob"], w["no_speech_prob"]])
        out += D(p + ".times", u.get("token_times", []))
    return out


# ---- one test per mode ----------------------------------------------------------------------------------------------------------
def test_slots(exe):
    """transcribe_submit on two slots (B 3 and 2, max_loop 9 and 11), transcribe_wait in the opposite order, transcribe_batch beside"""
    got = child(exe, "slots")
    cfg, m = model(3)
    a, b = mels(cfg, 3), mels(cfg, 2, 3)
    m.transcribe_submit(a, slot=0, max_loop=9, **KW)
    m.transcribe_submit(b, slot=1, max_loop=11, **KW)
    r1 = m.transcribe_wait(1)
    r0 = m.transcribe_wait(0)
    b0, b1 = m.transcribe_batch(a, max_loop=9, **KW), m.transcribe_batch(b, max_loop=11, **KW)
    m.close()
    assert len(r0) == 3 and len(r1) == 2 and all(x not in r0 for x in r1)  # the two slots hold different results
    assert r0 == b0 and r1 == b1
    same(got, rows(I, "wait1", r1) + rows(I, "wait0", r0) + rows(I, "batch0", b0) + rows(I, "batch1", b1))


def test_tt(exe):
    """set_alignment_heads + transcribe_batch_tt with the whole window and with ragged n_frames, then heads off and a plain decode"""
    got = child(exe, "tt")
    cfg, m = model(3)
    x = mels(cfg, 3)
    m.set_alignment_heads(HEADS)
    ids, t = m.transcribe_batch(x, max_loop=10, return_token_timestamps=True, **KW)
    ids2, t2 = m.transcribe_batch(x, max_loop=10, return_token_timestamps=True, n_frames=[200, 120, 60], **KW)
    m.set_alignment_heads([])
    plain = m.transcribe_batch(x, max_loop=10, **KW)
    m.close()
    assert any(v != 0 for r in t for v in r[3:])  # a generated id has a time
    assert any(p != q for r, s in zip(t, t2) for p, q in zip(r, s))  # the crop moves a time
    same(got, rows(I, "full.ids", ids) + rows(F, "full.times", t) + rows(I, "ragged.ids", ids2) + rows(F, "ragged.times", t2) + rows(I, "plain.ids", plain))


def test_lp_ns(exe):
    """transcribe_batch_lp_ns with the shared prompt and with per-row prompts of 2, 5 and 3 ids, n_init = 2"""
    got = child(exe, "lp_ns")
    cfg, m = model(3)
    x = mels(cfg, 3)
    ids, (lps, avg, nsp) = m.transcribe_batch(x, max_loop=9, return_logprobs=True, no_speech_token=NO_SPEECH, **KW)
    rid, (rlps, ravg, rnsp) = m.transcribe_batch(x, max_loop=9, return_logprobs=True, no_speech_token=NO_SPEECH, n_init=2,
                                                 prompts=[[1, 2], [11, 12, 13, 1, 2], [21, 1, 2]], **KW)
    m.close()
    assert len({len(r) for r in rid}) > 1  # rows of different n
    assert (nsp > 0).all() and len(set(rnsp.tolist())) == 3
    same(got, rows(I, "shared.ids", ids) + rows(F, "shared.lp", lps) + F("shared.avg", avg) + F("shared.nsp", nsp) + rows(I, "rows.ids", rid) +
         rows(F, "rows.lp", rlps) + F("rows.avg", ravg) + F("rows.nsp", rnsp))


SCORE_IDS = [[1, 2, 3, 40, 41, 42, 43], [1, 7], [1, 2, 3, 50, 51]]


def test_score(exe):
    """score on rows of 7, 2 (the minimum stride) and 5 ids, without and with context_len, with and without top ids"""
    got = child(exe, "score")
    cfg, m = model(3)
    x = mels(cfg, 3)
    lps, (sm, avg), top = m.score(x, SCORE_IDS, None, True)
    clps, (csm, cavg), ctop = m.score(x, SCORE_IDS, [3, 1, 3], True)
    nlps, (nsm, navg) = m.score(x, SCORE_IDS, [3, 1, 3])
    m.close()
    assert any(t != i for r, s in zip(top, SCORE_IDS) for t, i in zip(r[1:], s[1:]))  # the arg-max is not the scored id everywhere
    assert sm.tobytes() != csm.tobytes()  # the context changes the sums
    same(got, score_lines("plain", lps, sm, avg, top) + score_lines("ctx", clps, csm, cavg, ctop) + score_lines("notop", nlps, nsm, navg))


CANDIDATES = [[[1, 2, 3, 40, 41, 42], [1, 2, 3, 50], [1, 2, 3, 60, 61, 62, 63, 64]], [[1, 2, 3, 70, 71]]]


def test_nbest(exe):
    """score_candidates on two clips with 3 and 1 candidates of different lengths, per-row context_len, normalize off and on"""
    got = child(exe, "nbest")
    cfg, m = model(4)
    x = mels(cfg, 2)
    want, orders = [], []
    for normalize, tag in ((False, "sum"), (True, "norm")):
        res = m.score_candidates(x, CANDIDATES, context_len=[3, 3, 3, 2], normalize=normalize, return_top_ids=True)
        flat = lambda key: [r for d in res for r in d[key]]  # noqa: E731
        cat = lambda key: np.concatenate([np.asarray(d[key]) for d in res])  # noqa: E731
        want += score_lines(tag, flat("token_logprobs"), cat("sum_logprob"), cat("avg_logprob"), flat("top_ids"))
        want += I(tag + ".n_cand", [3, 1]) + I(tag + ".row0", [0, 3]) + I(tag + ".order", cat("order")) + I(tag + ".best", [d["best"] for d in res])
        want += F(tag + ".posterior", cat("posterior"))
        orders.append(res[0]["order"])
        assert any(t != i for d, c in zip(res, CANDIDATES) for r, s in zip(d["top_ids"], c) for t, i in zip(r[1:], s[1:]))
    m.close()
    assert any(o != [0, 1, 2] for o in orders), orders  # the ranking moves a candidate
    same(got, want)


def test_align(exe):
    """align without and with context_len and n_frames, with the score outputs and without"""
    got = child(exe, "align")
    cfg, m = model(3)
    x = mels(cfg, 3)
    ids = [[1, 2, 3, 40, 41, 42, 43], [1, 7, 8], [1, 2, 3, 50, 51]]
    m.set_alignment_heads(HEADS)
    t, (lps, (sm, avg)) = m.align(x, ids, return_logprobs=True)
    rt, (rlps, (rsm, ravg)) = m.align(x, ids, [3, 1, 3], [200, 120, 60], return_logprobs=True)
    nt = m.align(x, ids, [3, 1, 3], [200, 120, 60])
    m.close()
    assert any(v != 0 for r in t for v in r) and t != rt
    same(got, rows(F, "plain.times", t) + score_lines("plain", lps, sm, avg) + rows(F, "ragged.times", rt) + score_lines("ragged", rlps, rsm, ravg) +
         rows(F, "noscore.times", nt))


def test_lang(exe):
    """detect_language with probs; transcribe_batch_lang plain and with per-row prompts, log-probs and the no-speech probe; the same
    through transcribe_submit_lang / transcribe_wait_lang on two slots with lists of 4 and 5 languages, collected in reverse order"""
    got = child(exe, "lang")
    cfg, m = model(3)
    x, two = mels(cfg, 3), mels(cfg, 2, 3)
    dl, dp = m.detect_language(x, LANGS, sot=1)
    plain = m.transcribe_batch(x, detect_language=LANGS, max_loop=9, **KW)
    pr3, pr2 = [[1, 2, 3], [11, 12, 1, 2, 3], [21, 1, 2, 3]], [[31, 32, 33, 1, 2, 3], [1, 2, 3]]
    byrow = m.transcribe_batch(x, detect_language=LANGS, max_loop=9, prompts=pr3, n_init=3, return_logprobs=True, no_speech_token=NO_SPEECH, **KW)
    m.transcribe_submit(x, slot=0, detect_language=LANGS, max_loop=8, **KW)
    m.transcribe_submit(two, slot=1, detect_language=[7, 33, 12, 20, 45], max_loop=10, prompts=pr2, n_init=3, return_logprobs=True,
                        no_speech_token=NO_SPEECH, **KW)
    w1 = m.transcribe_wait(1)
    w0 = m.transcribe_wait(0)
    m.close()
    assert len(set(dl.tolist())) > 1 or len({dp[b].tobytes() for b in range(3)}) == 3  # not one language, or at least not one distribution
    assert [r[1] for r in plain[0]] == plain[1][0].tolist() and all(int(v) in LANGS for v in dl)
    same(got, I("detect.ids", dl) + F("detect.probs", dp) + lang_lines("plain", plain) + lang_lines("rows", byrow) + lang_lines("wait1", w1) +
         lang_lines("wait0", w0))


def test_long(exe):
    """set_timestamps + transcribe_long on three recordings of 500 mel frames (2.5 windows) with n_frames 500 / 330 / 40: defaults
    (ragged and whole), condition_on_prev_tokens + prompt_ids in both condition types, LongThresholds (log-prob alone; every window
    skipped; some skipped), lang_ids + lang_out, token_timestamps, and token_timestamps with conditioning and languages.
    The thresholds are inputs chosen for the raw micro model, not taken from tests/test_gpu_long_no_speech.py (whose fixture model has
    a planted <|nospeech|> row the C++ program cannot rebuild): every avg_logprob is below 0 and every no_speech_prob above 0, so
    (0, 0) skips all six windows; the windows' no_speech_prob lie in 0.000788 .. 0.000795, so (0, 0.00079) skips some of them."""
    from whisper_mojo_amd import synth
    got = child(exe, "long")
    cfg, m = model(3)
    x = np.stack([synth.synth_long_mel(cfg, 95 + b, 500) for b in range(3)])
    nf, pids = [500, 330, 40], [PREV_SOT, 11, 12, 13, 14]
    kw = dict(max_loop=12, timestamps=TS, return_stats=True, **KW)
    cond = dict(condition_on_prev_tokens=True, prompt_ids=pids, prev_sot_token=PREV_SOT)
    plain, st = m.transcribe_long_form(x, n_frames=nf, **kw)
    full, _ = m.transcribe_long_form(x, **kw)
    first, st_first = m.transcribe_long_form(x, n_frames=nf, prompt_condition_type="first-segment", **cond, **kw)
    every, st_all = m.transcribe_long_form(x, n_frames=nf, prompt_condition_type="all-segments", **cond, **kw)
    lpth, _ = m.transcribe_long_form(x, n_frames=nf, logprob_threshold=-1.0, no_speech_token=NO_SPEECH, **kw)
    skipall, st_skip = m.transcribe_long_form(x, n_frames=nf, logprob_threshold=0.0, no_speech_threshold=0.0, no_speech_token=NO_SPEECH, **kw)
    skipsome, st_some = m.transcribe_long_form(x, n_frames=nf, logprob_threshold=0.0, no_speech_threshold=0.00079, no_speech_token=NO_SPEECH, **kw)
    lang, _, lang_out = m.transcribe_long_form(x, n_frames=nf, detect_language=LANGS, **kw)
    m.set_alignment_heads(HEADS)
    tt, _ = m.transcribe_long_form(x, n_frames=nf, return_token_timestamps=True, **kw)
    ttlang, _, tt_out = m.transcribe_long_form(x, n_frames=nf, return_token_timestamps=True, detect_language=LANGS, **cond, **kw)
    m.close()
    print("long-form windows per utterance", [len(u["windows"]) for u in lpth], "no_speech_prob", [[w["no_speech_prob"] for w in u["windows"]] for u in lpth],
          "skipped", st_skip["skipped_windows"], st_some["skipped_windows"], "of", st_some["windows"])
    assert any(len(u["windows"]) >= 2 and len(u["segments"]) >= 2 for u in lpth)
    assert [u["sequence"] for u in lpth] == [u["sequence"] for u in plain]
    assert st_first["longest_prompt"] > st["longest_prompt"] and st_all["longest_prompt"] > st["longest_prompt"]
    assert st_skip["skipped_windows"] == st_skip["windows"] >= 5 and not any(u["segments"] for u in skipall)
    assert 1 <= st_some["skipped_windows"] < st_some["windows"]  # skipped windows beside kept ones in one result
    for u in tt:
        for sg in u["segments"]:
            assert (np.diff(sg["token_timestamps"]) >= 0).all()
    assert sum(len(u["token_times"]) for u in tt) > 0 and any(v > 0 for u in tt for v in u["token_times"])
    same(got, long_lines("plain", plain) + long_lines("full", full) + long_lines("first", first) + long_lines("all", every) + long_lines("lpth", lpth) +
         long_lines("skipall", skipall) + long_lines("skipsome", skipsome) + long_lines("lang", lang) + I("lang.out", lang_out) + long_lines("tt", tt) +
         long_lines("ttlang", ttlang) + I("ttlang.out", tt_out))


def test_resample(exe):
    """resample from float32 at 8 kHz (rows of 700 and 333 samples in a stride of 800) and from int16 at 44.1 kHz (1000 and 441 in
    1200).  The Python host packs rows to the longest, so the stride form is wm_resample_pcm called directly; frontend.resample on the
    rows alone must give the same bits."""
    from whisper_mojo_amd import _lib, frontend
    got = child(exe, "resample")
    cfg, m = model(2)
    ip = C.POINTER(C.c_int32)

    def direct(buf, dt, n, sr):
        n = np.asarray(n, np.int32)
        longest = max(1, max(_lib.resample_len(int(v), sr) for v in n))
        out, n_out = np.zeros((len(n), longest), np.float32), np.zeros(len(n), np.int32)
        _lib.check(_lib.lib().wm_resample_pcm(m._h, buf.ctypes.data_as(C.c_void_p), dt, 0, n.ctypes.data_as(ip), len(n), buf.shape[1], sr,
                                              out.ctypes.data_as(C.c_void_p), 0, longest, n_out.ctypes.data_as(ip)))
        return [out[b, :n_out[b]].copy() for b in range(len(n))]

    f = np.ascontiguousarray(pcm_rows(2, 800))
    q = np.ascontiguousarray((pcm_rows(2, 1200) * np.float32(32768.0)).astype(np.int16))
    rf, rq = direct(f, _lib.WM_F32, [700, 333], 8000), direct(q, _lib.WM_I16, [1000, 441], 44100)
    pf, pq = frontend.resample(m, [f[0, :700], f[1, :333]], 8000), frontend.resample(m, [q[0, :1000], q[1, :441]], 44100)
    m.close()
    assert [len(r) for r in rf] == [1400, 666] and [len(r) for r in rq] == [363, 160] and all(np.abs(r).max() > 0.01 for r in rf + rq)
    for a, b in zip(rf + rq, pf + pq):
        assert a.tobytes() == b.tobytes()
    same(got, rows(F, "f32", rf) + rows(F, "i16", rq))


def test_chunked(exe):
    """transcribe_chunked (with the chunks, with other strides, with a language list) and transcribe_chunked_ts (segments, then words)
    on two recordings of 70000 and 50000 samples, chunks of one micro window (32000 samples): three and two chunks"""
    from whisper_mojo_amd import _lib, frontend
    got = child(exe, "chunked")
    cfg, m = model(2)
    pcm = pcm_rows(2, 70000)
    audios, n = [pcm[0], pcm[1, :50000]], [70000, 50000]
    kw = dict(prompt=(891, 892, 893), eot=890, max_loop=10, first_special=890, no_repeat_ngram_size=2)

    def plain(tag, res, tab):
        out = []
        for r, u in enumerate(res):
            p = f"{tag}.r{r}"
            ch = u.get("chunks", [])
            out += I(p + ".seq", u["sequence"]) + I(p + ".nchunks", [len(ch)])
            for c, row in zip(ch, [t for t in tab.tolist() if t[0] == r]):
                out += I(p + ".chunk.at", row[1:5]) + I(p + ".chunk.ids", c[4])
        return out

    tab = _lib.chunk_table(n, 32000, 5333, 5333)
    chunks = frontend.transcribe_audio_chunked(m, audios, 2.0, None, return_chunks=True, **kw)
    merged = frontend.transcribe_audio_chunked(m, audios, 2.0, (0.25, 0.1875), **kw)
    lang = frontend.transcribe_audio_chunked(m, audios, 2.0, None, return_chunks=True, detect_language=[895, 894, 896], **kw)
    want = plain("chunks", chunks, tab) + plain("merged", merged, tab) + plain("lang", lang, tab)
    m.set_alignment_heads(HEADS)
    for mode, tag in ((True, "segs"), ("word", "word")):
        res = frontend.transcribe_audio_chunked(m, audios, 2.0, None, return_timestamps=mode, timestamps=(899, 898, 50), **kw)
        for r, u in enumerate(res):
            p = f"{tag}.r{r}"
            want += I(p + ".seq", u["sequence"]) + I(p + ".nseg", [len(u["segments"])])
            for sg in u["segments"]:
                want += D(p + ".seg.span", [np.nan if v is None else v for v in sg["timestamp"]]) + I(p + ".seg.tokens", sg["ids"])
                want += D(p + ".seg.pairs", [v for pr in sg.get("token_timestamps", []) for v in pr])
        assert sum(len(u["segments"]) for u in res) >= 2 and (mode is True or any(sg["token_timestamps"] for u in res for sg in u["segments"]))
    m.close()
    kept = [[sum(t < 890 for t in c[4]) for c in u["chunks"]] for u in chunks]
    print("chunked: ids below first_special per chunk", kept, "merged", [len(u["sequence"]) for u in chunks])
    assert [len(k) for k in kept] == [3, 2] and any(sum(v > 0 for v in k) >= 2 for k in kept)  # two chunks with ids were merged
    assert all(u["sequence"] for u in chunks) and all(c[4][1] in (895, 894, 896) for u in lang for c in u["chunks"])
    same(got, want)


def test_processors(exe):
    """set_repeat_options, set_sequence_bias (a one-id and a two-id sequence, one bad word), set_constraint + constraint_match and
    set_timestamps, each switched on, decoded with transcribe_batch_lp and switched off; the last plain decode repeats the first"""
    got = child(exe, "processors")
    cfg, m = model(3)
    x = mels(cfg, 3)
    kw = dict(max_loop=10, return_logprobs=True, **KW)
    runs = [("plain", m.transcribe_batch(x, **kw)),
            ("repeat", m.transcribe_batch(x, repetition_penalty=1.3, no_repeat_ngram_size=2, **kw)),
            ("bias", m.transcribe_batch(x, sequence_bias={(13,): 1.5, (3, 17): 2.0}, bad_words_ids=[[18]], **kw))]
    cid, clp, match = m.transcribe_batch(x, constraint=[[11, 12], [13], [14, 15, 16]], **kw)
    runs += [("constraint", (cid, clp)), ("timestamps", m.transcribe_batch(x, timestamps=TS, **kw)), ("again", m.transcribe_batch(x, **kw))]
    m.close()
    want = []
    for tag, (ids, (lps, avg)) in runs:
        want += rows(I, tag + ".ids", ids) + rows(F, tag + ".lp", lps) + F(tag + ".avg", avg)
        if tag == "constraint":
            want += I("constraint.match", match)
        if tag not in ("plain", "again"):  # the processor changed an id or a log-prob
            assert ids != runs[0][1][0] or any(np.asarray(a, np.float32).tobytes() != np.asarray(b, np.float32).tobytes()
                                               for a, b in zip(lps, runs[0][1][1][0])), tag
    assert (match >= 0).any()
    assert [ln.replace("again.", "plain.", 1) for ln in got if ln.startswith("again.")] == [ln for ln in got if ln.startswith("plain.")]
    same(got, want)
