"""End-to-end tests (-m gpu) of the top-k alternatives: transcribe_batch / transcribe_submit / transcribe_wait with
return_logprobs=True, top_k=k on the micro model (fp32, HF mode), against the float64 restatement of tests/test_topk_ref.py over the
raw logits of tests/golden/topk_micro_hf.npz.

Bars: ids at (position, rank) equal the restatement's wherever its score lies more than MARGIN_TOL (1e-3, the project's fp32 margin)
from both neighbouring ranks' — the fixture keeps the rest below 2 % of all pairs, asserted on the CPU by tests/test_topk_ref.py and
again here before any GPU work; log-probs within 1e-4 (tests/test_gpu_logprobs.py's bar: a difference of two quantities each within
the 5e-5 fp32 logits bar); rank 0 bit for bit the emitted id and its token log-prob."""
import ctypes as C

import numpy as np
import pytest

from test_topk_ref import MARGIN_TOL, SKIP_CAP, decidable, fixture_ts, load_fixture, restate_topk

pytestmark = pytest.mark.gpu
BAR = 1e-4


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()
    import whisper_mojo_amd as pkg
    return pkg


_REF = {}


def ref():
    """the fixture and its restatement at k = 8, computed once: (cfg, weights, z, rows); rows carry ref_ids / ref_lps / ref_gaps"""
    if not _REF:
        from whisper_mojo_amd import WhisperConfig, synth
        cfg = WhisperConfig.micro()
        z, rows = load_fixture()
        prompt = z["prompt"].tolist()
        pairs = skipped = 0
        for r in rows:
            ids, r["ref_ids"], r["ref_lps"], r["ref_gaps"] = restate_topk(r["raw"], prompt, 8, z["suppress"].tolist(), z["begin_suppress"].tolist(),
                                                                          fixture_ts(z, r["ts"]))
            assert ids == r["ids"][len(prompt):]
            fin = np.isfinite(r["ref_lps"])
            pairs += int(fin.sum())
            skipped += int((fin & ~decidable(r["ref_gaps"], MARGIN_TOL)).sum())
        assert skipped <= SKIP_CAP * pairs, (skipped, pairs)  # before any GPU work
        _REF["v"] = (cfg, synth.synth_weights(cfg, 0), z, rows)
    return _REF["v"]


def _model(cfg, w, max_batch=4, coalesce=0):
    from whisper_mojo_amd import GELU_ERF, POS_HF
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=max_batch, coalesce=coalesce)
    m.load(WeightLoader.from_array(w))
    return m


def _kw(z, ts_on):
    kw = dict(prompt=z["prompt"].tolist(), eot=int(z["eos"]), max_loop=int(z["max_loop"]), suppress_tokens=z["suppress"].tolist(),
              begin_suppress_tokens=z["begin_suppress"].tolist(), return_logprobs=True)
    if ts_on:
        kw["timestamps"] = (int(z["timestamp_begin"]), int(z["no_ts"]), int(z["max_init"]))
    return kw


def _mels(cfg, rows):
    from whisper_mojo_amd import synth
    return np.stack([synth.synth_mel(cfg, r["seed"]) for r in rows])


def _same(a, b):
    """two results of a top-k call, bit for bit"""
    ids_a, (lps_a, avg_a), (ti_a, tl_a) = a
    ids_b, (lps_b, avg_b), (ti_b, tl_b) = b
    assert ids_a == ids_b
    assert [np.asarray(v, np.float32).tobytes() for v in lps_a] == [np.asarray(v, np.float32).tobytes() for v in lps_b]
    assert avg_a.tobytes() == avg_b.tobytes()
    for x, y in zip(ti_a + tl_a, ti_b + tl_b):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("ts_on", [0, 1])
def test_topk_matches_the_restatement(hip, k, ts_on):
    cfg, w, z, rows = ref()
    rows = [r for r in rows if r["ts"] == ts_on]
    L = len(z["prompt"])
    m = _model(cfg, w)
    ids, (lps, avg), (top_ids, top_lps) = m.transcribe_batch(_mels(cfg, rows), top_k=k, **_kw(z, ts_on))
    worst = skipped = pairs = 0
    for b, r in enumerate(rows):
        assert ids[b] == r["ids"], b
        n = len(r["ids"]) - L
        assert top_ids[b].shape == (n, k) and top_lps[b].shape == (n, k) and top_ids[b].dtype == np.int32 and top_lps[b].dtype == np.float32
        np.testing.assert_array_equal(top_ids[b][:, 0], r["ids"][L:])  # rank 0: the emitted id, its stored log-prob bit for bit
        assert top_lps[b][:, 0].tobytes() == np.asarray(lps[b][L:], np.float32).tobytes()
        want_ids, want_lps, gaps = r["ref_ids"][:, :k], r["ref_lps"][:, :k], r["ref_gaps"][:, :k]
        fin = np.isfinite(want_lps)
        np.testing.assert_array_equal(np.isfinite(top_lps[b]), fin)
        assert (top_ids[b][~fin] == -1).all() and (top_lps[b][~fin] == -np.inf).all()
        d = decidable(r["ref_gaps"], MARGIN_TOL)[:, :k] & fin
        np.testing.assert_array_equal(top_ids[b][d], want_ids[d])
        pairs += int(fin.sum())
        skipped += int((fin & ~d).sum())
        worst = max(worst, np.abs(top_lps[b][fin].astype(np.float64) - want_lps[fin]).max())
    print(f"k {k} rules {'on' if ts_on else 'off'}: max |lp - restatement| {worst:.2e} (bar {BAR}); {skipped} of {pairs} id comparisons skipped")
    assert worst <= BAR
    m.close()


def test_batch_of_three_equals_three_single_runs(hip):
    cfg, w, z, rows = ref()
    mels = _mels(cfg, rows)[:3]
    m = _model(cfg, w)
    kw = _kw(z, 1)
    ids, (lps, avg), (ti, tl) = m.transcribe_batch(mels, top_k=8, **kw)
    for b in range(3):
        one = m.transcribe_batch(mels[b:b + 1], top_k=8, **kw)
        _same(one, ([ids[b]], ([lps[b]], avg[b:b + 1]), ([ti[b]], [tl[b]])))
    m.close()


@pytest.mark.parametrize("coalesce", [0, 2])
def test_pipelined_and_coalesced_equal_the_synchronous_call(hip, coalesce):
    """Four submits in flight (coalesce = 2: two pairs on 2·B-row states), collected in another order, return the synchronous call's
    ids, log-probs and top-k tables bit for bit."""
    cfg, w, z, rows = ref()
    mels = _mels(cfg, rows)
    kw = _kw(z, 1)
    batches = [mels[:3], mels[[2, 1, 0]].copy(), mels[[1, 3, 0]].copy(), mels[1:4]]
    m = _model(cfg, w, 4, coalesce)
    want = [m.transcribe_batch(mb, top_k=5, **kw) for mb in batches]
    for s, mb in enumerate(batches):
        m.transcribe_submit(mb, slot=s, top_k=5, **kw)
    for s in (1, 0, 3, 2):
        _same(m.transcribe_wait(s), want[s])
    m.close()


def test_with_every_processor(hip):
    """repetition_penalty, no_repeat_ngram_size, sequence_bias, bad_words_ids and the timestamp rules together: a banned id appears at
    no rank of any position, and the first generated position — whose raw logits the fixture holds whatever the processors choose
    later — lists exactly what the restatement lists: the biased id at its new rank."""
    cfg, w, z, rows = ref()
    rows = [r for r in rows if r["ts"] == 1]
    prompt = z["prompt"].tolist()
    m = _model(cfg, w)
    for r in rows:
        base = r["ref_ids"][0]
        banned, biased = int(base[1]), int(base[5])
        extra = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, sequence_bias={(biased,): 3.0}, bad_words_ids=[[banned]])
        ids, _, (ti, tl) = m.transcribe_batch(_mels(cfg, [r]), top_k=8, **extra, **_kw(z, 1))
        assert not (ti[0] == banned).any()
        want = restate_topk(r["raw"], prompt, 8, z["suppress"].tolist(), z["begin_suppress"].tolist(), fixture_ts(z, 1), penalty=1.3, ngram=2,
                            sequence_bias=[((biased,), 3.0)], bad_words=[[banned]], eos=int(z["eos"]), steps=1)
        d = decidable(want[3], MARGIN_TOL)[0]
        np.testing.assert_array_equal(ti[0][0][d], want[1][0][d])
        assert list(want[1][0]).index(biased) < 5 and banned not in want[1][0]  # the restatement itself: the bias moved it up
        assert np.abs(tl[0][0].astype(np.float64) - want[2][0]).max() <= BAR
    m.close()


def test_finished_row_stores_nothing_and_off_means_off(hip):
    """A row that reaches eot early has no entries past its length and its neighbour is what it is alone; without top_k the ids and
    log-probs are bit for bit those of the top-k call."""
    cfg, w, z, rows = ref()
    rows = [r for r in rows if r["ts"] == 0]
    L = len(z["prompt"])
    kw = dict(_kw(z, 0), no_repeat_ngram_size=1)  # every id of a row is new (the synthetic model alone repeats one id)
    m = _model(cfg, w)
    mels = _mels(cfg, rows)
    kw["eot"] = -1  # never emitted: both rows run the whole loop
    full_ids, (full_lps, _), (full_ti, full_tl) = m.transcribe_batch(mels, top_k=8, **kw)
    g0, g1 = full_ids[0][L:], full_ids[1][L:]
    assert len(set(g0)) == len(g0) == len(g1)
    j = next(i for i in range(2, len(g0)) if g0[i] not in g1)  # an id row 0 emits at step j and row 1 never
    kw["eot"] = g0[j]  # the rules are off, so eot is nothing but the stop id: row 0 stops after j + 1 ids
    ids, (lps, avg), (ti, tl) = m.transcribe_batch(mels, top_k=8, **kw)
    assert len(ids[0]) == L + j + 1 and ti[0].shape == (j + 1, 8) and tl[0].shape == (j + 1, 8)
    assert ids[0] == full_ids[0][:L + j + 1] and ti[0].tobytes() == full_ti[0][:j + 1].tobytes() and tl[0].tobytes() == full_tl[0][:j + 1].tobytes()
    assert ids[1] == full_ids[1] and ti[1].tobytes() == full_ti[1].tobytes() and tl[1].tobytes() == full_tl[1].tobytes()
    assert not (ti[1] == -1).any()
    for row in range(2):  # no_repeat_ngram_size = 1: nothing of a row's history comes back at any rank
        for i in range(ti[row].shape[0]):
            assert not np.isin(ti[row][i], ids[row][:L + i]).any()
    alone = m.transcribe_batch(mels[1:], top_k=8, **kw)
    _same(alone, ([ids[1]], ([lps[1]], avg[1:]), ([ti[1]], [tl[1]])))
    off_ids, (off_lps, off_avg) = m.transcribe_batch(mels, **kw)
    assert off_ids == ids and off_avg.tobytes() == avg.tobytes()
    assert [np.asarray(v, np.float32).tobytes() for v in off_lps] == [np.asarray(v, np.float32).tobytes() for v in lps]
    m.close()


def test_refusals(hip):
    from whisper_mojo_amd import _lib
    cfg, w, z, rows = ref()
    m = _model(cfg, w)
    L = _lib.lib()
    mels = _mels(cfg, rows[:1])
    for bad in (9, 0, -1):
        with pytest.raises(ValueError):
            m.transcribe_batch(mels, top_k=bad, **_kw(z, 0))
    kw = _kw(z, 0)
    kw["return_logprobs"] = False
    with pytest.raises(ValueError, match="return_logprobs"):
        m.transcribe_batch(mels, top_k=3, **kw)
    assert L.wm_set_top_k(m._h, 9) != 0 and b"top_k" in L.wm_last_error()
    ids = np.zeros((1, 64, 3), np.int32)
    lps = np.zeros((1, 64, 3), np.float32)
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    assert L.wm_transcribe_top_k(m._h, 0, ids.ctypes.data_as(ip), lps.ctypes.data_as(fp)) != 0  # no top-k pass was collected on the slot
    m.transcribe_batch(mels, **_kw(z, 0))
    assert L.wm_transcribe_top_k(m._h, 0, ids.ctypes.data_as(ip), lps.ctypes.data_as(fp)) != 0  # a log-prob pass without top_k leaves none
    # the long-form and chunked entries refuse to run while the setting is on
    _lib.check(L.wm_set_top_k(m._h, 3))
    opts, keep = m._opts(z["prompt"].tolist(), int(z["eos"]), 4, False, (), (), (int(z["timestamp_begin"]), int(z["no_ts"]), int(z["max_init"])))
    h = C.c_void_p()
    long_mel = np.zeros((1, cfg.n_mels, cfg.n_frames), np.float32)
    assert L.wm_transcribe_long(m._h, long_mel.ctypes.data_as(C.c_void_p), 0, 1, cfg.n_frames, None, C.byref(opts), C.byref(h)) != 0
    assert b"long-form" in L.wm_last_error()
    pcm = np.zeros((1, 16000), np.float32)
    n, merged, mlen = np.array([16000], np.int32), np.zeros((1, 64), np.int32), np.zeros(1, np.int32)
    rc = L.wm_transcribe_chunked(m._h, pcm.ctypes.data_as(C.c_void_p), 0, n.ctypes.data_as(ip), 1, 16000, 8000, 1000, 1000, C.byref(opts), None, 0,
                                 int(z["eos"]), merged.ctypes.data_as(ip), mlen.ctypes.data_as(ip), 64, None, None, None)
    assert rc != 0 and b"chunked" in L.wm_last_error()
    _lib.check(L.wm_set_top_k(m._h, 0))
    m.close()


def _rank0_at_own_offset(ids, lps, top_ids, top_lps, plens):
    """rank 0 of every generated position is the emitted id with its stored log-prob, at each row's own prompt offset"""
    for b, L in enumerate(plens):
        assert top_ids[b].shape[0] == len(ids[b]) - L
        np.testing.assert_array_equal(top_ids[b][:, 0], ids[b][L:])
        assert top_lps[b][:, 0].tobytes() == np.asarray(lps[b][L:], np.float32).tobytes()
        assert (np.asarray(lps[b][:L]) == 0).all()


def _close_to(tag, got, want):
    """two top-k results of one row from two code paths of the library (key-window prefill against the shared-prompt one): the ids
    are equal wherever the reference path's own log-probs lie more than MARGIN_TOL from both neighbouring ranks', every log-prob
    within BAR"""
    (gi, gl), (wi, wl) = got, want
    assert gi.shape == wi.shape
    with np.errstate(invalid="ignore"):
        gap = -np.diff(wl.astype(np.float64), axis=1)
    gaps = np.concatenate([gap, np.full((gap.shape[0], 1), np.inf)], 1)
    fin = np.isfinite(wl)
    np.testing.assert_array_equal(np.isfinite(gl), fin, err_msg=tag)
    with np.errstate(invalid="ignore"):
        d = decidable(gaps, MARGIN_TOL) & fin
    np.testing.assert_array_equal(gi[d], wi[d], err_msg=tag)
    np.testing.assert_array_equal(gi[~fin], wi[~fin], err_msg=tag)  # (-1 where nothing finite is left; rank 0 of such a step: id 0)
    assert np.abs(gl[fin].astype(np.float64) - wl[fin]).max() <= BAR, tag


@pytest.mark.parametrize("ts_on", [0, 1])
def test_ragged_per_row_prompts(hip, ts_on):
    """prompts= of lengths 4, 1, 9 and 6 with top_k: the key-window prefill ends in its own selection launch under the begin mask, and
    the tables are cut at each row's own prompt length.  Bit for bit three single-row per-row-prompt passes; against the shared-prompt
    pass of each row alone the ids of the decidable ranks and every log-prob (1e-4); without top_k the same ids and log-probs."""
    cfg, w, z, rows = ref()
    P = z["prompt"].tolist()
    prompts = [P, P[:1], [11, 12, 13, 14, 15] + P, [21, 22] + P]
    plens = [len(p) for p in prompts]
    mels = _mels(cfg, rows)
    kw = _kw(z, ts_on)
    del kw["prompt"]
    m = _model(cfg, w)
    ids, (lps, avg), (ti, tl) = m.transcribe_batch(mels, prompts=prompts, top_k=8, **kw)
    assert [i[:L] for i, L in zip(ids, plens)] == prompts
    _rank0_at_own_offset(ids, lps, ti, tl, plens)
    off_ids, (off_lps, off_avg) = m.transcribe_batch(mels, prompts=prompts, **kw)
    assert off_ids == ids and off_avg.tobytes() == avg.tobytes()
    assert [np.asarray(v, np.float32).tobytes() for v in off_lps] == [np.asarray(v, np.float32).tobytes() for v in lps]
    for b in range(4):
        one = m.transcribe_batch(mels[b:b + 1], prompts=prompts[b:b + 1], top_k=8, **kw)
        _same(one, ([ids[b]], ([lps[b]], avg[b:b + 1]), ([ti[b]], [tl[b]])))
        sid, _, (si, sl) = m.transcribe_batch(mels[b:b + 1], prompt=prompts[b], top_k=8, **kw)
        assert sid[0] == ids[b]
        _close_to(f"row {b}", (ti[b], tl[b]), (si[0], sl[0]))
    # the pipelined form returns the same tables
    m.transcribe_submit(mels, slot=2, prompts=prompts, top_k=8, **kw)
    _same(m.transcribe_wait(2), (ids, (lps, avg), (ti, tl)))
    m.close()


def test_detect_language_with_top_k(hip):
    """detect_language= with top_k: the tables come last, behind the language result, and are those of a shared-prompt pass whose
    second id is the detected language; with per-row prompts beside it likewise, at each row's own offset."""
    cfg, w, z, rows = ref()
    P = z["prompt"].tolist()
    lang_ids = [40, 7, 300, 41, 555]
    mels = _mels(cfg, rows)[:3]
    kw = _kw(z, 1)
    del kw["prompt"]
    m = _model(cfg, w)
    ids, (lps, avg), (lang, probs), (ti, tl) = m.transcribe_batch(mels, prompt=P, detect_language=lang_ids, top_k=5, **kw)
    assert all(int(v) in lang_ids for v in lang) and [i[1] for i in ids] == [int(v) for v in lang]
    _rank0_at_own_offset(ids, lps, ti, tl, [len(P)] * 3)
    off = m.transcribe_batch(mels, prompt=P, detect_language=lang_ids, **kw)
    assert off[0] == ids and off[1][1].tobytes() == avg.tobytes() and off[2][0].tolist() == lang.tolist()
    for b in range(3):
        sid, _, (si, sl) = m.transcribe_batch(mels[b:b + 1], prompt=[P[0], int(lang[b])] + P[2:], top_k=5, **kw)
        assert sid[0] == ids[b]
        _close_to(f"lang row {b}", (ti[b], tl[b]), (si[0], sl[0]))
    prompts = [P, [9, 8, 7] + P, [5] + P]
    rid, (rlps, ravg), (rlang, _), (rti, rtl) = m.transcribe_batch(mels, prompts=prompts, n_init=len(P), detect_language=lang_ids, top_k=5, **kw)
    assert rlang.tolist() == lang.tolist()
    _rank0_at_own_offset(rid, rlps, rti, rtl, [len(p) for p in prompts])
    assert rid[0] == ids[0] and rti[0].tobytes() == ti[0].tobytes() and rtl[0].tobytes() == tl[0].tobytes()  # row 0: the same prompt, the same path
    m.transcribe_submit(mels, slot=1, prompt=P, detect_language=lang_ids, top_k=5, **kw)
    wid, (wlps, wavg), (wlang, _), (wti, wtl) = m.transcribe_wait(1)
    _same((wid, (wlps, wavg), (wti, wtl)), (ids, (lps, avg), (ti, tl)))
    m.close()


def test_transcribe_audio_passes_top_k_through(hip):
    """frontend.transcribe_audio(..., return_logprobs=True, top_k=k) is transcribe_batch on the GPU-made log-mel of the samples"""
    from whisper_mojo_amd import frontend
    cfg, w, z, rows = ref()
    m = _model(cfg, w)
    r = np.random.default_rng(3)
    audios = [(0.1 * r.standard_normal(n)).astype(np.float32) for n in (16000, 9000)]
    P = z["prompt"].tolist()
    got = frontend.transcribe_audio(m, audios, prompt=P, eot=int(z["eos"]), max_loop=6, return_logprobs=True, top_k=3)
    want = m.transcribe_batch(frontend.log_mel(m, audios), prompt=P, eot=int(z["eos"]), max_loop=6, return_logprobs=True, top_k=3)
    _same(got, want)
    assert got[2][0][0].shape[1] == 3 and len(frontend.transcribe_audio(m, audios, prompt=P, eot=int(z["eos"]), max_loop=6, return_logprobs=True)) == 2
    m.close()


@pytest.mark.parametrize("per_row", [False, True])
def test_cpp_host_top_k_equals_python(hip, per_row):
    """include/whisper_mi.hpp: Whisper::set_top_k + transcribe_batch_lp + top_k (tests/cpp/topk_check.cpp) return the Python host's
    ids and tables bit for bit, with the shared prompt and with per-row prompts (the table stride of a per-row pass is the longest
    prompt's, which is what both hosts pass as prompt_stride)."""
    import os
    import shutil
    import subprocess
    from whisper_mojo_amd import WhisperConfig, synth
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cpp", "topk_check")
    csrc = os.path.join(root, "whisper.mojo_amd", "csrc")
    subprocess.check_call([shutil.which("g++") or shutil.which("c++"), "-std=c++17", "-Wall", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "topk_check.cpp"), "-o", exe, "-L", csrc, "-lwhispermi", "-Wl,-rpath," + csrc])
    out = subprocess.run([exe, "5", "9"] + (["rows"] if per_row else []), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    cfg = WhisperConfig.micro()
    m = Whisper(cfg, max_batch=2)
    m.load(WeightLoader.from_array(synth.synth_weights(cfg, 0)))
    mels = np.stack([synth.synth_mel(cfg, 1000 + b) for b in range(2)])
    kw = dict(prompts=[[1, 2, 3, 4], [2, 3]]) if per_row else dict(prompt=(1, 2, 3, 4))
    ids, _, (ti, tl) = m.transcribe_batch(mels, eot=-1, max_loop=9, return_logprobs=True, top_k=5, **kw)
    for b in range(2):
        assert [int(t) for t in lines[2 * b].split()[1:]] == ids[b]
        pairs = [t.split(":") for t in lines[2 * b + 1].split()[1:]]
        assert [int(a) for a, _ in pairs] == ti[b].ravel().tolist()
        assert [int(h, 16) for _, h in pairs] == tl[b].ravel().view(np.uint32).tolist()
    m.close()
