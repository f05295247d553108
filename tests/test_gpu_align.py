"""End-to-end tests (-m gpu) of forced alignment: wm_align / wm_align_submit / wm_align_wait / wm_align_pcm.

Exact equality with HF throughout, as tests/test_gpu_token_timestamps.py: the fixtures keep only inputs whose DTW path survives 1e-5
relative noise on the attentions (tools/make_golden_token_timestamps.py, tools/make_golden_align.py), the fp32 models' probabilities
are within 1e-6 of HF's.  Not covered here: the multi-lane refusal.  It is score_check's own line (shared by wm_score and wm_align),
and a multi-lane decode state exists only in the developer build (WM_DEC_LANES), which the suite does not load."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from test_token_timestamps import restate_times

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -5


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()
    return True


def make_model(cfg, weights, hf_mode=True, **kw):
    from whisper_mojo_amd import GELU_ERF, GELU_TANH, POS_HF, POS_REF
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, gelu_mode=GELU_ERF if hf_mode else GELU_TANH, pos_mode=POS_HF if hf_mode else POS_REF, **kw)
    m.load(WeightLoader.from_array(weights))
    return m


def _cfg_w(name, micro_cfg, micro_weights, tiny_cfg, tiny_weights):
    return (micro_cfg, micro_weights) if name == "micro" else (tiny_cfg, tiny_weights)


def _mels(cfg, seeds):
    from whisper_mojo_amd import synth
    return np.stack([synth.synth_mel(cfg, int(s)) for s in seeds])


def _f32(rows):
    return [np.asarray(r, np.float32) for r in rows]


# ---- 3. the greedy timestamp fixtures need no new reference ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["micro", "tiny"])
@pytest.mark.parametrize("mode", ["hf", "ref"])
def test_align_reproduces_greedy_timestamp_fixtures(hip, name, mode, micro_cfg, micro_weights, tiny_cfg, tiny_weights):
    cfg, w = _cfg_w(name, micro_cfg, micro_weights, tiny_cfg, tiny_weights)
    g = golden(f"token_timestamps_{name}_{mode}")
    mels = _mels(cfg, [g[f"c{c}_mel_seed"] for c in range(3)])
    heads = [tuple(p) for p in g["heads"]]
    m = make_model(cfg, w, hf_mode=mode == "hf", max_batch=3)
    m.set_alignment_heads(heads)
    ids = [g[f"c{c}_ids"].tolist() for c in range(3)]
    nf = g["n_frames"]
    assert len(g["prompt"]) == 4
    for fr, key in ((None, "full"), (nf, "full_nf")):
        times = m.align(mels, ids, context_len=4, n_frames=fr)
        if name == "micro":
            W = m.alignment_weights()
            assert W.shape == (3, len(heads), int(g["max_loop"]), cfg.n_audio_ctx)
        for c in range(3):
            if name == "micro":
                d = np.abs(W[c] - g[f"c{c}_probs"]).max()
                print(f"{name} {mode} clip {c} {key}: max |probs - HF| {d:.2e}")
                assert d <= 1e-6
            np.testing.assert_array_equal(np.asarray(times[c], np.float32), g[f"c{c}_times_{key}"], err_msg=f"clip {c} {key}")
    # one ragged batch: the uncut ids of clip 0, the ids cut at the shared eot of clips 1 and 2
    cut = [ids[c][:int(g[f"c{c}_n_cut"])] for c in range(3)]
    times = m.align(mels, [ids[0], cut[1], cut[2]], context_len=4)
    np.testing.assert_array_equal(np.asarray(times[0], np.float32), g["c0_times_full"])
    for c in (1, 2):
        np.testing.assert_array_equal(np.asarray(times[c], np.float32), g[f"c{c}_times_cut"], err_msg=f"clip {c} cut")
    m.close()


# ---- 4. the align fixtures ---------------------------------------------------------------------------------------------------------
CASES = ["ctx1", "ctx4", "prev_text", "other_clip", "random", "rows0", "rows1", "in16", "in17", "in33"]


def _fixture(name):
    g = golden(f"align_{name}_hf")
    names = [str(n) for n in g["names"]]
    rows = [dict(case=n, seed=int(g[n + "_seed"]), ids=g[n + "_ids"].tolist(), ctx=int(g[n + "_context_len"]), nf=int(g[n + "_n_frames"]),
                 times=g[n + "_times"], times_nf=g[n + "_times_nf"], probs=g[n + "_probs"] if name == "micro" else None) for n in names]
    return g, rows


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_align_matches_hf_fixture(hip, name, micro_cfg, micro_weights, tiny_cfg, tiny_weights):
    cfg, w = _cfg_w(name, micro_cfg, micro_weights, tiny_cfg, tiny_weights)
    g, rows = _fixture(name)
    assert [r["case"] for r in rows] == CASES + (["len448"] if name == "tiny" else [])  # every case present, nothing skipped
    lens = {r["case"]: len(r["ids"]) for r in rows}
    assert (lens["in16"], lens["in17"], lens["in33"]) == (17, 18, 34)
    assert lens["rows0"] == 5 and lens["rows1"] == 6 and rows[0]["ctx"] == 1 and rows[2]["ctx"] == 30
    if name == "tiny":
        assert lens["len448"] == 448 and rows[-1]["ctx"] == 4
    B = len(rows)
    m = make_model(cfg, w, max_batch=B)
    m.set_alignment_heads([tuple(p) for p in g["heads"]])
    mels = _mels(cfg, [r["seed"] for r in rows])
    ids, ctx, nf = [r["ids"] for r in rows], [r["ctx"] for r in rows], [r["nf"] for r in rows]
    batch = {}
    for fr, key in ((None, "times"), (nf, "times_nf")):
        got = _f32(m.align(mels, ids, ctx, n_frames=fr))
        batch[key] = got
        if name == "micro":
            W = m.alignment_weights()
        for b, r in enumerate(rows):
            if name == "micro":
                R = len(r["ids"]) - r["ctx"] - 1
                d = np.abs(W[b][:, :R] - r["probs"]).max() if R else 0.0
                print(f"{name} {r['case']} {key}: max |probs - HF| {d:.2e}")
                assert d <= 1e-6 and not W[b][:, R:].any()
            assert got[b].shape == (len(r["ids"]),)
            np.testing.assert_array_equal(got[b], r[key], err_msg=f"{name} {r['case']} {key}")
    # every row alone, bitwise
    for b, r in enumerate(rows):
        one = _f32(m.align(mels[b:b + 1], [ids[b]], [ctx[b]], n_frames=[nf[b]]))
        np.testing.assert_array_equal(one[0], batch["times_nf"][b], err_msg=f"{name} {r['case']} alone")
    # the batch in reversed order
    rev = _f32(m.align(mels[::-1], ids[::-1], ctx[::-1], n_frames=nf[::-1]))
    for b in range(B):
        np.testing.assert_array_equal(rev[B - 1 - b], batch["times_nf"][b], err_msg=f"{name} {rows[b]['case']} reversed")
    m.close()


# ---- 5. log-probs from the same pass ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos_hf", [True, False])
def test_align_logprobs_are_scores(hip, pos_hf, micro_cfg, micro_weights):
    g, rows = _fixture("micro")
    m = make_model(micro_cfg, micro_weights, hf_mode=pos_hf, max_batch=len(rows))
    m.set_alignment_heads([tuple(p) for p in g["heads"]])
    mels = _mels(micro_cfg, [r["seed"] for r in rows])
    ids, ctx = [r["ids"] for r in rows], [r["ctx"] for r in rows]
    lps, (sm, avg) = m.score(mels, ids, ctx)
    plain = m.align(mels, ids, ctx)
    times, (alps, (asm, aavg)) = m.align(mels, ids, ctx, return_logprobs=True)
    assert times == plain and alps == lps
    np.testing.assert_array_equal(asm, sm)
    np.testing.assert_array_equal(aavg, avg)
    assert m.score(mels, ids, ctx)[0] == lps  # and a score after an align
    m.close()


# ---- 6. 16-bit and absorbed-path configurations -----------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["f32", "bf16enc_f32kv", "bf16", "base_f16"])
def test_align_restatement_on_own_weights(hip, config, tiny_cfg, tiny_weights):
    from test_gpu_token_timestamps import CONFIGS
    from whisper_mojo_amd import WhisperConfig, synth
    dims, kw = CONFIGS[config]
    if dims == "tiny":
        cfg, w = tiny_cfg, tiny_weights
    else:
        cfg = WhisperConfig.base()
        w = synth.synth_weights(cfg, 0)
    mels = _mels(cfg, (1000, 1001, 1017))
    m = make_model(cfg, w, hf_mode=False, max_batch=3, **kw)
    m.set_alignment_heads([(cfg.n_layers - 1, 0), (1, cfg.n_heads - 1), (cfg.n_layers - 1, 2)])
    rng = np.random.default_rng(11)
    ids = [rng.integers(0, cfg.vocab_size, n).tolist() for n in (30, 19, 6)]
    ctx = [4, 1, 5]  # the last row has no row at all
    nf = np.asarray([2 * cfg.n_audio_ctx, 1777, 901], np.int32)
    times = m.align(mels, ids, ctx, n_frames=nf)
    W = m.alignment_weights()
    assert W.shape[2] == 25
    for c in range(3):
        R = len(ids[c]) - ctx[c] - 1
        ref = restate_times(W[c][:, :R, :int(nf[c]) // 2], ctx[c])
        np.testing.assert_array_equal(np.asarray(times[c], np.float32), ref, err_msg=f"{config} row {c}")
    m.close()


# ---- 7. hygiene ------------------------------------------------------------------------------------------------------------------
def _hygiene_inputs(cfg):
    g, rows = _fixture("micro")
    rows = rows[:4]
    return g, _mels(cfg, [r["seed"] for r in rows]), [r["ids"] for r in rows], [r["ctx"] for r in rows], [r["nf"] for r in rows], rows


def test_align_and_greedy_timestamps_do_not_disturb_each_other(hip, micro_cfg, micro_weights):
    g, mels, ids, ctx, nf, rows = _hygiene_inputs(micro_cfg)
    heads = [tuple(p) for p in g["heads"]]
    kw = dict(prompt=(1, 2, 3, 4), eot=-1, max_loop=20, return_token_timestamps=True, n_frames=nf)
    fresh = make_model(micro_cfg, micro_weights, max_batch=4)
    fresh.set_alignment_heads(heads)
    want_tt = fresh.transcribe_batch(mels, **kw)
    fresh.close()
    m = make_model(micro_cfg, micro_weights, max_batch=4)
    m.set_alignment_heads(heads)
    a0 = m.align(mels, ids, ctx, n_frames=nf)  # an align on a fresh model
    for b, r in enumerate(rows):
        np.testing.assert_array_equal(np.asarray(a0[b], np.float32), r["times_nf"])
    assert m.transcribe_batch(mels, **kw) == want_tt  # a greedy timestamp pass after an align
    assert m.align(mels, ids, ctx, n_frames=nf) == a0  # an align after a greedy timestamp pass
    assert m.transcribe_batch(mels, **kw) == want_tt  # and the captured step graph again
    # aligning the greedy pass's own ids with context_len = its prompt length returns its own times
    own = m.align(mels, want_tt[0], 4, n_frames=nf)
    assert own == want_tt[1]
    m.close()


def test_align_submit_wait_four_in_flight(hip, micro_cfg, micro_weights):
    g, mels, ids, ctx, nf, rows = _hygiene_inputs(micro_cfg)
    m = make_model(micro_cfg, micro_weights, max_batch=4, coalesce=2)
    m.set_alignment_heads([tuple(p) for p in g["heads"]])
    want = m.align(mels, ids, ctx, n_frames=nf, return_logprobs=True)
    kw = dict(prompt=[1, 2, 3], eot=900, max_loop=10)
    want_t = m.transcribe_batch(mels, **kw)
    m.transcribe_submit(mels, slot=7, **kw)  # coalesce = 2: held for a partner, which an align submit never is
    for k in range(4):
        m.align_submit(mels[k:], ids[k:], slot=k, context_len=ctx[k:], n_frames=nf[k:], return_logprobs=k % 2 == 0)
    for k in (2, 0, 3, 1):
        got = m.align_wait(k)
        times, sc = got if k % 2 == 0 else (got, None)
        assert times == want[0][k:]
        if sc is not None:
            assert sc[0] == want[1][0][k:]
            np.testing.assert_array_equal(sc[1][0], want[1][1][0][k:])
        W = m.alignment_weights(k)
        assert W.shape[0] == 4 - k
    assert m.transcribe_wait(7) == want_t
    m.close()


def test_align_wait_families_and_errors(hip, micro_cfg, micro_weights):
    from whisper_mojo_amd import _lib
    g, mels, ids, ctx, nf, rows = _hygiene_inputs(micro_cfg)
    mels = np.ascontiguousarray(mels, np.float32)
    L = _lib.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    f, i = (lambda a: a.ctypes.data_as(fp)), (lambda a: a.ctypes.data_as(ip))
    m = make_model(micro_cfg, micro_weights, max_batch=4)
    with pytest.raises(_lib.WhisperMiError, match=r"error -5\b.*alignment heads"):  # WM_E_STATE, align_cols' message
        m.align(mels, ids, ctx)
    with pytest.raises(_lib.WhisperMiError, match=r"error -5\b"):
        m.align_submit(mels, ids, slot=2, context_len=ctx)
    assert 2 not in m._align_pending
    m.set_alignment_heads([tuple(p) for p in g["heads"]])
    want = m.align(mels, ids, ctx)
    stride = 64
    tt, lps, top = np.zeros((4, stride), np.float32), np.zeros((4, stride), np.float32), np.zeros((4, stride), np.int32)
    sm, avg = np.zeros(4, np.float32), np.zeros(4, np.float32)
    toks, n = np.zeros((4, stride), np.int32), np.zeros(4, np.int32)
    # an align slot: the transcribe and score waits refuse it, wm_align_wait refuses log-probs it did not compute; then it is collected
    m.align_submit(mels, ids, slot=3, context_len=ctx)
    assert L.wm_transcribe_wait(m._h, 3, i(toks), i(n)) == E_STATE
    assert L.wm_transcribe_wait_tt(m._h, 3, i(toks), i(n), f(tt)) == E_STATE
    assert L.wm_score_wait(m._h, 3, f(lps), i(top), f(sm), f(avg)) == E_STATE
    assert L.wm_align_wait(m._h, 3, f(tt), f(lps), f(sm), f(avg)) == E_STATE
    with pytest.raises(_lib.WhisperMiError):
        m.score_wait(3)
    # refused calls while the slot is pending leave it untouched: bad n_frames length / value, an id out of range, a bad context
    with pytest.raises(ValueError):
        m.align_submit(mels, ids, slot=3, context_len=ctx, n_frames=[100, 100])
    with pytest.raises(ValueError):
        m.align(mels, ids, ctx, n_frames=[1, 100, 100, 100])
    with pytest.raises(ValueError):
        m.align(mels, [ids[0], ids[1], ids[2], ids[3][:-1] + [micro_cfg.vocab_size]], ctx)
    with pytest.raises(ValueError):
        m.align(mels, ids, [1, 1, 1, len(ids[3])])
    with pytest.raises(_lib.WhisperMiError, match=r"error -5\b"):  # the slot still holds a pass
        m.align_submit(mels, ids, slot=3, context_len=ctx)
    assert m.align_wait(3) == want
    # the library's own refusals, before anything is launched
    tab = np.zeros((4, stride), np.int32)
    for b, r in enumerate(ids):
        tab[b, :len(r)] = r
    lens, cx = np.asarray([len(r) for r in ids], np.int32), np.asarray(ctx, np.int32)
    call = lambda tab=tab, nfr=None, B=4, lp=None: L.wm_align(m._h, mels.ctypes.data_as(C.c_void_p), 0, B, m.pos_mode, i(tab), i(lens), stride, i(cx),
                                                                None if nfr is None else i(np.asarray(nfr, np.int32)), f(tt), lp, None, None)
    assert call() == 0
    for b in range(4):
        assert tt[b, :lens[b]].tolist() == want[b] and not tt[b, lens[b]:].any()
    assert call(nfr=[100, 100, 1, 100]) == E_ARG
    assert call(nfr=[100, 100, 201, 100]) == E_ARG
    bad = tab.copy()
    bad[2, 1] = micro_cfg.vocab_size
    assert call(tab=bad) == E_ARG
    assert call(lp=f(lps)) == E_ARG  # the three log-prob outputs go together
    big = make_model(micro_cfg, micro_weights, max_batch=2)
    big.set_alignment_heads([(0, 0)])
    assert L.wm_align(big._h, mels.ctypes.data_as(C.c_void_p), 0, 4, 1, i(tab), i(lens), stride, i(cx), None, f(tt), None, None, None) == E_ARG
    big.close()
    # a score slot and a transcribe slot refuse wm_align_wait, and are collected by their own calls
    m.score_submit(mels, ids, slot=1, context_len=ctx)
    assert L.wm_align_wait(m._h, 1, f(tt), None, None, None) == E_STATE
    with pytest.raises(_lib.WhisperMiError):
        m.align_wait(1)
    m.score_wait(1)
    m.transcribe_submit(mels, slot=1, prompt=[1, 2, 3], eot=900, max_loop=4)
    assert L.wm_align_wait(m._h, 1, f(tt), None, None, None) == E_STATE
    m.transcribe_wait(1)
    assert L.wm_align_wait(m._h, 1, f(tt), None, None, None) == E_STATE  # nothing pending
    m.set_alignment_heads([])
    with pytest.raises(_lib.WhisperMiError, match=r"error -5\b"):
        m.align(mels, ids, ctx)
    m.close()


def test_align_audio_equals_align_on_log_mel(hip, micro_cfg, micro_weights):
    from whisper_mojo_amd import frontend
    m = make_model(micro_cfg, micro_weights, max_batch=2)
    m.set_alignment_heads([(1, 0), (0, 1)])
    r = np.random.default_rng(3)
    audios = [r.standard_normal(16000).astype(np.float32) * 0.1, r.standard_normal(9000).astype(np.float32) * 0.1]
    ids = [[1, 2, 3, 40, 41, 42, 43, 44, 900], [1, 2, 3, 77, 78, 79]]
    nf = [min(2 * micro_cfg.n_audio_ctx, -(-len(a) // 160)) for a in audios]
    a = frontend.align_audio(m, audios, ids, context_len=3, return_logprobs=True)
    b = m.align(frontend.log_mel(m, audios), ids, context_len=3, n_frames=nf, return_logprobs=True)
    assert a[0] == b[0] and a[1][0] == b[1][0]
    m.close()
