"""End-to-end tests (-m gpu) of wm_transcribe_lp_ns / wm_transcribe_submit_lp_ns / wm_transcribe_wait_lp_ns against the HF
fixtures of tools/make_golden_no_speech.py: fp32 models, micro and tiny.

Bar: |log no_speech_prob - log HF's| <= 1e-4, the tolerance tests/test_gpu_logprobs.py holds log-probs to (a log-probability is the
difference of a logit and a logsumexp, each within the project's 5e-5 fp32 logits bar); the token log-probs and avg_logprob keep it."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
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


_CACHE = {}


def setup(name):
    if name not in _CACHE:
        from whisper_mojo_amd import WhisperConfig, synth
        cfg = WhisperConfig.micro() if name == "micro" else WhisperConfig.tiny()
        z = np.load(os.path.join(GOLDEN, f"no_speech_{name}_hf.npz"))
        rows = []
        for i in range(int(z["s_rows"])):
            k = f"s{i}_"
            rows.append(dict(case=str(z[k + "case"]), seed=int(z[k + "seed"]), prompt=z[k + "prompt"].tolist(), ids=z[k + "ids"].tolist(),
                             lps=z[k + "logprobs"], avg=float(z[k + "avg_logprob"]), nsp=float(z[k + "no_speech_prob"])))
        _CACHE[name] = (cfg, synth.synth_weights(cfg, 0), z, rows)
    return _CACHE[name]


def _kw(z):
    return dict(eot=int(z["eos"]), max_loop=int(z["s_max_loop"]), suppress_tokens=z["s_suppress"].tolist(),
                begin_suppress_tokens=z["s_begin_suppress"].tolist(), timestamps=(int(z["timestamp_begin"]), int(z["no_ts"]), int(z["s_max_init"])))


def _mels(cfg, rows):
    from whisper_mojo_amd import synth
    return np.stack([synth.synth_mel(cfg, r["seed"]) for r in rows])


def _model(cfg, w, max_batch, coalesce=0, dtype=0):
    """HF mode (erf GELU, HF positions), as the fixtures were generated"""
    from whisper_mojo_amd import GELU_ERF, POS_HF
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, compute_dtype=dtype, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=max_batch, coalesce=coalesce)
    m.load(WeightLoader.from_array(w))
    return m


def _check(tag, rows, ids, lps, avg, nsp):
    for b, r in enumerate(rows):
        assert ids[b] == r["ids"], (tag, b)
        L = len(r["prompt"])
        err = np.abs(np.asarray(lps[b], np.float64)[L:] - r["lps"].astype(np.float64)).max()
        aerr = abs(float(avg[b]) - r["avg"])
        nerr = abs(np.log(float(nsp[b])) - np.log(r["nsp"]))
        print(f"{tag} row {b} (prompt {L}): no_speech_prob {nsp[b]:.6e} (HF {r['nsp']:.6e}), |Δ log| {nerr:.2e}; max |logprob - HF| {err:.2e}, "
              f"|avg - HF| {aerr:.2e}")
        assert nerr <= BAR and err <= BAR and aerr <= BAR, (tag, b, nerr, err, aerr)


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_shared_prompt_matches_hf_and_equals_lp_pass(hip, name):
    cfg, w, z, rows = setup(name)
    rows = [r for r in rows if r["case"] == "shared"]
    tok = int(z["no_speech_token"])
    m = _model(cfg, w, max_batch=4)
    kw = dict(prompt=rows[0]["prompt"], return_logprobs=True, **_kw(z))
    ids, (lps, avg, nsp) = m.transcribe_batch(_mels(cfg, rows), no_speech_token=tok, **kw)
    tab = m.last_logprobs.copy()
    _check(f"{name} shared", rows, ids, lps, avg, nsp)
    # ids, token log-probs and avg_logprob are bit for bit the _lp pass's; n_init defaults to the shared prompt's length
    ids2, (lps2, avg2) = m.transcribe_batch(_mels(cfg, rows), **kw)
    assert ids2 == ids
    np.testing.assert_array_equal(m.last_logprobs.view(np.uint32), tab.view(np.uint32))
    np.testing.assert_array_equal(avg2.view(np.uint32), avg.view(np.uint32))
    _, (_, _, nsp3) = m.transcribe_batch(_mels(cfg, rows), no_speech_token=tok, n_init=len(rows[0]["prompt"]), **kw)
    np.testing.assert_array_equal(nsp3.view(np.uint32), nsp.view(np.uint32))
    m.close()


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_per_row_prompts_match_hf(hip, name):
    """One ragged pass: prefixes of 0 .. 30 ids in front of the 3 initial ids; the longest row's <|startoftranscript|> slot (30 of 33)
    lies in the second of three 16-position prefill chunks, not the last."""
    cfg, w, z, rows = setup(name)
    rows = [r for r in rows if r["case"] == "rows"]
    n_init = len(z["init"])
    Lmax = max(len(r["prompt"]) for r in rows)
    assert (Lmax - n_init) // 16 < (Lmax - 1) // 16
    tok = int(z["no_speech_token"])
    m = _model(cfg, w, max_batch=4)
    kw = dict(prompts=[r["prompt"] for r in rows], return_logprobs=True, **_kw(z))
    ids, (lps, avg, nsp) = m.transcribe_batch(_mels(cfg, rows), no_speech_token=tok, n_init=n_init, **kw)
    tab = m.last_logprobs.copy()
    _check(f"{name} rows", rows, ids, lps, avg, nsp)
    ids2, (lps2, avg2) = m.transcribe_batch(_mels(cfg, rows), **kw)
    assert ids2 == ids
    np.testing.assert_array_equal(m.last_logprobs.view(np.uint32), tab.view(np.uint32))
    np.testing.assert_array_equal(avg2.view(np.uint32), avg.view(np.uint32))
    # a row alone gives the value it has in the ragged pass, bitwise
    for b in (0, len(rows) - 1):
        _, (_, _, one) = m.transcribe_batch(_mels(cfg, rows[b:b + 1]), prompts=[rows[b]["prompt"]], return_logprobs=True, no_speech_token=tok,
                                            n_init=n_init, **_kw(z))
        assert one.view(np.uint32)[0] == nsp.view(np.uint32)[b]
    m.close()


@pytest.mark.parametrize("coalesce", [0, 2])
def test_pipelined_and_coalesced_are_bitwise_the_synchronous_call(hip, coalesce):
    cfg, w, z, rows = setup("micro")
    rows = [r for r in rows if r["case"] == "shared"]
    tok = int(z["no_speech_token"])
    kw = dict(prompt=rows[0]["prompt"], return_logprobs=True, no_speech_token=tok, **_kw(z))
    mels = _mels(cfg, rows)
    batches = [mels, mels[::-1].copy(), mels[[1, 0, 2]].copy(), mels]
    m = _model(cfg, w, 4, coalesce)
    want = []
    for mb in batches:
        ids, (lps, avg, nsp) = m.transcribe_batch(mb, **kw)
        want.append((ids, m.last_logprobs.copy(), avg.copy(), nsp.copy()))
    for s, mb in enumerate(batches):
        m.transcribe_submit(mb, slot=s, **kw)
    for s in range(4):
        ids, (lps, avg, nsp) = m.transcribe_wait(s)
        assert ids == want[s][0]
        np.testing.assert_array_equal(m.last_logprobs.view(np.uint32), want[s][1].view(np.uint32))
        np.testing.assert_array_equal(avg.view(np.uint32), want[s][2].view(np.uint32))
        np.testing.assert_array_equal(nsp.view(np.uint32), want[s][3].view(np.uint32))
    if coalesce == 2:  # a probe submit pairs neither with an _lp submit nor with another token: each runs alone, with its own result
        kw_lp = dict(kw)
        del kw_lp["no_speech_token"]
        m.transcribe_submit(mels, slot=0, **kw_lp)
        m.transcribe_submit(mels, slot=1, **kw)
        m.transcribe_submit(mels, slot=2, **dict(kw, no_speech_token=tok - 1))
        ids1, (_, _, nsp1) = m.transcribe_wait(1)
        ids0, (_, avg0) = m.transcribe_wait(0)
        ids2, (_, _, nsp2) = m.transcribe_wait(2)
        assert ids0 == ids1 == ids2 == want[0][0]
        np.testing.assert_array_equal(nsp1.view(np.uint32), want[0][3].view(np.uint32))
        np.testing.assert_array_equal(avg0.view(np.uint32), want[0][2].view(np.uint32))
        assert (nsp2 != nsp1).any()
    m.close()


def test_alternating_passes_on_one_slot(hip):
    """probe / plain / _lp passes in turn on the same state: every pass returns what it returns alone"""
    cfg, w, z, rows = setup("tiny")
    rows = [r for r in rows if r["case"] == "shared"]
    tok = int(z["no_speech_token"])
    base = dict(prompt=rows[0]["prompt"], **_kw(z))
    mels = _mels(cfg, rows)
    m = _model(cfg, w, max_batch=4)
    plain = m.transcribe_batch(mels, **base)
    ids, (lps, avg, nsp) = m.transcribe_batch(mels, return_logprobs=True, no_speech_token=tok, **base)
    assert ids == plain == [r["ids"] for r in rows]
    for _ in range(2):
        assert m.transcribe_batch(mels, **base) == plain
        ids_lp, (lps_lp, avg_lp) = m.transcribe_batch(mels, return_logprobs=True, **base)
        assert ids_lp == ids and lps_lp == lps
        ids2, (lps2, avg2, nsp2) = m.transcribe_batch(mels, return_logprobs=True, no_speech_token=tok, **base)
        assert ids2 == ids and lps2 == lps
        np.testing.assert_array_equal(nsp2.view(np.uint32), nsp.view(np.uint32))
    m.close()


def test_refusals_launch_nothing(hip):
    from whisper_mojo_amd import _lib
    cfg, w, z, rows = setup("micro")
    rows = [r for r in rows if r["case"] == "shared"]
    tok = int(z["no_speech_token"])
    kw = _kw(z)
    mels = _mels(cfg, rows)
    m = _model(cfg, w, max_batch=4)
    want = m.transcribe_batch(mels, prompt=rows[0]["prompt"], return_logprobs=True, no_speech_token=tok, **kw)
    steps = m.loop_steps(0)
    L = _lib.lib()
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    B = len(rows)
    p = rows[0]["prompt"]
    opts, _keep = m._opts(p, kw["eot"], kw["max_loop"], False, kw["suppress_tokens"], kw["begin_suppress_tokens"], kw["timestamps"])
    total = len(p) + 1 + kw["max_loop"]
    toks, n = np.zeros((B, total), np.int32), np.zeros(B, np.int32)
    lps, avg, nsp = np.zeros((B, total), np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32)
    out = (toks.ctypes.data_as(ip), n.ctypes.data_as(ip), lps.ctypes.data_as(fp), avg.ctypes.data_as(fp), nsp.ctypes.data_as(fp))
    args = (m._h, C.c_void_p(mels.ctypes.data), 0, B, C.byref(opts))
    tab, lens = np.tile(np.asarray([7] + p, np.int32), (B, 1)), np.full(B, len(p) + 1, np.int32)
    lens[1] = 2
    E_ARG, E_STATE = -1, -5
    assert L.wm_transcribe_lp_ns(*args, None, None, 0, -1, len(p), *out) == E_ARG                 # token outside the vocabulary
    assert L.wm_transcribe_lp_ns(*args, None, None, 0, cfg.vocab_size, len(p), *out) == E_ARG
    assert L.wm_transcribe_lp_ns(*args, None, None, 0, tok, 0, *out) == E_ARG                     # n_init < 1
    assert L.wm_transcribe_lp_ns(*args, None, None, 0, tok, len(p) + 1, *out) == E_ARG            # larger than the shared prompt
    assert L.wm_transcribe_lp_ns(*args, tab.ctypes.data_as(ip), lens.ctypes.data_as(ip), tab.shape[1], tok, 3, *out) == E_ARG  # than row 1's
    assert L.wm_transcribe_lp_ns(*args, None, None, 0, tok, len(p), *out[:4], None) == E_ARG
    assert L.wm_transcribe_submit_lp_ns(m._h, 1, C.c_void_p(mels.ctypes.data), 0, B, C.byref(opts), None, None, 0, cfg.vocab_size, len(p)) == E_ARG
    assert m.loop_steps(0) == steps
    # wm_transcribe_wait_lp_ns on a slot submitted without the probe: WM_E_STATE; the slot still delivers what it computed
    m.transcribe_submit(mels, slot=1, prompt=p, return_logprobs=True, **kw)
    assert L.wm_transcribe_wait_lp_ns(m._h, 1, *out) == E_STATE
    ids, (l1, a1) = m.transcribe_wait(1)
    assert ids == want[0]
    # the older waits on a probe slot return what they always return
    m.transcribe_submit(mels, slot=2, prompt=p, return_logprobs=True, no_speech_token=tok, **kw)
    m._pending.pop(2)
    _lib.check(L.wm_transcribe_wait_lp(m._h, 2, *out[:4]))
    assert [toks[b, :n[b]].tolist() for b in range(B)] == want[0]
    np.testing.assert_array_equal(avg.view(np.uint32), want[1][1].view(np.uint32))
    m.transcribe_submit(mels, slot=2, prompt=p, return_logprobs=True, no_speech_token=tok, **kw)
    m._pending.pop(2)
    _lib.check(L.wm_transcribe_wait(m._h, 2, toks.ctypes.data_as(ip), n.ctypes.data_as(ip)))
    assert [toks[b, :n[b]].tolist() for b in range(B)] == want[0]
    assert m.transcribe_batch(mels, prompt=p, return_logprobs=True, no_speech_token=tok, **kw)[0] == want[0]
    m.close()


def test_bf16_smoke(hip):
    """bf16 tiny, B = 64: finite probabilities in (0, 1), ids of the plain pass"""
    cfg, w, z, rows = setup("tiny")
    from whisper_mojo_amd import synth
    kw = _kw(z)
    kw["max_loop"] = 12
    mels = np.stack([synth.synth_mel(cfg, 7000 + b) for b in range(64)])
    prompt = z["init"].tolist()
    m = _model(cfg, w, 64, dtype=1)
    plain = m.transcribe_batch(mels, prompt=prompt, **kw)
    ids, (lps, avg, nsp) = m.transcribe_batch(mels, prompt=prompt, return_logprobs=True, no_speech_token=int(z["no_speech_token"]), **kw)
    assert ids == plain
    assert np.isfinite(nsp).all() and (nsp > 0).all() and (nsp < 1).all()
    m.close()
