"""End-to-end tests (-m gpu) of wm_transcribe_lp / wm_transcribe_submit_lp / wm_transcribe_wait_lp against the HF
fixtures of tools/make_golden_logprobs.py: fp32 models, micro and tiny.

Bar: |logprob - HF| <= 1e-4, twice the project's 5e-5 fp32 logits bar — a log-prob is the difference of two quantities (the chosen
logit and the logsumexp, itself 1-Lipschitz in the logits) each within that bar; avg_logprob, a mean of such values, gets the same."""
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


def _setup(name):
    from whisper_mojo_amd import WhisperConfig, synth
    cfg = WhisperConfig.micro() if name == "micro" else WhisperConfig.tiny()
    z = np.load(os.path.join(GOLDEN, f"logprobs_{name}_hf.npz"))
    rows = []
    for i in range(int(z["n_rows"])):
        k = f"r{i}_"
        rows.append(dict(case=str(z[k + "case"]), seed=int(z[k + "seed"]), ts=int(z[k + "ts"]), prompt=z[k + "prompt"].tolist(),
                         ids=z[k + "ids"].tolist(), lps=z[k + "logprobs"], avg=float(z[k + "avg_logprob"])))
    return cfg, synth.synth_weights(cfg, 0), z, rows


_CACHE = {}


def setup(name):
    if name not in _CACHE:
        _CACHE[name] = _setup(name)
    return _CACHE[name]


def _kw(z, ts_on):
    kw = dict(eot=int(z["eos"]), max_loop=int(z["max_loop"]), suppress_tokens=z["suppress"].tolist(),
              begin_suppress_tokens=z["begin_suppress"].tolist())
    if ts_on:
        kw["timestamps"] = (int(z["timestamp_begin"]), int(z["no_ts"]), int(z["max_init"]))
    return kw


def _mels(cfg, rows):
    from whisper_mojo_amd import synth
    return np.stack([synth.synth_mel(cfg, r["seed"]) for r in rows])


def _check_rows(tag, rows, ids, lps, avg, table, counts):
    worst = 0.0
    for b, r in enumerate(rows):
        assert ids[b] == r["ids"], (tag, b)  # the precondition the parity tests establish
        L = len(r["prompt"])
        got = np.asarray(lps[b], np.float64)
        assert (got[:L] == 0).all()
        assert (table[b, counts[b]:] == 0).all()  # tail positions of the table
        err = np.abs(got[L:] - r["lps"].astype(np.float64)).max()
        aerr = abs(float(avg[b]) - r["avg"])
        worst = max(worst, err, aerr)
        print(f"{tag} row {b}: {len(r['lps'])} ids, max |logprob - HF| {err:.2e}, |avg - HF| {aerr:.2e} (avg {avg[b]:.4f})")
        assert err <= BAR and aerr <= BAR, (tag, b, err, aerr)
    return worst


@pytest.mark.parametrize("name", ["micro", "tiny"])
@pytest.mark.parametrize("case", ["shared", "off"])
def test_logprobs_match_hf(hip, name, case):
    cfg, w, z, rows = setup(name)
    rows = [r for r in rows if r["case"] == case]
    assert len({tuple(r["prompt"]) for r in rows}) == 1
    m = make_model(cfg, w, max_batch=4)
    ids, (lps, avg) = m.transcribe_batch(_mels(cfg, rows), prompt=rows[0]["prompt"], return_logprobs=True, **_kw(z, rows[0]["ts"]))
    _check_rows(f"{name} {case}", rows, ids, lps, avg, m.last_logprobs, m.last_counts)
    m.close()


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_logprobs_per_row_prompts_match_hf(hip, name):
    cfg, w, z, rows = setup(name)
    rows = [r for r in rows if r["case"] == "rows"]
    assert len({len(r["prompt"]) for r in rows}) > 1
    m = make_model(cfg, w, max_batch=4)
    ids, (lps, avg) = m.transcribe_batch(_mels(cfg, rows), prompts=[r["prompt"] for r in rows], return_logprobs=True, **_kw(z, 1))
    _check_rows(f"{name} rows", rows, ids, lps, avg, m.last_logprobs, m.last_counts)
    m.close()


def _model(cfg, w, max_batch, coalesce=0, dtype=0):
    """HF mode (erf GELU, HF positions), as the fixtures were generated"""
    from whisper_mojo_amd import GELU_ERF, POS_HF
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, compute_dtype=dtype, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=max_batch, coalesce=coalesce)
    m.load(WeightLoader.from_array(w))
    return m


def make_model(cfg, w, max_batch):
    return _model(cfg, w, max_batch)


@pytest.mark.parametrize("coalesce", [0, 2])
def test_pipelined_and_coalesced_are_bitwise_the_synchronous_call(hip, coalesce):
    """Four _lp submits in flight (coalesce = 2: two pairs on 2·B-row states) return exactly the synchronous call's ids and log-probs."""
    cfg, w, z, rows = setup("micro")
    rows = [r for r in rows if r["case"] == "shared"]
    kw = _kw(z, 1)
    mels = _mels(cfg, rows)
    batches = [mels, mels[::-1].copy(), mels[[1, 0, 2]].copy(), mels]
    m = _model(cfg, w, 4, coalesce)
    want = []
    for mb in batches:
        ids, (lps, avg) = m.transcribe_batch(mb, prompt=rows[0]["prompt"], return_logprobs=True, **kw)
        want.append((ids, m.last_logprobs.copy(), avg.copy()))
    for s, mb in enumerate(batches):
        m.transcribe_submit(mb, slot=s, prompt=rows[0]["prompt"], return_logprobs=True, **kw)
    for s in range(4):
        ids, (lps, avg) = m.transcribe_wait(s)
        assert ids == want[s][0]
        np.testing.assert_array_equal(m.last_logprobs.view(np.uint32), want[s][1].view(np.uint32))
        np.testing.assert_array_equal(avg.view(np.uint32), want[s][2].view(np.uint32))
    if coalesce == 2:  # an _lp submit does not pair with a plain one: each runs alone and gets its own result
        plain = m.transcribe_batch(mels, prompt=rows[0]["prompt"], **kw)
        m.transcribe_submit(mels, slot=0, prompt=rows[0]["prompt"], **kw)
        m.transcribe_submit(mels, slot=1, prompt=rows[0]["prompt"], return_logprobs=True, **kw)
        ids, (lps, avg) = m.transcribe_wait(1)
        assert ids == want[0][0]
        np.testing.assert_array_equal(m.last_logprobs.view(np.uint32), want[0][1].view(np.uint32))
        assert m.transcribe_wait(0) == plain
    m.close()


def test_mode_switch_keeps_plain_ids(hip):
    """A plain pass before and after an _lp pass on the same state returns the same ids (the step graph is recaptured both ways);
    wm_transcribe_wait on an _lp slot returns the ids."""
    cfg, w, z, rows = setup("tiny")
    rows = [r for r in rows if r["case"] == "shared"]
    kw = _kw(z, 1)
    mels = _mels(cfg, rows)
    m = make_model(cfg, w, max_batch=4)
    before = m.transcribe_batch(mels, prompt=rows[0]["prompt"], **kw)
    ids, (lps, avg) = m.transcribe_batch(mels, prompt=rows[0]["prompt"], return_logprobs=True, **kw)
    assert ids == before == [r["ids"] for r in rows]
    assert m.transcribe_batch(mels, prompt=rows[0]["prompt"], **kw) == before
    ids2, (lps2, avg2) = m.transcribe_batch(mels, prompt=rows[0]["prompt"], return_logprobs=True, **kw)
    assert ids2 == ids and lps2 == lps
    m.transcribe_submit(mels, slot=2, prompt=rows[0]["prompt"], return_logprobs=True, **kw)
    B, total, _keep, _tag = m._pending.pop(2)
    toks, n = np.zeros((B, total), np.int32), np.zeros(B, np.int32)
    ip = C.POINTER(C.c_int32)
    from whisper_mojo_amd import _lib
    _lib.check(_lib.lib().wm_transcribe_wait(m._h, 2, toks.ctypes.data_as(ip), n.ctypes.data_as(ip)))
    assert [toks[b, :n[b]].tolist() for b in range(B)] == before
    m.close()


def test_refusals_launch_nothing(hip):
    from whisper_mojo_amd import _lib
    cfg, w, z, rows = setup("micro")
    rows = [r for r in rows if r["case"] == "shared"]
    kw = _kw(z, 1)
    mels = _mels(cfg, rows)
    m = make_model(cfg, w, max_batch=4)
    m.set_alignment_heads([(0, 0)])
    want = m.transcribe_batch(mels, prompt=rows[0]["prompt"], return_logprobs=True, **kw)[0]
    steps = m.loop_steps(0)
    L = _lib.lib()
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    B = len(rows)
    opts, _keep = m._opts(rows[0]["prompt"], kw["eot"], kw["max_loop"], False, kw["suppress_tokens"], kw["begin_suppress_tokens"], kw["timestamps"])
    total = len(rows[0]["prompt"]) + 1 + kw["max_loop"]
    toks, n = np.zeros((B, total), np.int32), np.zeros(B, np.int32)
    lps, avg = np.zeros((B, total), np.float32), np.zeros(B, np.float32)
    out = (toks.ctypes.data_as(ip), n.ctypes.data_as(ip), lps.ctypes.data_as(fp), avg.ctypes.data_as(fp))
    args = (m._h, C.c_void_p(mels.ctypes.data), 0, B, C.byref(opts))
    tab, lens = np.tile(np.asarray(rows[0]["prompt"], np.int32), (B, 1)), np.full(B, len(rows[0]["prompt"]), np.int32)
    bad = lens.copy()
    bad[1] = 0
    assert L.wm_transcribe_lp(*args, None, None, 0, toks.ctypes.data_as(ip), n.ctypes.data_as(ip), None, avg.ctypes.data_as(fp)) == -1  # WM_E_ARG
    assert L.wm_transcribe_lp(*args, None, None, 0, toks.ctypes.data_as(ip), n.ctypes.data_as(ip), lps.ctypes.data_as(fp), None) == -1
    assert L.wm_transcribe_lp(*args, None, lens.ctypes.data_as(ip), 3, *out) == -1           # prompt_len without prompts
    assert L.wm_transcribe_lp(*args, tab.ctypes.data_as(ip), bad.ctypes.data_as(ip), tab.shape[1], *out) == -1  # prompt_len[b] = 0
    assert L.wm_transcribe_submit_lp(m._h, 9, C.c_void_p(mels.ctypes.data), 0, B, C.byref(opts), None, None, 0) == -1
    assert m.loop_steps(0) == steps
    with pytest.raises(ValueError):  # log-probs and token timestamps do not combine
        m.transcribe_batch(mels, prompt=rows[0]["prompt"], return_logprobs=True, return_token_timestamps=True, **kw)
    with pytest.raises(ValueError):
        m.transcribe_submit(mels, slot=1, prompt=rows[0]["prompt"], return_logprobs=True, return_token_timestamps=True, **kw)
    assert m.loop_steps(0) == steps
    # wm_transcribe_wait_lp on a slot submitted without log-probs: WM_E_STATE (-5); the slot still delivers its ids
    m.transcribe_submit(mels, slot=1, prompt=rows[0]["prompt"], **kw)
    assert L.wm_transcribe_wait_lp(m._h, 1, *out) == -5
    assert m.transcribe_wait(1) == want
    assert L.wm_transcribe_wait_lp(m._h, 3, *out) == -5  # nothing submitted
    assert m.transcribe_batch(mels, prompt=rows[0]["prompt"], return_logprobs=True, **kw)[0] == want
    m.close()


def test_bf16_smoke(hip):
    """bf16 tiny, B = 64: finite values <= 0, avg_logprob = the mean of the row's entries to fp32 rounding, ids of the plain pass."""
    cfg, w, z, rows = setup("tiny")
    from whisper_mojo_amd import synth
    kw = _kw(z, 1)
    kw["max_loop"] = 12
    mels = np.stack([synth.synth_mel(cfg, 7000 + b) for b in range(64)])
    prompt = z["init"].tolist()
    m = _model(cfg, w, 64, dtype=1)
    plain = m.transcribe_batch(mels, prompt=prompt, **kw)
    ids, (lps, avg) = m.transcribe_batch(mels, prompt=prompt, return_logprobs=True, **kw)
    assert ids == plain
    for b in range(64):
        g = np.asarray(lps[b][len(prompt):], np.float32)
        assert g.size and np.isfinite(g).all() and (g <= 0).all()
        assert (np.asarray(lps[b][:len(prompt)]) == 0).all()
        assert abs(float(avg[b]) - float(g.astype(np.float64).mean())) <= 4 * g.size * 2.0 ** -24 * max(1.0, float(np.abs(g).sum()))
    m.close()
