"""End-to-end tests (-m gpu) of wm_detect_language and the wm_transcribe_lang trio against the HF fixture of
tools/make_golden_lang.py: micro (an unsorted, non-contiguous list of 12 ids) and tiny (ids 50259 … 50357), fp32 decoder.

Bars: detected ids equal HF's; language probabilities within 1e-4 of the stored float64 softmax, token log-probs, avg_logprob and
log no_speech_prob within 1e-4 of HF's — the tolerance of tests/test_gpu_logprobs.py and tests/test_gpu_no_speech.py (a
log-probability is a logit minus a logsumexp, each within the project's 5e-5 fp32 logits bar; a probability <= 1 moves by no more)."""
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


def setup(name="tiny"):
    if name not in _CACHE:
        from whisper_mojo_amd import WhisperConfig, synth
        cfg = WhisperConfig.micro() if name == "micro" else WhisperConfig.tiny()
        z = np.load(os.path.join(GOLDEN, f"lang_detect_{name}_hf.npz"))
        lang_ids = z["lang_ids"].tolist()
        w = synth.synth_weights(cfg, 0)  # the fixture model: language rows of the token embedding replaced, cross-attention outputs scaled
        for l in range(cfg.n_layers):
            synth.split_weights(cfg, w)[f"dec.{l}.cross.o.w"][:] *= np.float32(z["cross_o_scale"])
        emb = synth.split_weights(cfg, w)["dec.tok_emb"]
        emb[lang_ids] = (np.random.default_rng(int(z["lang_row_seed"])).standard_normal((len(lang_ids), cfg.d_model)) *
                         float(z["lang_row_scale"])).astype(np.float32)
        ramp = np.linspace(-1, 1, cfg.n_mels, dtype=np.float32)[:, None]
        rows = []
        for i in range(int(z["s_rows"])):
            k = f"s{i}_"
            g, t = np.float32(z[k + "gain"]), np.float32(z[k + "tilt"])
            mel = (g * synth.synth_mel(cfg, int(z[k + "seed"])) - (np.float32(1) - g) + t * ramp).astype(np.float32)
            rows.append(dict(case=str(z[k + "case"]), mel=mel, prompt=z[k + "prompt"].tolist(), ids=z[k + "ids"].tolist(), lps=z[k + "logprobs"],
                             avg=float(z[k + "avg_logprob"]), nsp=float(z[k + "no_speech_prob"]), lang=int(z[k + "lang"]),
                             probs=z[k + "lang_probs"]))
        _CACHE[name] = (cfg, w, z, rows, lang_ids)
    return _CACHE[name]


def _kw(z):
    return dict(eot=int(z["eos"]), max_loop=int(z["s_max_loop"]), suppress_tokens=z["s_suppress"].tolist(),
                begin_suppress_tokens=z["s_begin_suppress"].tolist(), timestamps=(int(z["timestamp_begin"]), int(z["no_ts"]), int(z["s_max_init"])))


def _model(cfg, w, max_batch, dtype=0):
    """HF mode (erf GELU, HF positions), as the fixture was generated"""
    from whisper_mojo_amd import GELU_ERF, POS_HF
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, compute_dtype=dtype, gelu_mode=GELU_ERF, pos_mode=POS_HF, max_batch=max_batch)
    m.load(WeightLoader.from_array(w))
    return m


def _placeholder(rows, n_init, other):
    """the rows' prompts with another language id at the language slot (the pass must overwrite it)"""
    out = []
    for r in rows:
        p = list(r["prompt"])
        p[len(p) - n_init + 1] = other
        out.append(p)
    return out


def _check(tag, rows, n_init, ids, lps, avg, nsp, lang, probs):
    for b, r in enumerate(rows):
        L = len(r["prompt"])
        assert int(lang[b]) == r["lang"], (tag, b, int(lang[b]), r["lang"])
        assert ids[b][L - n_init + 1] == r["lang"], (tag, b)
        assert ids[b] == r["ids"], (tag, b)
        perr = np.abs(probs[b].astype(np.float64) - r["probs"]).max()
        err = np.abs(np.asarray(lps[b], np.float64)[L:] - r["lps"].astype(np.float64)).max()
        aerr = abs(float(avg[b]) - r["avg"])
        nerr = abs(np.log(float(nsp[b])) - np.log(r["nsp"]))
        print(f"{tag} row {b} (prompt {L}): language {lang[b]} p {probs[b].max():.4f}, max |p - HF| {perr:.2e}; max |logprob - HF| {err:.2e}, "
              f"|avg - HF| {aerr:.2e}, |Δ log no_speech_prob| {nerr:.2e}")
        assert perr <= BAR and err <= BAR and aerr <= BAR and nerr <= BAR, (tag, b, perr, err, aerr, nerr)


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_detect_language_matches_hf(hip, name):
    cfg, w, z, rows, lang_ids = setup(name)
    assert name == "tiny" or (lang_ids != sorted(lang_ids) and max(np.diff(sorted(lang_ids))) > 1)
    m = _model(cfg, w, len(rows))
    ids, probs = m.detect_language(np.stack([r["mel"] for r in rows]), lang_ids, sot=int(z["init"][0]))
    for b, r in enumerate(rows):
        perr = np.abs(probs[b].astype(np.float64) - r["probs"]).max()
        print(f"row {b}: language {ids[b]} (HF {r['lang']}), max |p - HF| {perr:.2e}, sum {probs[b].astype(np.float64).sum():.7f}")
        assert int(ids[b]) == r["lang"] and perr <= BAR
    one, p1 = m.detect_language(rows[4]["mel"][None], lang_ids, sot=int(z["init"][0]))  # a row alone: the same bits
    assert one[0] == ids[4]
    np.testing.assert_array_equal(p1[0], probs[4])
    m.close()


@pytest.mark.parametrize("name", ["micro", "tiny"])
@pytest.mark.parametrize("case", ["shared", "rows"])
def test_transcribe_with_detection_matches_hf_and_the_two_call_route(hip, case, name):
    """ids, language slot, log-probs, avg_logprob and no_speech_prob against HF; and the fused pass is bit-identical to
    detect_language followed by transcribe_batch(prompts=…) with those languages"""
    cfg, w, z, rows, lang_ids = setup(name)
    rows = [r for r in rows if r["case"] == case]
    n_init, ns_tok, other = len(z["init"]), int(z["no_speech_token"]), int(z["init"][1])
    assert all(r["lang"] != other for r in rows)
    mels = np.stack([r["mel"] for r in rows])
    m = _model(cfg, w, len(rows))
    kw = _kw(z)
    if case == "shared":
        ids, (lps, avg, nsp), (lang, probs) = m.transcribe_batch(mels, prompt=z["init"].tolist(), detect_language=lang_ids, return_logprobs=True,
                                                                 no_speech_token=ns_tok, **kw)
    else:
        ids, (lps, avg, nsp), (lang, probs) = m.transcribe_batch(mels, prompts=_placeholder(rows, n_init, other), n_init=n_init,
                                                                 detect_language=lang_ids, return_logprobs=True, no_speech_token=ns_tok, **kw)
    _check(f"{name} {case}", rows, n_init, ids, lps, avg, nsp, lang, probs)
    plain, (lang2, probs2) = m.transcribe_batch(mels, prompts=_placeholder(rows, n_init, other), n_init=n_init, detect_language=lang_ids, **kw)
    assert plain == ids  # without log-probs and probe: the same ids
    np.testing.assert_array_equal(lang2, lang)
    np.testing.assert_array_equal(probs2, probs)
    dl, dp = m.detect_language(mels, lang_ids, sot=int(z["init"][0]))
    np.testing.assert_array_equal(dl, lang)
    np.testing.assert_array_equal(dp, probs)
    detected = [p[:len(p) - n_init + 1] + [int(dl[b])] + p[len(p) - n_init + 2:] for b, p in enumerate(_placeholder(rows, n_init, other))]
    ids3, (lps3, avg3, nsp3) = m.transcribe_batch(mels, prompts=detected, n_init=n_init, return_logprobs=True, no_speech_token=ns_tok, **kw)
    assert ids3 == ids
    for b in range(len(rows)):
        np.testing.assert_array_equal(np.asarray(lps3[b], np.float32), np.asarray(lps[b], np.float32))
    np.testing.assert_array_equal(avg3, avg)
    np.testing.assert_array_equal(nsp3, nsp)
    m.close()


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_pipelined_slots_mode_switch_and_wait_state(hip, name):
    cfg, w, z, rows, lang_ids = setup(name)
    n_init, ns_tok, other = len(z["init"]), int(z["no_speech_token"]), int(z["init"][1])
    ra, rb = [r for r in rows if r["case"] == "rows"], [r for r in rows if r["case"] == "shared"]
    m = _model(cfg, w, 4)
    kw = _kw(z)
    args = lambda rs: dict(prompts=_placeholder(rs, n_init, other), n_init=n_init, detect_language=lang_ids, return_logprobs=True,
                           no_speech_token=ns_tok, **kw)
    ma, mb = np.stack([r["mel"] for r in ra]), np.stack([r["mel"] for r in rb])
    plain_before = m.transcribe_batch(mb, prompt=rb[0]["prompt"], **kw)
    sync_a, sync_b = m.transcribe_batch(ma, **args(ra)), m.transcribe_batch(mb, **args(rb))
    assert m.transcribe_batch(mb, prompt=rb[0]["prompt"], **kw) == plain_before  # a _lang pass leaves nothing behind on the state
    m.transcribe_submit(ma, slot=1, **args(ra))
    m.transcribe_submit(mb, slot=2, **args(rb))
    for slot, want in ((1, sync_a), (2, sync_b)):
        ids, (lps, avg, nsp), (lang, probs) = m.transcribe_wait(slot)
        assert ids == want[0]
        for b in range(len(ids)):
            np.testing.assert_array_equal(np.asarray(lps[b], np.float32), np.asarray(want[1][0][b], np.float32))
        np.testing.assert_array_equal(avg, want[1][1])
        np.testing.assert_array_equal(nsp, want[1][2])
        np.testing.assert_array_equal(lang, want[2][0])
        np.testing.assert_array_equal(probs, want[2][1])
    # wm_transcribe_wait_lang on a slot submitted without detection: WM_E_STATE (-5), and the slot is still collectable
    from whisper_mojo_amd import _lib
    L = _lib.lib()
    m.transcribe_submit(mb, slot=1, prompt=rb[0]["prompt"], **kw)
    B, total = len(rb), len(rb[0]["prompt"]) + 1 + kw["max_loop"]
    toks, n, lo = np.zeros((B, total), np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    ip = C.POINTER(C.c_int32)
    rc = L.wm_transcribe_wait_lang(m._h, 1, toks.ctypes.data_as(ip), n.ctypes.data_as(ip), None, None, None, lo.ctypes.data_as(ip), None)
    assert rc == -5 and b"language detection" in L.wm_last_error()
    assert m.transcribe_wait(1) == plain_before
    # the older waits on a _lang slot return what they always return
    m.transcribe_submit(mb, slot=1, **args(rb))
    m._pending.pop(1)
    assert L.wm_transcribe_wait(m._h, 1, toks.ctypes.data_as(ip), n.ctypes.data_as(ip)) == 0
    assert [toks[b, :n[b]].tolist() for b in range(B)] == sync_b[0]
    m.close()


def test_refusals_launch_nothing(hip):
    cfg, w, z, rows, lang_ids = setup()
    from whisper_mojo_amd import _lib
    L = _lib.lib()
    m = _model(cfg, w, 2)
    kw = _kw(z)
    mels = np.stack([r["mel"] for r in rows[:2]])
    good = m.transcribe_batch(mels, prompt=z["init"].tolist(), detect_language=lang_ids, **kw)
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    opts, _keep = m._opts(z["init"].tolist(), kw["eot"], kw["max_loop"], False, kw["suppress_tokens"], kw["begin_suppress_tokens"], kw["timestamps"])
    toks, n, lo = np.zeros((2, 3 + 1 + kw["max_loop"]), np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)
    mp = mels.ctypes.data_as(C.c_void_p)

    def tr(ids, n_init=3, prompts=None, lens=None, stride=0):
        ids = np.asarray(ids, np.int32)
        return L.wm_transcribe_lang(m._h, mp, 0, 2, C.byref(opts), prompts, lens, stride, -1, n_init, ids.ctypes.data_as(ip), ids.size,
                                    toks.ctypes.data_as(ip), n.ctypes.data_as(ip), None, None, None, lo.ctypes.data_as(ip), None)

    def det(ids, sot=50258):
        ids = np.asarray(ids, np.int32)
        return L.wm_detect_language(m._h, mp, 0, 2, sot, ids.ctypes.data_as(ip), ids.size, lo.ctypes.data_as(ip), None)

    assert tr(lang_ids) == 0 and det(lang_ids) == 0
    for bad in ([], list(range(129)), [50259, cfg.vocab_size], [50259, -1], [50259, 50260, 50259]):
        assert tr(bad) == -1 and det(bad) == -1, bad  # WM_E_ARG
    assert tr(lang_ids, n_init=1) == -1 and tr(lang_ids, n_init=4) == -1
    assert det(lang_ids, sot=cfg.vocab_size) == -1 and det(lang_ids, sot=-1) == -1
    tab = np.asarray([[7, 50258, 50259, 50359], [50258, 50259, 50359, 0]], np.int32)
    lens = np.asarray([4, 3], np.int32)
    assert tr(lang_ids, 3, tab.ctypes.data_as(ip), lens.ctypes.data_as(ip), 4) == 0
    assert tr(lang_ids, 4, tab.ctypes.data_as(ip), lens.ctypes.data_as(ip), 4) == -1  # n_init larger than row 1's prompt
    assert m.transcribe_batch(mels, prompt=z["init"].tolist(), detect_language=lang_ids, **kw)[0] == good[0]  # the state is intact
    m.close()


def test_bf16_decoder_smoke(hip):
    """bf16 operands: detected ids lie in the list, every row's probabilities are finite and sum to 1 within 1e-5"""
    from whisper_mojo_amd import DT_BF16
    cfg, w, z, rows, lang_ids = setup()
    m = _model(cfg, w, len(rows), dtype=DT_BF16)
    mels = np.stack([r["mel"] for r in rows])
    ids, probs = m.detect_language(mels, lang_ids, sot=int(z["init"][0]))
    assert all(int(t) in lang_ids for t in ids)
    assert np.isfinite(probs).all() and np.abs(probs.astype(np.float64).sum(1) - 1).max() <= 1e-5
    out, (lang, probs2) = m.transcribe_batch(mels, prompt=z["init"].tolist(), detect_language=lang_ids, **_kw(z))
    np.testing.assert_array_equal(lang, ids)
    np.testing.assert_array_equal(probs2, probs)
    assert all(o[1] == int(lang[b]) for b, o in enumerate(out))
    m.close()
