"""CPU tests of transcript scoring's definition and host interface.

  * The header declares the new functions, the library exports them, the Python mirror lists them; the ABI version is still 5.
  * A numpy restatement of the definition — logprob[t] = z[t-1][y[t]] - logsumexp(z[t-1]) over the fixture's raw logits, the sum and
    the mean over t >= context_len — reproduces what HF's own forward recorded (tools/make_golden_score.py): the log-probs, the sum,
    the mean, and -loss of HF's labels= path with -100 on the context.
  * At most 5 % of a fixture's positions carry no asserted top id.
  * The refusals that need no GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("wm_score", "wm_score_submit", "wm_score_wait", "wm_score_pcm", "wm_op_score_logits", "wm_score_phases")


def test_header_declares_and_library_exports_the_score_entries():
    from whisper_mojo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "whisper_mi.h")).read()
    L = _lib.lib()
    for s in NEW:
        assert re.search(r"\bint " + s + r"\(", hdr), s
        assert hasattr(L, s) and s in _lib.SYMBOLS, s
    assert re.search(r"#define WM_ABI_VERSION 5\b", hdr)
    assert L.wm_abi_version() == 5 == _lib.ABI_VERSION


def _rows(name):
    z = np.load(os.path.join(GOLDEN, f"score_{name}_hf.npz"))
    return z, int(z["n_rows"])


def test_numpy_restatement_reproduces_hf():
    z, n = _rows("micro")
    cases, ctxs = set(), set()
    for i in range(n):
        k = f"r{i}_"
        if k + "raw" not in z.files:  # the long rows carry no raw logits (file size)
            continue
        ctxs.add(int(z[k + "context_len"]))
        y, ctx, raw = z[k + "ids"], int(z[k + "context_len"]), z[k + "raw"].astype(np.float64)
        assert raw.shape[0] == len(y) - 1 and 1 <= ctx <= len(y) - 1
        mx = raw.max(1, keepdims=True)
        lse = (mx + np.log(np.exp(raw - mx).sum(1, keepdims=True)))[:, 0]
        lp = np.zeros(len(y))
        lp[1:] = raw[np.arange(len(y) - 1), y[1:]] - lse
        assert np.abs(lp - z[k + "logprobs"]).max() <= 1e-5
        s = lp[ctx:].sum()  # positions 1 .. ctx - 1 are reported, not summed
        assert abs(s - float(z[k + "sum"])) <= 1e-5 * (len(y) - ctx)
        assert abs(s / (len(y) - ctx) - float(z[k + "mean"])) <= 1e-5
        assert abs(s / (len(y) - ctx) - float(z[k + "neg_loss"])) <= 1e-5  # HF's own reduction over the labels that are not -100
        if ctx > 1:  # the context exclusion matters: the mean over all positions is another number
            assert abs(lp[1:].mean() - float(z[k + "neg_loss"])) > 1e-3
        top = z[k + "top_ids"]
        keep = top[1:] >= 0
        np.testing.assert_array_equal(raw.argmax(1)[keep], top[1:][keep])  # numpy's argmax: the lowest index
        assert top[0] == -1 and z[k + "logprobs"][0] == 0
        cases.add(str(z[k + "case"]))
    assert cases == {"greedy", "other_clip", "random", "len2"} and max(ctxs) > 1 and min(ctxs) == 1


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_fixture_rows_and_unasserted_cap(name):
    from whisper_mojo_amd import WhisperConfig
    cfg = WhisperConfig.micro() if name == "micro" else WhisperConfig.tiny()
    z, n = _rows(name)
    total = missing = 0
    lens, ctxs = [], []
    for i in range(n):
        k = f"r{i}_"
        top = z[k + "top_ids"]
        total += len(top) - 1
        missing += int((top[1:] < 0).sum())
        lens.append(len(z[k + "ids"]))
        ctxs.append(int(z[k + "context_len"]))
        assert (z[k + "logprobs"][1:] < 0).all()
    assert missing <= 0.05 * total
    assert 2 in lens and cfg.n_text_ctx in lens and max(ctxs) > 16  # length 2, full context, a context past one prefill chunk
    assert z["r2_logprobs"][1:].mean() < z["r0_logprobs"][int(z["r0_context_len"]):].mean()  # random ids score worse than greedy ones
    assert os.path.getsize(os.path.join(GOLDEN, f"score_{name}_hf.npz")) < 1 << 20


def test_refusals_that_need_no_gpu():
    import ctypes as C
    from whisper_mojo_amd import WhisperConfig, _lib
    from whisper_mojo_amd.whisper import Whisper
    cfg = WhisperConfig.micro()
    m = Whisper(cfg, max_batch=2)  # not loaded: every refusal below comes before the model is touched
    mel = np.zeros((2, cfg.n_mels, cfg.n_frames), np.float32)
    ok = [[1, 2, 3, 4], [1, 2]]
    for ids, ctx in (([[1], [1, 2]], None),                      # a row shorter than 2
                     ([[1, 2], list(range(cfg.n_text_ctx + 1))], None),  # longer than the decoder context
                     ([[1, 2, cfg.vocab_size], [1, 2]], None),    # not a vocabulary id
                     ([[1, -1], [1, 2]], None),
                     (ok, 0), (ok, [1, 2]), (ok, [4, 1]),          # context_len outside [1, len - 1]
                     ([[1, 2]], None)):                           # rows != clips
        with pytest.raises(ValueError):
            m.score(mel, ids, ctx)
        with pytest.raises(ValueError):
            m.score_submit(mel, ids, 1, ctx)
    with pytest.raises(ValueError):  # B over max_batch
        m.score(np.zeros((3, cfg.n_mels, cfg.n_frames), np.float32), [[1, 2]] * 3)
    with pytest.raises(_lib.WhisperMiError):  # accepted arguments reach the model check
        m.score(mel, ok, [3, 1])
    with pytest.raises(_lib.WhisperMiError):  # nothing was recorded by the refused submits
        m.score_wait(1)
    tab, lens, ctx = _lib.score_args(ok, None, 2, cfg.vocab_size, cfg.n_text_ctx, 2)
    assert tab.shape == (2, 4) and lens.tolist() == [4, 2] and ctx.tolist() == [1, 1]
    # the C entries refuse a null model before anything else
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    f, i = (lambda a: a.ctypes.data_as(fp)), (lambda a: a.ctypes.data_as(ip))
    out, top, sm = np.zeros((2, 4), np.float32), np.zeros((2, 4), np.int32), np.zeros(2, np.float32)
    L = _lib.lib()
    assert L.wm_score(None, mel.ctypes.data_as(C.c_void_p), 0, 2, 1, i(tab), i(lens), 4, i(ctx), f(out), i(top), f(sm), f(sm)) == -1
    assert L.wm_score_submit(None, 0, mel.ctypes.data_as(C.c_void_p), 0, 2, 1, i(tab), i(lens), 4, i(ctx)) == -1
    assert L.wm_score_wait(None, 0, f(out), i(top), f(sm), f(sm)) == -1
    x = np.zeros((2, 256), np.float32)
    assert L.wm_op_score_logits(f(sm), i(top), f(x), f(x), f(x), f(x), i(lens), 2, 2, 256, 0) == -1  # K: refused before any upload
