"""GPU: sequential long-form transcription (wm_transcribe_long*, wm_log_mel_long) against HF generate's long-form
path (fixtures of tools/make_golden_long_form.py), against itself under other schedules, and against the window loop of
tests/test_long_form.py composed with the existing transcribe_batch."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from test_long_form import restate_long_form

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()
    return True


def make_model(cfg, weights, **kw):
    from whisper_mojo_amd import GELU_ERF, POS_HF
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, gelu_mode=GELU_ERF, pos_mode=POS_HF, **kw)
    m.load(WeightLoader.from_array(weights))
    return m


def fixture_case(g, case, cfg):
    from whisper_mojo_amd import synth
    lengths = [int(v) for v in g[case + "_lengths"]]
    mels = [synth.synth_long_mel(cfg, int(s), n) for s, n in zip(g[case + "_seeds"], lengths)]
    kw = dict(prompt=tuple(int(v) for v in g["prompt"]), eot=int(g["eos"]), max_loop=int(g[case + "_max_new_tokens"]) - 1,
              suppress_tokens=g[case + "_suppress"].tolist(), begin_suppress_tokens=g[case + "_begin_suppress"].tolist(),
              timestamps=(int(g["timestamp_begin"]), int(g["no_ts"]), int(g[case + "_max_init"])))
    return mels, lengths, kw


def assert_same(got, want):
    assert len(got) == len(want)
    for b, (x, y) in enumerate(zip(got, want)):
        assert x["sequence"] == y["sequence"], b
        assert len(x["segments"]) == len(y["segments"]), b
        for s, t in zip(x["segments"], y["segments"]):
            assert s["tokens"] == t["tokens"] and s["start"] == t["start"] and s["end"] == t["end"], b


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_matches_hf_long_form_fp32(hip, name, micro_cfg, micro_weights, tiny_cfg, tiny_weights):
    cfg, w = (micro_cfg, micro_weights) if name == "micro" else (tiny_cfg, tiny_weights)
    g = golden(f"long_form_{name}_hf")
    m = make_model(cfg, w, max_batch=4)
    for case in g["cases"]:
        case = str(case)
        mels, lengths, kw = fixture_case(g, case, cfg)
        got = m.transcribe_long_form(mels, **kw)
        for b in range(len(lengths)):
            assert got[b]["sequence"] == g[f"{case}_u{b}_sequence"].tolist(), (case, b)
            counts = [len(s["tokens"]) for s in got[b]["segments"]]
            assert counts == g[f"{case}_u{b}_count"].tolist(), (case, b)
            # float64, bit for bit
            assert [s["start"] for s in got[b]["segments"]] == g[f"{case}_u{b}_start"].tolist(), (case, b)
            assert [s["end"] for s in got[b]["segments"]] == g[f"{case}_u{b}_end"].tolist(), (case, b)
    m.close()


def _logmel_audios():
    from oracle import logmel_oracle as lo
    g = golden("long_form_logmel")
    return g, [lo.synth_audio(int(s), int(n)) for s, n in zip(g["seeds"], g["n_samples"])]


def test_log_mel_long_matches_hf_and_feeds_pcm_path(hip, tiny_cfg, tiny_weights):
    from whisper_mojo_amd import frontend
    g, audios = _logmel_audios()
    m = make_model(tiny_cfg, tiny_weights, max_batch=4)
    mel, nf = frontend.log_mel_long(m, audios)
    assert mel.shape == (3, 80, int(g["n_samples"].max()) // 160)
    assert nf.tolist() == g["n_frames"].tolist()
    err = np.abs(mel[:, :, g["cols"]] - g["mel_cols"])
    assert err.max() < 2e-3 and err.mean() < 1e-4, (err.max(), err.mean())
    assert np.abs(mel.max(axis=(1, 2)) - g["mel_max"]).max() < 2e-3
    assert np.abs(mel.astype(np.float64).sum(2) - g["mel_rowsum"]).max() / mel.shape[2] < 1e-4
    # PCM in equals the library's own long mel in, bit for bit
    kw = dict(prompt=(50258, 50259, 50359), eot=50257, max_loop=24, timestamps=(50364, 50363, 50))
    a = frontend.transcribe_audio_long_form(m, audios, **kw)
    b = m.transcribe_long_form(mel, n_frames=nf, **kw)
    assert_same(a, b)
    assert sum(len(r["segments"]) for r in a) >= 4
    m.close()


def test_scheduling_invariance(hip, tiny_cfg, tiny_weights):
    """5 utterances on max_batch = 2 (passes of 2 rows, two in flight, queueing) = each alone = max_batch = 8, bitwise.  tiny
    in HF mode seeks at timestamp pairs mid-window, so windows start at data-dependent frames."""
    from whisper_mojo_amd import synth
    lengths = [9000, 4400, 2100, 6500, 3100]
    mels = [synth.synth_long_mel(tiny_cfg, 70 + b, n) for b, n in enumerate(lengths)]
    kw = dict(prompt=(50258, 50259, 50359), eot=50257, max_loop=30, timestamps=(50364, 50363, 50))
    m2 = make_model(tiny_cfg, tiny_weights, max_batch=2)
    got2, st2 = m2.transcribe_long_form(mels, return_stats=True, **kw)
    alone = [m2.transcribe_long_form([x], **kw)[0] for x in mels]
    m2.close()
    m8 = make_model(tiny_cfg, tiny_weights, max_batch=8)
    got8, st8 = m8.transcribe_long_form(mels, return_stats=True, **kw)
    m8.close()
    assert_same(got2, alone)
    assert_same(got2, got8)
    assert (st2["windows"], st2["stalled"]) == (st8["windows"], st8["stalled"])
    assert st2["windows"] > sum(-(-n // tiny_cfg.n_frames) for n in lengths)  # some windows moved by a pair, not by 30 s
    assert st2["rows"] == 2 * st2["passes"] and st8["rows"] == 3 * st8["passes"]  # R = min(max_batch, ceil(B / 2))
    assert st2["windows"] <= st2["rows"] and st8["windows"] <= st8["rows"]


def test_input_forms_and_shape_checks(hip, micro_cfg, micro_weights):
    """A torch CUDA tensor (any float dtype) gives the numpy result; a feature tensor with the wrong mel count is refused
    before anything reads it."""
    import torch
    from whisper_mojo_amd import synth
    m = make_model(micro_cfg, micro_weights, max_batch=2)
    mels = np.stack([synth.synth_long_mel(micro_cfg, 95, 450), synth.synth_long_mel(micro_cfg, 96, 450)])
    kw = dict(prompt=(1, 2, 3), eot=900, max_loop=30, timestamps=(941, 940, 50), n_frames=[450, 330])
    want = m.transcribe_long_form(mels, **kw)
    t = torch.from_numpy(mels).cuda()
    assert m.transcribe_long_form(t, **kw) == want
    assert m.transcribe_long_form(torch.from_numpy(mels), **kw) == want  # CPU tensor
    t16 = t.to(torch.bfloat16)
    assert m.transcribe_long_form(t16, **kw) == m.transcribe_long_form(t16.float().cpu().numpy(), **kw)
    bad = mels[:, :-1]
    for x in (bad, torch.from_numpy(np.ascontiguousarray(bad)).cuda(), list(bad), mels[0, 0]):
        with pytest.raises(ValueError):
            m.transcribe_long_form(x, **kw)
    m.close()


@pytest.mark.parametrize("prec", ["headline", "bf16"])
def test_composition_with_transcribe_batch(hip, prec, tiny_cfg, tiny_weights):
    """The library's loop = the numpy window loop over the library's own long mel and the existing transcribe_batch."""
    from whisper_mojo_amd import DT_BF16, DT_F32, frontend
    from oracle import logmel_oracle as lo
    kwm = dict(compute_dtype=DT_BF16, kv_dtype=DT_F32, decoder_fp32=True) if prec == "headline" else dict(compute_dtype=DT_BF16)
    m = make_model(tiny_cfg, tiny_weights, max_batch=4, **kwm)
    audios = [lo.synth_audio(41 + i, n) for i, n in enumerate([16000 * 75, 16000 * 38, 16000 * 4])]
    kw = dict(prompt=(50258, 50259, 50359), eot=50257, max_loop=30, timestamps=(50364, 50363, 50))
    got = frontend.transcribe_audio_long_form(m, audios, **kw)
    mel, nf = frontend.log_mel_long(m, audios)
    W = tiny_cfg.n_frames

    def decode(items):
        win = np.zeros((len(items), tiny_cfg.n_mels, W), np.float32)
        for r, (b, s, snf) in enumerate(items):
            win[r, :, :snf] = mel[b, :, s:s + snf]
        ids = m.transcribe_batch(win, **kw)
        return [x[len(kw["prompt"]):] for x in ids]

    want, _ = restate_long_form(decode, nf.tolist(), W, 50364, 50257)
    assert_same(got, want)
    m.close()


def test_errors_empty_and_pending_slot(hip, micro_cfg, micro_weights):
    from whisper_mojo_amd import _lib, synth
    m = make_model(micro_cfg, micro_weights, max_batch=2)
    mels = [synth.synth_long_mel(micro_cfg, 90, 450), synth.synth_long_mel(micro_cfg, 91, 300)]
    kw = dict(prompt=(1, 2, 3), eot=900, max_loop=30)
    ts = (941, 940, 50)
    # a pending slot pass and its later wait are untouched by a long-form call
    win = np.stack([mels[0][:, :200], mels[1][:, :200]])
    want = m.transcribe_batch(win, timestamps=ts, **kw)
    m.transcribe_submit(win, slot=1, timestamps=ts, **kw)
    res = m.transcribe_long_form(mels, timestamps=ts, **kw)
    assert m.transcribe_wait(1) == want
    assert m.transcribe_long_form(mels, timestamps=ts, **kw) == res
    # an utterance of 0 frames has an empty result; the others are unchanged
    feats = np.zeros((3, micro_cfg.n_mels, 450), np.float32)
    feats[0], feats[2, :, :300] = mels[0], mels[1]
    r3 = m.transcribe_long_form(feats, n_frames=[450, 0, 300], timestamps=ts, **kw)
    assert r3[1] == {"sequence": [], "segments": []} and r3[0] == res[0] and r3[2] == res[1]
    E_ARG, E_STATE = -1, -5

    def rc(n_frames=(450, 0, 300), **over):
        o = dict(kw, timestamps=ts)
        o.update(over)
        with pytest.raises(_lib.WhisperMiError, match=r"error (-?\d+)") as e:
            m.transcribe_long_form(feats, n_frames=list(n_frames), **o)
        return int(str(e.value).split("error ")[1].split(":")[0])

    assert rc(timestamps=(0, -1, -1)) == E_ARG
    assert rc(n_frames=[451, 0, 0]) == E_ARG
    assert rc(n_frames=[-1, 0, 0]) == E_ARG
    assert rc(max_loop=micro_cfg.n_text_ctx - 3) == E_ARG  # n_prompt + 1 + max_loop > n_text_ctx
    opts, _keep = m._opts((1, 2, 3), 900, 30, True, timestamps=ts)  # ignore_eot
    h = C.c_void_p()
    fp = np.ascontiguousarray(feats)
    assert _lib.lib().wm_transcribe_long(m._h, C.c_void_p(fp.ctypes.data), 0, 3, 450, None, C.byref(opts), C.byref(h)) == E_ARG
    m.close()
    mc = make_model(micro_cfg, micro_weights, max_batch=2, coalesce=2)
    mc.transcribe_submit(win, slot=0, timestamps=ts, **kw)  # held, waiting for a partner
    with pytest.raises(_lib.WhisperMiError, match="-5"):
        mc.transcribe_long_form(mels, timestamps=ts, **kw)
    assert mc.transcribe_wait(0) == want
    mc.close()


def log_mel_long_raw(m, buf, n):
    """wm_log_mel_long on rows that are already padded to one stride -> (mel [B, n_mels, stride // 160], n_frames [B])"""
    from whisper_mojo_amd import _lib
    B, stride = buf.shape
    out = np.empty((B, m.config.n_mels, stride // 160), np.float32)
    nf = np.zeros(B, np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    _lib.check(_lib.lib().wm_log_mel_long(m._h, buf.ctypes.data_as(fp), n.ctypes.data_as(ip), B, stride, out.ctypes.data_as(fp),
                                          nf.ctypes.data_as(ip)))
    return out, nf


@pytest.mark.parametrize("B,F", [(96, 1000), (33, 1473)])
def test_log_mel_long_across_frame_chunk_seams(hip, micro_cfg, micro_weights, B, F):
    """The long path runs frames / DFT / mel over chunks of nt frames of all rows at once: B = 96 rows of 1000 frames take chunks of 480
    (seams at 480 and 960), B = 33 rows of 1473 frames chunks of 1440 and a last one of 33.  A row alone takes one chunk, and has to
    give the same bits."""
    from oracle import logmel_oracle as lo
    from test_frontend_ref import long_chunk_frames
    nt = long_chunk_frames(F, B)
    assert nt < F and long_chunk_frames(F, 1) >= F, "the case no longer crosses a chunk seam"
    assert (nt, F % nt) == {96: (480, 40), 33: (1440, 33)}[B]
    stride = 160 * F
    m = make_model(micro_cfg, micro_weights, max_batch=2)
    distinct = [lo.synth_audio(60 + k, stride) for k in range(4)]
    buf = np.stack([distinct[b % 4] for b in range(B)])
    n = np.full(B, stride, np.int32)
    short = {5: stride - 1, B // 2: 160 * (F // 2) + 7, B - 1: 1234}  # the samples behind a length stay in the buffer
    for b, v in short.items():
        n[b] = v
    mel, nf = log_mel_long_raw(m, buf, n)
    assert mel.shape == (B, micro_cfg.n_mels, F)
    assert nf.tolist() == [min(-(-int(v) // 160), F) for v in n]
    for b in (0, B // 2, B - 1):
        alone, nf1 = log_mel_long_raw(m, buf[b:b + 1], n[b:b + 1])
        assert nf1[0] == nf[b]
        assert np.array_equal(alone[0].view(np.uint32), mel[b].view(np.uint32)), b
    for b in list(range(4)) + sorted(short):  # the four recordings and the three shortened rows
        err = np.abs(mel[b] - lo.log_mel(buf[b, :n[b]], n_frames=F, n_mels=micro_cfg.n_mels))
        assert err.max() < 2e-3 and err.mean() < 1e-4, (b, int(n[b]), err.max(), err.mean())
    for b in range(4, B):  # every copy of a recording equals the first
        if b not in short:
            assert np.array_equal(mel[b].view(np.uint32), mel[b % 4].view(np.uint32)), b
    m.close()
