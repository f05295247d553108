"""GPU: token-level timestamps (wm_*_tt, kernels_align.hip) against HF's _extract_token_timestamps (fixtures of
tools/make_golden_token_timestamps.py) and against the CPU restatement of tests/test_token_timestamps.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from test_token_timestamps import restate_times

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()
    return True


def make_model(cfg, weights, hf_mode=False, **kw):
    from whisper_mojo_amd import GELU_ERF, GELU_TANH, POS_HF, POS_REF
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, gelu_mode=GELU_ERF if hf_mode else GELU_TANH, pos_mode=POS_HF if hf_mode else POS_REF, **kw)
    m.load(WeightLoader.from_array(weights))
    return m


def stream(name, mode):
    g = golden(f"token_timestamps_{name}_{mode}")
    from whisper_mojo_amd import WhisperConfig, synth
    cfg = WhisperConfig.micro() if name == "micro" else WhisperConfig.tiny()
    mels = np.stack([synth.synth_mel(cfg, int(g[f"c{c}_mel_seed"])) for c in range(3)])
    return g, mels


def test_kat_op_token_times(hip):
    from whisper_mojo_amd import _lib
    g = golden("token_timestamps_tables")
    n_prompt = int(g["n_prompt"])
    fp = C.POINTER(C.c_float)
    for name in g["names"]:
        name = str(name)
        w = np.ascontiguousarray(g[name + "_q"].astype(np.float32) / np.float32(65536))
        n_sel, R, F = w.shape
        want = g[name + "_times"]
        got = np.full(n_prompt + R + 1, -7.0, np.float32)
        _lib.check(_lib.lib().wm_op_token_times(got.ctypes.data_as(fp), w.ctypes.data_as(fp), n_sel, R, F, n_prompt))
        np.testing.assert_array_equal(got, want, err_msg=name)


def test_capture_kat_micro_fp32(hip, micro_cfg, micro_weights):
    """wm_alignment_weights after a micro fp32 pass = HF's cross-attention probabilities of the selected heads, to 1e-6."""
    for mode in ("hf", "ref"):
        g, mels = stream("micro", mode)
        m = make_model(micro_cfg, micro_weights, hf_mode=mode == "hf", max_batch=3)
        m.set_alignment_heads([tuple(p) for p in g["heads"]])
        L = int(g["max_loop"])
        ids, times = m.transcribe_batch(mels, prompt=tuple(g["prompt"]), eot=-1, max_loop=L, return_token_timestamps=True)
        W = m.alignment_weights()
        assert W.shape == (3, len(g["heads"]), L, micro_cfg.n_audio_ctx)
        for c in range(3):
            assert ids[c] == g[f"c{c}_ids"].tolist()
            np.testing.assert_allclose(W[c], g[f"c{c}_probs"], rtol=0, atol=1e-6)
            np.testing.assert_array_equal(np.asarray(times[c], np.float32), g[f"c{c}_times_full"])
        m.close()


@pytest.mark.parametrize("name", ["micro", "tiny"])
@pytest.mark.parametrize("mode", ["hf", "ref"])
def test_end_to_end_fp32_matches_hf(hip, name, mode, micro_cfg, micro_weights, tiny_cfg, tiny_weights):
    cfg, w = (micro_cfg, micro_weights) if name == "micro" else (tiny_cfg, tiny_weights)
    g, mels = stream(name, mode)
    heads = [tuple(p) for p in g["heads"]]
    prompt, eot, L, nf = tuple(g["prompt"]), int(g["eot"]), int(g["max_loop"]), g["n_frames"]
    m = make_model(cfg, w, hf_mode=mode == "hf", max_batch=4)
    m.set_alignment_heads(heads)
    cut = [g[f"c{c}_ids"][:int(g[f"c{c}_n_cut"])].tolist() for c in range(3)]
    # B = 1, uncut loop, with and without n_frames
    for c in range(3):
        for fr, key in ((None, "full"), ([int(nf[c])], "full_nf")):
            ids, times = m.transcribe_batch(mels[c:c + 1], prompt=prompt, eot=-1, max_loop=L, return_token_timestamps=True, n_frames=fr)
            assert ids[0] == g[f"c{c}_ids"].tolist()
            np.testing.assert_array_equal(np.asarray(times[0], np.float32), g[f"c{c}_times_{key}"], err_msg=f"clip {c} {key}")
    # a batch that stops at a shared eot (ragged stop lengths where the clips differ)
    for fr, key in ((None, "cut"), (nf, "cut_nf")):
        ids, times = m.transcribe_batch(mels, prompt=prompt, eot=eot, max_loop=L, return_token_timestamps=True, n_frames=fr)
        for c in range(3):
            assert ids[c] == cut[c]
            np.testing.assert_array_equal(np.asarray(times[c], np.float32), g[f"c{c}_times_{key}"], err_msg=f"clip {c} {key}")
    # submit / wait, four in flight
    for k in range(4):
        c = k % 3
        m.transcribe_submit(mels[c:c + 1], slot=k, prompt=prompt, eot=eot, max_loop=L, return_token_timestamps=True, n_frames=[int(nf[c])])
    for k in range(4):
        c = k % 3
        ids, times = m.transcribe_wait(k)
        assert ids[0] == cut[c]
        np.testing.assert_array_equal(np.asarray(times[0], np.float32), g[f"c{c}_times_cut_nf"])
    m.close()
    # coalesce = 2: pairs of timestamp submits share one state, each gets its own rows
    m = make_model(cfg, w, hf_mode=mode == "hf", max_batch=2, coalesce=2)
    m.set_alignment_heads(heads)
    order = [(0, 1), (2, 0), (1, 2), (0, 2)]
    for k, (a, b) in enumerate(order):
        m.transcribe_submit(mels[[a, b]], slot=k, prompt=prompt, eot=eot, max_loop=L, return_token_timestamps=True, n_frames=nf[[a, b]])
    for k, (a, b) in enumerate(order):
        ids, times = m.transcribe_wait(k)
        for row, c in enumerate((a, b)):
            assert ids[row] == cut[c]
            np.testing.assert_array_equal(np.asarray(times[row], np.float32), g[f"c{c}_times_cut_nf"])
    m.close()


CONFIGS = {  # name: (model dims, Whisper kwargs)
    "f32": ("tiny", dict(compute_dtype=0, kv_dtype=0)),
    "bf16enc_f32kv": ("tiny", dict(compute_dtype=1, kv_dtype=0, decoder_fp32=True)),  # the absorbed cross-attention (xattn) path
    "bf16": ("tiny", dict(compute_dtype=1, kv_dtype=1)),
    "base_f16": ("base", dict(compute_dtype=2, kv_dtype=2)),
}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_non_interference_and_restatement(hip, config, tiny_cfg, tiny_weights):
    """Asking for timestamps leaves the ids bit-identical; the times equal the CPU restatement applied to the GPU's own weights."""
    from whisper_mojo_amd import WhisperConfig, synth
    dims, kw = CONFIGS[config]
    if dims == "tiny":
        cfg, w = tiny_cfg, tiny_weights
    else:
        cfg = WhisperConfig.base()
        w = synth.synth_weights(cfg, 0)
    mels = np.stack([synth.synth_mel(cfg, s) for s in (1000, 1001, 1017)])
    L = 40
    m = make_model(cfg, w, max_batch=3, **kw)
    want = m.transcribe_batch(mels, eot=-1, max_loop=L)
    m.set_alignment_heads([(cfg.n_layers - 1, 0), (1, cfg.n_heads - 1), (cfg.n_layers - 1, 2)])
    nf = np.asarray([2 * cfg.n_audio_ctx, 1777, 901], np.int32)
    ids, times = m.transcribe_batch(mels, eot=-1, max_loop=L, return_token_timestamps=True, n_frames=nf)
    assert ids == want
    W = m.alignment_weights()
    for c in range(3):
        R = len(ids[c]) - 4 - 1
        ref = restate_times(W[c][:, :R, :int(nf[c]) // 2], 4)
        np.testing.assert_array_equal(np.asarray(times[c], np.float32), ref, err_msg=f"{config} clip {c}")
    assert m.transcribe_batch(mels, eot=-1, max_loop=L) == want  # and a plain call after a timestamp call
    m.close()


def test_errors(hip, micro_cfg, micro_weights):
    from whisper_mojo_amd import _lib
    from whisper_mojo_amd import synth
    m = make_model(micro_cfg, micro_weights, max_batch=2)
    mels = synth.synth_mels(micro_cfg, 0, 2)
    kw = dict(prompt=(1, 2, 3, 4), eot=-1, max_loop=8)
    with pytest.raises(_lib.WhisperMiError, match=r"error -5\b"):  # WM_E_STATE: no alignment heads
        m.transcribe_batch(mels, return_token_timestamps=True, **kw)
    for bad in ([(2, 0)], [(0, 2)], [(0, 1), (0, 1)], [(-1, 0)], [(0, 0)] * 33):
        with pytest.raises(_lib.WhisperMiError, match=r"error -1\b"):  # WM_E_ARG
            m.set_alignment_heads(bad)
    m.set_alignment_heads([(1, 1), (0, 0)])
    for nf in ([200, 1], [0, 100], [201, 100]):
        with pytest.raises(_lib.WhisperMiError, match=r"error -1\b"):
            m.transcribe_batch(mels, return_token_timestamps=True, n_frames=nf, **kw)
    m.transcribe_submit(mels, slot=1, **kw)
    toks = np.zeros((2, 13), np.int32)
    n = np.zeros(2, np.int32)
    t = np.zeros((2, 13), np.float32)
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    rc = _lib.lib().wm_transcribe_wait_tt(m._h, 1, toks.ctypes.data_as(ip), n.ctypes.data_as(ip), t.ctypes.data_as(fp))
    assert rc == -5  # the pass was submitted without timestamps
    assert m.transcribe_wait(1) == m.transcribe_batch(mels, **kw)
    m.set_alignment_heads([])  # off again
    with pytest.raises(_lib.WhisperMiError, match=r"error -5\b"):
        m.transcribe_batch(mels, return_token_timestamps=True, **kw)
    m.close()


def test_pcm_entry(hip, micro_cfg, micro_weights):
    """transcribe_audio(return_token_timestamps=True): n_frames from the clip lengths; ids as without timestamps, times as the
    restatement on the pass's own weights."""
    from whisper_mojo_amd.frontend import transcribe_audio
    m = make_model(micro_cfg, micro_weights, max_batch=2)
    rng = np.random.default_rng(5)
    audios = [rng.standard_normal(n).astype(np.float32) * 0.1 for n in (16000 * 2, 9000)]
    kw = dict(prompt=(1, 2, 3, 4), eot=-1, max_loop=12)
    want = transcribe_audio(m, audios, **kw)
    m.set_alignment_heads([(1, 0), (0, 1)])
    ids, times = transcribe_audio(m, audios, return_token_timestamps=True, **kw)
    assert ids == want
    from whisper_mojo_amd import _lib
    out = np.zeros((2, 2, 12, micro_cfg.n_audio_ctx), np.float32)
    _lib.check(_lib.lib().wm_alignment_weights(m._h, 0, out.ctypes.data_as(C.POINTER(C.c_float))))
    for c, a in enumerate(audios):
        nf = min(2 * micro_cfg.n_audio_ctx, -(-len(a) // 160))
        R = len(ids[c]) - 5
        np.testing.assert_array_equal(np.asarray(times[c], np.float32), restate_times(out[c][:, :R, :nf // 2], 4))
    m.close()
