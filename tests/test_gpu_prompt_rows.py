"""GPU: per-utterance decoder prompts (wm_transcribe_rows, wm_op_attention_cached_lo).  The self-attention with a key
window against float64 (the bound of tests/test_gpu_decode_layer.py, taken over as it is) and, with key_lo = 0, bitwise against
wm_op_attention_cached; a ragged batch against HF's ids of every row decoded alone (tests/golden/prompt_rows_*_hf.npz, exact, every
row); order / pass independence; equal prompts == wm_transcribe bitwise, with the step graph recaptured both ways; the refusals."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from test_gpu_decode_layer import ODTS, _attn_check, _attn_inputs, _wt, prefill_counts
from test_gpu_decode_ops import DT_BF16, DT_F16, DT_F32
from test_gpu_parity import _attention_cached_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()
    return True


def _window_ref(q, k, v, H, lo, counts, q_B):
    """float64 over the keys [lo[u], counts[r]) of utterance u = r % q_B (or r); an empty window gives zeros"""
    out = np.zeros(q.shape, np.float64)
    for r in range(q.shape[0]):
        u = r % q_B if q_B > 0 else r
        if counts[r] > lo[u]:
            out[r] = _attention_cached_ref(q[r:r + 1], k[u:u + 1, lo[u]:counts[r]], v[u:u + 1, lo[u]:counts[r]], H)[0]
    return out


@pytest.mark.parametrize("kvdt", [DT_F32, DT_BF16, DT_F16])
@pytest.mark.parametrize("H", [2, 6, 8])
def test_key_window_single_query_vs_float64(hip, H, kvdt):
    """key_lo of 0, 1, mid and len (one key) in one call; the cache rows outside every window hold NaN and must not reach the
    output.  key_lo = 0 for every row is wm_op_attention_cached bit for bit."""
    wt = _wt()
    B = 4
    for i, t in enumerate((1, 7, 33, 130, 448)):
        r = np.random.default_rng(100 * H + t + kvdt)
        odt = ODTS[(i + H) % 3]
        q, k, v = _attn_inputs(r, B, t, H, kvdt, "random")
        lo = [0, min(1, t - 1), (t - 1) // 2, t - 1]
        kn, vn = k.copy(), v.copy()
        for b in range(B):
            kn[b, :lo[b]] = np.nan
            vn[b, :lo[b]] = np.nan
        pad = np.full((B, 2, 64 * H), np.nan, np.float32)
        out = np.zeros_like(q)
        wt.attention_cached(out, q, np.concatenate([kn, pad], 1), np.concatenate([vn, pad], 1), H, kv_dtype=kvdt, out_dtype=odt, len=t - 1,
                            key_lo=lo)
        _attn_check(f"lo H {H} kv {kvdt} t {t} out {odt}", out, _window_ref(q, k, v, H, lo, [t] * B, 0), odt)
        zero, plain = np.zeros_like(q), np.zeros_like(q)
        wt.attention_cached(zero, q, k, v, H, kv_dtype=kvdt, out_dtype=odt, len=t - 1, key_lo=[0] * B)
        wt.attention_cached(plain, q, k, v, H, kv_dtype=kvdt, out_dtype=odt, len=t - 1)
        np.testing.assert_array_equal(zero, plain)
        # a row's window result is what the row gives alone on a cache that starts at its window (the unpadded prompt)
        for b in range(B):
            one = np.zeros((1, 64 * H), np.float32)
            wt.attention_cached(one, q[b:b + 1], k[b:b + 1, lo[b]:], v[b:b + 1, lo[b]:], H, kv_dtype=kvdt, out_dtype=odt, len=t - 1 - lo[b])
            np.testing.assert_array_equal(one[0], out[b])


@pytest.mark.parametrize("kvdt,H,q_B", [(DT_F32, 2, 4), (DT_BF16, 6, 4), (DT_F16, 8, 4), (DT_F32, 6, 5)])
def test_key_window_causal_prefill_vs_float64(hip, kvdt, H, q_B):
    """The causal prefill form: row p·q_B + b sweeps [key_lo[b], len + 1 + p).  key_lo beyond a row's position is an empty window:
    zeros, finite.  key_lo = 0 is the plain prefill bit for bit."""
    wt = _wt()
    cap_rows = 40
    for length, P in ((0, 16), (16, 7), (5, 1)):
        r = np.random.default_rng(H + q_B + P + kvdt + length)
        q, k, v = _attn_inputs(r, P * q_B, cap_rows, H, kvdt, "random")
        k, v = k[:q_B].copy(), v[:q_B].copy()
        k[:, length + P:] = np.nan
        v[:, length + P:] = np.nan
        top = length + P - 1
        lo = ([0, 1, (length + P) // 2, top, length + 3][:q_B] + [2] * q_B)[:q_B]
        lo = [min(x, top) for x in lo]
        kn, vn = k.copy(), v.copy()
        for b in range(q_B):
            kn[b, :lo[b]] = np.nan
            vn[b, :lo[b]] = np.nan
        odt = ODTS[(P + H) % 3]
        counts = prefill_counts(P, q_B, length)
        out = np.full_like(q, 7.0)
        wt.attention_cached(out, q, kn, vn, H, kv_dtype=kvdt, out_dtype=odt, q_B=q_B, len=length, key_lo=lo)
        _attn_check(f"lo prefill H {H} kv {kvdt} q_B {q_B} len {length} P {P} out {odt}", out, _window_ref(q, k, v, H, lo, counts, q_B), odt)
        empty = [row for row in range(P * q_B) if counts[row] <= lo[row % q_B]]
        assert all((out[row] == 0).all() for row in empty)
        if P > 1 and length < top:
            assert empty  # some row of the case lies in front of its utterance's window
        zero, plain = np.zeros_like(q), np.zeros_like(q)
        wt.attention_cached(zero, q, k, v, H, kv_dtype=kvdt, out_dtype=odt, q_B=q_B, len=length, key_lo=[0] * q_B)
        wt.attention_cached(plain, q, k, v, H, kv_dtype=kvdt, out_dtype=odt, q_B=q_B, len=length)
        np.testing.assert_array_equal(zero, plain)


def test_key_window_refuses_bad_arguments(hip):
    from whisper_mojo_amd import _lib
    wt = _wt()
    E = _lib.WhisperMiError
    q, k = np.zeros((2, 128), np.float32), np.zeros((2, 64, 128), np.float32)
    with pytest.raises(E):  # the chunked form has no key window
        wt.attention_cached(np.zeros_like(q), q, k, k, 2, n_chunks=2, key_lo=[0, 0])
    with pytest.raises(E):
        wt.attention_cached(np.zeros_like(q), q, k, k, 2, len=10, key_lo=[0, -1])
    with pytest.raises(E):
        wt.attention_cached(np.zeros_like(q), q, k, k, 2, len=10, key_lo=[0, 65])
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    z = np.zeros_like(q)
    assert _lib.lib().wm_op_attention_cached_lo(z.ctypes.data_as(fp), q.ctypes.data_as(fp), k.ctypes.data_as(fp), k.ctypes.data_as(fp), 2, 64, 2,
                                                0, 1, 0, 0, 10, 0, None) == -1


# ---- wm_transcribe_rows ----------------------------------------------------------------------------------------------------------
def make_model(cfg, weights, **kw):
    from whisper_mojo_amd import GELU_ERF, POS_HF
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, gelu_mode=GELU_ERF, pos_mode=POS_HF, **kw)
    m.load(WeightLoader.from_array(weights))
    return m


def _fixture_rows(g, cfg, ts_on):
    from whisper_mojo_amd import synth
    rows = [r for r in range(int(g["n_rows"])) if int(g[f"r{r}_ts"]) == ts_on]
    mels = np.stack([synth.synth_mel(cfg, int(g[f"r{r}_seed"])) for r in rows])
    prompts = [g[f"r{r}_prompt"].tolist() for r in rows]
    want = [g[f"r{r}_ids"].tolist() for r in rows]
    kw = dict(eot=int(g["eos"]), max_loop=int(g["max_loop"]),
              timestamps=(int(g["timestamp_begin"]), int(g["no_ts"]), int(g["max_init"])) if ts_on else None)
    return mels, prompts, want, kw


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_ragged_batch_matches_hf_rows_fp32(hip, name, micro_cfg, micro_weights, tiny_cfg, tiny_weights):
    """One pass carries every prompt length of the fixture (1 .. 31 / 1 .. 228 ids); every row gives the ids HF gives for that
    recording decoded alone with its own prompt.  Then the same rows in another order, and split over max_batch-limited passes."""
    cfg, w = (micro_cfg, micro_weights) if name == "micro" else (tiny_cfg, tiny_weights)
    g = golden(f"prompt_rows_{name}_hf")
    m = make_model(cfg, w, max_batch=8)
    m2 = make_model(cfg, w, max_batch=2)
    for ts_on in (0, 1):
        mels, prompts, want, kw = _fixture_rows(g, cfg, ts_on)
        n = len(prompts)
        assert n >= 5 and len({len(p) for p in prompts}) == n
        got = m.transcribe_batch(mels, prompts=prompts, **kw)
        for b in range(n):
            assert got[b] == want[b], (name, ts_on, b, len(prompts[b]))
        perm = [(3 * i + 2) % n for i in range(n)] if n % 3 else list(reversed(range(n)))
        assert sorted(perm) == list(range(n))
        again = m.transcribe_batch(mels[perm], prompts=[prompts[i] for i in perm], **kw)
        assert again == [got[i] for i in perm]
        split = []
        for i in range(0, n, 2):  # passes of at most two rows: another longest prompt, another padding per row
            split += m2.transcribe_batch(mels[i:i + 2], prompts=prompts[i:i + 2], **kw)
        assert split == got
        # the pipelined entry
        m.transcribe_submit(mels, slot=2, prompts=prompts, **kw)
        assert m.transcribe_wait(2) == got
    m.close()
    m2.close()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_equal_prompts_are_wm_transcribe_bitwise(hip, prec, tiny_cfg, tiny_weights):
    """All rows carrying the same 4-id prompt through wm_transcribe_rows == wm_transcribe with that prompt; and wm_transcribe after
    it still gives what it gave before (the step graph is recaptured both ways)."""
    from whisper_mojo_amd import synth
    from test_gpu_parity import make_model as parity_model
    m = parity_model(tiny_cfg, tiny_weights, dtype=0 if prec == "fp32" else 1, max_batch=4)
    mels = np.stack([synth.synth_mel(tiny_cfg, 1000 + b) for b in range(3)])
    prompt = [50258, 50259, 50359, 50363]
    kw = dict(eot=50257, max_loop=40)
    before = m.transcribe_batch(mels, prompt=prompt, **kw)
    rows = m.transcribe_batch(mels, prompts=[prompt] * 3, **kw)
    assert rows == before
    after = m.transcribe_batch(mels, prompt=prompt, **kw)
    assert after == before
    assert m.transcribe_batch(mels, prompts=[prompt] * 3, **kw) == before
    # with the timestamp rules and a one-id prompt among the rows
    ts = dict(eot=50257, max_loop=30, timestamps=(50364, 50363, 50))
    alone = [m.transcribe_batch(mels[b:b + 1], prompt=p, **ts)[0] for b, p in enumerate(([50258], prompt[:3], prompt[:3]))]
    assert m.transcribe_batch(mels, prompts=[[50258], prompt[:3], prompt[:3]], **ts) == alone
    m.close()


def test_refusals_launch_nothing(hip, micro_cfg, micro_weights):
    from whisper_mojo_amd import _lib, synth
    m = make_model(micro_cfg, micro_weights, max_batch=2)
    m.set_alignment_heads([(0, 0)])
    mels = np.stack([synth.synth_mel(micro_cfg, 5), synth.synth_mel(micro_cfg, 6)])
    kw = dict(eot=900, max_loop=20, timestamps=(941, 940, 50))
    good = [[7, 8, 1, 2, 3], [1, 2, 3]]
    want = m.transcribe_batch(mels, prompts=good, **kw)

    def refused(prompts, **over):
        o = dict(kw)
        o.update(over)
        with pytest.raises(_lib.WhisperMiError, match=r"error -1:"):
            m.transcribe_batch(mels, prompts=prompts, **o)
        assert m.loop_steps(0) == steps  # nothing ran on the slot
        assert m.transcribe_batch(mels, prompts=good, **kw) == want  # the next valid call works

    steps = m.loop_steps(0)
    refused([[1, 2, 3], []])                                       # prompt_len[b] = 0
    refused([[1, 2, 3], [1, micro_cfg.vocab_size, 3]])             # id out of range
    refused([[1, 2, 3], [1, -4, 3]])
    refused([list(range(4, 4 + 44)), [1, 2, 3]])                   # Lmax + 1 + max_loop = 65 > n_text_ctx
    refused(good, max_loop=micro_cfg.n_text_ctx - 5)
    with pytest.raises(ValueError):                                # no token timestamps with per-row prompts
        m.transcribe_batch(mels, prompts=good, return_token_timestamps=True, **kw)
    with pytest.raises(ValueError):
        m.transcribe_submit(mels, slot=1, prompts=good, return_token_timestamps=True, **kw)
    with pytest.raises(ValueError):
        m.transcribe_batch(mels, prompts=good[:1], **kw)
    # C level: prompt_stride shorter than a row, null tables
    opts, _keep = m._opts((1, 2, 3), 900, 20, False, timestamps=(941, 940, 50))
    ip = C.POINTER(C.c_int32)
    tab, lens = np.asarray([[1, 2, 3], [1, 2, 3]], np.int32), np.asarray([3, 4], np.int32)
    toks, n = np.zeros((2, 64), np.int32), np.zeros(2, np.int32)
    args = (m._h, C.c_void_p(mels.ctypes.data), 0, 2, C.byref(opts))
    L = _lib.lib()
    assert L.wm_transcribe_rows(*args, tab.ctypes.data_as(ip), lens.ctypes.data_as(ip), 3, toks.ctypes.data_as(ip), n.ctypes.data_as(ip)) == -1
    assert L.wm_transcribe_rows(*args, None, lens.ctypes.data_as(ip), 3, toks.ctypes.data_as(ip), n.ctypes.data_as(ip)) == -1
    assert L.wm_transcribe_rows(*args, tab.ctypes.data_as(ip), None, 3, toks.ctypes.data_as(ip), n.ctypes.data_as(ip)) == -1
    assert L.wm_transcribe_submit_rows(m._h, 9, C.c_void_p(mels.ctypes.data), 0, 2, C.byref(opts), tab.ctypes.data_as(ip), lens.ctypes.data_as(ip), 3) == -1
    assert m.transcribe_batch(mels, prompts=good, **kw) == want
    m.close()
    # coalesce = 2: a per-row submit runs alone and leaves a held plain submit its own result
    mc = make_model(micro_cfg, micro_weights, max_batch=2, coalesce=2)
    plain = mc.transcribe_batch(mels, prompt=(1, 2, 3), **kw)
    mc.transcribe_submit(mels, slot=0, prompt=(1, 2, 3), **kw)  # held, waiting for a partner
    mc.transcribe_submit(mels, slot=1, prompts=good, **kw)
    assert mc.transcribe_wait(1) == want
    assert mc.transcribe_wait(0) == plain
    mc.close()
