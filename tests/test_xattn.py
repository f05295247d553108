"""Cross-attention over the bf16 encoder output with the K/V projections absorbed (models with bf16 encoder operands and an fp32
K/V cache): q' = (scale·q_h)·Wk_h is handed to the MFMA sweep as three bf16 terms, and so are the softmax weights.

CPU: the three-way split reproduces fp32 values of both kinds exactly.  GPU: a known-answer test at the fp32 bar (Wk / Wv and
the encoder output pre-rounded to bf16, so the oracle computes the same function in fp32), and the bitwise invariances of the
path (block prefill == stepwise, batch == singles)."""
import numpy as np
import pytest


def split3(x):  # restatement of split3_1 in kernels_decoder.hip
    x = np.ascontiguousarray(x, np.float32)
    h = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r1 = x - h
    m = (r1.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return h, m, r1 - m


def test_split3_of_absorbed_queries_and_softmax_weights_is_exact():
    rng = np.random.default_rng(11)
    q = (rng.standard_normal(300000) * 10.0 ** rng.uniform(-3, 2, 300000)).astype(np.float32)  # q' = scale·q·Wk: O(1e-3..1e2)
    # exp(s - m) in (0, 1] down to e^-60 (the split is exact while its third term is a normal number: p > 2^-110)
    p = np.exp(-rng.uniform(0, 60, 300000)).astype(np.float32)
    p = np.concatenate([p, np.float32([1.0, 0.0, np.nextafter(np.float32(1), np.float32(0))])])
    for x in (q, p):
        h, m, l = split3(x)
        for part in (h, m, l):
            assert not np.any(part.view(np.uint32) & np.uint32(0xFFFF))  # bf16 values
        assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), x.astype(np.float64))


def _bf16(a):
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()
    import whisper_mojo_amd as pkg
    return pkg


def _model(cfg, w, max_batch, coalesce=0):
    from whisper_mojo_amd.loader import WeightLoader
    from whisper_mojo_amd.whisper import Whisper
    m = Whisper(cfg, compute_dtype=1, kv_dtype=0, max_batch=max_batch, decoder_fp32=True, coalesce=coalesce)
    m.load(WeightLoader.from_array(w))
    return m


@pytest.mark.gpu
def test_xattn_kat_at_fp32_bar_195_steps(hip, tiny_cfg, tiny_weights):
    """Every weight and the encoder output pre-rounded to bf16: the headline precision's only 16-bit roundings (Wk / Wv and X
    in bf16) are then exact, and the path must match the oracle's fp32 arithmetic at the fp32 bar — 5e-5 on the logits of all
    196 teacher-forced positions, the same top-1 wherever the oracle's margin exceeds 1e-3."""
    from oracle import oracle
    from whisper_mojo_amd.whisper import KVCache
    w = _bf16(tiny_weights)
    from whisper_mojo_amd import synth
    ref = oracle.OracleModel(tiny_cfg, w)
    enc = _bf16(ref.encode(synth.synth_mel(tiny_cfg, 1000)))
    want, want_lg = ref.transcribe(enc_out=enc, eot=-1, max_loop=195, want_logits=True)
    m = _model(tiny_cfg, w, 64)  # max_batch 64: the headline's key chunking (8 chunks, several tiles per wave, cross-tile rescale)
    cache = KVCache(m, 1)
    lg = [m.decoder.forward(want[:4].tolist(), enc, cache, start_pos=0)]
    for i in range(4, len(want) - 1):
        lg.append(m.decoder.forward([int(want[i])], None, cache, start_pos=cache.current_len - 1))
    lg = np.stack(lg)
    assert lg.shape == want_lg.shape == (196, tiny_cfg.vocab_size)
    err = np.abs(lg - want_lg).max()
    print(f"absorbed cross-attention KAT: max |logit - oracle| {err:.2e} over {len(lg)} positions")
    assert err < 5e-5, err
    s = np.sort(want_lg, 1)
    clear = (s[:, -1] - s[:, -2]) > 1e-3
    assert clear.sum() >= 190
    assert np.array_equal(lg.argmax(1)[clear], want_lg.argmax(1)[clear])
    m.close()


@pytest.mark.gpu
def test_xattn_prefill_and_batch_invariance_bitwise(hip, tiny_cfg, tiny_weights):
    """At the path's own precision: the 4-token block prefill equals four single steps, and a batch of three equals each
    utterance alone, bit for bit (key chunks per utterance are a function of the model's max_batch only)."""
    from whisper_mojo_amd import synth
    from whisper_mojo_amd.whisper import KVCache
    m = _model(tiny_cfg, tiny_weights, 4)
    mels = np.stack([synth.synth_mel(tiny_cfg, 1000 + i) for i in range(3)])
    prompt = [50258, 50259, 50359, 50363]
    follow = [50364, 440, 1002, 13, 50257, 291]

    def run(mel_rows, block):
        B = len(mel_rows)
        cache = KVCache(m, B)
        m.encoder.forward(mel_rows, cache)
        if block:
            out = [m.decoder.forward(np.array([prompt] * B), None, cache, start_pos=0)]
        else:
            for i, t in enumerate(prompt):
                lg = m.decoder.forward(np.array([[t]] * B), None, cache, start_pos=i)
            out = [lg]
        for t in follow:
            out.append(m.decoder.forward(np.array([[t]] * B), None, cache, start_pos=cache.current_len - 1))
        return np.stack(out, 1)

    block = run(mels, True)
    assert np.array_equal(block, run(mels, False))
    for b in range(3):
        assert np.array_equal(block[b], run(mels[b:b + 1], True)[0])
    assert np.array_equal(m.transcribe_batch(mels, max_loop=24, ignore_eot=True),
                          [m.transcribe_batch(mels[b], max_loop=24, ignore_eot=True)[0] for b in range(3)])
    m.close()


@pytest.mark.gpu
def test_xattn_bench_protocol_equals_synchronous_passes(hip, tiny_cfg, tiny_weights):
    """The benched form at this path's precision: 64 clips per submit, coalesce = 2, eight submits in flight (four 128-row
    passes), 1 prefill + 99 decode steps — every submit's ids equal one synchronous pass of its batch, bit for bit."""
    import ctypes as C
    from whisper_mojo_amd import _lib
    L = _lib.lib()
    mels = np.empty((128, 80, 3000), np.float32)
    for i in range(128):
        L.wm_synth_mel_host(2000 + i, 80, 3000, mels[i].ctypes.data_as(C.POINTER(C.c_float)))
    kw = dict(max_loop=99, ignore_eot=True)
    plain = _model(tiny_cfg, tiny_weights, 64)
    want = [plain.transcribe_batch(mels[:64], **kw), plain.transcribe_batch(mels[64:], **kw)]
    plain.close()
    m = _model(tiny_cfg, tiny_weights, 64, coalesce=2)
    order = [0, 1, 1, 0, 0, 1, 1, 0]
    for slot, half in enumerate(order):
        m.transcribe_submit(mels[64 * half:64 * half + 64], slot=slot, **kw)
    for slot, half in enumerate(order):
        assert m.transcribe_wait(slot) == want[half], slot
    m.close()
