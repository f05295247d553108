"""GPU: sampling_rate= and int16 input through the audio entries, on the micro model with synthetic weights.

Every entry with sampling_rate= must return exactly what the same entry returns for frontend.resample's output: the resampler runs
first and nothing else changes.  The chunked entry keeps the resampled samples on the device, the others pass them through host memory;
both must give the same ids, segments and times.  The micro model's window is 2 s, so the long recordings are 5 s: 2.5 windows."""
import numpy as np
import pytest

from test_gpu_long_form import make_model

pytestmark = pytest.mark.gpu

CHUNK_S = 2.0
FIRST_SPECIAL, TB = 890, 899
KW = dict(prompt=(891, 892, 893), eot=890, max_loop=20, suppress_tokens=tuple(range(891, 899)), timestamps=(TB, 898, 50), no_repeat_ngram_size=2)
KW_AUDIO = dict(prompt=(891, 892, 893), eot=890, max_loop=12)
KW_LONG = dict(prompt=(1, 2, 3), eot=900, max_loop=30, timestamps=(941, 940, 50))


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def model(hip, micro_cfg, micro_weights):
    m = make_model(micro_cfg, micro_weights, max_batch=2)
    yield m
    m.close()


def chords(sr, seconds, seed):
    """a new three-tone chord every 0.4 s, below 7 kHz so that every rate here carries it"""
    rng = np.random.default_rng(seed)
    n, step = int(sr * seconds), int(0.4 * sr)
    x = np.zeros(n, np.float32)
    for b0 in range(0, n, step):
        t = np.arange(min(step, n - b0)) / float(sr)
        x[b0:b0 + len(t)] = sum(rng.uniform(0.02, 0.3) * np.sin(2 * np.pi * rng.uniform(100, 7000) * t) for _ in range(3)).astype(np.float32)
    return x


def as_int16(x):
    return np.round(x * 32767.0).astype(np.int16)


def test_resample_returns_the_op_rows(model, hip):
    from whisper_mojo_amd import frontend
    rows = [chords(44100, 0.31, 1), chords(44100, 0.05, 2)]
    got = frontend.resample(model, rows, 44100)
    want, n = hip.op_resample(rows, 44100)
    assert [g.dtype for g in got] == [np.float32] * 2 and [len(g) for g in got] == n.tolist()
    for b in range(2):
        assert np.array_equal(got[b], want[b, :n[b]])
    # the packed result is zero behind each row: what the model path hands on
    out, n2 = frontend._resample(model, rows, 44100, False)
    assert (out[1, n2[1]:] == 0).all() and out.shape[1] == n2[0]
    assert frontend.resample(model, rows, 44100)[1].tolist() == got[1].tolist()  # the cached table


def test_transcribe_audio_at_48k_and_int16_at_44k(model):
    from whisper_mojo_amd import frontend
    a48 = chords(48000, 1.7, 3)
    want = frontend.transcribe_audio(model, frontend.resample(model, [a48], 48000), **KW_AUDIO)
    assert frontend.transcribe_audio(model, [a48], sampling_rate=48000, **KW_AUDIO) == want
    assert len(want[0]) > len(KW_AUDIO["prompt"])
    i44 = as_int16(chords(44100, 1.3, 4))
    want = frontend.transcribe_audio(model, frontend.resample(model, [i44], 44100), **KW_AUDIO)
    assert frontend.transcribe_audio(model, [i44], sampling_rate=44100, **KW_AUDIO) == want
    # int16 is scaled by 1 / 32768: the same clip as float32 gives the same samples
    f = frontend.resample(model, [i44.astype(np.float32) / np.float32(32768.0)], 44100)
    assert np.array_equal(f[0], frontend.resample(model, [i44], 44100)[0])


def test_log_mel_at_44k_bit_for_bit(model):
    from whisper_mojo_amd import frontend
    a44 = [chords(44100, 1.1, 5), chords(44100, 2.6, 6)]
    want = frontend.log_mel(model, frontend.resample(model, a44, 44100))
    got = frontend.log_mel(model, a44, sampling_rate=44100)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got, frontend.log_mel(model, a44))  # read as 16 kHz the same samples are another clip
    ml, nf = frontend.log_mel_long(model, a44, sampling_rate=44100)
    wl, wf = frontend.log_mel_long(model, frontend.resample(model, a44, 44100))
    assert nf.tolist() == wf.tolist() and np.array_equal(ml.view(np.uint32), wl.view(np.uint32))


def test_chunked_at_48k_keeps_ids_segments_and_times(model):
    from whisper_mojo_amd import frontend
    rec = [chords(48000, 5.0, 7), chords(48000, 2.2, 8)]
    at16 = frontend.resample(model, rec, 48000)
    assert [len(a) for a in at16] == [80000, 35200]
    for mode in (False, True):
        want = model.transcribe_chunked(at16, CHUNK_S, return_chunks=True, return_timestamps=mode, first_special=FIRST_SPECIAL, **KW)
        got = model.transcribe_chunked(rec, CHUNK_S, return_chunks=True, return_timestamps=mode, first_special=FIRST_SPECIAL,
                                       sampling_rate=48000, **KW)
        assert got == want, mode
        assert len(got[0]["chunks"]) >= 3 and got[0]["chunks"][1][0] > 0  # several chunks, their starts in seconds of audio
    one = frontend.transcribe_audio_chunked(model, as_int16(rec[1]), CHUNK_S, first_special=FIRST_SPECIAL, sampling_rate=48000, **KW)
    assert isinstance(one, dict)  # a single array in, a single dict out
    assert one == frontend.transcribe_audio_chunked(model, frontend.resample(model, [as_int16(rec[1])], 48000)[0], CHUNK_S,
                                                    first_special=FIRST_SPECIAL, **KW)


def test_long_form_at_48k_keeps_ids_segments_and_times(model):
    from whisper_mojo_amd import frontend
    rec = [chords(48000, 5.0, 9), chords(48000, 3.1, 10)]
    want = frontend.transcribe_audio_long_form(model, frontend.resample(model, rec, 48000), **KW_LONG)
    got = frontend.transcribe_audio_long_form(model, rec, sampling_rate=48000, **KW_LONG)
    assert got == want
    assert len(got[0]["sequence"]) > 0 and got[0]["segments"][-1]["end"] <= 5.0 + 1e-9  # seconds of audio, not of 48 kHz samples


def test_the_default_rate_is_the_old_path(model):
    from whisper_mojo_amd import frontend
    a = [chords(16000, 1.4, 11), chords(16000, 0.6, 12)]
    assert frontend.transcribe_audio(model, a, sampling_rate=16000, **KW_AUDIO) == frontend.transcribe_audio(model, a, **KW_AUDIO)
    assert np.array_equal(frontend.log_mel(model, a, sampling_rate=16000), frontend.log_mel(model, a))
    long = [chords(16000, 5.0, 13)]
    assert frontend.transcribe_audio_long_form(model, long, sampling_rate=16000, **KW_LONG) == frontend.transcribe_audio_long_form(model, long, **KW_LONG)
    kw = dict(KW, first_special=FIRST_SPECIAL, return_timestamps=True)
    assert model.transcribe_chunked(long, CHUNK_S, sampling_rate=16000, **kw) == model.transcribe_chunked(long, CHUNK_S, **kw)
    assert frontend.resample(model, a, 16000)[0].tolist() == a[0].tolist()  # the identity


def test_refusals_leave_the_model_usable(model, hip):
    from whisper_mojo_amd import frontend
    a = [chords(16000, 0.2, 14)]
    with pytest.raises(hip.WhisperMiError, match="sr_in.*1024"):
        frontend.transcribe_audio(model, a, sampling_rate=16001, **KW_AUDIO)
    with pytest.raises(ValueError, match="sampling_rate"):
        frontend.log_mel(model, a, sampling_rate=0)
    import torch
    with pytest.raises(ValueError, match="device PCM"):
        model.transcribe_chunked(torch.zeros(1, 32000, device="cuda"), CHUNK_S, sampling_rate=48000, first_special=FIRST_SPECIAL, **KW)
    assert frontend.transcribe_audio(model, a, **KW_AUDIO) == frontend.transcribe_audio(model, a, sampling_rate=16000, **KW_AUDIO)
