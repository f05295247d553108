"""GPU: chunked long-form transcription end to end (wm_transcribe_chunked) on the micro model with synthetic PCM.

The micro model's window is 2 s (n_audio_ctx 100), and a chunk may not exceed the model's window, so chunk_length_s is 2.0 here: the
recordings of 0.5 s, 30 s, 30 s + 1 sample and 70 s become 1, 22, 22 and 52 chunks, and one window and one window + 1 sample are
added because those are the lengths at which the table goes from one chunk to two.  max_batch = 2, so the longer recordings span
many passes and both slots, and passes mix the chunks of neighbouring recordings.

Every chunk's ids must equal, bit for bit, what that chunk's samples give when decoded alone (the library is batch invariant):
frontend.log_mel + transcribe_batch with the same options, and frontend.transcribe_audio where it takes the options
(test_asymmetric_strides).  "sequence" must equal merge_ref (tests/test_chunked_ref.py, pinned to HF's _find_longest_common_sequence
by the fixture) of those lists.  The decoder prompt lies above first_special, as Whisper's real prompt does, so it is stripped; the
ids above first_special are suppressed and no_repeat_ngram_size = 1 keeps the synthetic model from echoing one id, so every chunk
yields 12 distinct text ids.

The audio is what makes these comparisons mean something.  Stationary noise decodes to the same 12 ids in every chunk (each chunk
has its own clamp max), and then a chunk gathered from the wrong place, packed into the wrong row or encoded from the other slot's
log-mel would still "equal that chunk decoded alone".  So every recording is a sequence of three-tone chords, a new chord every
21 334 samples (one chunk step), each recording from its own seed: neighbouring chunks, and chunks of different recordings, decode
differently.  The micro model tells only so many chords apart within 12 ids — on the CPU reference 67 of the 100 chunks of the main
case are distinct and 3 neighbours in table order are equal — so test_the_chunks_differ asserts at least 60 distinct and at most 8
equal neighbours; a systematic routing error moves many chunks and cannot hide in that remainder.  The merges are no longer
trivial either: unrelated 12-id lists still share a few positions, so HF's fault-tolerant rule merges some pairs and concatenates
others, each as merge_ref says; test_same_audio_twice_is_halved asks for a full fold on purpose, the same window fed twice under
strides (0, 0).  The rules one by one are tests/test_gpu_chunk_ops.py's."""
import numpy as np
import pytest

from test_chunked_ref import merge_ref
from test_gpu_long_form import make_model

pytestmark = pytest.mark.gpu

SR = 16000
CHUNK_S = 2.0
FIRST_SPECIAL = 900
KW = dict(prompt=(950, 951, 952, 953), eot=-1, max_loop=11, suppress_tokens=tuple(range(900, 1000)), no_repeat_ngram_size=1)  # 12 new ids
KW_AUDIO = dict(prompt=(950, 951, 952, 953), eot=-1, max_loop=11, no_repeat_ngram_size=1)  # what frontend.transcribe_audio takes
LANGS = list(range(960, 972))
CHORD = 21334  # samples per chord: the step of 2 s chunks under the default strides
SECONDS = {"0.5s": 8000, "window": 32000, "window+1": 32001, "30s": 480000, "30s+1": 480001, "70s": 1120000}


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def recordings():
    out = {}
    for k, (name, n) in enumerate(SECONDS.items()):
        rng = np.random.default_rng(2040 + k)
        x = np.zeros(n, np.float32)
        for b0 in range(0, n, CHORD):  # a new three-tone chord every chunk step
            t = np.arange(min(CHORD, n - b0)) / float(SR)
            x[b0:b0 + len(t)] = sum(rng.uniform(0.02, 0.5) * np.sin(2 * np.pi * rng.uniform(100, 7500) * t) for _ in range(3)).astype(np.float32)
        out[name] = x
    return out


@pytest.fixture(scope="module")
def model(hip, micro_cfg, micro_weights):
    m = make_model(micro_cfg, micro_weights, max_batch=2)
    yield m
    m.close()


def chunk_refs(model, hip, audios, chunk_s=CHUNK_S, stride_s=None, call=None):
    """per recording the (start, len, stride_l, stride_r) in samples and the ids of every chunk decoded on its own"""
    from whisper_mojo_amd import frontend
    cl, sl, sr = hip.chunk_strides(chunk_s, stride_s)
    tab = hip.chunk_table([len(a) for a in audios], cl, sl, sr)
    cuts = [audios[r][s:s + n] for r, s, n, _, _, _ in tab.tolist()]
    call = call or (lambda group: model.transcribe_batch(frontend.log_mel(model, group), **KW))
    ids = []
    for k in range(0, len(cuts), 2):
        ids += call(cuts[k:k + 2])
    per = [[] for _ in audios]
    for row, i in zip(tab.tolist(), ids):
        per[row[0]].append((tuple(row[1:5]), i))
    return per


def check(got, ref):
    assert len(got) == len(ref)
    for r, (g, want) in enumerate(zip(got, ref)):
        assert len(g["chunks"]) == len(want), r
        for k, (c, (cut, ids)) in enumerate(zip(g["chunks"], want)):
            assert c[:4] == tuple(v / SR for v in cut), (r, k)
            assert c[4] == ids, (r, k)
        assert g["sequence"] == merge_ref([ids for _, ids in want], FIRST_SPECIAL), r


@pytest.fixture(scope="module")
def all_six(model, hip, recordings):
    audios = [recordings[n] for n in SECONDS]
    got, stats = model.transcribe_chunked(audios, CHUNK_S, return_chunks=True, first_special=FIRST_SPECIAL, return_stats=True, **KW)
    return audios, got, stats, chunk_refs(model, hip, audios)


def test_chunks_and_sequence_of_every_length(all_six):
    audios, got, stats, ref = all_six
    assert [len(r) for r in ref] == [1, 1, 2, 22, 22, 52]
    check(got, ref)
    assert stats == {"chunks": 100, "passes": 50}  # max_batch = 2: passes run across recording boundaries
    for r in ref:  # 16 ids per chunk, the four prompt ids stripped, 12 text ids left
        assert all(sum(t < FIRST_SPECIAL for t in ids) == 12 for _, ids in r)


def test_the_chunks_differ(all_six):
    """what makes the equalities above able to fail: neighbouring chunks and chunks of different recordings decode differently"""
    _, got, _, ref = all_six
    flat = [tuple(ids) for r in ref for _, ids in r]
    assert len(flat) == 100
    assert len(set(flat)) >= 60, len(set(flat))
    assert sum(a == b for a, b in zip(flat, flat[1:])) <= 8
    assert sum(a == b for a, b in zip(flat[::2], flat[1::2])) <= 4  # the two rows of a pass
    long_ones = [g["sequence"] for g in got[3:]]
    assert len({tuple(s) for s in long_ones}) == 3 and all(len(s) > 24 for s in long_ones)  # neither folded into one list nor alike


@pytest.mark.parametrize("name", ["0.5s", "window+1", "30s+1"])
def test_a_recording_alone_equals_itself_in_the_batch(model, all_six, recordings, name):
    _, got, _, _ = all_six
    alone = model.transcribe_chunked(recordings[name], CHUNK_S, return_chunks=True, first_special=FIRST_SPECIAL, **KW)
    assert alone == got[list(SECONDS).index(name)]
    assert model.transcribe_chunked(recordings[name], CHUNK_S, first_special=FIRST_SPECIAL, **KW) == {"sequence": alone["sequence"]}


def test_coalesced_model_gives_the_same_ids(hip, micro_cfg, micro_weights, all_six, recordings):
    _, got, _, _ = all_six
    m = make_model(micro_cfg, micro_weights, max_batch=2, coalesce=2)
    names = ["window+1", "30s+1", "0.5s"]  # 2 + 22 + 1 chunks: 13 passes, so pairs of passes and an odd one left over that runs alone
    res = m.transcribe_chunked([recordings[n] for n in names], CHUNK_S, return_chunks=True, first_special=FIRST_SPECIAL, **KW)
    m.close()
    assert res == [got[list(SECONDS).index(n)] for n in names]


def test_asymmetric_strides(model, hip, recordings):
    audios = [recordings["30s"][:200001], recordings["window+1"]]
    from whisper_mojo_amd import frontend
    got = model.transcribe_chunked(audios, 1.5, (0.1, 0.4), return_chunks=True, first_special=FIRST_SPECIAL, **KW)
    check(got, chunk_refs(model, hip, audios, 1.5, (0.1, 0.4)))
    got = model.transcribe_chunked(audios, 1.5, (0.1, 0.4), return_chunks=True, first_special=FIRST_SPECIAL, **KW_AUDIO)
    check(got, chunk_refs(model, hip, audios, 1.5, (0.1, 0.4), call=lambda group: frontend.transcribe_audio(model, group, **KW_AUDIO)))


def test_pcm_on_the_device_equals_pcm_on_the_host(model, all_six, recordings):
    import torch
    _, got, _, _ = all_six
    names = ["30s+1", "0.5s", "window+1"]
    n = [len(recordings[k]) for k in names]
    dev = torch.full((3, max(n) + 5), 7.0, dtype=torch.float32, device="cuda")  # a stride beyond the longest, junk past each length
    for r, k in enumerate(names):
        dev[r, :n[r]] = torch.from_numpy(recordings[k]).cuda()
    res = model.transcribe_chunked(dev, CHUNK_S, return_chunks=True, first_special=FIRST_SPECIAL, n_samples=n, **KW)
    assert res == [got[list(SECONDS).index(k)] for k in names]
    with pytest.raises(ValueError):
        model.transcribe_chunked(dev, CHUNK_S, first_special=FIRST_SPECIAL, n_samples=[n[0], n[1]], **KW)


def test_detect_language_per_chunk(model, hip, recordings):
    from whisper_mojo_amd import frontend
    audios = [recordings["30s"][:100000], recordings["0.5s"], recordings["window+1"]]

    def call(group):
        return model.transcribe_batch(frontend.log_mel(model, group), detect_language=LANGS, **KW)[0]
    ref = chunk_refs(model, hip, audios, call=call)
    got = model.transcribe_chunked(audios, CHUNK_S, return_chunks=True, first_special=FIRST_SPECIAL, detect_language=LANGS, **KW)
    check(got, ref)
    assert all(ids[1] in LANGS for r in ref for _, ids in r)


def test_repetition_options_per_chunk(model, hip, recordings):
    from whisper_mojo_amd import frontend
    audios = [recordings["30s"][:100000], recordings["0.5s"]]
    rp = dict(KW, repetition_penalty=1.5, no_repeat_ngram_size=2)
    ref = chunk_refs(model, hip, audios, call=lambda group: model.transcribe_batch(frontend.log_mel(model, group), **rp))
    plain = chunk_refs(model, hip, audios)
    got = model.transcribe_chunked(audios, CHUNK_S, return_chunks=True, first_special=FIRST_SPECIAL, **rp)
    check(got, ref)
    assert ref != plain  # the options did change what was decoded
    check(model.transcribe_chunked(audios, CHUNK_S, return_chunks=True, first_special=FIRST_SPECIAL, **KW), plain)  # and were switched off again


def test_same_audio_twice_is_halved(model, hip, recordings):
    x = recordings["window"]
    audio = np.concatenate([x, x])
    got = model.transcribe_chunked(audio, CHUNK_S, (0.0, 0.0), return_chunks=True, first_special=FIRST_SPECIAL, **KW)
    (_, _, _, _, a), (_, _, _, _, b) = got["chunks"]
    assert a == b
    text = [t for t in a if t < FIRST_SPECIAL]
    assert len(text) == 12
    assert got["sequence"] == merge_ref([a, b], FIRST_SPECIAL) == text  # folded into one copy, not concatenated


def test_refusals_leave_the_model_usable(model, hip, recordings):
    from whisper_mojo_amd import frontend
    with pytest.raises(hip.WhisperMiError, match="window"):
        model.transcribe_chunked(recordings["window+1"], 2.5, first_special=FIRST_SPECIAL, **KW)
    with pytest.raises(hip.WhisperMiError):
        model.transcribe_chunked(recordings["window+1"], 2.0, (1.0, 1.0), first_special=FIRST_SPECIAL, **KW)
    assert model.transcribe_chunked(np.zeros(0, np.float32), CHUNK_S, return_chunks=True, first_special=FIRST_SPECIAL, **KW) == {"sequence": [], "chunks": []}
    model.transcribe_submit(frontend.log_mel(model, [recordings["0.5s"]]), slot=1, **KW_AUDIO)
    with pytest.raises(hip.WhisperMiError, match="slot 1"):
        model.transcribe_chunked(recordings["window+1"], CHUNK_S, first_special=FIRST_SPECIAL, **KW)
    assert model.transcribe_wait(1) == frontend.transcribe_audio(model, [recordings["0.5s"]], **KW_AUDIO)
