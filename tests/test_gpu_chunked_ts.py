"""GPU: chunked long-form transcription with timestamps end to end (wm_transcribe_chunked_ts) on the micro model.

As tests/test_gpu_chunked.py: window 2 s, so chunk_length_s = 2.0; max_batch = 2; the chord recordings of that file.  The micro
vocabulary is laid out for this test as first_special = 890 (<|endoftext|>), a prompt of specials without the no-timestamps id, and
timestamp_begin = 899, so that 899 .. 999 are the 101 timestamp ids of a 2 s window at 0.02 s.

Every chunk's ids, and in word mode its token times, must equal that chunk decoded alone (transcribe_batch with
return_token_timestamps=True and n_frames = its samples // 160); segments, ids and pairs must equal segments_ref
(tests/test_chunked_ts_ref.py, pinned to HF's _decode_asr by the fixture) applied to those per-chunk results, on the bits.  Before
anything is compared, test_the_case_exercises_the_machine asserts from the per-chunk results that segments close, that timestamps
are skipped inside strides and that a merge finds an overlap: otherwise the equalities would hold for a stitch that does nothing."""
import numpy as np
import pytest

from test_chunked_ts_ref import seg_bits, segments_ref
from test_gpu_chunked import CHUNK_S, SECONDS, recordings  # noqa: F401  (the fixture)
from test_gpu_long_form import make_model

pytestmark = pytest.mark.gpu

SR = 16000
FIRST_SPECIAL, TB = 890, 899
HEADS = [(0, 1), (1, 0), (1, 1)]
# no_repeat_ngram_size = 2 keeps the synthetic model from echoing one id between two timestamps: with it the 100 chunks close 31 segments,
# skip 500 timestamp ids inside strides and find 48 overlaps (8 / 244 / 42 without it)
KW = dict(prompt=(891, 892, 893), eot=890, max_loop=20, suppress_tokens=tuple(range(891, 899)), timestamps=(TB, 898, 50), no_repeat_ngram_size=2)
PAR = dict(timestamp_begin=TB, first_special=FIRST_SPECIAL, time_precision=0.02, segment_size=100)
NAMES = ["0.5s", "window", "window+1", "30s", "30s+1", "70s"]  # 1 + 1 + 2 + 22 + 22 + 52 = 100 chunks


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
    m.set_alignment_heads(HEADS)
    yield m
    m.close()


def chunk_refs(model, hip, audios):
    """per recording [(ids, (len, stride_l, stride_r) samples, float32 times)]: every chunk decoded alone, one chunk per call, so that
    nothing of the reference depends on which rows share a pass or on the ragged n_frames of a neighbour"""
    from whisper_mojo_amd import frontend
    cl, sl, sr = hip.chunk_strides(CHUNK_S, None)
    tab = hip.chunk_table([len(a) for a in audios], cl, sl, sr)
    per = [[] for _ in audios]
    for r, s, n, esl, esr, _ in tab.tolist():
        cut = audios[r][s:s + n]
        ids, times = model.transcribe_batch(frontend.log_mel(model, [cut]), return_token_timestamps=True, n_frames=[len(cut) // 160], **KW)
        per[r].append((ids[0], (n, esl, esr), np.asarray(times[0], np.float32)))
    return per


@pytest.fixture(scope="module")
def case(model, hip, recordings):  # noqa: F811
    audios = [recordings[n] for n in NAMES]
    ref = chunk_refs(model, hip, audios)
    word = model.transcribe_chunked(audios, CHUNK_S, return_chunks=True, return_timestamps="word", first_special=FIRST_SPECIAL, **KW)
    segs = model.transcribe_chunked(audios, CHUNK_S, return_chunks=True, return_timestamps=True, first_special=FIRST_SPECIAL, **KW)
    return audios, ref, word, segs


def test_the_case_exercises_the_machine(case):
    _, ref, _, _ = case
    st = {}
    for r in ref:
        segments_ref(r, True, stats=st, **PAR)
    print("chunked timestamps, non-triviality:", st, "chunks", sum(len(r) for r in ref))
    assert st["closed"] >= 10, st
    assert st["skipped"] >= 3, st
    assert st["overlaps"] >= 1, st


def test_every_chunk_equals_the_chunk_decoded_alone(case):
    _, ref, word, segs = case
    for r, (want, gw, gs) in enumerate(zip(ref, word, segs)):
        assert len(gw["chunks"]) == len(gs["chunks"]) == len(want), r
        for k, ((ids, (n, sl, sr), tt), cw, cs) in enumerate(zip(want, gw["chunks"], gs["chunks"])):
            assert cw[1:4] == cs[1:4] == (n / SR, sl / SR, sr / SR), (r, k)
            assert cw[4] == cs[4] == ids, (r, k)
            assert np.array_equal(np.asarray(cw[5], np.float32).view(np.uint32), tt.view(np.uint32)), (r, k)  # the times, bit for bit


@pytest.mark.parametrize("mode", ["segments", "word"])
def test_segments_ids_and_pairs_equal_the_restatement(case, mode):
    _, ref, word, segs = case
    got = word if mode == "word" else segs
    for r, (chunks, g) in enumerate(zip(ref, got)):
        want = segments_ref(chunks, mode == "word", **PAR)
        assert seg_bits(g["segments"]) == seg_bits(want), r
        assert g["sequence"] == [t for s in want for t in s["ids"]], r
        assert all(("token_timestamps" in s) == (mode == "word") for s in g["segments"])


@pytest.mark.parametrize("name", ["window+1", "30s+1"])
def test_a_recording_alone_equals_itself_in_the_batch(model, case, recordings, name):  # noqa: F811
    _, _, word, segs = case
    for mode, got in (("word", word), (True, segs)):
        alone = model.transcribe_chunked(recordings[name], CHUNK_S, return_chunks=True, return_timestamps=mode, first_special=FIRST_SPECIAL, **KW)
        assert alone == got[NAMES.index(name)]


def test_coalesced_model_gives_the_same(hip, micro_cfg, micro_weights, case, recordings):  # noqa: F811
    _, _, word, segs = case
    m = make_model(micro_cfg, micro_weights, max_batch=2, coalesce=2)
    m.set_alignment_heads(HEADS)
    names = ["window+1", "30s+1", "0.5s"]  # 25 chunks, 13 passes: pairs of passes and an odd one that runs alone
    audios = [recordings[n] for n in names]
    w = m.transcribe_chunked(audios, CHUNK_S, return_chunks=True, return_timestamps="word", first_special=FIRST_SPECIAL, **KW)
    s = m.transcribe_chunked(audios, CHUNK_S, return_chunks=True, return_timestamps=True, first_special=FIRST_SPECIAL, **KW)
    m.close()
    assert w == [word[NAMES.index(n)] for n in names]
    assert s == [segs[NAMES.index(n)] for n in names]


def test_pcm_on_the_device_equals_pcm_on_the_host(model, case, recordings):  # noqa: F811
    import torch
    _, _, word, _ = case
    names = ["30s+1", "0.5s", "window+1"]
    n = [len(recordings[k]) for k in names]
    dev = torch.full((3, max(n) + 5), 7.0, dtype=torch.float32, device="cuda")
    for r, k in enumerate(names):
        dev[r, :n[r]] = torch.from_numpy(recordings[k]).cuda()
    res = model.transcribe_chunked(dev, CHUNK_S, return_chunks=True, return_timestamps="word", first_special=FIRST_SPECIAL, n_samples=n, **KW)
    assert res == [word[NAMES.index(k)] for k in names]


def test_without_timestamps_nothing_changes(model, hip, recordings):  # noqa: F811
    """return_timestamps=False is transcribe_chunked as it was: wm_transcribe_chunked's ids, chunk for chunk, and merge_ref's sequence"""
    from test_chunked_ref import merge_ref
    audios = [recordings["30s+1"], recordings["window+1"]]
    plain = model.transcribe_chunked(audios, CHUNK_S, return_chunks=True, first_special=FIRST_SPECIAL, **KW)
    off = model.transcribe_chunked(audios, CHUNK_S, return_chunks=True, return_timestamps=False, first_special=FIRST_SPECIAL, **KW)
    assert off == plain and all(set(g) == {"sequence", "chunks"} for g in off)
    ref = chunk_refs(model, hip, audios)
    for g, want in zip(off, ref):
        assert [c[4] for c in g["chunks"]] == [ids for ids, _, _ in want]
        assert g["sequence"] == merge_ref([ids for ids, _, _ in want], FIRST_SPECIAL)


def test_words_with_a_tokenizer(model, recordings):  # noqa: F811
    from whisper_mojo_amd.tokenizer import Tokenizer, collate_words
    tok = Tokenizer({i: (" w%d" % i if i % 3 else "x%d" % i) for i in range(FIRST_SPECIAL)})
    got = model.transcribe_chunked(recordings["window+1"], CHUNK_S, return_timestamps="word", tokenizer=tok, first_special=FIRST_SPECIAL, **KW)
    assert got["segments"]
    for s in got["segments"]:
        assert s["words"] == collate_words(tok, s["ids"], s["token_timestamps"])


def test_refusals_leave_the_model_usable(model, hip, micro_cfg, micro_weights, recordings, case):  # noqa: F811
    _, _, word, segs = case
    x = recordings["window+1"]
    with pytest.raises(ValueError):  # no timestamp rule
        model.transcribe_chunked(x, CHUNK_S, return_timestamps=True, first_special=FIRST_SPECIAL, **dict(KW, timestamps=None))
    with pytest.raises(ValueError):
        model.transcribe_chunked(x, CHUNK_S, return_timestamps="words", first_special=FIRST_SPECIAL, **KW)
    import ctypes as C
    from whisper_mojo_amd import frontend
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)

    def call(m, mode, timestamps, name="window+1", seg_cap=None):
        pcm = recordings[name]
        buf = np.ascontiguousarray(pcm[None])
        n = np.asarray([len(pcm)], np.int32)
        cap = len(word[NAMES.index(name)]["chunks"]) * 24  # chunks x (3 prompt ids + 1 + max_loop)
        seg_cap = cap + 1 if seg_cap is None else seg_cap
        merged, mlen, nseg = np.zeros(cap, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
        segt, segr, pairs = np.zeros((seg_cap, 2)), np.zeros((seg_cap, 2), np.int32), np.zeros((cap, 2))
        opts, _keep = m._opts(KW["prompt"], KW["eot"], KW["max_loop"], False, KW["suppress_tokens"], (), timestamps)
        m._set_repeat(hip.repeat_args(None, KW["no_repeat_ngram_size"]))
        return hip.lib().wm_transcribe_chunked_ts(m._h, buf.ctypes.data_as(C.c_void_p), 0, n.ctypes.data_as(ip), 1, buf.shape[1], 32000, 5333, 5333,
                                                  C.byref(opts), None, 0, FIRST_SPECIAL, mode, 0.0, merged.ctypes.data_as(ip), mlen.ctypes.data_as(ip),
                                                  cap, nseg.ctypes.data_as(ip), segt.ctypes.data_as(dp), segr.ctypes.data_as(ip), seg_cap,
                                                  pairs.ctypes.data_as(dp), None, None, None, None)
    assert call(model, 1, None) == -1        # WM_E_ARG: opts carries no timestamp rule
    assert call(model, 3, KW["timestamps"]) == -1
    bare = make_model(micro_cfg, micro_weights, max_batch=2)
    assert call(bare, 2, KW["timestamps"]) == -1  # WM_E_ARG: word mode without alignment heads
    assert call(bare, 1, KW["timestamps"]) == 0
    bare.close()
    n_seg = len(segs[NAMES.index("30s+1")]["segments"])  # 22 chunks
    assert n_seg > 1
    assert call(model, 1, KW["timestamps"], "30s+1", seg_cap=n_seg - 1) == -2  # WM_E_SIZE: one segment more than seg_cap
    assert call(model, 1, KW["timestamps"], "30s+1", seg_cap=n_seg) == 0       # exactly enough
    assert call(model, 2, KW["timestamps"]) == 0
    assert model.transcribe_chunked(x, CHUNK_S, return_chunks=True, return_timestamps="word", first_special=FIRST_SPECIAL, **KW) == word[NAMES.index("window+1")]
    assert frontend.transcribe_audio(model, [recordings["0.5s"]], prompt=KW["prompt"], eot=KW["eot"], max_loop=4)  # still usable
