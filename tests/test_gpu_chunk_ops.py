"""GPU: the two kernels of chunked long-form transcription alone.

wm_op_chunk_merge (chunk_merge_kernel) against merge_ref of tests/test_chunked_ref.py, which the fixture pins to HF's
_find_longest_common_sequence: ids are integers and the score is formed in float64 with Python's operations, so every case must be
equal exactly.  The fixture's cases are chosen so that each rule decides an answer at least once (test_chunked_ref.py shows which).
wm_op_chunk_gather (chunk_gather_kernel): the body bit-equal to the source, the padding exact zeros, over an output that starts as a
sentinel so that a missed store shows."""
import numpy as np
import pytest

from conftest import golden
from test_chunked_ref import FIRST_SPECIAL, fixture_chunks, merge_names, merge_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def cases():
    g = golden("chunked_hf")
    return {n: (fixture_chunks(g, n), g[f"merge_{n}_want"].tolist()) for n in merge_names(g)}


REQUIRED = ["clean_overlap_2", "clean_overlap_5", "clean_overlap_40", "one_substitution", "single_match_no_merge", "eps_decides",
            "exact_tie_lowest_i", "no_overlap", "left_longer", "right_longer", "right_len_1", "empty_middle", "empty_end", "single_chunk",
            "chain_6", "L448_R448", "strip_specials", "all_special"]


@pytest.mark.parametrize("name", REQUIRED)
def test_merge_case_equals_hf(hip, cases, name):
    chunks, want = cases[name]
    assert merge_ref(chunks) == want  # the reference itself, on this machine
    assert hip.op_chunk_merge([chunks]) == [want]


def test_merge_every_fixture_case_in_one_launch(hip, cases):
    names = sorted(cases)
    assert set(REQUIRED) <= set(names)
    got = hip.op_chunk_merge([cases[n][0] for n in names])
    for n, ids in zip(names, got):
        assert ids == cases[n][1], n


def test_merge_three_recordings_and_alone(hip, cases):
    recs = [cases[n][0] for n in ("batch_rec_1", "batch_rec_4", "batch_rec_9")]
    assert [len(r) for r in recs] == [1, 4, 9]
    want = [cases[n][1] for n in ("batch_rec_1", "batch_rec_4", "batch_rec_9")]
    got = hip.op_chunk_merge(recs)
    assert got == want
    for r, w in zip(recs, want):  # a recording alone equals the same recording inside the batch
        assert hip.op_chunk_merge([r]) == [w]
    assert hip.op_chunk_merge(recs[::-1]) == want[::-1]


def test_merge_first_special_is_an_argument(hip):
    chunks = [[1, 2, 900, 3, 4, 5], [950, 4, 5, 6, 7, 999]]
    for fs in (900, 951, 1000):
        assert hip.op_chunk_merge([chunks], first_special=fs) == [merge_ref(chunks, first_special=fs)]
    assert hip.op_chunk_merge([chunks], first_special=900) == [[1, 2, 3, 4, 5, 6, 7]]


def test_merge_refuses_bad_tables(hip):
    import ctypes as C
    ip = C.POINTER(C.c_int32)
    ids, lens, off = np.zeros((2, 4), np.int32), np.asarray([4, 5], np.int32), np.asarray([0, 2], np.int32)
    out, n = np.zeros((1, 16), np.int32), np.zeros(1, np.int32)
    call = lambda st, cap, o: hip.lib().wm_op_chunk_merge(out.ctypes.data_as(ip), n.ctypes.data_as(ip), ids.ctypes.data_as(ip),  # noqa: E731
                                                          lens.ctypes.data_as(ip), o.ctypes.data_as(ip), 2, 1, st, cap, FIRST_SPECIAL)
    assert call(4, 16, off) == -1  # a length beyond the stride
    lens[1] = 4
    assert call(4, 7, off) == -1  # cap below the recording's ids
    assert call(4, 16, np.asarray([0, 3], np.int32)) == -1  # offsets past the rows
    assert call(4, 16, off) == 0


def test_gather_lengths_offsets_and_padding(hip):
    N = 480000
    rng = np.random.default_rng(7)
    T = [1000003, 480001]  # two recordings with different T
    pcm = np.zeros((2, max(T)), np.float32)
    for r, t in enumerate(T):
        pcm[r, :t] = rng.standard_normal(t).astype(np.float32)
    items = [(0, 0, 1), (0, 1, 479999), (0, 320001, 480000), (0, 520003, 480000), (1, 2, 479999), (1, 1, 480000), (1, 480000, 1), (0, 7, 0)]
    out = hip.op_chunk_gather(pcm, items, N, fill=np.float32(-123.5))
    assert out.shape == (len(items), N)
    for k, (r, s, n) in enumerate(items):
        assert np.array_equal(out[k, :n].view(np.uint32), pcm[r, s:s + n].view(np.uint32)), k  # the body, bit for bit
        assert np.array_equal(out[k, n:].view(np.uint32), np.zeros(N - n, np.uint32)), k       # the padding: +0.0, no sentinel left


def test_gather_small_window_and_refusals(hip):
    rng = np.random.default_rng(8)
    pcm = rng.standard_normal((3, 5003)).astype(np.float32)
    items = [(2, 5002, 1), (1, 3, 1001), (0, 0, 1023), (2, 1234, 1024)]
    out = hip.op_chunk_gather(pcm, items, 1025, fill=np.float32(9.0))  # a row that is no multiple of the workgroup
    for k, (r, s, n) in enumerate(items):
        assert np.array_equal(out[k, :n], pcm[r, s:s + n]) and not out[k, n:].any(), k
    for bad in [(3, 0, 1), (0, 5000, 4), (0, -1, 1), (0, 0, 1026)]:
        with pytest.raises(hip.WhisperMiError):
            hip.op_chunk_gather(pcm, [bad], 1025)
