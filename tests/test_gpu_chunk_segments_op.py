"""GPU: chunk_segments_kernel alone (wm_op_chunk_segments) against the fixture tools/make_golden_chunked_ts.py recorded
from HF's real _decode_asr / _find_longest_common_sequence, in both modes.

Ids and ranges are integers; every time is float64 formed with Python's operations in Python's order and rounded as Python's
round(x, 2), so every case must be equal on the bits (seg_bits).  Every output starts as a sentinel: _lib.op_chunk_segments asserts
that nothing was stored past a recording's ids, segments or pairs, also when the call is refused."""
import numpy as np
import pytest

from conftest import golden
from test_chunked_ts_ref import MODES, REQUIRED, case_input, case_names, case_want, seg_bits, segments_ref

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
    g = golden("chunked_ts_hf")
    out = {}
    for mode in MODES:
        for n in case_names(g):
            chunks, par = case_input(g, n, mode == "word")
            out[n, mode] = (chunks, par, case_want(g, n, mode))
    return out


ALL = REQUIRED + ["rounding_ties", "micro_layout"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ALL)
def test_case_equals_hf(hip, cases, name, mode):
    chunks, par, want = cases[name, mode]
    assert seg_bits(segments_ref(chunks, mode == "word", **par)) == seg_bits(want)  # the reference itself, on this machine
    got = hip.op_chunk_segments([chunks], mode == "word", **par)
    assert seg_bits(got[0]) == seg_bits(want)


@pytest.mark.parametrize("mode", MODES)
def test_every_fixture_case_in_one_launch(hip, cases, mode):
    """all recordings with Whisper's id layout in one launch (micro_layout has its own ids: alone, above)"""
    names = sorted(n for n, m in cases if m == mode and cases[n, m][1] == cases["single_two_segments", m][1])
    assert len(names) >= 21 and set(REQUIRED) <= set(names)
    got = hip.op_chunk_segments([cases[n, mode][0] for n in names], mode == "word", **cases[names[0], mode][1])
    for n, segs in zip(names, got):
        assert seg_bits(segs) == seg_bits(cases[n, mode][2]), n


@pytest.mark.parametrize("mode", MODES)
def test_three_recordings_and_alone(hip, cases, mode):
    names = ("batch_rec_1", "batch_rec_4", "batch_rec_9")
    recs = [cases[n, mode][0] for n in names]
    par = cases[names[0], mode][1]
    assert [len(r) for r in recs] == [1, 4, 9]
    want = [seg_bits(cases[n, mode][2]) for n in names]
    assert [seg_bits(s) for s in hip.op_chunk_segments(recs, mode == "word", **par)] == want
    assert [seg_bits(s) for s in hip.op_chunk_segments(recs[::-1], mode == "word", **par)] == want[::-1]


def test_the_word_mode_merge_is_another_merge(hip, cases):
    chunks, par, want_w = cases["pair_out_of_order", "word"]
    got_w = hip.op_chunk_segments([chunks], True, **par)[0]
    got_s = hip.op_chunk_segments([[(i, s, None) for i, s, _ in chunks]], False, **par)[0]
    assert [t for s in got_w for t in s["ids"]] != [t for s in got_s for t in s["ids"]]
    assert seg_bits(got_w) == seg_bits(want_w)


def test_capacities_too_small_are_refused_and_nothing_lands_beyond(hip, cases):
    chunks, par, want = cases["batch_rec_4", "word"]
    n_ids, n_seg = sum(len(i) for i, _, _ in chunks), len(want)
    assert n_seg > 4
    with pytest.raises(hip.WhisperMiError, match="libwhispermi error -2"):  # WM_E_SIZE: cap below the recording's ids, nothing launched
        hip.op_chunk_segments([chunks], True, cap=n_ids - 1, **par)
    with pytest.raises(hip.WhisperMiError, match="libwhispermi error -2"):  # more segments than seg_cap: the sentinels past it stay
        hip.op_chunk_segments([chunks], True, seg_cap=n_seg - 2, **par)
    with pytest.raises(hip.WhisperMiError, match="libwhispermi error -2"):
        hip.op_chunk_segments([chunks], False, seg_cap=1, **par)
    assert seg_bits(hip.op_chunk_segments([chunks], True, seg_cap=n_seg, cap=n_ids, **par)[0]) == seg_bits(want)  # exactly enough


def test_refuses_bad_arguments(hip, cases):
    chunks, par, _ = cases["single_two_segments", "segments"]
    for bad in (dict(time_precision=0.0), dict(segment_size=0), dict(timestamp_begin=par["first_special"] - 1)):
        with pytest.raises(hip.WhisperMiError):
            hip.op_chunk_segments([chunks], False, **dict(par, **bad))
