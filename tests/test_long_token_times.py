"""CPU-only: the host side of token timestamps in long-form transcription — the argument checks of the Python layer and
the per-window slicing / offset helper (wm_op_long_token_times) against a numpy restatement on hand-made windows."""
import numpy as np
import pytest

TB = 941  # micro's timestamp_begin


def restate_window_times(rel, seek, segs):
    """The definition: a kept id's time = its window-relative float32 time + float64(seek) * 0.02 / 2, summed in float64; one entry per
    id of a segment, in segment order."""
    rel = np.asarray(rel, np.float32)
    off = np.float64(seek) * np.float64(0.02) / np.float64(2)
    out = [rel[first:first + count].astype(np.float64) + off for first, count, _s, _e in segs]
    return np.concatenate(out) if out else np.zeros(0, np.float64)


def _rel(n, seed):
    # multiples of 0.02 rounded to float32, as the chain stores them, non-decreasing
    steps = np.random.default_rng(seed).integers(0, 9, n).cumsum()
    return (steps.astype(np.float64) * 0.02).astype(np.float32)


WINDOWS = {
    # name: (ids without the trailing eot, seek, seek_num_frames)
    "no_pair": ([TB, 5, 6, 7, TB + 40], 0, 200),
    "single_end": ([TB, 5, 6, TB + 10, TB + 10, 8, 9, TB + 30], 200, 200),
    "last_ids_dropped": ([TB, 5, 6, TB + 10, TB + 10, 8, 9, TB + 30, TB + 30, 11, 12], 1234567, 200),
    "pair_at_end": ([TB, 5, TB + 20, TB + 20], 400, 137),
    "only_a_timestamp": ([TB + 3], 77, 50),
    "text_only": ([5, 6, 7], 3, 9),
    "empty": ([], 600, 40),
    "zero_advance": ([TB, TB], 800, 200),
}


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_window_times_match_the_restatement(name):
    from whisper_mojo_amd import _lib as L
    ids, seek, snf = WINDOWS[name]
    segs, _adv = L.long_segments(ids, TB, seek, snf)
    rel = _rel(len(ids), len(name))
    got = L.long_token_times(rel, seek, segs)
    want = restate_window_times(rel, seek, segs)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got.view(np.int64), want.view(np.int64))  # bit for bit
    kept = sum(s[1] for s in segs)
    assert got.size == kept <= len(ids)
    if name == "last_ids_dropped":  # the ids behind the last pair wait for the next window: no entry
        assert kept == 9 and len(ids) == 11
        assert np.array_equal(got, rel[:9].astype(np.float64) + seek * 0.02 / 2)
    if name == "empty":
        assert got.size == 0


def test_offset_is_added_in_float64_not_float32():
    from whisper_mojo_amd import _lib as L
    rel = np.asarray([0.02, 29.98], np.float32)
    seek = 360000 * 100 + 1  # 100 h in: float32 could not hold the sum to a centisecond
    got = L.long_token_times(rel, seek, [(0, 2, 0.0, 0.0)])
    assert np.array_equal(got, rel.astype(np.float64) + np.float64(seek) * 0.02 / 2)
    assert not np.array_equal(got, (rel + np.float32(seek * 0.01)).astype(np.float64))


def test_op_refuses_bad_arguments():
    from whisper_mojo_amd import _lib as L
    rel = np.zeros(3, np.float32)
    for segs in ([(2, 2, 0.0, 0.0)], [(-1, 1, 0.0, 0.0)], [(0, -1, 0.0, 0.0)]):
        with pytest.raises(L.WhisperMiError, match="error -1"):
            L.long_token_times(rel, 0, segs)
    with pytest.raises(L.WhisperMiError, match="error -1"):
        L.long_token_times(rel, -5, [(0, 1, 0.0, 0.0)])


def test_python_layer_checks_before_anything_is_loaded(micro_cfg):
    """return_token_timestamps with either threshold is a ValueError raised before the model is looked at (an unloaded model here)."""
    from whisper_mojo_amd import _lib, frontend
    from whisper_mojo_amd.whisper import Whisper
    assert _lib.long_tt_args(False, -1.0, 0.6) is False and _lib.long_tt_args(True, None, None) is True
    for a in ((-1.0, None), (None, 0.6), (-1.0, 0.6)):
        with pytest.raises(ValueError, match="return_token_timestamps"):
            _lib.long_tt_args(True, *a)
    m = Whisper(micro_cfg)
    feats = np.zeros((1, micro_cfg.n_mels, 300), np.float32)
    kw = dict(prompt=(1, 2, 3), eot=900, max_loop=8, timestamps=(941, 940, 50), return_token_timestamps=True)
    with pytest.raises(ValueError, match="return_token_timestamps"):
        m.transcribe_long_form(feats, logprob_threshold=-1.0, **kw)
    with pytest.raises(ValueError, match="return_token_timestamps"):
        m.transcribe_long_form(feats, logprob_threshold=-1.0, no_speech_threshold=0.6, no_speech_token=939, **kw)
    with pytest.raises(ValueError, match="return_token_timestamps"):
        frontend.transcribe_audio_long_form(m, [np.zeros(16000, np.float32)], logprob_threshold=-1.0, **kw)
    with pytest.raises(_lib.WhisperMiError, match="not loaded"):  # the flag alone gets as far as the model
        m.transcribe_long_form(feats, **kw)
