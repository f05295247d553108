"""CPU: chunked timestamps only add to the boundary — the ABI version stays 5, the new entry points are declared,
exported and bound, and the hosts carry the option."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wm_transcribe_chunked_ts", "wm_op_chunk_segments")


def test_abi_version_is_still_5():
    from whisper_mojo_amd import _lib
    txt = open(os.path.join(ROOT, "include", "whisper_mi.h")).read()
    assert re.search(r"#define\s+WM_ABI_VERSION\s+5\b", txt)
    assert _lib.ABI_VERSION == 5
    assert _lib.lib().wm_abi_version() == 5


def test_new_symbols_are_declared_exported_and_bound():
    from whisper_mojo_amd import _lib
    txt = open(os.path.join(ROOT, "include", "whisper_mi.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for s in NEW:
        assert re.search(r"\bint\s+" + s + r"\s*\(", txt), s
        assert hasattr(lib, s), s
        assert s in _lib.SYMBOLS
        assert getattr(L, s).argtypes, s
    assert "Not here: token timestamps in chunked mode" not in txt


def test_hosts_carry_return_timestamps():
    from whisper_mojo_amd import frontend, tokenizer
    from whisper_mojo_amd.whisper import Whisper
    hpp = open(os.path.join(ROOT, "include", "whisper_mi.hpp")).read()
    assert "transcribe_chunked_ts(" in hpp and "wm_transcribe_chunked_ts(" in hpp
    sig = inspect.signature(Whisper.transcribe_chunked)
    assert list(sig.parameters)[1:6] == ["pcm", "chunk_length_s", "stride_length_s", "return_chunks", "return_timestamps"]
    assert sig.parameters["return_timestamps"].default is False
    p = inspect.signature(frontend.transcribe_audio_chunked).parameters
    assert p["return_timestamps"].default is False and "tokenizer" in p and "time_precision" in p
    assert list(inspect.signature(tokenizer.collate_words).parameters)[:3] == ["tokenizer", "ids", "pairs"]


def test_return_timestamps_takes_bools_and_word_only():
    """0 and 1 equal False and True but are refused like any other value, before the model is looked at: 0 must not switch times on"""
    import numpy as np
    import pytest
    from whisper_mojo_amd import frontend
    for bad in (0, 1, None, "words", "True", 2.0):
        with pytest.raises(ValueError, match="return_timestamps is False, True or"):
            frontend.transcribe_audio_chunked(None, np.zeros(16, np.float32), return_timestamps=bad)
    with pytest.raises(ValueError, match="needs timestamps="):  # a bool and "word" get past that check
        frontend.transcribe_audio_chunked(None, np.zeros(16, np.float32), return_timestamps=True)
    with pytest.raises(ValueError, match="needs timestamps="):
        frontend.transcribe_audio_chunked(None, np.zeros(16, np.float32), return_timestamps="word")
