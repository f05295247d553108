"""CPU: chunked long-form transcription only adds to the boundary — the ABI version stays 5, the new entry points are
declared, exported and bound, and the C++ mirror carries the method."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wm_chunk_table", "wm_transcribe_chunked", "wm_op_chunk_gather", "wm_op_chunk_merge")


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


def test_hosts_carry_transcribe_chunked():
    from whisper_mojo_amd import frontend
    from whisper_mojo_amd.whisper import Whisper
    hpp = open(os.path.join(ROOT, "include", "whisper_mi.hpp")).read()
    assert "transcribe_chunked(" in hpp and "wm_transcribe_chunked(" in hpp
    sig = inspect.signature(Whisper.transcribe_chunked)
    assert list(sig.parameters)[1:5] == ["pcm", "chunk_length_s", "stride_length_s", "return_chunks"]
    assert sig.parameters["chunk_length_s"].default == 30.0 and sig.parameters["stride_length_s"].default is None
    assert "detect_language" in inspect.signature(frontend.transcribe_audio_chunked).parameters
