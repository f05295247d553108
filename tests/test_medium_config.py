"""WhisperConfig.medium() (CPU): the dims of openai/whisper-medium, the weight count the C side computes for them, and the ABI
version the new shape did not have to change."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_medium_dims():
    from whisper_mojo_amd import WhisperConfig
    c = WhisperConfig.medium()
    assert (c.d_model, c.n_heads, c.n_layers, c.vocab_size, c.ffn, c.n_mels, c.n_audio_ctx, c.n_text_ctx) == \
        (1024, 16, 24, 51865, 4096, 80, 1500, 448)
    assert c.d_model == 64 * c.n_heads


def test_medium_weight_count_matches_the_library():
    from whisper_mojo_amd import WhisperConfig, _lib
    c = WhisperConfig.medium()
    dims = c.dims()
    assert c.weight_count() == _lib.lib().wm_weight_count(C.byref(dims))
    assert 760e6 < c.weight_count() < 775e6  # openai/whisper-medium: 769 M parameters


def test_header_still_says_abi_5():
    src = open(os.path.join(ROOT, "include", "whisper_mi.h")).read()
    assert re.search(r"#define\s+WM_ABI_VERSION\s+5\b", src)
    assert "wm_op_dec_linear_long" in src
    hpp = open(os.path.join(ROOT, "include", "whisper_mi.hpp")).read()
    assert "medium()" in hpp and "1024, 16, 24, 4096, 80, 1500, 448, 51865" in hpp
