"""WhisperConfig.small() (CPU): the dims of openai/whisper-small, the weight count the C side computes for them, and the ABI version
the new shape did not have to change."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_small_dims():
    from whisper_mojo_amd import WhisperConfig
    c = WhisperConfig.small()
    assert (c.d_model, c.n_heads, c.n_layers, c.vocab_size, c.ffn, c.n_mels, c.n_audio_ctx, c.n_text_ctx) == \
        (768, 12, 12, 51865, 3072, 80, 1500, 448)
    assert c.d_model == 64 * c.n_heads


def test_small_weight_count_matches_the_library():
    from whisper_mojo_amd import WhisperConfig, _lib
    c = WhisperConfig.small()
    dims = c.dims()
    assert c.weight_count() == _lib.lib().wm_weight_count(C.byref(dims))
    assert 240e6 < c.weight_count() < 250e6  # openai/whisper-small: 244 M parameters


def test_header_still_says_abi_5():
    src = open(os.path.join(ROOT, "include", "whisper_mi.h")).read()
    assert re.search(r"#define\s+WM_ABI_VERSION\s+5\b", src)
    hpp = open(os.path.join(ROOT, "include", "whisper_mi.hpp")).read()
    assert "small()" in hpp and "768, 12, 12, 3072, 80, 1500, 448, 51865" in hpp
