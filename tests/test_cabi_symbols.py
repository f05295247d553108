"""CPU-only: the C-ABI library loads and exports every symbol include/whisper_mi.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "whisper_mi.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(wm_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_the_boundary():
    syms = declared_symbols()
    for s in ("wm_model_load", "wm_transcribe", "wm_encode", "wm_decode_step", "wm_state_new", "wm_op_matmul_nt",
              "wm_op_layer_norm", "wm_op_gelu", "wm_op_softmax_rows", "wm_op_conv1d_k3", "wm_op_argmax",
              "wm_op_attention_batch", "wm_op_layer_norm_t", "wm_op_gemm_nt_epi", "wm_op_gemm_nt_ring", "wm_op_fe_tables", "wm_op_fe_frames", "wm_op_fe_mel_log",
              "wm_op_fe_mel_norm", "wm_op_window_gather", "wm_op_ts_states", "wm_op_init_tokens", "wm_op_set_rows_step", "wm_op_set_step",
              "wm_op_pack_tokens", "wm_op_dec_embed", "wm_op_rows_copy", "wm_op_mel_transpose_pad"):
        assert s in syms


def test_library_exports_every_declared_symbol():
    from whisper_mojo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, missing
    assert sorted(_lib.SYMBOLS) == declared_symbols()


def test_missing_library_fails_loudly(monkeypatch):
    from whisper_mojo_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libwhispermi.so")
    with pytest.raises(_lib.WhisperMiError):
        _lib.lib()


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under whisper.mojo_amd/ may reference it."""
    pkg = os.path.join(ROOT, "whisper.mojo_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert "oracle" not in src.replace("test_oracle", ""), f"{f} mentions the oracle"


def test_package_import_sets_hw_queue_default():
    """Pipelined passes need one hardware queue per slot stream: the package sets GPU_MAX_HW_QUEUES before HIP
    initialises unless the user already chose a value.  A fresh child process each time: this process's environment may
    carry a value of its own."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}

    def queues_after_import(**extra):
        code = "import os, whisper_mojo_amd; print(os.environ.get('GPU_MAX_HW_QUEUES', '0'))"
        return int(subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, **extra), capture_output=True, text=True,
                                  check=True).stdout)
    assert queues_after_import() >= 8
    assert queues_after_import(GPU_MAX_HW_QUEUES="12") == 12


def test_op_wrappers_validate_shapes_before_calling_the_library():
    """The host mirrors of the op entry points refuse wrong shapes themselves (no GPU, no library call needed to see it)."""
    import numpy as np
    import pytest
    from whisper_mojo_amd import whisper_tensor as wt
    x = np.zeros((4, 128), np.float32)
    with pytest.raises(ValueError):  # fc1 must be [ffn, d]
        wt.mlp_block(x, np.ones(128), np.zeros(128), np.zeros((256, 64), np.float32), np.zeros(256), np.zeros((128, 256), np.float32), np.zeros(128))
    with pytest.raises(ValueError):  # fc2 must be [d, ffn]
        wt.mlp_block(x, np.ones(128), np.zeros(128), np.zeros((256, 128), np.float32), np.zeros(256), np.zeros((128, 128), np.float32), np.zeros(128))
    with pytest.raises(ValueError):  # in place: x must be a C-contiguous float32 array
        wt.mlp_block(x.astype(np.float64), np.ones(128), np.zeros(128), np.zeros((256, 128), np.float32), np.zeros(256), np.zeros((128, 256), np.float32), np.zeros(128))
    q = np.zeros((10, 128), np.float32)
    with pytest.raises(ValueError):  # d must be 64 * n_heads
        wt.attention(np.zeros_like(q), q, q, q, 3)
    with pytest.raises(ValueError):  # k of another length
        wt.attention(np.zeros_like(q), q, np.zeros((9, 128), np.float32), q, 2)
    with pytest.raises(ValueError):  # out of the wrong shape
        wt.attention(np.zeros((10, 64), np.float32), q, q, q, 2)
    with pytest.raises(ValueError):  # the batched form takes [B, n_ctx, d]
        wt.attention_batch(np.zeros_like(q), q, q, q, 2)
    with pytest.raises(ValueError):  # LayerNorm with neither store asked for
        wt.layer_norm_t(x, np.ones(128), np.zeros(128))
    with pytest.raises(ValueError):  # cached keys must be [B, t, d]
        wt.attention_cached(np.zeros_like(q), q, q, q, 2)
    with pytest.raises(ValueError):  # another batch size in the cache
        wt.attention_cached(np.zeros_like(q), q, np.zeros((9, 5, 128), np.float32), np.zeros((9, 5, 128), np.float32), 2)
    with pytest.raises(ValueError):  # prefill rows: k holds q_B utterances, not one per row
        wt.attention_cached(np.zeros_like(q), q, np.zeros((10, 5, 128), np.float32), np.zeros((10, 5, 128), np.float32), 2, q_B=5, len=0)
    with pytest.raises(ValueError):  # prefill rows are P * q_B
        wt.attention_cached(np.zeros_like(q), q, np.zeros((3, 5, 128), np.float32), np.zeros((3, 5, 128), np.float32), 2, q_B=3, len=0)
    W = np.zeros((384, 128), np.float32)
    with pytest.raises(ValueError):  # W must be [N, K]
        wt.dec_linear(x, np.zeros((384, 64), np.float32))
    with pytest.raises(ValueError):  # bias of another width
        wt.dec_linear(x, W, bias=np.zeros(128, np.float32))
    with pytest.raises(ValueError):  # LayerNorm gamma / beta have K elements
        wt.dec_linear(x, W, ln=(np.ones(384, np.float32), np.zeros(384, np.float32)))
    with pytest.raises(ValueError):  # residual must be [B, N]
        wt.dec_linear(x, W, residual=np.zeros((4, 128), np.float32))
    with pytest.raises(ValueError):  # QKV mode: the caches are [n_utt, cap_rows, N / 3]
        wt.dec_linear(x, W, kv=(np.zeros((4, 8, 384), np.float32), np.zeros((4, 8, 384), np.float32)))
    with pytest.raises(ValueError):  # capture: one row per activation row, 64 columns per head, 32 selectors
        wt.dec_linear(x, W[:128], cap=np.zeros((3, 2, 1, 64), np.float32), cap_sel=np.full(32, -1, np.int8))
    with pytest.raises(ValueError):
        wt.dec_linear(x, W[:128], cap=np.zeros((4, 2, 1, 64), np.float32), cap_sel=np.full(16, -1, np.int8))
