"""CPU: argument validation of Whisper.align (_lib.align_args) and the align fixtures' self-consistency."""
import numpy as np
import pytest

from conftest import golden
from test_token_timestamps import restate_times

V, CTX, MAXB, T = 1000, 64, 4, 100


def _args(ids, context_len=None, n_frames=None, B=None):
    from whisper_mojo_amd import _lib
    return _lib.align_args(ids, context_len, n_frames, len(ids) if B is None else B, V, CTX, MAXB, T)


def test_align_args_accepts_and_packs():
    tab, lens, ctx, nf = _args([[1, 2, 3, 4, 5], [7, 8]], [4, 1], [200, 2])
    assert tab.dtype == lens.dtype == ctx.dtype == nf.dtype == np.int32
    assert tab.tolist() == [[1, 2, 3, 4, 5], [7, 8, 0, 0, 0]] and lens.tolist() == [5, 2]
    assert ctx.tolist() == [4, 1] and nf.tolist() == [200, 2]
    tab, lens, ctx, nf = _args([[1, 2, 3]])
    assert ctx.tolist() == [1] and nf is None
    assert _args([[1, 2, 3], [4, 5, 6]], 2)[2].tolist() == [2, 2]  # one number serves every row; R = 0 is allowed


@pytest.mark.parametrize("ids, context_len, n_frames, B", [
    ([[1, 2], [1]], None, None, None),              # a row of one id
    ([list(range(CTX + 1))], None, None, None),     # longer than the decoder context
    ([[1, 2, V]], None, None, None),                # an id outside the vocabulary
    ([[1, 2, -1]], None, None, None),
    ([[1, 2, 3]], 0, None, None),                   # context_len < 1
    ([[1, 2, 3]], 3, None, None),                   # context_len > len - 1
    ([[1, 2, 3]] * 2, None, None, 3),               # rows != clips
    ([[1, 2, 3]] * (MAXB + 1), None, None, None),   # over max_batch
    ([[1, 2, 3]] * 2, None, [100], None),           # n_frames: one entry per row
    ([[1, 2, 3]] * 2, None, [100, 1], None),        # n_frames < 2
    ([[1, 2, 3]] * 2, None, [2 * T + 1, 100], None),  # n_frames > 2 * n_audio_ctx
])
def test_align_args_refuses(ids, context_len, n_frames, B):
    with pytest.raises(ValueError):
        _args(ids, context_len, n_frames, B)


def test_micro_fixture_is_self_consistent():
    """The stored HF probabilities of the rows that count give the stored HF times through the restatement, with and without the
    crop: pins tools/make_golden_align.py to the arithmetic the GPU tests lean on."""
    g = golden("align_micro_hf")
    names = [str(n) for n in g["names"]]
    assert {"ctx1", "ctx4", "prev_text", "other_clip", "random", "rows0", "rows1", "in16", "in17", "in33"} <= set(names)
    for n in names:
        ids, ctx, p = g[n + "_ids"], int(g[n + "_context_len"]), g[n + "_probs"]
        R = len(ids) - ctx - 1
        assert p.shape == (len(g["heads"]), R, T)
        np.testing.assert_array_equal(restate_times(p, ctx), g[n + "_times"], err_msg=n)
        np.testing.assert_array_equal(restate_times(p[:, :, :int(g[n + "_n_frames"]) // 2], ctx), g[n + "_times_nf"], err_msg=n)
    assert not g["rows0_times"].any() and len(g["rows1_times"]) == 6


def test_tiny_fixture_has_the_long_row():
    g = golden("align_tiny_hf")
    assert len(g["len448_ids"]) == 448 and int(g["len448_context_len"]) == 4 and g["len448_times"].shape == (448,)
