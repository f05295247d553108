"""GPU op tests of forced alignment's two kernel changes: dec_linear's capture by row map (wm_op_dec_linear_capmap) and the
align chain with per-table row counts and offsets (wm_op_token_times_rows)."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    return _lib.lib()


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("d_model", [128, 384])
@pytest.mark.parametrize("kv_B", [1, 3])
@pytest.mark.parametrize("P", [1, 3, 16])
def test_capture_by_row_map(hip, P, kv_B, d_model, dtype):
    """LNx -> cross q over P * kv_B position-major rows with a row map: a permutation of the destination rows with some -1s.  Every
    mapped slot holds the matching 64 columns of `out` bit for bit, every other float of cap still holds the sentinel, and `out` is
    wm_op_dec_linear's for the same operands."""
    from whisper_mojo_amd import _lib, whisper_tensor as wt
    rng = np.random.default_rng(1000 * P + 100 * kv_B + d_model + dtype)
    B, H = P * kv_B, d_model // 64
    x = rng.standard_normal((B, d_model)).astype(np.float32)
    W = (rng.standard_normal((d_model, d_model)) / np.sqrt(d_model)).astype(np.float32)
    bias = rng.standard_normal(d_model).astype(np.float32)
    g, be = (1 + 0.1 * rng.standard_normal(d_model)).astype(np.float32), (0.1 * rng.standard_normal(d_model)).astype(np.float32)
    n_sel = min(H, 2)
    sel = np.full(32, -1, np.int8)
    sel[H - 1] = 0  # the last head goes to slot 0 ...
    if n_sel == 2:
        sel[0] = 1  # ... the first to slot 1; every other head is not captured
    cap_dst = B + 2  # two destination rows nobody maps to
    cmap = rng.permutation(cap_dst)[:B].astype(np.int32)
    drop = rng.random(B) < 0.3
    if B > 1:
        drop[0], drop[B - 1] = True, False  # at least one row dropped and one kept
    cmap[drop] = -1
    cap = np.full((cap_dst, n_sel, 64), SENTINEL, np.float32)
    out = np.zeros((B, d_model), np.float32)
    _lib.check(hip.wm_op_dec_linear_capmap(_fp(out), _fp(cap), _fp(x), _fp(W), _fp(bias), _fp(g), _fp(be), B, d_model, d_model, dtype,
                                           sel.ctypes.data_as(C.POINTER(C.c_int8)), n_sel, _ip(cmap), cap_dst))
    want = np.full_like(cap, SENTINEL)
    for r in range(B):
        if cmap[r] >= 0:
            for h in range(H):
                if sel[h] >= 0:
                    want[cmap[r], sel[h]] = out[r, 64 * h:64 * h + 64]
    np.testing.assert_array_equal(cap, want)
    np.testing.assert_array_equal(out, wt.dec_linear(x, W, bias, ln=(g, be), dtype=dtype))
    assert np.isfinite(out).all() and np.abs(out).max() > 0.1


def test_ragged_chain_tables(hip):
    """The 24 HF tables of token_timestamps_tables.npz through the ragged chain: tables of one width F (and one head count: the
    fixture has one- and two-head tables) share ONE normalisation and ONE DTW launch whatever their row counts, each with its own
    output offset row0 in {1, 4, 9}.  Every table's times are HF's, shifted to its row0, and wm_op_token_times' for the table alone."""
    from whisper_mojo_amd import _lib
    g = golden("token_timestamps_tables")
    n_prompt = int(g["n_prompt"])
    groups = {}
    for name in (str(n) for n in g["names"]):
        w = g[name + "_q"].astype(np.float32) / np.float32(65536)
        groups.setdefault((w.shape[2], w.shape[0]), []).append((name, w))
    assert sum(len(v) for v in groups.values()) == 24
    assert any(len({w.shape[1] for _, w in v}) >= 4 for v in groups.values())  # launches that really are ragged
    k = 0
    for (F, n_sel), tabs in sorted(groups.items()):
        n_tab = len(tabs)
        R = np.asarray([w.shape[1] for _, w in tabs], np.int32)
        L = max(1, int(R.max()))
        row0 = np.asarray([(1, 4, 9)[(k + i) % 3] for i in range(n_tab)], np.int32)
        k += n_tab
        packed = np.full((n_tab, n_sel, L, F), np.nan, np.float32)  # rows past R_b must never be read
        for i, (_, w) in enumerate(tabs):
            packed[i, :, :w.shape[1]] = w
        stride = int((row0 + R).max()) + 1 + 2
        got = np.full((n_tab, stride), -7.0, np.float32)
        _lib.check(hip.wm_op_token_times_rows(_fp(got), _fp(packed), n_tab, n_sel, L, F, _ip(R), _ip(np.full(n_tab, F, np.int32)), _ip(row0), stride))
        for i, (name, w) in enumerate(tabs):
            hf = g[name + "_times"]
            want = np.zeros(stride, np.float32)
            want[row0[i]:row0[i] + R[i] + 1] = hf[n_prompt:]
            np.testing.assert_array_equal(got[i], want, err_msg=f"{name} row0 {row0[i]}")
            alone = np.full(row0[i] + R[i] + 1, -7.0, np.float32)
            wc = np.ascontiguousarray(w)
            _lib.check(hip.wm_op_token_times(_fp(alone), _fp(wc) if R[i] else None, n_sel, int(R[i]), F, int(row0[i])))
            np.testing.assert_array_equal(got[i, :alone.size], alone, err_msg=name)


def test_ragged_chain_refusals(hip):
    w = np.ones((1, 1, 2, 8), np.float32)
    t = np.zeros((1, 4), np.float32)
    one = lambda v: _ip(np.asarray([v], np.int32))
    assert hip.wm_op_token_times_rows(_fp(t), _fp(w), 1, 1, 2, 8, one(2), one(8), one(1), 4) == 0
    assert hip.wm_op_token_times_rows(_fp(t), _fp(w), 1, 1, 2, 8, one(2), one(8), one(2), 4) == -1  # out_stride < row0 + R + 1
    assert hip.wm_op_token_times_rows(_fp(t), _fp(w), 1, 1, 2, 8, one(3), one(8), one(0), 4) == -1  # R > L
    assert hip.wm_op_token_times_rows(_fp(t), _fp(w), 1, 1, 2, 8, one(2), one(9), one(0), 4) == -1  # F > T
