"""GPU: xattn_absorb_kernel with its Wk rows requested before q is staged against the loop it replaces
(wm_op_xattn_absorb, late_loads), bit for bit on the three bf16 images of q', and the images' sum against the product in float64."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wt():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()  # raises if the HIP library is missing: no fallback
    from whisper_mojo_amd import whisper_tensor
    return whisper_tensor


def bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("rows", [1, 4, 5, 17])  # a workgroup serves R = 4 rows: one partly filled, full, full + 1, four full + 1
@pytest.mark.parametrize("H", [1, 6, 8])
def test_absorb_early_loads_equal_late_loads_and_the_product(wt, H, rows):
    r = np.random.default_rng(100 * H + rows)
    d = 64 * H
    q = r.standard_normal((rows, d)).astype(np.float32)
    Wk = bf16_round(r.standard_normal((d, d)) / np.sqrt(d))  # bf16 values: the upload is exact
    early, late = wt.xattn_absorb(q, Wk, H), wt.xattn_absorb(q, Wk, H, late_loads=True)
    assert early.shape == (rows, 3, H, d)
    assert np.array_equal(early.view(np.uint32), late.view(np.uint32)), np.argwhere(early != late)[:4].tolist()
    for img in range(3):
        assert not np.any(early[:, img].view(np.uint32) & np.uint32(0xFFFF))  # bf16 values
    # the split check of tests/test_xattn.py: h + m + l, summed in float64, IS an fp32 value x — the kernel's accumulator
    s = early.astype(np.float64).sum(1)  # [rows, H, d]
    x = s.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), s)
    # x against q'[r, h, c] = Σ_e (0.125·q[r, h·64 + e])·Wk[h·64 + e, c] in float64.  0.125·q is exact; the kernel is 64 fmaf in
    # sequence, one rounding each: |x − ref| <= γ_64 · Σ_e |0.125·q_e·Wk_ec|, γ_n = n·u / (1 − n·u), u = 2^-24 (Higham, Accuracy and
    # Stability of Numerical Algorithms, §3.1)
    a = (0.125 * q.astype(np.float64)).reshape(rows, H, 64)
    W = Wk.astype(np.float64).reshape(H, 64, d)
    ref = np.einsum("rhe,hec->rhc", a, W)
    u = 2.0 ** -24
    bound = (64 * u / (1 - 64 * u)) * np.einsum("rhe,hec->rhc", np.abs(a), np.abs(W))
    err = np.abs(x.astype(np.float64) - ref)
    print(f"H {H} rows {rows}: max err {err.max():.3g}, worst err/bound {(err / bound).max():.3g}")
    assert (err <= bound).all(), (np.argwhere(err > bound)[:4].tolist(), err.max())
