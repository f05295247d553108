"""CPU-only: the float64 absorbed cross-attention reference of tests/test_gpu_decode_ops.py equals the direct (cached K/V) form
of the same attention, so the GPU test's reference is the attention it claims to be."""
import numpy as np

from test_gpu_decode_ops import xattn_ref, xattn_ref_direct


def test_absorbed_reference_equals_direct_form():
    r = np.random.default_rng(5)
    for H, n_keys, rows, q_B in ((1, 7, 2, 0), (3, 40, 4, 2), (2, 1, 1, 0)):
        d = 64 * H
        q = r.standard_normal((rows, d)).astype(np.float32)
        Wk = (r.standard_normal((d, d)) * 2 / np.sqrt(d)).astype(np.float32)
        Wv = (r.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
        bv = r.standard_normal(d).astype(np.float32)
        X = r.standard_normal((q_B if q_B else rows, n_keys, d)).astype(np.float32)
        a = xattn_ref(q, Wk, Wv, bv, X, H, q_B)
        b = xattn_ref_direct(q, Wk, Wv, bv, X, H, q_B)
        assert np.abs(a - b).max() < 1e-12 * max(1.0, np.abs(b).max())
