"""Op-level tests (-m gpu) of the no-speech probe (wm_op_no_speech: the LP instantiation of the logits kernel's stage 1 without mask
and ranges + no_speech_finish_kernel) against float64 on the operands as rounded on upload.

Reference: s = the float64 logits of tests/test_gpu_decode_ops.py (_logits_ref); log p = s[token] - logsumexp(s) over ALL columns.

Bound on |Δ log p|: 2·e + r, the form tests/test_gpu_logits_lp.py derives.
  e: the largest per-logit bound _logits_ref derives for the row.  It covers logsumexp (which moves by at most the largest
     perturbation of its arguments) and the token's logit: the finish kernel recomputes that one logit as a K-term fp32 dot product
     of the LayerNorm output (rounded to the operand dtype) with the embedding row — at most K roundings of products that are
     exact for 16-bit operands, i.e. inside the order-independent accumulation term of e for every kernel variant, and its
     LayerNorm statistics are summed K/64 deep per lane plus 6 butterfly adds, not deeper than the K/8 + 3 _ln_err assumes.
  r: the fp32 cost of the exp-sum, re-derived for the finish kernel's merge (u = 2^-24; expf / logf within 2u).  One term
     exp(v - m) on its way to S:
       created            expf 2u, and its argument fl(v - m) carries u·|v - m|
       lane               <= 7 adds                                                   7u
       4 lanes of a row   2 merges, each expf + product + add                         8u
       8 waves            expf + product, <= 8 adds                                  11u
       finish             expf + product, <= parts - 1 adds in ascending part order  (2 + parts)u
     (no text ∪ timestamps join: 30 + parts in all) and the rescales' arguments telescope to u·(M - v) as there.  Then logf
     (2u·|log S|), s[token] - M (u·|s[token] - M|), the final subtraction (u·|log p|), and — the op returns p, not log p — expf and
     the rounding of p (3u).  Nothing in it is fitted to an observed error."""
import numpy as np
import pytest

from test_gpu_decode_ops import DT_BF16, DT_F16, DT_F32, U, _ct, _decoder_like, _logits_ref, hip  # noqa: F401

pytestmark = pytest.mark.gpu

MICRO_V, MULTI_V = 1000, 51865  # the micro model's and the multilingual vocabulary

# (dtype, K, B, N): the kernel variant the probe's sweep reaches is named beside each case (its LP instantiation)
CASES = [
    (DT_F32, 128, 1, MICRO_V),    # dec_logits_split_kernel<1,1>
    (DT_F32, 128, 3, MULTI_V),    # dec_logits_split_kernel<1,1>
    (DT_F32, 128, 64, MICRO_V),   # dec_logits_split_kernel<1,4>
    (DT_F32, 128, 128, MICRO_V),  # dec_logits_split128_kernel<1>
    (DT_F32, 384, 1, MULTI_V),    # dec_logits_split_kernel<3,1>
    (DT_F32, 384, 3, MICRO_V),    # dec_logits_split_kernel<3,1>
    (DT_F32, 384, 64, MULTI_V),   # dec_logits_split_kernel<3,4>, the real part count (250)
    (DT_F32, 384, 128, MICRO_V),  # dec_logits_split128_kernel<3>
    (DT_F32, 512, 1, MICRO_V),    # dec_logits_kernel<float,4,1>
    (DT_F32, 512, 3, MULTI_V),    # dec_logits_kernel<float,4,1>
    (DT_F32, 512, 64, MICRO_V),   # dec_logits_kernel<float,4,4>
    (DT_F32, 512, 128, MICRO_V),  # dec_logits_kernel<float,4,4> (two row blocks: 16-bit and d_model 512 have no 128-row kernel)
    (DT_BF16, 128, 1, MICRO_V),   # dec_logits_kernel<bf16,1,1>
    (DT_BF16, 384, 3, MULTI_V),   # dec_logits_kernel<bf16,3,1>
    (DT_BF16, 384, 64, MICRO_V),  # dec_logits_kernel<bf16,3,4>
    (DT_BF16, 512, 128, MICRO_V),  # dec_logits_kernel<bf16,4,4>
    (DT_F16, 128, 64, MICRO_V),   # dec_logits_kernel<f16,1,4>
    (DT_F16, 384, 1, MICRO_V),    # dec_logits_kernel<f16,3,1>
    (DT_F16, 512, 3, MULTI_V),    # dec_logits_kernel<f16,4,1>
]


def _probe(x, g, b, emb, dt, token):
    from whisper_mojo_amd import whisper_tensor as wt
    return wt.no_speech(x, g, b, emb, token, dtype=dt)


def _ref(ref, bound, token, N):
    """-> (log p float64 [B], lse [B], bound [B]) by the module docstring's rule"""
    parts = (N + 16 * _ct(N) - 1) // (16 * _ct(N))
    M = ref.max(1, keepdims=True)
    w = np.exp(ref - M)
    S = w.sum(1)
    lse = M[:, 0] + np.log(S)
    lp = ref[:, token] - lse
    rel = (w * ((30 + parts) * U + U * (M - ref))).sum(1) / S
    r = rel + U * (2 * np.abs(np.log(S)) + np.abs(ref[:, token] - M[:, 0]) + np.abs(lp) + 3)
    return lp, lse, 2 * bound.max(1) + r


def _check(tag, prob, lse, ref, bound, token, N):
    want, want_lse, bnd = _ref(ref, bound, token, N)
    assert np.isfinite(prob).all() and np.isfinite(lse).all()
    assert (prob > 0).all() and (prob <= 1).all()
    ratio = np.abs(np.log(prob.astype(np.float64)) - want) / bnd
    ratio_lse = np.abs(lse - want_lse) / (bnd + U * np.abs(want_lse))
    print(f"{tag}: worst err/bound {ratio.max():.3g} (lse {ratio_lse.max():.3g}), max |err| {np.abs(np.log(prob.astype(np.float64)) - want).max():.3g}, "
          f"bounds {bnd.min():.2g}..{bnd.max():.2g}")
    assert ratio.max() <= 1.0, (tag, int(np.argmax(ratio)))
    assert ratio_lse.max() <= 1.0, (tag, int(np.argmax(ratio_lse)))


@pytest.mark.parametrize("dt,K,B,N", CASES)
def test_no_speech_vs_float64(hip, dt, K, B, N):
    """log p within 2·e + r of float64 for the token at id 0, at the last id, on a part boundary and mid-vocabulary."""
    r = np.random.default_rng(17 * K + 5 * B + N + dt)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    per_part = 16 * _ct(N)
    for token in (0, N - 1, per_part, per_part - 1, N // 2 + 3):
        prob, lse = _probe(x, g, b, emb, dt, token)
        _check(f"dt {dt} K {K} B {B} N {N} token {token}", prob, lse, ref, bound, token, N)


@pytest.mark.parametrize("dt,K", [(DT_F32, 128), (DT_F32, 384), (DT_F32, 512), (DT_BF16, 384)])
def test_no_speech_row_alone_equals_row_in_batch(hip, dt, K):
    """A row's value is bitwise the same alone, in a batch of 64 and in a 128-row call (other row-block forms, same merge order)."""
    N, token = MICRO_V, 939
    r = np.random.default_rng(K + dt)
    x, g, b, emb = _decoder_like(r, 128, K, N, dt)
    p128, l128 = _probe(x, g, b, emb, dt, token)
    p64, l64 = _probe(x[:64], g, b, emb, dt, token)
    np.testing.assert_array_equal(p64, p128[:64])
    np.testing.assert_array_equal(l64, l128[:64])
    for row in (0, 37, 63):
        p1, l1 = _probe(x[row:row + 1], g, b, emb, dt, token)
        assert p1[0] == p64[row] == p128[row], (row, p1[0], p64[row], p128[row])
        assert l1[0] == l64[row] == l128[row]


@pytest.mark.parametrize("dt,K,B", [(DT_F32, 384, 64), (DT_F32, 128, 128), (DT_F32, 512, 3), (DT_BF16, 384, 3)])
def test_no_speech_offset_1e4(hip, dt, K, B):
    """Every logit moved by 1e4 through the LayerNorm bias (feature 0: gamma 0, beta 1e4, embedding column 1): no overflow, no inf or
    NaN, the value within the bound of the shifted problem."""
    N, token = MICRO_V, 939
    r = np.random.default_rng(K + B)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    g[0], b[0], emb[:, 0] = 0.0, 1e4, 1.0
    ref, bound = _logits_ref(x, g, b, emb, dt)
    assert ref.min() > 9e3
    prob, lse = _probe(x, g, b, emb, dt, token)
    _check(f"offset 1e4 dt {dt} K {K} B {B}", prob, lse, ref, bound, token, N)


def test_no_speech_refuses_bad_arguments(hip):
    from whisper_mojo_amd import _lib
    r = np.random.default_rng(1)
    x, g, b, emb = _decoder_like(r, 2, 128, 100, DT_F32)
    for token in (-1, 100):
        with pytest.raises(_lib.WhisperMiError):
            _probe(x, g, b, emb, DT_F32, token)
    with pytest.raises(_lib.WhisperMiError):
        _probe(x[:, :64], g[:64], b[:64], emb[:, :64], DT_F32, 0)
