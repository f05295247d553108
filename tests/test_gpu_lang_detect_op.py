"""Op-level tests (-m gpu) of lang_detect_kernel (wm_op_lang_detect) against float64 on the operands as rounded on upload.

Reference: s = the float64 logits of tests/test_gpu_decode_ops.py (_logits_ref) at the candidate columns only (its reference and
bound are per column); log p_c = s_c - logsumexp over the n_lang candidates; the id = the candidate with the largest s.

Bound on |Δ log p_c|: 2·e + r.
  e: the largest per-logit bound _logits_ref derives for the row's candidates.  It covers the candidate's own logit and the
     logsumexp (which moves by at most the largest perturbation of its arguments).  The kernel forms a logit as the no-speech finish
     does: a K-term fp32 dot product of the LayerNorm output (rounded to the operand dtype) with the embedding row, K/64 products per
     lane and 6 butterfly adds — at most K roundings, inside the order-independent accumulation term of e for every variant — and
     LayerNorm statistics summed K/64 deep per lane plus 6 butterfly adds, not deeper than the K/8 + 3 _ln_err assumes.
  r: the fp32 cost of the n_lang-term exp-sum in list order (u = 2^-24; expf within 2u), with M the largest computed logit (the
     shift by M cancels exactly in a softmax, so which logit won costs nothing):
       one term t_j = expf(fl(s_j - M))     expf 2u, and its argument carries u·|s_j - M|
       S = t_0 + t_1 + …  by one thread     a term passes through at most n_lang - 1 adds          (n_lang - 1)·u
     so S is off by at most Σ_j t_j·u·(2 + |s_j - M| + n_lang - 1) / S relatively, the candidate's own term by u·(2 + |s_c - M|),
     and the division t_c / S rounds once (u).  Nothing in it is fitted to an observed error.

Arg-max: equal to float64's on every row whose float64 top-2 gap exceeds 2·e; SEEDS below were chosen on the CPU (reference and
bound are numpy) so that no row of any case is left out, and the test asserts that."""
import numpy as np
import pytest

from test_gpu_decode_ops import DT_BF16, DT_F16, DT_F32, U, _decoder_like, _logits_ref, hip  # noqa: F401

pytestmark = pytest.mark.gpu

MICRO_V, MULTI_V = 1000, 51865

# (dtype, K, B, N, n_lang)
CASES = [
    (DT_F32, 128, 1, MICRO_V, 1),
    (DT_F32, 128, 3, MULTI_V, 5),
    (DT_F32, 128, 64, MICRO_V, 99),
    (DT_F32, 128, 128, MICRO_V, 128),
    (DT_F32, 384, 1, MULTI_V, 99),
    (DT_F32, 384, 64, MULTI_V, 128),
    (DT_F32, 384, 128, MICRO_V, 5),
    (DT_F32, 512, 3, MULTI_V, 99),
    (DT_F32, 512, 64, MICRO_V, 128),
    (DT_F32, 512, 128, MICRO_V, 1),
    (DT_BF16, 128, 1, MICRO_V, 5),
    (DT_BF16, 384, 3, MULTI_V, 99),
    (DT_BF16, 384, 64, MICRO_V, 5),    # (16-bit: 2·e is ~0.06, a quarter of the median top-2 gap among 99 candidates — no seed
    (DT_BF16, 512, 128, MICRO_V, 1),   #  clears 64 rows x 99 candidates, so the large batches carry the short lists)
    (DT_BF16, 512, 3, MICRO_V, 128),
    (DT_F16, 128, 64, MICRO_V, 99),
    (DT_F16, 384, 1, MICRO_V, 128),
    (DT_F16, 512, 3, MULTI_V, 5),
]
# per case: the first seed (base + 1000·k) for which every row's float64 top-2 gap exceeds 2·e (found by _find_seeds below on the CPU)
SEEDS = {}


def _base_seed(dt, K, B, N, n_lang):
    return 23 * K + 7 * B + N + 3 * dt + 131 * n_lang


def _lang_list(r, N, n_lang):
    """unsorted, with id N - 1 and (from two entries on) id 0"""
    if n_lang == 1:
        return np.asarray([N - 1], np.int32)
    rest = r.choice(np.arange(1, N - 1), n_lang - 2, replace=False)
    ids = np.concatenate([[N - 1], rest, [0]]).astype(np.int32)
    mid = ids[1:-1]
    r.shuffle(mid)
    return ids  # N - 1 first, 0 last: never sorted


def _data(dt, K, B, N, n_lang, seed):
    r = np.random.default_rng(seed)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    return x, g, b, emb, _lang_list(r, N, n_lang)


def _ref(x, g, b, emb, ids, dt):
    """-> (log p float64 [B, n], bound [B, n], float64 arg-max ids [B], top-2 gap [B], e [B])"""
    return _ref_from(*_logits_ref(x, g, b, emb[ids], dt), ids)


def _ref_from(ref, bound, ids):
    """the same from the candidates' float64 logits and their per-logit bound (tests/test_gpu_fused_ln_op.py brings its own)"""
    n = len(ids)
    M = ref.max(1, keepdims=True)
    w = np.exp(ref - M)
    S = w.sum(1, keepdims=True)
    lp = ref - M - np.log(S)
    rel = (w * U * (n + 1 + (M - ref))).sum(1, keepdims=True) / S
    r = rel + U * (3 + (M - ref))
    e = bound.max(1)
    srt = np.sort(ref, 1)
    gap = srt[:, -1] - srt[:, -2] if n > 1 else np.full(len(ref), np.inf)
    return lp, 2 * e[:, None] + r, ids[np.argmax(ref, 1)], gap, e


def _find_seeds():
    """CPU: python -c "import sys; sys.path.insert(0, 'tests'); import test_gpu_lang_detect_op as t; t._find_seeds()" """
    for c in CASES:
        seed = _base_seed(*c)
        while True:
            x, g, b, emb, ids = _data(*c, seed)
            _, _, _, gap, e = _ref(x, g, b, emb, ids, c[0])
            if (gap > 2 * e).all():
                break
            seed += 1000
        print(f"    {c}: {seed},", flush=True)


SEEDS.update({
    (DT_F32, 128, 1, MICRO_V, 1): 4082,
    (DT_F32, 128, 3, MULTI_V, 5): 55485,
    (DT_F32, 128, 64, MICRO_V, 99): 17361,
    (DT_F32, 128, 128, MICRO_V, 128): 21608,
    (DT_F32, 384, 1, MULTI_V, 99): 73673,
    (DT_F32, 384, 64, MULTI_V, 128): 79913,
    (DT_F32, 384, 128, MICRO_V, 5): 11383,
    (DT_F32, 512, 3, MULTI_V, 99): 76631,
    (DT_F32, 512, 64, MICRO_V, 128): 29992,
    (DT_F32, 512, 128, MICRO_V, 1): 13803,
    (DT_BF16, 128, 1, MICRO_V, 5): 4609,
    (DT_BF16, 384, 3, MULTI_V, 99): 73690,
    (DT_BF16, 384, 64, MICRO_V, 5): 59938,
    (DT_BF16, 512, 128, MICRO_V, 1): 13806,
    (DT_BF16, 512, 3, MICRO_V, 128): 32568,
    (DT_F16, 128, 64, MICRO_V, 99): 17367,
    (DT_F16, 384, 1, MICRO_V, 128): 26613,
    (DT_F16, 512, 3, MULTI_V, 5): 64323,
})


def _run(x, g, b, emb, ids, dt):
    from whisper_mojo_amd import whisper_tensor as wt
    return wt.lang_detect(x, g, b, emb, ids, dtype=dt)


def _check(tag, got, probs, x, g, b, emb, ids, dt, need_all=True, refs=None):
    lp, bnd, want, gap, e = _ref(x, g, b, emb, ids, dt) if refs is None else _ref_from(*refs, ids)
    assert np.isfinite(probs).all() and (probs > 0).all() and (probs <= 1).all(), tag
    ratio = np.abs(np.log(probs.astype(np.float64)) - lp) / bnd
    print(f"{tag}: worst err/bound {ratio.max():.3g}, max |err| {np.abs(np.log(probs.astype(np.float64)) - lp).max():.3g}, "
          f"bounds {bnd.min():.2g}..{bnd.max():.2g}, smallest top-2 gap / 2e {(gap / (2 * e)).min():.3g}")
    assert ratio.max() <= 1.0, (tag, np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    clear = gap > 2 * e
    if need_all:
        assert clear.all(), (tag, "rows left out of the arg-max check", np.flatnonzero(~clear))
    np.testing.assert_array_equal(got[clear], want[clear], err_msg=tag)


@pytest.mark.parametrize("dt,K,B,N,n_lang", CASES)
def test_lang_detect_vs_float64(hip, dt, K, B, N, n_lang):
    """every candidate's log-probability within 2·e + r of float64; the id = float64's arg-max on every row (none left out)"""
    c = (dt, K, B, N, n_lang)
    x, g, b, emb, ids = _data(*c, SEEDS[c])
    got, probs = _run(x, g, b, emb, ids, dt)
    assert probs.shape == (B, n_lang)
    _check(f"dt {dt} K {K} B {B} N {N} n_lang {n_lang}", got, probs, x, g, b, emb, ids, dt)


@pytest.mark.parametrize("dt,K,B", [(DT_BF16, 384, 64), (DT_BF16, 512, 128), (DT_F16, 384, 128)])
def test_lang_detect_16bit_large_batch_long_list_logprobs(hip, dt, K, B):
    """16-bit operands, 64 / 128 rows x 99 candidates: the log-probabilities within the bound on every row (they need no gap), the id
    on the rows whose float64 top-2 gap exceeds 2·e (no seed clears every row here, see CASES)"""
    x, g, b, emb, ids = _data(dt, K, B, MICRO_V, 99, 7 * K + B + dt)
    got, probs = _run(x, g, b, emb, ids, dt)
    _check(f"dt {dt} K {K} B {B} n_lang 99 (log-probs on every row)", got, probs, x, g, b, emb, ids, dt, need_all=False)


@pytest.mark.parametrize("dt", [DT_F32, DT_BF16])
def test_lang_detect_tie_goes_to_the_smaller_id(hip, dt):
    """candidates with identical embedding rows, larger ids listed first: the smaller id wins (what an arg-max over the vocabulary
    row with the rest at -inf returns), and the tied candidates get the same probability"""
    r = np.random.default_rng(5)
    x, g, b, emb = _decoder_like(r, 3, 384, MICRO_V, dt)
    emb[700] = emb[12]
    got, probs = _run(x, g, b, emb, np.asarray([700, 12], np.int32), dt)
    assert (got == 12).all(), got
    np.testing.assert_array_equal(probs[:, 0], probs[:, 1])
    emb[0] = emb[999] = emb[12]  # all candidates tied, the smallest id in the middle of the list
    got, probs = _run(x, g, b, emb, np.asarray([999, 700, 0, 12], np.int32), dt)
    assert (got == 0).all(), got
    np.testing.assert_array_equal(probs, np.full((3, 4), 0.25, np.float32))


@pytest.mark.parametrize("dt,K", [(DT_F32, 128), (DT_F32, 384), (DT_F32, 512), (DT_BF16, 384)])
def test_lang_detect_row_alone_equals_row_in_batch(hip, dt, K):
    """a row's id and probabilities are bitwise the same alone, in a batch of 64 and in a 128-row call"""
    r = np.random.default_rng(K + dt)
    x, g, b, emb = _decoder_like(r, 128, K, MICRO_V, dt)
    ids = _lang_list(r, MICRO_V, 99)
    i128, p128 = _run(x, g, b, emb, ids, dt)
    i64, p64 = _run(x[:64], g, b, emb, ids, dt)
    np.testing.assert_array_equal(i64, i128[:64])
    np.testing.assert_array_equal(p64, p128[:64])
    for row in (0, 37, 63):
        i1, p1 = _run(x[row:row + 1], g, b, emb, ids, dt)
        assert i1[0] == i64[row]
        np.testing.assert_array_equal(p1[0], p64[row])


@pytest.mark.parametrize("dt,K,B", [(DT_F32, 384, 64), (DT_F32, 128, 128), (DT_F32, 512, 3), (DT_BF16, 384, 3)])
def test_lang_detect_offset_1e4(hip, dt, K, B):
    """every logit moved by 1e4 through the LayerNorm bias (feature 0: gamma 0, beta 1e4, embedding column 1): finite values within
    the bound of the shifted problem"""
    r = np.random.default_rng(K + B)
    x, g, b, emb = _decoder_like(r, B, K, MICRO_V, dt)
    ids = _lang_list(r, MICRO_V, 99)
    g[0], b[0], emb[:, 0] = 0.0, 1e4, 1.0
    ref, _ = _logits_ref(x, g, b, emb[ids], dt)
    assert ref.min() > 9e3
    got, probs = _run(x, g, b, emb, ids, dt)
    _check(f"offset 1e4 dt {dt} K {K} B {B}", got, probs, x, g, b, emb, ids, dt, need_all=False)


def test_lang_detect_refuses_bad_arguments(hip):
    """the library's own refusals (ctypes, past the Python wrapper's host checks)"""
    import ctypes as C

    from whisper_mojo_amd import _lib
    L = _lib.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    r = np.random.default_rng(1)
    x, g, b, emb = _decoder_like(r, 2, 128, 100, DT_F32)
    out, probs = np.zeros(2, np.int32), np.zeros((2, 129), np.float32)

    def call(ids, K=128):
        ids = np.asarray(ids, np.int32)
        return L.wm_op_lang_detect(out.ctypes.data_as(ip), probs.ctypes.data_as(fp), x.ctypes.data_as(fp), g.ctypes.data_as(fp),
                                   b.ctypes.data_as(fp), emb.ctypes.data_as(fp), ids.ctypes.data_as(ip), ids.size, 2, 100, K, DT_F32)

    assert call([3, 7]) == 0
    for bad in ([], list(range(100)) + list(range(29)), [3, 100], [3, -1], [3, 7, 3]):
        assert call(bad) != 0, bad
    assert call([3, 7], K=64) != 0
