"""Op-level tests (-m gpu) of the n-best scoring kernels.

Map forms of the cross-attention (wm_op_attention_cached_map, wm_op_xattn_map): bit for bit the existing hooks on the gathered
operands K[map], V[map] / X[map].  The existing hooks are pinned to float64 by tests/test_gpu_decode_ops.py, so bit equality carries
that bound over.  Shapes, K/V dtypes, key counts (65: the fewest chunks the hook's chunked form takes — 2 for the cached form, 1 for
the absorbed sweep; 130: ragged chunks; 1500: the model's count), row maps and chunk shapes as the issue lists them; every (shape,
dtype) runs every (P, key count) pair and rotates through the three row maps, so each map meets each P and each key count.

score_rank_kernel (wm_op_score_rank) against the float64 reference of tests/test_nbest_ref.py: order / best exact, the posterior
within the bound of the reduction as written, with u = 2^-24, d_j = key_j - M <= 0 and p_j the float64 posterior:
    t_j = expf(fl(key_j - M))          expf within 2u, its argument carries u·|d_j|       relative (2 + |d_j|)·u
    S = t_0 + t_1 + ...  in order      a term passes through at most n - 1 adds           relative (n - 1)·u
    so S is off relatively by at most sum_j p_j·(2 + |d_j| + n - 1)·u, the candidate's own term by (2 + |d_c|)·u, and t_c / S
    rounds once (u):   k_c = (2 + |d_c|) + sum_j p_j·(2 + |d_j|) + (n - 1) + 1,   |Δp_c| <= p_c · k_c·u / (1 - k_c·u)
plus the fp32 underflow floor: a term below 2^-126 is rounded to a multiple of 2^-149 or flushed, an absolute 2^-126 at most on t_c
(S >= 1 since the largest term is exactly 1).  Nothing in it is fitted to an observed error."""
import numpy as np
import pytest

from test_gpu_decode_ops import DT_BF16, DT_F16, DT_F32, hip  # noqa: F401
from test_nbest_ref import rank_reference

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
GUARD = 12345.0
ROWMAPS = [(5, 2, [1, 0, 1, 1, 0]), (3, 1, [0, 0, 0]), (1, 1, [0])]  # (batch slots, clips, map)
KEYS = [(65, 2, 1), (130, 4, 4), (1500, 12, 12)]  # (keys, n_chunks of the cached form, nsplit of the absorbed sweep)
PS = [1, 3, 4, 16]

_OPS = {}


def _operands(H, with_w):
    """q [16 * 5, d], K / V (or X) [2, 1500, d] (sliced per case), once per width"""
    if (H, with_w) not in _OPS:
        r = np.random.default_rng(4000 + H)
        d = 64 * H
        q = r.standard_normal((16 * 5, d)).astype(np.float32)
        K = r.standard_normal((2, 1500, d)).astype(np.float32)
        V = r.standard_normal((2, 1500, d)).astype(np.float32)
        W = [(r.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32) for _ in range(2)] if with_w else None
        bv = r.standard_normal(d).astype(np.float32)
        for a in [q, K, V, bv] + (W or []):
            a.setflags(write=False)
        _OPS[(H, with_w)] = (q, K, V, W, bv)
    return _OPS[(H, with_w)]


def _guarded(shape):
    n = int(np.prod(shape))
    buf = np.full(n + 64, GUARD, np.float32)
    return buf, buf[32:32 + n].reshape(shape)


def _form(P, slots):
    """-> (B rows, q_B, nq) of a chunk of P positions as launch_cross_attn wires it"""
    return P * slots, (slots if P > 1 else 0), (4 if P == 4 else 0)


@pytest.mark.parametrize("kv_dtype", [DT_F32, DT_BF16, DT_F16])
@pytest.mark.parametrize("H", [2, 6, 12, 16])
def test_cached_map_equals_gathered(hip, H, kv_dtype):
    from whisper_mojo_amd import whisper_tensor as wt
    q, K, V, _, _ = _operands(H, False)
    n = 0
    for ip, P in enumerate(PS):
        for ik, (t, n_chunks, _) in enumerate(KEYS):
            slots, n_utt, umap = ROWMAPS[(ip + ik + H) % 3]
            B, q_B, nq = _form(P, slots)
            k, v = K[:n_utt, :t], V[:n_utt, :t]
            m = np.asarray(umap)
            buf, out = _guarded((B, 64 * H))
            wt.attention_cached_map(out, q[:B], k, v, umap, H, kv_dtype, n_chunks, DT_F32, q_B, nq)
            ref = np.zeros((B, 64 * H), np.float32)
            wt.attention_cached(ref, q[:B], k[m], v[m], H, kv_dtype, n_chunks, DT_F32, q_B, -1, nq)
            assert np.isfinite(ref).all() and np.abs(ref).max() > 0
            assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), (P, t, umap)
            assert (buf[:32] == GUARD).all() and (buf[-32:] == GUARD).all()
            n += 1
    assert n == 12


@pytest.mark.parametrize("H", [2, 6])
def test_xattn_map_equals_gathered(hip, H):
    from whisper_mojo_amd import whisper_tensor as wt
    q, X, _, (Wk, Wv), bv = _operands(H, True)
    for ip, P in enumerate(PS):
        for ik, (t, _, nsplit) in enumerate(KEYS):
            slots, n_utt, umap = ROWMAPS[(ip + ik + H) % 3]
            rows, q_B, _ = _form(P, slots)
            x = X[:n_utt, :t]
            m = np.asarray(umap)
            for odt in (DT_F32, DT_BF16):
                buf, out = _guarded((rows, 64 * H))
                wt.xattn_map(out, q[:rows], Wk, Wv, bv, x, umap, H, nsplit, q_B, odt)
                ref = np.zeros((rows, 64 * H), np.float32)
                wt.xattn(ref, q[:rows], Wk, Wv, bv, x[m], H, nsplit, q_B, odt)
                assert np.isfinite(ref).all() and np.abs(ref).max() > 0
                assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), (P, t, umap, odt)
                assert (buf[:32] == GUARD).all() and (buf[-32:] == GUARD).all()


@pytest.mark.parametrize("P", PS)
def test_identity_map_equals_unmapped(hip, P):
    from whisper_mojo_amd import whisper_tensor as wt
    H, t, slots = 2, 130, 2
    q, K, V, (Wk, Wv), bv = _operands(H, True)
    B, q_B, nq = _form(P, slots)
    k, v = K[:slots, :t], V[:slots, :t]
    for kv_dtype in (DT_F32, DT_BF16, DT_F16):
        out, ref = np.zeros((B, 128), np.float32), np.zeros((B, 128), np.float32)
        wt.attention_cached_map(out, q[:B], k, v, [0, 1], H, kv_dtype, 4, DT_F32, q_B, nq)
        wt.attention_cached(ref, q[:B], k, v, H, kv_dtype, 4, DT_F32, q_B, -1, nq)
        assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    out, ref = np.zeros((B, 128), np.float32), np.zeros((B, 128), np.float32)
    wt.xattn_map(out, q[:B], Wk, Wv, bv, k, [0, 1], H, 4, q_B)
    wt.xattn(ref, q[:B], Wk, Wv, bv, k, H, 4, q_B)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))


def test_map_hooks_refuse(hip):
    from whisper_mojo_amd import _lib
    from whisper_mojo_amd import whisper_tensor as wt
    H = 2
    q, K, V, (Wk, Wv), bv = _operands(H, True)
    k, v = K[:2, :65], V[:2, :65]
    out = np.zeros((5, 128), np.float32)
    for bad in ([1, 0, 2, 1, 0], [1, 0, -1, 1, 0]):  # a map entry outside [0, n_utt): the library refuses
        with pytest.raises(_lib.WhisperMiError):
            wt.attention_cached_map(out, q[:5], k, v, bad, H, DT_F32, 2)
        with pytest.raises(_lib.WhisperMiError):
            wt.xattn_map(out, q[:5], Wk, Wv, bv, k, bad, H, 1)
    for bad in ([1, 0, 1, 1], [1, 0, 1, 1, 0, 0]):  # a wrong row count: refused before the call
        with pytest.raises(ValueError):
            wt.attention_cached_map(out, q[:5], k, v, bad, H, DT_F32, 2)
        with pytest.raises(ValueError):
            wt.xattn_map(out, q[:5], Wk, Wv, bv, k, bad, H, 1)
    with pytest.raises(ValueError):  # the single-workgroup (self-attention) forms take no map
        wt.attention_cached_map(out, q[:5], k, v, [1, 0, 1, 1, 0], H, DT_F32, 1)
    assert not out.any()


# ---- score_rank_kernel ---------------------------------------------------------------------------------------------------------
def _post_bound(key, n_cand, post64):
    key = np.asarray(key, np.float64)
    bnd = np.zeros(key.size)
    r0 = 0
    for n in np.asarray(n_cand).tolist():
        d = np.abs(key[r0:r0 + n] - key[r0:r0 + n].max())
        p = post64[r0:r0 + n]
        k = (2 + d) + (p * (2 + d)).sum() + (n - 1) + 1
        bnd[r0:r0 + n] = p * k * U32 / (1 - k * U32) + 2.0 ** -126
        r0 += n
    return bnd


def _check_rank(tag, key, n_cand):
    from whisper_mojo_amd import whisper_tensor as wt
    key = np.asarray(key, np.float32)
    order, best, post = wt.score_rank(key, n_cand)
    ro, rb, rp = rank_reference(key, n_cand)
    np.testing.assert_array_equal(order, ro)
    np.testing.assert_array_equal(best, rb)
    bnd = _post_bound(key, n_cand, rp)
    err = np.abs(post.astype(np.float64) - rp)
    print(f"{tag}: worst |posterior - float64| / bound {(err / bnd).max():.3g}, max err {err.max():.3g}, zeros {int((post == 0).sum())}")
    assert (err <= bnd).all(), (tag, int(np.argmax(err / bnd)))
    return order, best, post


N_CAND = [1, 2, 33, 64]


def _distinct_keys(r, lo, hi, n):
    """n keys of [lo, hi] whose distinct values differ by far more than fp32 resolution: multiples of 2^-10, no value drawn twice"""
    steps = int((hi - lo) * 1024)
    return (lo + r.choice(steps, n, replace=False) / 1024.0).astype(np.float32)


def test_rank_vs_float64(hip):
    r = np.random.default_rng(77)
    R = sum(N_CAND)
    _check_rank("typical sums", _distinct_keys(r, -40.0, -5.0, R), N_CAND)
    key = _distinct_keys(r, -200.0, 0.0, R)
    _, _, post = _check_rank("spread 0 .. -200", key, N_CAND)
    assert (post[3:] == 0).any()  # some posteriors underflow
    _, _, post = _check_rank("all equal", np.full(R, -3.25, np.float32), N_CAND)
    for r0, n in zip(np.cumsum(N_CAND) - N_CAND, N_CAND):
        assert np.array_equal(post[r0:r0 + n], np.full(n, np.float32(1) / np.float32(n)))
    key = _distinct_keys(r, -30.0, -1.0, R)
    key[3 + 5] = key[3 + 20] = key[3 + 7]            # exact ties inside the 33-candidate clip
    key[36:] = np.repeat(key[36:36 + 16], 4)          # the 64-candidate clip: sixteen values, each four times in a row
    order, _, _ = _check_rank("exact ties", key, N_CAND)
    o33 = order[3:36].tolist()
    assert o33.index(5) < o33.index(7) < o33.index(20)


def test_rank_clip_isolation(hip):
    from whisper_mojo_amd import whisper_tensor as wt
    r = np.random.default_rng(78)
    key = _distinct_keys(r, -60.0, -1.0, sum(N_CAND))
    a = wt.score_rank(key, N_CAND)
    key2 = key.copy()
    key2[3:36] = _distinct_keys(r, -200.0, 50.0, 33)  # clip 2 alone changes
    b = wt.score_rank(key2, N_CAND)
    keep = np.ones(key.size, bool)
    keep[3:36] = False
    assert np.array_equal(a[0][keep], b[0][keep]) and np.array_equal(a[2][keep].view(np.uint32), b[2][keep].view(np.uint32))
    assert np.array_equal(np.delete(a[1], 2), np.delete(b[1], 2))
    assert not np.array_equal(a[2][~keep], b[2][~keep])


def test_rank_refuses(hip):
    from whisper_mojo_amd import whisper_tensor as wt
    with pytest.raises(ValueError):
        wt.score_rank(np.zeros(3, np.float32), [2, 0, 1])
    with pytest.raises(ValueError):
        wt.score_rank(np.zeros(3, np.float32), [2, 2])
    from whisper_mojo_amd import _lib
    for bad in (np.nan, np.inf, -np.inf):  # NaN keys have no rank: the hook refuses non-finite keys
        with pytest.raises(_lib.WhisperMiError):
            wt.score_rank(np.asarray([-1.0, bad, -2.0], np.float32), [3])
