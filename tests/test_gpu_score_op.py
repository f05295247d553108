"""Op-level tests (-m gpu) of the score pass's vocabulary side (wm_op_score_logits: score_ln + score_logits + score_merge)
against float64 on the operands as rounded on upload.

Reference: z = the float64 logits of tests/test_gpu_decode_ops.py (_logits_ref: the LayerNorm and the MFMA arithmetic are the decode
step's per dtype and K), logprob = z[target] - logsumexp(z), top_id = the lowest index of the maximum.

Bound per element: 2·e + r.
  e: the row's largest per-logit bound from _logits_ref (it covers z[target], and logsumexp moves by at most the largest perturbation
     of its arguments).
  r: the fp32 cost of THIS kernel's exp-sum, from its arithmetic (u = 2^-24; expf and logf within 1 ulp = 2u, ROCm OCML's bound).
     A part covers T = (stages per part)·(tiles per stage) column tiles of 16; a lane owns 4 columns of every tile.  One term
     exp(v - m) on its way to the sum S:
       created            expf 2u, and its argument fl(v - m) carries u·|v - m|
       lane               4 adds per tile                                            4T·u
       lane rescales      at most one per tile (the running maximum moved): expf + product   3T·u
       4 lanes of a row   2 butterfly merges, each expf + product + add               8u
       merge              expf + product, <= parts adds in ascending part order       (3 + parts)u
     and every rescale's argument fl(m_small - m_big) carries u·|m_small - m_big|: the maxima only grow along the path, so those and
     the creation's telescope to u·(M - v), M the row's maximum.  Relative error of S: Σ_j w_j·((13 + 7T + parts)·u + u·(M - z_j)) / S
     with w_j = exp(z_j - M).  Then logf (2u·|log S|), z[target] - M (u·|z[target] - M|: the maxima leave first, so an offset of the
     whole row costs nothing) and the final subtraction (u·|logprob|).  r = that sum; nothing in it is fitted to an observed error.

top_id must equal float64's argmax wherever the float64 top-2 gap exceeds 2·e."""
import numpy as np
import pytest

from test_gpu_decode_ops import DT_BF16, DT_F16, DT_F32, U, _decoder_like, _logits_ref, hip  # noqa: F401

pytestmark = pytest.mark.gpu

MAX_PARTS = 32  # csrc/kernels_score.hip SCORE_MAX_PARTS


def _geometry(N, dt):
    """(parts, column tiles per part) as score_parts computes them: a function of N and the dtype alone"""
    cs = 2 if dt == DT_F32 else 4
    tiles = (N + 15) // 16
    stages = (tiles + cs - 1) // cs
    spp = (stages + MAX_PARTS - 1) // MAX_PARTS
    return (stages + spp - 1) // spp, spp * cs


RAGGED = 2 * 16 * 1 + 37  # the 2·16·ct + 37 form of tests/test_gpu_logits_lp.py (ct = 1 below 4096 ids): 69 = 4 tiles + 5 columns

# (dtype, K, M, N): every instantiated kernel (f32 split at 128 / 384, exact f32 at 512, bf16 / f16 at each K), one row, a ragged
# 16-row tile, a full block, a block + 1 row, three blocks with a ragged last one; N = 1000 (a ragged last tile of 8), the ragged
# form, and the real vocabulary once
CASES = [
    (DT_F32, 128, 1, 1000),
    (DT_F32, 128, 17, RAGGED),
    (DT_F32, 128, 300, 1000),
    (DT_F32, 384, 128, 1000),
    (DT_F32, 384, 129, 51865),
    (DT_F32, 384, 300, RAGGED),
    (DT_F32, 512, 17, RAGGED),
    (DT_F32, 512, 129, 1000),
    (DT_BF16, 128, 300, 1000),
    (DT_BF16, 384, 1, 1000),
    (DT_BF16, 384, 129, RAGGED),
    (DT_BF16, 512, 128, 1000),
    (DT_F16, 128, 129, RAGGED),
    (DT_F16, 384, 17, 1000),
    (DT_F16, 512, 1, RAGGED),
]


def _score(x, g, b, emb, tg, dt):
    from whisper_mojo_amd import whisper_tensor as wt
    return wt.score_logits(x, g, b, emb, tg, dtype=dt)


def _targets(r, ref, N):
    """per row, in turn: the last id N - 1, the row's argmax, not scored (-1), a random id, id 0"""
    M = ref.shape[0]
    tg = np.zeros(M, np.int32)
    for i in range(M):
        k = i % 5
        tg[i] = (N - 1, int(np.argmax(ref[i])), -1, int(r.integers(0, N)), 0)[k]
    return tg


def _want(ref, bound, tg, N, dt):
    parts, T = _geometry(N, dt)
    M = ref.shape[0]
    out, bnd = np.zeros(M), np.zeros(M)
    for i in range(M):
        if tg[i] < 0:
            continue
        z = ref[i]
        mx = z.max()
        w = np.exp(z - mx)
        S = w.sum()
        out[i] = z[tg[i]] - (mx + np.log(S))
        rel = (w * ((13 + 7 * T + parts) * U + U * (mx - z))).sum() / S
        r = rel + U * (2 * abs(np.log(S)) + abs(z[tg[i]] - mx) + abs(out[i]))
        bnd[i] = 2 * bound[i].max() + r
    return out, bnd


def _check(tag, lp, top, ref, bound, tg, N, dt):
    want, bnd = _want(ref, bound, tg, N, dt)
    assert np.isfinite(lp).all()
    off = tg < 0
    assert (lp[off] == 0).all()
    on = ~off
    if on.any():
        ratio = np.abs(lp[on] - want[on]) / bnd[on]
        print(f"{tag}: worst err/bound {ratio.max():.3g}, max |err| {np.abs(lp[on] - want[on]).max():.3g}, "
              f"bounds {bnd[on].min():.2g}..{bnd[on].max():.2g}")
        assert ratio.max() <= 1.0, (tag, int(np.flatnonzero(on)[np.argmax(ratio)]))
    srt = np.sort(ref, 1)
    clear = (srt[:, -1] - srt[:, -2]) > 2 * bound.max(1) if N > 1 else np.ones(len(ref), bool)
    assert ((top >= 0) & (top < N)).all()
    np.testing.assert_array_equal(top[clear], np.argmax(ref, 1)[clear])
    print(f"{tag}: top_id checked on {int(clear.sum())} of {len(clear)} rows")


@pytest.mark.parametrize("dt,K,M,N", CASES)
def test_score_logits_vs_float64(hip, dt, K, M, N):
    """Every log-prob within 2·e + r of float64, unscored rows exactly 0, the arg-max exact wherever float64 can tell."""
    r = np.random.default_rng(17 * K + 5 * M + N + dt)
    x, g, b, emb = _decoder_like(r, M, K, N, dt)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    tg = _targets(r, ref, N)
    lp, top = _score(x, g, b, emb, tg, dt)
    _check(f"dt {dt} K {K} M {M} N {N}", lp, top, ref, bound, tg, N, dt)


@pytest.mark.parametrize("dt,K", [(DT_F32, 128), (DT_F32, 384), (DT_F32, 512), (DT_BF16, 384), (DT_F16, 512)])
def test_score_row_alone_equals_row_in_batch(hip, dt, K):
    """Bitwise: a row gives the same log-prob and arg-max alone, in one block of 128 and in three blocks."""
    N = 1000
    r = np.random.default_rng(K + dt)
    x, g, b, emb = _decoder_like(r, 300, K, N, dt)
    tg = r.integers(0, N, 300).astype(np.int32)
    lp300, top300 = _score(x, g, b, emb, tg, dt)
    lp128, top128 = _score(x[:128], g, b, emb, tg[:128], dt)
    np.testing.assert_array_equal(lp128, lp300[:128])
    np.testing.assert_array_equal(top128, top300[:128])
    for row in (0, 37, 127, 128, 299):
        lp1, top1 = _score(x[row:row + 1], g, b, emb, tg[row:row + 1], dt)
        assert lp1[0] == lp300[row] and top1[0] == top300[row], (row, lp1[0], lp300[row])


@pytest.mark.parametrize("dt,K,M", [(DT_F32, 384, 129), (DT_F32, 512, 17), (DT_BF16, 128, 130)])
def test_score_offset_and_outlier(hip, dt, K, M):
    """The normaliser cannot overflow: every logit moved by 1e4 through the LayerNorm bias (feature 0: gamma 0, beta 1e4, embedding
    column 1) stays within the bound of the shifted problem; one embedding row scaled by 2^100 (a logit column of that scale) leaves
    every log-prob finite and within its bound."""
    N = 1000
    r = np.random.default_rng(K + M)
    x, g, b, emb = _decoder_like(r, M, K, N, dt)
    g[0], b[0], emb[:, 0] = 0.0, 1e4, 1.0
    ref, bound = _logits_ref(x, g, b, emb, dt)
    assert ref.min() > 9e3
    tg = _targets(r, ref, N)
    lp, top = _score(x, g, b, emb, tg, dt)
    _check(f"offset 1e4 dt {dt} K {K} M {M}", lp, top, ref, bound, tg, N, dt)
    x, g, b, emb = _decoder_like(r, M, K, N, dt)
    emb[N // 2] *= np.float32(2.0 ** 100)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    tg = _targets(r, ref, N)
    lp, top = _score(x, g, b, emb, tg, dt)
    _check(f"outlier 2^100 dt {dt} K {K} M {M}", lp, top, ref, bound, tg, N, dt)


def test_score_logits_refuses_bad_arguments(hip):
    r = np.random.default_rng(0)
    x, g, b, emb = _decoder_like(r, 4, 128, 100, DT_F32)
    with pytest.raises(ValueError):
        _score(x, g, b, emb, np.array([0, 1, 2, 100], np.int32), DT_F32)
    import ctypes as C
    from whisper_mojo_amd import _lib
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    x256 = np.zeros((4, 256), np.float32)
    lp, top, tg = np.zeros(4, np.float32), np.zeros(4, np.int32), np.zeros(4, np.int32)
    f = lambda a: a.ctypes.data_as(fp)
    i = lambda a: a.ctypes.data_as(ip)
    L = _lib.lib()
    assert L.wm_op_score_logits(f(lp), i(top), f(x256), f(x256), f(x256), f(x256), i(tg), 4, 4, 256, 0) == -1  # K
    tg[3] = 100
    assert L.wm_op_score_logits(f(lp), i(top), f(x), f(g), f(b), f(emb), i(tg), 4, 100, 128, 0) == -1  # target >= N
