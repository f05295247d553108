"""Op-level tests (-m gpu) of the log-probability path of the fused argmax (wm_op_logits_lp: the LP instantiation of the logits
kernel's stage 1 + argmax_step's merge) against float64 on the operands as rounded on upload.

Reference: s = the float64 logits of tests/test_gpu_decode_ops.py (_logits_ref) plus the mask; the candidates are what the mask and
the ranges leave; logprob = s[id] - logsumexp(s over the candidates), keyed on the id the kernel chose (a timestamp id: the forced
branch, normaliser over the admissible timestamps alone; a text id with the rules on: text ∪ timestamps; rules off: everything).

Bound per element: 2·e + r.
  e: the largest per-logit bound _logits_ref derives for the row's candidates (it covers s[id], and logsumexp moves by at most the
     largest perturbation of its arguments).
  r: the fp32 cost of the kernel's exp-sum, from its arithmetic (u = 2^-24; expf and logf within 1 ulp = 2u, ROCm OCML's bound).
     One term exp(v - m) on its way to the sum S:
       created            expf 2u, and its argument fl(v - m) carries u·|v - m|
       lane               <= 7 adds                                                   7u
       4 lanes of a row   2 merges, each expf + product + add                         8u
       8 waves            expf + product, <= 8 adds                                  11u
       stage 2            expf + product, <= parts - 1 adds in ascending order       (2 + parts)u
       text ∪ timestamps  expf + product + add                                        4u
     and every rescale's argument fl(m_small - m_big) carries u·|m_small - m_big|: the maxima only grow along the path, so those
     and the creation's telescope to u·(M - v), M the candidates' maximum.  Relative error of S: Σ_j w_j·((35 + parts)·u + u·(M - s_j)) / S
     with w_j = exp(s_j - M).  Then logf (2u·|log S|), s[id] - M (u·|s[id] - M|: the kernel subtracts the maxima first, so an offset
     of the whole row costs nothing) and the final subtraction (u·|logprob|); the compare's inputs are exact fp32 logits.  r = that
     sum; nothing in it is fitted to an observed error."""
import numpy as np
import pytest

from test_gpu_decode_ops import DT_BF16, DT_F16, DT_F32, U, _call_logits, _ct, _decoder_like, _logits_ref, hip  # noqa: F401

pytestmark = pytest.mark.gpu


def _ragged(N0=1000):
    """2·(ids per part) + 37 = 69 with 16 ids per part: five parts, the last one partial (5 ids); _tb puts timestamp_begin inside the second"""
    return 2 * 16 * _ct(N0) + 37


# (dtype, K, B, N): the kernel variant launch_dec_logits reaches is named beside each case (the LP instantiation of it)
LP_CASES = [
    (DT_F32, 128, 1, 1000),      # dec_logits_split_kernel<1,1>
    (DT_F32, 128, 16, _ragged()),  # dec_logits_split_kernel<1,1>
    (DT_F32, 128, 64, 1000),     # dec_logits_split_kernel<1,4>
    (DT_F32, 128, 65, _ragged()),  # dec_logits_split128_kernel<1> (one ragged row block)
    (DT_F32, 128, 128, 1000),    # dec_logits_split128_kernel<1>
    (DT_F32, 384, 1, _ragged()),   # dec_logits_split_kernel<3,1>
    (DT_F32, 384, 16, 1000),     # dec_logits_split_kernel<3,1>
    (DT_F32, 384, 64, _ragged()),  # dec_logits_split_kernel<3,4>
    (DT_F32, 384, 65, 1000),     # dec_logits_split128_kernel<3>
    (DT_F32, 384, 128, _ragged()),  # dec_logits_split128_kernel<3>
    (DT_F32, 384, 64, 51865),    # dec_logits_split_kernel<3,4>, the real part count (250)
    (DT_F32, 512, 1, 1000),      # dec_logits_kernel<float,4,1>
    (DT_F32, 512, 16, _ragged()),  # dec_logits_kernel<float,4,1>
    (DT_F32, 512, 64, 1000),     # dec_logits_kernel<float,4,4>
    (DT_F32, 512, 65, _ragged()),  # dec_logits_kernel<float,4,4> (two row blocks)
    (DT_F32, 512, 128, 1000),    # dec_logits_kernel<float,4,4>
    (DT_BF16, 128, 16, 1000),    # dec_logits_kernel<bf16,1,1>
    (DT_BF16, 384, 65, _ragged()),  # dec_logits_kernel<bf16,3,4>
    (DT_BF16, 512, 128, 1000),   # dec_logits_kernel<bf16,4,4>
    (DT_F16, 384, 64, 1000),     # dec_logits_kernel<f16,3,4>
    (DT_F16, 128, 1, _ragged()),   # dec_logits_kernel<f16,1,1>
]


def _tb(N):
    """timestamp_begin inside the second part, so that one part holds both text and timestamp ids"""
    return 16 * _ct(N) + 5 if N < 4000 else N - 1501


def _lp(x, g, b, emb, dt, **kw):
    return _call_logits(x, g, b, emb, dt, return_logprobs=True, **kw)


def _cands(N, mask, rng, id_, tb):
    """candidate ids of one row for the id the kernel chose.  The branch (forced / mixed) is read off the kernel's own id: that id is
    checked bitwise against wm_op_logits in the same test, and the decision itself against float64 in tests/test_gpu_decode_ops.py."""
    ok = np.ones(N, bool) if mask is None else np.isfinite(mask)
    if rng is None:
        return np.flatnonzero(ok)
    tlo, thi, qlo, qhi = (int(v) for v in rng)
    j = np.arange(N)
    ts = ok & (j >= qlo) & (j < qhi)
    if id_ >= tb and ts[id_]:
        return np.flatnonzero(ts)  # forced: the timestamps alone
    return np.flatnonzero(ts | (ok & (j >= tlo) & (j < thi)))


def _lp_ref(ref, bound, mask, ranges, ids, tb, N):
    """-> (logprob float64 [B], bound [B]) by the module docstring's rule"""
    parts = (N + 16 * _ct(N) - 1) // (16 * _ct(N))
    B = ref.shape[0]
    out, bnd = np.zeros(B), np.zeros(B)
    for b in range(B):
        c = _cands(N, mask, None if ranges is None else ranges[b], int(ids[b]), tb)
        if c.size == 0 or ids[b] not in c:
            out[b], bnd[b] = -np.inf, 0.0
            continue
        s = ref[b, c]
        M = s.max()
        w = np.exp(s - M)
        S = w.sum()
        lse = M + np.log(S)
        out[b] = ref[b, ids[b]] - lse
        rel = (w * ((35 + parts) * U + U * (M - s))).sum() / S
        r = rel + U * (2 * abs(np.log(S)) + abs(ref[b, ids[b]] - M) + abs(out[b]))
        bnd[b] = 2 * bound[b, c].max() + r
    return out, bnd


def _check(tag, lp, ref, bound, mask, ranges, ids, tb, N):
    want, bnd = _lp_ref(ref, bound, mask, ranges, ids, tb, N)
    assert not np.isnan(lp).any()
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isfinite(lp), fin)
    assert (lp[~fin] == -np.inf).all()
    assert (lp[fin] <= 0).all()
    ratio = np.abs(lp[fin] - want[fin]) / bnd[fin]
    print(f"{tag}: worst err/bound {ratio.max():.3g}, max |err| {np.abs(lp[fin] - want[fin]).max():.3g}, bounds {bnd[fin].min():.2g}..{bnd[fin].max():.2g}")
    assert ratio.max() <= 1.0, (tag, int(np.argmax(ratio)))


def _ranges(B, N, tb, kinds, ref=None, mask=None):
    """forced rows: one text id against every timestamp; mixed rows: all text against three timestamps.  With ref (the float64
    logits): the forced rows' text id is the row's lowest text logit and the mixed rows' timestamp range the single lowest timestamp
    logit, so that the branch a row takes does not hang on the draw."""
    rg = np.zeros((B, 4), np.int32)
    for b in range(B):
        t, q = 5, tb
        if ref is not None:
            v = ref[b] + (0 if mask is None else mask)
            if kinds[b]:
                t = int(np.argmin(np.where(np.isfinite(v[:tb]), v[:tb], np.inf)))
            else:
                q = tb + int(np.argmin(np.where(np.isfinite(v[tb:]), v[tb:], np.inf)))
        rg[b] = (t, t + 1, tb, N) if kinds[b] else (0, tb, q, min(N, q + (3 if ref is None else 1)))
    return rg


@pytest.mark.parametrize("dt,K,B,N", LP_CASES)
def test_logprob_vs_float64(hip, dt, K, B, N):
    """Every normaliser branch within 2·e + r of float64; ids and logits bitwise those of wm_op_logits."""
    r = np.random.default_rng(31 * K + 7 * B + N + dt)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    mask = np.zeros(N, np.float32)
    mask[[3, N // 2, N - 1]] = -np.inf
    tb = _tb(N)
    # rules off: everything the mask leaves
    logits, ids, lp = _lp(x, g, b, emb, dt, mask=mask)
    plain, pids = _call_logits(x, g, b, emb, dt, mask=mask)
    np.testing.assert_array_equal(logits, plain)
    np.testing.assert_array_equal(ids, pids)
    _check(f"dt {dt} K {K} B {B} N {N} rules off", lp, ref, bound, mask, None, ids, tb, N)
    # rules on: forced-timestamp and mixed rows (B = 1: one call each)
    seen = set()
    for kinds in ([b_ % 2 == 0 for b_ in range(B)], [b_ % 2 == 1 for b_ in range(B)])[:2 if B == 1 else 1]:
        rg = _ranges(B, N, tb, kinds, ref, mask)
        logits, ids, lp = _lp(x, g, b, emb, dt, mask=mask, ranges=rg, timestamp_begin=tb)
        plain, pids = _call_logits(x, g, b, emb, dt, mask=mask, ranges=rg, timestamp_begin=tb)
        np.testing.assert_array_equal(logits, plain)
        np.testing.assert_array_equal(ids, pids)
        _check(f"dt {dt} K {K} B {B} N {N} rules on", lp, ref, bound, mask, rg, ids, tb, N)
        seen |= {"forced" if i >= tb else "mixed" for i in ids}
    assert seen == {"forced", "mixed"}


@pytest.mark.parametrize("dt,K", [(DT_F32, 128), (DT_F32, 384), (DT_F32, 512), (DT_BF16, 384)])
def test_logprob_row_alone_equals_row_in_batch(hip, dt, K):
    """A row's log-prob is bitwise the same alone and in a batch of 64 or 128 (other row-block forms of the kernel, same merge order)."""
    N = _ragged()
    tb = _tb(N)
    r = np.random.default_rng(K + dt)
    x, g, b, emb = _decoder_like(r, 128, K, N, dt)
    rg = _ranges(128, N, tb, [i % 2 == 0 for i in range(128)])
    for kw in ({}, {"ranges": rg, "timestamp_begin": tb}):
        _, ids128, lp128 = _lp(x, g, b, emb, dt, **kw)
        kw64 = dict(kw, ranges=rg[:64]) if kw else kw
        _, ids64, lp64 = _lp(x[:64], g, b, emb, dt, **kw64)
        np.testing.assert_array_equal(lp64, lp128[:64])
        for row in (0, 37, 63):
            kw1 = dict(kw, ranges=rg[row:row + 1]) if kw else kw
            _, id1, lp1 = _lp(x[row:row + 1], g, b, emb, dt, **kw1)
            assert id1[0] == ids128[row] == ids64[row]
            assert lp1[0] == lp64[row] == lp128[row], (row, lp1[0], lp64[row], lp128[row])


@pytest.mark.parametrize("dt,K,B", [(DT_F32, 384, 64), (DT_F32, 128, 128), (DT_F32, 512, 16), (DT_BF16, 384, 16)])
def test_logprob_offset_1e4(hip, dt, K, B):
    """Every logit moved by 1e4 through the LayerNorm bias (feature 0: gamma 0, beta 1e4, embedding column 1): no overflow, no inf or
    NaN, every log-prob within the bound of the shifted problem."""
    N = 1000
    tb = _tb(N)
    r = np.random.default_rng(K + B)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    g[0], b[0], emb[:, 0] = 0.0, 1e4, 1.0
    ref, bound = _logits_ref(x, g, b, emb, dt)
    assert ref.min() > 9e3
    rg = _ranges(B, N, tb, [i % 2 == 0 for i in range(B)])
    for kw, rr in (({}, None), ({"ranges": rg, "timestamp_begin": tb}, rg)):
        logits, ids, lp = _lp(x, g, b, emb, dt, **kw)
        assert np.isfinite(lp).all()
        _check(f"offset 1e4 dt {dt} K {K} B {B} {'on' if kw else 'off'}", lp, ref, bound, None, rr, ids, tb, N)


@pytest.mark.parametrize("dt,K,B", [(DT_F32, 384, 3), (DT_F32, 128, 70), (DT_BF16, 512, 20)])
def test_logprob_all_masked(hip, dt, K, B):
    """A mask over the whole vocabulary: id 0, log-prob -inf (never NaN), with the rules off and on."""
    N = _ragged()
    tb = _tb(N)
    r = np.random.default_rng(K)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    mask = np.full(N, -np.inf, np.float32)
    for kw in ({}, {"ranges": np.tile(np.array([[0, tb, tb, N]], np.int32), (B, 1)), "timestamp_begin": tb}):
        _, ids, lp = _lp(x, g, b, emb, dt, mask=mask, **kw)
        assert (ids == 0).all()
        assert (lp == -np.inf).all()
