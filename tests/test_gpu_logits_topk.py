"""Op-level tests (-m gpu) of the top-k alternatives (wm_op_logits_topk): the logits kernel's stored, processed rows, the
top-k instantiation of argmax_step and the selection launch behind it, against float64 on the operands as rounded on upload.

Three bars, the ones the feature's contract names:
  exact   the k ids are the stable top-k (value descending, lowest id first among equals) of the kernel's OWN fp32 logits over the
          candidates the mask and the ranges leave — bit for bit, ties included; missing ranks are (-1, -inf);
  ids     against float64 (tests/test_gpu_decode_ops.py _logits_ref): rank r's id equals the reference's wherever the reference's
          gaps to both neighbouring ranks exceed the product-error bound of the two logits compared (their bounds' sum);
  lp      |lp - (ref[id] - logsumexp64)| <= 2·e + r, the bar of tests/test_gpu_logits_lp.py: e the largest per-logit bound among the
          row's candidates, r the fp32 cost of the exp-sum derived there.  A rank's value is (v - ref) - logz in fp32 with the very
          (ref, logz) the chosen id's log-prob was formed from, so the two extra roundings are the ones r already counts (u·|s[id] - M|
          and u·|logprob|).
Rank 0 equals wm_op_logits_lp's id and log-prob bit for bit.  Each case prints worst err / bound."""
import numpy as np
import pytest

from test_gpu_decode_ops import DT_BF16, DT_F16, DT_F32, U, _ct, _decoder_like, _logits_ref, hip  # noqa: F401
from test_gpu_logits_lp import _cands, _lp, _ragged, _ranges, _tb

pytestmark = pytest.mark.gpu


def _topk(x, g, b, emb, dt, k, **kw):
    from whisper_mojo_amd import whisper_tensor as wt
    return wt.logits_topk(x, g, b, emb, k, dtype=dt, **kw)


def _stable_topk(vals, ids, k):
    """the k ids of `ids` with the largest finite `vals`, descending, lowest id first among equals; -1 where none is left"""
    fin = np.isfinite(vals)
    v, i = vals[fin], ids[fin]
    order = np.lexsort((i, -v))[:k]
    out = np.full(k, -1, np.int64)
    out[:order.size] = i[order]
    return out


def _check(tag, out, ref, bound, mask, ranges, tb, N, k):
    logits, ids, lp, top_ids, top_lp = out
    B = ref.shape[0]
    parts = (N + 16 * _ct(N) - 1) // (16 * _ct(N))
    assert not np.isnan(top_lp).any()
    np.testing.assert_array_equal(top_ids[:, 0], ids)
    np.testing.assert_array_equal(top_lp[:, 0].view(np.uint32), lp.view(np.uint32))
    worst, worst_at, compared, skipped = 0.0, None, 0, 0
    mk = np.zeros(N) if mask is None else mask.astype(np.float64)
    for b in range(B):
        c = _cands(N, mask, None if ranges is None else ranges[b], int(ids[b]), tb)
        # exact: the stable top-k of the kernel's own logits
        want = _stable_topk(logits[b, c].astype(np.float64) + mk[c], c, k)
        n_fin = int((want >= 0).sum())
        if n_fin == 0:
            want[0] = 0  # nothing finite: the emitted id 0 with -inf
        np.testing.assert_array_equal(top_ids[b], want, err_msg=f"{tag} row {b}")
        assert (top_lp[b, n_fin:] == -np.inf).all() and (top_ids[b, max(n_fin, 1):] == -1).all()
        if n_fin == 0:
            continue
        assert np.isfinite(top_lp[b, :n_fin]).all() and (top_lp[b, :n_fin] <= 0).all()
        assert (np.diff(top_lp[b, :n_fin]) <= 0).all()
        # ids against float64 where the reference's gaps exceed the product-error bound
        s = ref[b, c]
        order = np.lexsort((c, -s))[:k + 1]
        rid, rs, rb = c[order], s[order], bound[b, c[order]]
        for r in range(min(k, n_fin)):
            up = np.inf if r == 0 else rs[r - 1] - rs[r] - (rb[r - 1] + rb[r])
            dn = np.inf if r + 1 >= rid.size else rs[r] - rs[r + 1] - (rb[r] + rb[r + 1])
            if up > 0 and dn > 0:
                compared += 1
                assert top_ids[b, r] == rid[r], (tag, b, r, top_ids[b], rid)
            else:
                skipped += 1
        # log-probs: 2·e + r per rank
        M = s.max()
        w = np.exp(s - M)
        S = w.sum()
        lse = M + np.log(S)
        rel = (w * ((35 + parts) * U + U * (M - s))).sum() / S
        e = bound[b, c].max()
        for r in range(n_fin):
            t = ref[b, top_ids[b, r]]
            want_lp = t - lse
            bnd = 2 * e + rel + U * (2 * abs(np.log(S)) + abs(t - M) + abs(want_lp))
            ratio = abs(float(top_lp[b, r]) - want_lp) / bnd
            if ratio > worst:
                worst, worst_at = ratio, (b, r)
    print(f"{tag}: lp worst err/bound {worst:.3g} at {worst_at}; ids vs float64: {compared} compared, {skipped} inside the bound")
    assert worst <= 1.0, (tag, worst_at)
    return compared


# (dtype, K, B, N, k): every width, dtype, row regime (1, 17, 64, 128: the 128-row fp32 kernel) and k of the contract; the full
# vocabulary (250 parts, the last one ragged) where the float64 reference stays below ~2e9 multiply-adds
CASES = [
    (DT_F32, 128, 1, 1000, 1),       # dec_logits_split_kernel<1,1>
    (DT_F32, 128, 17, _ragged(), 5),  # dec_logits_split_kernel<1,4>
    (DT_F32, 128, 128, 51865, 8),    # dec_logits_split128_kernel<1>
    (DT_F32, 384, 64, 1000, 8),      # dec_logits_split_kernel<3,4>
    (DT_F32, 384, 128, 1000, 5),     # dec_logits_split128_kernel<3>
    (DT_F32, 384, 17, 51865, 8),     # dec_logits_split_kernel<3,4>
    (DT_F32, 512, 17, 1000, 5),      # dec_logits_kernel<float,4,4>
    (DT_F32, 512, 64, 51865, 1),     # dec_logits_kernel<float,4,4>
    (DT_F32, 768, 1, 51865, 8),      # dec_logits_kernel<float,6,1>
    (DT_F32, 768, 64, 1000, 5),      # dec_logits_kernel<float,6,2>
    (DT_F32, 1024, 17, 1000, 8),     # dec_logits_kernel<float,8,2>
    (DT_F32, 1024, 128, 1000, 1),    # dec_logits_kernel<float,8,2>
    (DT_BF16, 128, 64, 1000, 5),     # dec_logits_kernel<bf16,1,4>
    (DT_BF16, 384, 128, _ragged(), 8),  # dec_logits_kernel<bf16,3,8> / <3,4>
    (DT_BF16, 512, 17, 51865, 8),    # dec_logits_kernel<bf16,4,4>
    (DT_BF16, 1024, 1, 1000, 5),     # dec_logits_kernel<bf16,8,1>
    (DT_F16, 128, 128, 1000, 5),     # dec_logits_kernel<f16,1,8> / <1,4>
    (DT_F16, 384, 17, 1000, 8),      # dec_logits_kernel<f16,3,4>
    (DT_F16, 768, 64, 1000, 1),      # dec_logits_kernel<f16,6,4>
]


@pytest.mark.parametrize("dt,K,B,N,k", CASES)
def test_topk_vs_float64(hip, dt, K, B, N, k):
    """Rules off (everything the mask leaves) and on (forced-timestamp rows beside mixed ones): the three bars of the module
    docstring, and rank 0 bitwise wm_op_logits_lp's."""
    r = np.random.default_rng(17 * K + 5 * B + N + dt + k)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    mask = np.zeros(N, np.float32)
    mask[[3, N // 2, N - 1]] = -np.inf
    mask[np.argsort(-ref[0])[1]] = -np.inf  # row 0's runner-up is masked: it must not come back at any rank
    tb = _tb(N)
    out = _topk(x, g, b, emb, dt, k, mask=mask)
    plain, pids, plp = _lp(x, g, b, emb, dt, mask=mask)
    np.testing.assert_array_equal(out[0], plain)
    np.testing.assert_array_equal(out[1], pids)
    np.testing.assert_array_equal(out[2].view(np.uint32), plp.view(np.uint32))
    assert not np.isin(out[3], np.flatnonzero(~np.isfinite(mask))).any()
    n = _check(f"dt {dt} K {K} B {B} N {N} k {k} rules off", out, ref, bound, mask, None, tb, N, k)
    assert n > 0 or B * k < 16  # (the test's own sanity: the draw leaves ranks the reference can decide)
    seen = set()
    for kinds in ([b_ % 2 == 0 for b_ in range(B)], [b_ % 2 == 1 for b_ in range(B)])[:2 if B == 1 else 1]:
        rg = _ranges(B, N, tb, kinds, ref, mask)
        out = _topk(x, g, b, emb, dt, k, mask=mask, ranges=rg, timestamp_begin=tb)
        _, pids, plp = _lp(x, g, b, emb, dt, mask=mask, ranges=rg, timestamp_begin=tb)
        np.testing.assert_array_equal(out[1], pids)
        np.testing.assert_array_equal(out[2].view(np.uint32), plp.view(np.uint32))
        _check(f"dt {dt} K {K} B {B} N {N} k {k} rules on", out, ref, bound, mask, rg, tb, N, k)
        for row in range(B):  # a forced row holds timestamps alone; a mixed row's lone timestamp may sit at any rank
            if out[1][row] >= tb:
                seen.add("forced")
                assert (out[3][row][out[3][row] >= 0] >= tb).all()
            else:
                seen.add("mixed")
    assert seen == {"forced", "mixed"}


def _plant(emb, src, where, factors):
    """embedding rows `where` become emb[src] scaled by `factors`: their logits are the source's, scaled (exactly equal for factor 1)"""
    for p, f in zip(where, factors):
        emb[p] = emb[src] * np.float32(f)


@pytest.mark.parametrize("dt,K,N,where,name", [
    (DT_F32, 384, 1000, list(range(33, 41)), "one part"),                  # 16 ids per part: all eight inside part 2
    (DT_F32, 128, 1000, list(range(44, 52)), "part edge"),                 # four on each side of the edge at 48
    (DT_BF16, 384, 1000, list(range(44, 52)), "part edge, 16-bit"),
    (DT_F32, 384, 4097, [7 + 256 * j for j in range(9)], "one thread"),    # nine ids one selection thread sweeps: its list overflows
    (DT_F32, 128, 51865, [51860, 51861, 51864, 12, 207, 208, 415, 416], "last part"),  # the ragged last part and the first edges
])
def test_planted_winners(hip, dt, K, N, where, name):
    """The winners sit where the selection can go wrong: inside one part of the logits kernel, across a part edge, all in the ids one
    selection thread sweeps (more than its list holds), in the ragged last part.  Row 0's float64 top-8 is exactly the planted ids."""
    r = np.random.default_rng(N + K + len(name))
    B, k = 3, 8
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    ref, _ = _logits_ref(x, g, b, emb, dt)
    src = int(np.argmax(ref[0]))
    assert ref[0, src] > 0 and src not in where
    _plant(emb, src, where, [3.0 - 0.125 * j for j in range(len(where))])  # distinct, exactly representable factors, all > 1
    ref, bound = _logits_ref(x, g, b, emb, dt)
    np.testing.assert_array_equal(np.argsort(-ref[0])[:k], where[:k])
    out = _topk(x, g, b, emb, dt, k)
    np.testing.assert_array_equal(out[3][0], where[:k])
    _check(f"planted {name}", out, ref, bound, None, None, _tb(N), N, k)


@pytest.mark.parametrize("dt,K", [(DT_F32, 128), (DT_F32, 512), (DT_BF16, 384)])
def test_exact_ties_lowest_id_first(hip, dt, K):
    """Copies of one embedding row give bitwise equal logits: inside a part (ids 10, 11), across parts (20, 300), in one selection
    thread's sweep (5, 261, 517) and across its waves (70, 140).  They tie for the top: the ranks list them by ascending id, with one
    log-prob."""
    N, B, k = 1000, 17, 8
    r = np.random.default_rng(K + dt)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    ref, _ = _logits_ref(x, g, b, emb, dt)
    src = int(np.argmax(ref[0]))
    assert ref[0, src] > 0
    tied = [5, 10, 11, 20, 70, 140, 261, 300, 517]
    _plant(emb, src, tied, [2.0] * len(tied))
    ref, bound = _logits_ref(x, g, b, emb, dt)
    out = _topk(x, g, b, emb, dt, k)
    logits, top_ids, top_lp = out[0], out[3], out[4]
    assert len(set(logits[0, tied].tolist())) == 1  # the kernel's logits of the copies are bitwise equal
    np.testing.assert_array_equal(top_ids[0], tied[:k])
    assert len(set(top_lp[0].tolist())) == 1
    _check(f"ties dt {dt} K {K}", out, ref, bound, None, None, _tb(N), N, k)
    for kk in (1, 5):  # a smaller k is the prefix
        o2 = _topk(x, g, b, emb, dt, kk)
        np.testing.assert_array_equal(o2[3], top_ids[:, :kk])
        np.testing.assert_array_equal(o2[4].view(np.uint32), top_lp[:, :kk].view(np.uint32))


@pytest.mark.parametrize("dt,K,B", [(DT_F32, 384, 17), (DT_F32, 128, 128), (DT_F16, 512, 64)])
def test_winners_split_between_text_and_timestamps(hip, dt, K, B):
    """Mixed rows with wide timestamp ranges: planted winners alternate between the text and the timestamp side, so the merged list
    interleaves the two; forced rows (one weak text id) list timestamps alone."""
    N, k = 1000, 8
    tb = _tb(N)
    r = np.random.default_rng(K + B)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    ref, _ = _logits_ref(x, g, b, emb, dt)
    src = int(np.argmax(ref[0]))
    where = [7, tb + 3, 12, tb + 200, 18, 600, 2, N - 2]  # (tb = 21: text ids lie below it)
    assert tb == 21 and src not in where and ref[0, src] > 0
    _plant(emb, src, where, [8.0, 3.5, 3.0, 2.5, 2.0, 1.75, 1.5, 1.25])  # (the text leader far ahead of the timestamps' whole mass)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    ts0 = ref[0, tb:]
    assert ts0.max() + np.log(np.exp(ts0 - ts0.max()).sum()) < ref[0, 7] - 0.1  # row 0 in float64: the text winner is not overruled
    rg = np.tile(np.array([[0, tb, tb, N]], np.int32), (B, 1))
    out = _topk(x, g, b, emb, dt, k, ranges=rg, timestamp_begin=tb)
    _check(f"text/timestamp split dt {dt} K {K} B {B}", out, ref, bound, None, rg, tb, N, k)
    np.testing.assert_array_equal(out[3][0], where)
    assert {"forced" if i >= tb else "mixed" for i in out[1]} >= {"mixed"}


@pytest.mark.parametrize("dt,K,B,k", [(DT_F32, 384, 3, 8), (DT_F32, 128, 70, 5), (DT_BF16, 512, 20, 8)])
def test_three_finite_candidates_and_none(hip, dt, K, B, k):
    """A mask that leaves three ids: ranks 3.. hold (-1, -inf); a mask over everything: rank 0 is the emitted id 0 with -inf, the
    rest (-1, -inf) — never NaN, with the rules off and on."""
    N = _ragged()
    tb = _tb(N)
    r = np.random.default_rng(K + k)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    keep = [2, tb + 1, N - 1]
    mask = np.full(N, -np.inf, np.float32)
    mask[keep] = 0
    rg = np.tile(np.array([[0, tb, tb, N]], np.int32), (B, 1))
    for kw, rr in (({}, None), ({"ranges": rg, "timestamp_begin": tb}, rg)):
        out = _topk(x, g, b, emb, dt, k, mask=mask, **kw)
        _check(f"three finite dt {dt} K {K} B {B} {'on' if kw else 'off'}", out, ref, bound, mask, rr, tb, N, k)
        n_fin = np.where(out[1] >= tb, 2, 3) if kw else np.full(B, 3)  # a forced row keeps the two timestamps
        for row in range(B):
            assert set(out[3][row][:n_fin[row]].tolist()) <= set(keep)
            assert (out[3][row][n_fin[row]:] == -1).all() and (out[4][row][n_fin[row]:] == -np.inf).all()
        none = _topk(x, g, b, emb, dt, k, mask=np.full(N, -np.inf, np.float32), **kw)
        assert (none[3][:, 0] == 0).all() and (none[3][:, 1:] == -1).all() and (none[4] == -np.inf).all()


def test_with_repetition_sets(hip):
    """seen / ban sets ahead of the selection: a banned id appears at no rank, a penalised one moves as the processed logits say."""
    dt, K, B, N, k = DT_F32, 384, 17, 1000, 8
    r = np.random.default_rng(5)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    words = (N + 31) // 32
    seen, ban = np.zeros((B, words), np.uint32), np.zeros((B, words), np.uint32)
    top = np.argsort(-ref, 1)
    proc, pb = ref.copy(), bound.copy()
    for row in range(B):
        t0, t1 = int(top[row, 0]), int(top[row, 1])
        ban[row, t0 >> 5] |= np.uint32(1 << (t0 & 31))
        seen[row, t1 >> 5] |= np.uint32(1 << (t1 & 31))
        proc[row, t0] = -np.inf
        f = 4.0 if ref[row, t1] < 0 else 0.25  # (a power of two: the penalty itself is exact)
        proc[row, t1], pb[row, t1] = ref[row, t1] * f, bound[row, t1] * f
    out = _topk(x, g, b, emb, dt, k, seen=seen, ban=ban, penalty=4.0)
    for row in range(B):
        assert int(top[row, 0]) not in out[3][row]
    mask = None
    fin = np.where(np.isfinite(proc), proc, -1e30)  # the banned id as a hopeless finite candidate of the reference
    keep = np.isfinite(proc)
    for row in range(B):  # (the reference set: everything but the banned id)
        assert np.isfinite(out[0][row][keep[row]]).all() and out[0][row][~keep[row]][0] == -np.inf
    logits = np.where(np.isfinite(out[0]), out[0], np.float32(-1e30))
    _check("repetition sets", (logits,) + out[1:], fin, pb, mask, None, _tb(N), N, k)


def test_refusals(hip):
    from whisper_mojo_amd import whisper_tensor as wt
    r = np.random.default_rng(0)
    x, g, b, emb = _decoder_like(r, 2, 128, 100, DT_F32)
    for bad in (0, 9, True, 2.5):
        with pytest.raises(ValueError):
            wt.logits_topk(x, g, b, emb, bad)
