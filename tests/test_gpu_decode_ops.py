"""Op-level tests (-m gpu) of two of the four decoder kernel families that run on every decode step, against float64 on the
operands exactly as the kernels receive them (the other two — the per-layer skinny linears and the cached attention — are in
tests/test_gpu_decode_layer.py):

  * the final LayerNorm + tied-embedding logits with the fused argmax (wm_op_logits: launch_dec_logits + argmax_step), over every
    kernel variant the release dispatch reaches, ties and masks at the reduction boundaries, and the timestamp decision;
  * the absorbed cross-attention (wm_op_xattn: absorb, X sweep, merge) for 1..8 heads, ragged and empty key chunks.

The float64 references live in this file; tests/test_decode_ops_ref.py checks the absorbed attention reference on the CPU."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # fp32 unit roundoff
DT_F32, DT_BF16, DT_F16 = 0, 1, 2


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()  # raises if the HIP library is missing: no fallback
    import whisper_mojo_amd as pkg
    return pkg


def _round(a, dt):
    """fp32 -> the upload dtype's value (round to nearest even), as float64."""
    import torch
    a = np.ascontiguousarray(a, np.float32)
    if dt == DT_BF16:
        return torch.from_numpy(a).bfloat16().double().numpy()
    if dt == DT_F16:
        return a.astype(np.float16).astype(np.float64)
    return a.astype(np.float64)


# ---- logits: reference and error bound ---------------------------------------------------------------------------------------

def _ln64(x, g, b):
    """The oracle's one-pass LayerNorm (E[x²] - E[x]², eps 1e-5) in float64."""
    x = x.astype(np.float64)
    mean = x.mean(1, keepdims=True)
    var = (x * x).mean(1, keepdims=True) - mean * mean
    return (x - mean) / np.sqrt(var + 1e-5) * g.astype(np.float64) + b.astype(np.float64)


def _ln_stats(x, n=None):
    """The row statistics of _ln_err and their fp32 error: (x float64, mean, var, Δmean, Δvar), each [rows, 1], for statistics summed
    n deep (default: the logits kernels' K/8 + 3).  tests/test_fused_ln_ref.py builds its interval bound from the same terms."""
    x = x.astype(np.float64)
    K = x.shape[1]
    gam = (K // 8 + 3 if n is None else n) * U
    mu = x.mean(1, keepdims=True)
    m2 = (x * x).mean(1, keepdims=True)
    var = m2 - mu * mu
    d_mu = gam * np.abs(x).mean(1, keepdims=True) + U * np.abs(mu)
    d_m2 = (gam + 2 * U) * m2
    d_var = d_m2 + 2 * np.abs(mu) * d_mu + U * mu * mu + U * (np.abs(var) + 1e-5)
    return x, mu, var, d_mu, d_var


def _ln_err(x, g, b, n=None):
    """First-order bound on |fp32 LayerNorm - float64 LayerNorm| per element, for the logits kernels' fp32 LayerNorm: each of 8
    threads per row sums K/8 elements (and their squares) in sequence, three butterfly adds join them (γ_n, n = K/8 + 3); then
    mean = s/K, var = q/K - mean², rstd = 1/sqrtf(var + eps), y = ((x - mean)·rstd)·g + b, every operation rounded once.
    n: the summation depth of another kernel's statistics (default: the logits kernels')."""
    x, mu, var, d_mu, d_var = _ln_stats(x, n)
    r = 1.0 / np.sqrt(var + 1e-5)
    rho = 0.5 * d_var / (var + 1e-5) + 2 * U
    y = (x - mu) * r * g + b
    return np.abs(g) * r * (np.abs(x - mu) * (rho + 3 * U) + d_mu) + U * np.abs(y)


def _ulp_tw(v, dt):
    """Spacing of the 16-bit grid at |v| (the larger of the two sides at a power of two) and just below it."""
    p = 8 if dt == DT_BF16 else 11
    _, e = np.frexp(np.abs(v))
    ulp = np.ldexp(1.0, e - p)
    if dt == DT_F16:
        ulp = np.maximum(ulp, 2.0 ** -24)
    return ulp, ulp / 2


def _logits_ref(x, g, b, emb, dt):
    """-> (ref [B, N] float64, bound [B, N]).

    ref = a·ŵᵀ over a = LN64(x) and ŵ = emb rounded to dt; for 16-bit weights a is rounded to dt too, as the kernel rounds its own
    LayerNorm output into the LDS operand image.  bound per element, from the arithmetic:
      * accumulation: the kernel sums n exact products into an fp32 accumulator (MFMA chains; a bf16 x bf16 / f16 x f16 product and
        the 3×bf16 split's products are exact in fp32), so in any order the error is <= (n - 1)·u·Σ|terms| (the order-independent
        γ_n bound): n = K for the 16-bit and the exact-fp32 kernel, 6K for the split kernels (six products per k);
      * fp32 weights, split kernels: the three dropped products wm·xl + wl·xm + wl·xl <= 2^-21 |w·x| (tests/test_split3.py);
      * fp32 weights: the kernel multiplies its fp32 LayerNorm output, which differs from a by <= _ln_err: Σ_k err_k |ŵ_k|;
      * 16-bit weights: the fp32 LayerNorm only shows where float64 a_k lies within _ln_err of a rounding midpoint of dt — there the
        two may round apart by one ulp: those elements add ulp_dt(a_k)·|ŵ_k| to their column's bound (no blanket 16-bit tolerance).
    """
    a = _ln64(x, g, b)
    e = _ln_err(x, g, b)
    K = x.shape[1]
    w = _round(emb, dt)
    if dt == DT_F32:
        split = K in (128, 384)
        c = (6 * K if split else K) * U + (2.0 ** -21 if split else 0.0)
        v = c * np.abs(a) * (1 + 3 * 2.0 ** -7) + e  # Σ|terms| of the split: (|wh| + |wm| + |wl|)(...) <= (1 + 2^-7 + ...)² |w||x|
        ref = a @ w.T
    else:
        at = _round(a, dt)
        ulp, ulp_below = _ulp_tw(at, dt)
        near = (0.5 * np.minimum(ulp, ulp_below) - np.abs(a - at)) <= e
        v = K * U * np.abs(at) + near * ulp
        ref = at @ w.T
    bound = np.abs(v) @ np.abs(w).T
    return ref, bound


def _lowest_argmax(v):
    """lowest index of the maximum (all -inf -> 0), per row"""
    out = np.zeros(len(v), np.int64)
    for i, row in enumerate(v):
        m = row.max()
        out[i] = int(np.flatnonzero(row == m)[0]) if m > -np.inf else 0
    return out


def _decoder_like(r, B, K, N, dt, scale=0.04):
    """Rows like the decoder's last hidden state: a DC offset of a few σ, per-row scale, a few large-magnitude feature columns;
    γ/β away from 1/0; embedding rows of logit scale."""
    sig = r.uniform(0.5, 3.0, (B, 1))
    x = r.standard_normal((B, K)) * sig + r.uniform(-4, 4, (B, 1)) * sig
    big = r.choice(K, 3, replace=False)
    x[:, big] += r.choice([-1, 1], (B, 3)) * 12 * sig
    g = 1 + 0.3 * r.standard_normal(K)
    b = 0.2 * r.standard_normal(K)
    emb = r.standard_normal((N, K)) * scale
    return x.astype(np.float32), g.astype(np.float32), b.astype(np.float32), emb.astype(np.float32)


def _ct(N):
    tiles = (N + 15) // 16
    return max(1, min(16, (tiles + 255) // 256))


# (dtype, K, B, N): every logits variant launch_dec_logits reaches in a release build (a comment names each).  Full vocabulary with
# 150 rows only for three of them: the float64 reference of one such case is ~8e9 multiply-adds.
LOGITS_CASES = [
    (DT_F32, 128, 1, 51865),    # dec_logits_split_kernel<1,1>
    (DT_F32, 128, 17, 4097),    # dec_logits_split_kernel<1,4>
    (DT_F32, 128, 150, 51865),  # dec_logits_split128_kernel<1> (two row blocks, the second ragged: 128 + 22)
    (DT_F32, 384, 16, 51864),   # dec_logits_split_kernel<3,1>
    (DT_F32, 384, 64, 37),      # dec_logits_split_kernel<3,4>
    (DT_F32, 384, 150, 51865),  # dec_logits_split128_kernel<3>
    (DT_F32, 384, 65, 1000),    # dec_logits_split128_kernel<3> (one ragged row block)
    (DT_F32, 512, 16, 4097),    # dec_logits_kernel<float,4,1>
    (DT_F32, 512, 65, 51865),   # dec_logits_kernel<float,4,4>
    (DT_BF16, 128, 16, 37),     # dec_logits_kernel<bf16,1,1>
    (DT_BF16, 128, 64, 51865),  # dec_logits_kernel<bf16,1,4>
    (DT_BF16, 384, 1, 51865),   # dec_logits_kernel<bf16,3,1>
    (DT_BF16, 384, 150, 4097),  # dec_logits_kernel<bf16,3,4> (three row blocks)
    (DT_BF16, 512, 16, 1000),   # dec_logits_kernel<bf16,4,1>
    (DT_BF16, 512, 150, 51865), # dec_logits_kernel<bf16,4,4>
    (DT_F16, 128, 1, 4097),     # dec_logits_kernel<f16,1,1>
    (DT_F16, 128, 17, 1000),    # dec_logits_kernel<f16,1,4>
    (DT_F16, 384, 16, 51865),   # dec_logits_kernel<f16,3,1>
    (DT_F16, 384, 65, 37),      # dec_logits_kernel<f16,3,4>
    (DT_F16, 512, 16, 51864),   # dec_logits_kernel<f16,4,1>
    (DT_F16, 512, 64, 4097),    # dec_logits_kernel<f16,4,4>
]


def _call_logits(x, g, b, emb, dt, **kw):
    from whisper_mojo_amd import whisper_tensor as wt
    return wt.logits_argmax(x, g, b, emb, dtype=dt, **kw)


@pytest.mark.parametrize("dt,K,B,N", LOGITS_CASES)
def test_logits_vs_float64(hip, dt, K, B, N):
    """Every element within the arithmetic's bound of float64; the fused argmax exact on the kernel's own logits and within one
    bound of the float64 maximum; rows independent of the other rows of the call (bitwise)."""
    r = np.random.default_rng(1000 * K + 7 * B + N + dt)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    logits, ids = _call_logits(x, g, b, emb, dt)
    assert np.isfinite(logits).all()
    ref, bound = _logits_ref(x, g, b, emb, dt)
    ratio = np.abs(logits - ref) / bound
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"dt {dt} K {K} B {B} N {N}: worst err/bound {ratio.max():.3g} at {worst}, max |err| {np.abs(logits - ref).max():.3g}")
    assert ratio.max() <= 1.0, (worst, logits[worst], ref[worst], bound[worst])
    np.testing.assert_array_equal(ids, _lowest_argmax(logits))
    top = ref.max(1)
    assert (ref[np.arange(B), ids] >= top - bound[np.arange(B), ids]).all()
    if B > 1:  # a row's logits and id do not depend on the other rows of its call (same variant: same row count)
        perm = r.permutation(B)
        lp, ip = _call_logits(x[perm], g, b, emb, dt)
        np.testing.assert_array_equal(lp, logits[perm])
        np.testing.assert_array_equal(ip, ids[perm])


def _tie_columns(N):
    """(lower, higher) id pairs at the fused argmax's reduction boundaries, for a vocabulary of N ids."""
    ct = _ct(N)
    P = 16 * ct  # ids per part (one workgroup)
    parts = (N + P - 1) // P
    pairs = [(16 * 3 + 4 * 2 + 1, 16 * 3 + 4 * 2 + 3),  # the 4 columns one lane holds
             (16 * 5 + 2, 16 * 5 + 13)]                 # one 16-column tile, two lanes
    if ct > 8:
        pairs.append((P * 2 + 16 * 1 + 5, P * 2 + 16 * 9 + 5))  # the two tiles of wave 1
    if ct > 4:
        pairs.append((P * 3 + 16 * 1 + 3, P * 3 + 16 * 4 + 3))  # two waves
    else:
        pairs.append((P * 1 + 1, P * 1 + 16 + 1))
    for k in (1, parts // 2, parts - 1):  # a part boundary: k·P - 1 and k·P
        if 0 < k * P < N:
            pairs.append((k * P - 1, k * P))
    pairs.append((P + 7, (parts - 1) * P + 2 if parts > 2 else N - 2))  # distant workgroups
    last0 = (N - 1) // 16 * 16
    pairs.append((last0, N - 1) if last0 < N - 1 else (N - 17, N - 1))  # the last (partial) tile, the maximum at id N - 1
    return sorted({p for p in pairs if 0 <= p[0] < p[1] < N})


@pytest.mark.parametrize("dt,K,B,N", [
    (DT_F32, 384, 16, 51865),   # split<3,1>
    (DT_F32, 128, 150, 51865),  # split128<1>
    (DT_F32, 512, 40, 4097),    # dec_logits<float,4,4>
    (DT_BF16, 384, 40, 51865),  # dec_logits<bf16,3,4>
    (DT_F16, 128, 16, 37),      # dec_logits<f16,1,1>
    (DT_BF16, 512, 16, 1000),   # dec_logits<bf16,4,1>
])
def test_argmax_ties_masks_near_ties(hip, dt, K, B, N):
    """Duplicate embedding rows make exact ties at every reduction boundary of the fused argmax (lane, tile, the two tiles of a
    wave, waves, workgroup parts, the last partial tile): the lowest id must win; a -inf mask on the lower one moves the pick to the
    higher one.  Built near-ties a few bounds apart: the pick is within one bound of the float64 maximum."""
    r = np.random.default_rng(31 * K + N + dt)
    x, g, b, emb = _decoder_like(r, B, K, N, dt)
    a = _ln64(x, g, b)
    pairs = _tie_columns(N)
    rows, used = {}, set()
    for i, (lo, hi) in enumerate(pairs):
        row = i % B
        if row in rows or lo in used or hi in used:  # one pair per row, every id in one pair only
            continue
        used |= {lo, hi}
        d = a[row] / np.linalg.norm(a[row])
        emb[lo] = emb[hi] = (d * 0.04 * np.sqrt(K) * 6).astype(np.float32)  # ~6x the typical largest random logit
        rows[row] = (lo, hi)
    near = {}
    if N > 64:  # rows with a near-tie: the HIGHER id larger by about m bounds (one coordinate moved; 16-bit grids are coarser)
        free = [row for row in range(B) if row not in rows][:3]
        spare = [j for j in range(9, N, 40) if j not in used and N - 1 - j not in used and j < N - 1 - j]
        for m, row, lo in zip((0.5, 2.0, 6.0), free, spare):
            hi = N - 1 - lo
            d = a[row] / np.linalg.norm(a[row])
            base = (d * 0.04 * np.sqrt(K) * 6).astype(np.float32)
            emb[lo] = emb[hi] = base
            ref0, bd = _logits_ref(x[row:row + 1], g, b, emb[[lo]], dt)
            k = int(np.argmax(np.abs(a[row])))
            emb[hi, k] += np.float32(m * bd[0, 0] / a[row, k])
            near[row] = (lo, hi)
    logits, ids = _call_logits(x, g, b, emb, dt)
    np.testing.assert_array_equal(ids, _lowest_argmax(logits))
    for row, (lo, hi) in rows.items():
        assert logits[row, lo] == logits[row, hi], (row, lo, hi)  # the tie is real: identical operands, identical logits
        assert logits[row].max() == logits[row, lo] and ids[row] == lo, (row, lo, hi, ids[row])
    ref, bound = _logits_ref(x, g, b, emb, dt)
    assert (np.abs(logits - ref) <= bound).all()
    sel = np.arange(B)
    assert (ref[sel, ids] >= ref.max(1) - bound[sel, ids]).all()
    for row, (lo, hi) in near.items():
        print(f"near-tie row {row}: ref gap {(ref[row, hi] - ref[row, lo]) / bound[row, hi]:.2f} bounds, pick {ids[row]} ({lo}, {hi})")
    # the mask: -inf on the lower id of every tied pair moves each such row's pick to the higher id; logits are unchanged
    mask = np.zeros(N, np.float32)
    for lo, _ in rows.values():
        mask[lo] = -np.inf
    lm, im = _call_logits(x, g, b, emb, dt, mask=mask)
    np.testing.assert_array_equal(lm, logits)
    np.testing.assert_array_equal(im, _lowest_argmax(logits + mask))
    for row, (lo, hi) in rows.items():
        assert im[row] == hi, (row, lo, hi, im[row])
    # every candidate masked: id 0
    _, iall = _call_logits(x[:2], g, b, emb, dt, mask=np.full(N, -np.inf, np.float32))
    assert (iall == 0).all()


def test_logits_128_row_kernel_equals_64_row_kernel_bitwise(hip):
    """fp32 weights, K in {128, 384}: rows of a B > 64 call (dec_logits_split128_kernel) equal the same rows computed with B = 40
    (dec_logits_split_kernel<KD,4>) bit for bit, as the 128-row kernel's comment claims (same LayerNorm order, same k order)."""
    for K in (128, 384):
        r = np.random.default_rng(K)
        x, g, b, emb = _decoder_like(r, 150, K, 4097, DT_F32)
        big, ib = _call_logits(x, g, b, emb, DT_F32)
        for s in (0, 40, 110):
            small, is_ = _call_logits(x[s:s + 40], g, b, emb, DT_F32)
            np.testing.assert_array_equal(big[s:s + 40], small)
            np.testing.assert_array_equal(ib[s:s + 40], is_)


# ---- the timestamp decision ---------------------------------------------------------------------------------------------------

def _ts_decision(logits, mask, ranges):
    """float64 form of argmax_step's rule on the kernel's own logits -> (pick, margin = logsumexp(ts) - best text, bound).
    bound: the fp32 error of the kernel's logsumexp.  A term exp(v - max) is rounded in its argument (u·|v - max|) and value,
    then passes at most 8 lane adds, 2 shuffle and 7 wave merges and one merge per timestamp part, each an add and a rescale
    (expf + product): relative (4·(17 + parts) + 2)·u + u·|v - max| per term, weighted by the term; then logf, the add to the
    max and the compare: u·(|log s| + 2|lse|)."""
    B, N = logits.shape
    v = logits.astype(np.float64) + (0 if mask is None else mask)
    out = []
    for b in range(B):
        tlo, thi, qlo, qhi = ranges[b]
        text = v[b, max(tlo, 0):max(min(thi, N), 0)]
        ts = v[b, max(qlo, 0):max(min(qhi, N), 0)]
        q0 = max(qlo, 0)
        fin = np.flatnonzero(ts > -np.inf)
        best = text.max() if text.size and text.max() > -np.inf else -np.inf
        tid = (max(tlo, 0) + int(np.argmax(text))) if best > -np.inf else None
        if fin.size:
            m = ts.max()
            qid = q0 + int(np.argmax(ts))
            ts = ts[fin]
            wts = np.exp(ts - m)
            s = wts.sum()
            lse = m + np.log(s)
            parts = (min(qhi, N) - 1) // (16 * _ct(N)) - max(qlo, 0) // (16 * _ct(N)) + 1
            rel = ((4 * (17 + parts) + 2) * U * wts + U * np.abs(ts - m) * wts).sum() / s
            bnd = rel + U * (abs(np.log(s)) + 2 * abs(lse))
        else:
            lse, qid, bnd = -np.inf, None, 0.0
        if qid is not None and (tid is None or lse > best):
            pick = qid
        else:
            pick = tid if tid is not None else 0
        margin = lse - best if (qid is not None and tid is not None) else np.inf
        out.append((pick, margin, bnd))
    return out


def _steer(K, N, targets, r, dt):
    """x = a ±1 pattern (mean 0, variance 1; γ = 1, β = 0: LN(x) = x / sqrt(1 + 1e-5)), embedding rows c·pattern / K give logit ~c;
    random rows (logits ~ N(0, 0.5²)) fill the rest.  targets: per row {id: logit}."""
    B = len(targets)
    pat = np.where(np.arange(K) % 2 == 0, 1.0, -1.0)
    perm = np.stack([r.permutation(K) for _ in range(B)])
    x = pat[perm].astype(np.float32)
    emb = (r.standard_normal((N, K)) * 0.5 / np.sqrt(K)).astype(np.float32)
    rr = np.sqrt(1 + 1e-5)
    for b, tg in enumerate(targets):
        for j, c in tg.items():
            emb[j] = (x[b] * (c * rr / K)).astype(np.float32)
    return x, np.ones(K, np.float32), np.zeros(K, np.float32), emb


def _ts_rows(N, tb, P):
    """(targets, ranges) of the decision cases for a vocabulary N with timestamp_begin tb and P ids per part.  Every steered id
    belongs to one row (an embedding row steers one logit of one row); ids tb, N - 1 and 50 are the out-of-range ones, 7 and
    N - 2 are masked."""
    T = 20.0
    part_end = min(N, (tb // P + 1) * P)
    A = iter(range(tb + 1, part_end))                  # the part holding tb (after tb itself)
    Bp = iter(range(part_end + P + 5, N - 2, 7))      # later parts
    text = iter(range(200, tb, 3))
    take = lambda it: next(it, None) if it is not A else (next(A, None) or next(Bp))
    full = (0, tb, tb, N)
    cases = []
    for k, dlt in enumerate((1e-1, -1e-1, 1e-2, -1e-2, 1e-3, -1e-3, 1e-4, -1e-4)):
        n = 1 + k % 3
        ids = [take(A) for _ in range(n)] if k % 2 == 0 else [take(A)] + [take(Bp) for _ in range(n - 1)]  # tb's part / spread
        tg = {take(text): T}
        tg.update({j: T + dlt - np.log(n) for j in ids})
        cases.append((tg, full))
    cases.append(({take(A): T + 1.0, take(text): T + 3.0}, (0, 0, tb, N)))        # empty text range: the best timestamp
    cases.append(({take(text): T, take(Bp): T + 5.0}, (0, tb, tb, tb)))           # empty timestamp range: the best text id
    cases.append(({take(text): T, tb: T + 12.0, take(Bp): T - 0.5}, (0, tb, tb + 1, N)))  # ts_lo > tb: tb is out
    cases.append(({take(text): T, N - 1: T + 12.0, take(Bp): T + 0.2}, (0, tb, tb, N - 1)))  # ts_hi < N: N - 1 is out
    cases.append(({50: T + 12.0, take(text): T, take(Bp): T - 0.3}, (100, tb, tb, N)))     # text_lo > 0: id 50 is out
    t1, t2 = take(text), take(text)
    cases.append(({t1: T, t2: T, take(Bp): T - 40.0}, full))                       # text tie, timestamps far below
    return [c[0] for c in cases], np.array([c[1] for c in cases], np.int32)


@pytest.mark.parametrize("dt,K,N,tb_kind,pad", [
    (DT_F32, 384, 51865, "inside", 0),   # split<3,1>; tb = 50364 inside part 242 (208 ids per part)
    (DT_F32, 384, 51865, "on", 0),       # tb on a part boundary
    (DT_F32, 384, 51865, "before", 0),   # tb one before a boundary
    (DT_F32, 384, 51865, "after", 0),    # tb one after a boundary
    (DT_F32, 128, 51865, "inside", 60),  # split128<1> (padding rows to B > 64)
    (DT_F32, 512, 4097, "after", 20),    # dec_logits<float,4,4>, 2 tiles per part
    (DT_BF16, 512, 51865, "inside", 0),  # dec_logits<bf16,4,1> (coarse steering: only margins above the bound count)
])
def test_timestamp_decision(hip, dt, K, N, tb_kind, pad):
    """HF rule 5 as argmax_step applies it: the best admissible text id unless logsumexp of the admissible timestamps exceeds it.
    The pick equals the float64 decision on the kernel's own logits wherever the margin exceeds the fp32 bound; both outcomes
    occur; mask and ranges leave the logits bitwise unchanged."""
    P = 16 * _ct(N)
    base = N - 1501 if N > 3000 else N - 1000
    tb = {"inside": base, "on": base // P * P, "before": base // P * P - 1, "after": base // P * P + 1}[tb_kind]
    if tb_kind == "inside":
        assert tb % P != 0
    r = np.random.default_rng(K + N + pad + len(tb_kind))
    targets, ranges = _ts_rows(N, tb, P)
    targets += [{} for _ in range(pad)]
    ranges = np.concatenate([ranges, np.tile([[0, tb, tb, N]], (pad, 1)).astype(np.int32)])
    x, g, b, emb = _steer(K, N, targets, r, dt)
    mask = np.zeros(N, np.float32)
    mask[[7, N - 2]] = -np.inf
    logits, ids = _call_logits(x, g, b, emb, dt, mask=mask, ranges=ranges, timestamp_begin=tb)
    plain, _ = _call_logits(x, g, b, emb, dt)
    np.testing.assert_array_equal(logits, plain)
    dec = _ts_decision(logits, mask, ranges)
    outcomes = set()
    checked = 0
    for row, (pick, margin, bnd) in enumerate(dec):
        if abs(margin) > bnd:
            assert ids[row] == pick, (row, ids[row], pick, margin, bnd, ranges[row])
            checked += 1
            if np.isfinite(margin):
                outcomes.add(bool(margin > 0))
        lo, hi = (ranges[row][2], ranges[row][3]) if ids[row] >= tb else (ranges[row][0], ranges[row][1])
        assert lo <= ids[row] < hi or (ids[row] == 0 and lo == hi), (row, ids[row], ranges[row])
    small = [abs(m) for (_, m, bd) in dec[:8] if np.isfinite(m) and abs(m) > bd]
    print(f"tb {tb} (part {tb // P}, {tb % P} into it): {checked} decisions checked, smallest margin {min(small):.2e}, "
          f"bounds {min(d[2] for d in dec):.1e}..{max(d[2] for d in dec):.1e}")
    assert outcomes == {True, False}
    if dt == DT_F32:
        assert min(small) < 2e-4  # the ±1e-4 cases are realised and decided


def test_logits_refuses_bad_arguments(hip):
    from whisper_mojo_amd import _lib, whisper_tensor as wt
    x = np.zeros((2, 256), np.float32)
    with pytest.raises(_lib.WhisperMiError):  # K = 256: no logits kernel
        wt.logits_argmax(x, np.ones(256), np.zeros(256), np.zeros((100, 256)))
    with pytest.raises(_lib.WhisperMiError):  # ranges without a timestamp_begin
        wt.logits_argmax(x[:, :128], np.ones(128), np.zeros(128), np.zeros((100, 128)), ranges=np.zeros((2, 4)))


# ---- absorbed cross-attention -------------------------------------------------------------------------------------------------

def xattn_ref(q, Wk, Wv, bv, X, n_heads, q_B=0):
    """float64, absorbed form, over the operands as the kernels receive them (Wk, Wv, X already rounded to bf16 by the caller):
    q'_h = 0.125·q_h·Wk_h, s = q'_h·X_j, o_h = (Σ_j p_j X_j / Σ_j p_j)·Wv_hᵀ + bv_h, X = X[utt(r)]."""
    rows, d = q.shape
    out = np.zeros((rows, d))
    for r in range(rows):
        Xu = X[r % q_B if q_B > 0 else r].astype(np.float64)
        for h in range(n_heads):
            sl = slice(64 * h, 64 * h + 64)
            qp = 0.125 * q[r, sl].astype(np.float64) @ Wk[sl].astype(np.float64)
            s = Xu @ qp
            p = np.exp(s - s.max())
            ybar = (p @ Xu) / p.sum()
            out[r, sl] = ybar @ Wv[sl].astype(np.float64).T + bv[sl]
    return out


def xattn_ref_direct(q, Wk, Wv, bv, X, n_heads, q_B=0):
    """float64, the cached form: K = X·Wkᵀ, V = X·Wvᵀ + bv, softmax(0.125·q_h·K_hᵀ)·V_h."""
    rows, d = q.shape
    out = np.zeros((rows, d))
    for r in range(rows):
        Xu = X[r % q_B if q_B > 0 else r].astype(np.float64)
        Kc, Vc = Xu @ Wk.astype(np.float64).T, Xu @ Wv.astype(np.float64).T + bv
        for h in range(n_heads):
            sl = slice(64 * h, 64 * h + 64)
            s = 0.125 * (Kc[:, sl] @ q[r, sl].astype(np.float64))
            p = np.exp(s - s.max())
            out[r, sl] = (p / p.sum()) @ Vc[:, sl]
    return out


def _xattn_inputs(r, H, n_keys, rows, q_B, nsplit, kind):
    """q, Wk, Wv, bv, X (X, Wk, Wv already bf16 values) for a score shape: random (scores ~N(0, 2²)), dominant (one key +12 above,
    in a chunk and wave other than the first), spread (keys outside one chunk ~80 below: those chunks underflow), equal (q = 0)."""
    d = 64 * H
    n_utt = q_B if q_B > 0 else rows
    q = r.standard_normal((rows, d)).astype(np.float32)
    Wk = _round(r.standard_normal((d, d)) * 2 / np.sqrt(d), DT_BF16)
    Wv = _round(r.standard_normal((d, d)) / np.sqrt(d), DT_BF16)
    bv = (0.1 * r.standard_normal(d)).astype(np.float32)
    X = r.standard_normal((n_utt, n_keys, d), dtype=np.float32)
    if kind == "equal":
        q[:] = 0
    chunk = -(-n_keys // nsplit)
    if kind in ("dominant", "spread"):
        for u in range(n_utt):
            rr = u  # the query row that sees this utterance first
            shift = np.zeros(d)
            for h in range(H):
                sl = slice(64 * h, 64 * h + 64)
                qp = 0.125 * q[rr, sl].astype(np.float64) @ Wk[sl]
                shift += qp / (qp @ qp)
            c = 1 if nsplit > 1 and n_keys > chunk else 0
            j0, j1 = c * chunk, min(n_keys, (c + 1) * chunk)
            if kind == "dominant":
                j = min(j1 - 1, j0 + 16 * 2 + 5)
                X[u, j] += 12 * shift
            else:
                out = np.ones(n_keys, bool)
                out[j0:j1] = False
                X[u, out] -= 80 * shift
    import torch
    Xb = torch.from_numpy(X).bfloat16().float().numpy()  # fp32 holding bf16 values (host memory: 67 x 1500 x 384 rows)
    return q, Wk.astype(np.float32), Wv.astype(np.float32), bv, Xb


# (H, n_keys, nsplit, rows, q_B, kind, out_dtype)
XATTN_CASES = [
    (1, 1500, 47, 5, 0, "random", DT_F32),
    (1, 1, 64, 3, 0, "random", DT_BF16),      # one key, 63 empty chunks
    (2, 100, 1, 3, 0, "dominant", DT_F32),    # micro's geometry
    (2, 17, 2, 67, 0, "random", DT_F32),      # rows % 4 != 0 in absorb / merge
    (3, 65, 64, 67, 0, "random", DT_F32),     # chunks of 2 keys, 31 empty chunks
    (3, 1500, 3, 6, 3, "spread", DT_BF16),    # prefill rows (P = 2, q_B = 3)
    (4, 15, 12, 8, 4, "random", DT_F32),      # prefill; chunks of 2 keys, the last ones empty
    (4, 1500, 12, 64, 0, "spread", DT_F32),   # chunks of 125 keys: tiles cross chunk ends
    (5, 17, 3, 5, 0, "equal", DT_F32),
    (5, 1500, 64, 5, 0, "dominant", DT_BF16), # chunks of 24 keys: waves 2, 3 without a tile
    (6, 1500, 32, 67, 0, "random", DT_F32),   # tiny's geometry
    (6, 16, 2, 3, 0, "dominant", DT_BF16),
    (7, 100, 12, 5, 0, "spread", DT_F32),     # chunks of 9 keys
    (7, 1500, 2, 3, 0, "equal", DT_BF16),
    (8, 1500, 47, 5, 0, "random", DT_F32),    # base's heads
    (8, 65, 3, 6, 2, "dominant", DT_F32),     # prefill P = 3
    (8, 300, 64, 67, 0, "spread", DT_BF16),
]


def _xattn_call(q, Wk, Wv, bv, X, H, nsplit, q_B=0, out_dtype=DT_F32):
    from whisper_mojo_amd import whisper_tensor as wt
    out = np.zeros(q.shape, np.float32)
    wt.xattn(out, q, Wk, Wv, bv, X, H, nsplit, q_B=q_B, out_dtype=out_dtype)
    return out


@pytest.mark.parametrize("H,n_keys,nsplit,rows,q_B,kind,odt", XATTN_CASES)
def test_xattn_vs_float64(hip, H, n_keys, nsplit, rows, q_B, kind, odt):
    """The absorbed cross-attention against float64 on the bf16 operands.  Tolerance 5e-6·max(1, |ref|), a quarter of
    test_op_attention_cached's 2e-5: every error source is a sum of independently rounded fp32 terms — q' (64 fmaf), the score
    (3·d/32 MFMA blocks of exact products), the chunk's P·X (three bf16 MFMA terms per 16-key tile, <= 94 tiles), the merges and
    the Wv apply (d fmaf) — which grow as √n·u: ~1e-6 at d = 512 with 1500 keys; the order-independent worst case n·u (3e-5 for
    the d = 512 Wv apply alone) is not approached by random-signed roundings.  bf16 output: the reference is rounded too, and
    one bf16 ulp is added."""
    r = np.random.default_rng(H * 100003 + n_keys * 7 + nsplit * 3 + rows + q_B)
    q, Wk, Wv, bv, X = _xattn_inputs(r, H, n_keys, rows, q_B, nsplit, kind)
    out = _xattn_call(q, Wk, Wv, bv, X, H, nsplit, q_B, odt)
    ref = xattn_ref(q, Wk, Wv, bv, X, H, q_B)
    tol = 5e-6 * max(1.0, np.abs(ref).max())
    if odt == DT_BF16:
        assert np.array_equal(_round(out, DT_BF16), out)
        ref = _round(ref, DT_BF16)
        tol = tol + _ulp_tw(ref, DT_BF16)[0]
    err = np.abs(out - ref)
    print(f"H {H} keys {n_keys} nsplit {nsplit} rows {rows} q_B {q_B} {kind}: max err {err.max():.3g}, worst err/tol "
          f"{(err / tol).max():.3g}")
    assert (err <= tol).all(), (np.unravel_index(np.argmax(err / tol), err.shape), err.max())


@pytest.mark.parametrize("H,n_keys,nsplit", [(6, 1500, 12), (3, 65, 64), (8, 100, 3)])
def test_xattn_row_invariance(hip, H, n_keys, nsplit):
    """A row's output does not depend on the row count or the other rows (bitwise); a prefill row equals the decode row with the
    same query and utterance (bitwise); another nsplit changes the output only within tolerance."""
    r = np.random.default_rng(H + n_keys + nsplit)
    q, Wk, Wv, bv, X = _xattn_inputs(r, H, n_keys, 5, 0, nsplit, "random")
    full = _xattn_call(q, Wk, Wv, bv, X, H, nsplit)
    for i in (0, 3, 4):
        one = _xattn_call(q[i:i + 1], Wk, Wv, bv, X[i:i + 1], H, nsplit)
        np.testing.assert_array_equal(one[0], full[i])
    sub = _xattn_call(q[[4, 1, 2]], Wk, Wv, bv, X[[4, 1, 2]], H, nsplit)
    np.testing.assert_array_equal(sub, full[[4, 1, 2]])
    # prefill: 3 positions x 2 utterances, row p·2 + b reads utterance b
    qp = r.standard_normal((6, 64 * H)).astype(np.float32)
    pre = _xattn_call(qp, Wk, Wv, bv, X[:2], H, nsplit, q_B=2)
    for row in range(6):
        dec = _xattn_call(qp[row:row + 1], Wk, Wv, bv, X[row % 2:row % 2 + 1], H, nsplit)
        np.testing.assert_array_equal(dec[0], pre[row])
    ref = xattn_ref(q, Wk, Wv, bv, X, H)
    for ns in (1, 2, 47):
        other = _xattn_call(q, Wk, Wv, bv, X, H, ns)
        assert np.abs(other - full).max() <= 1e-5 * max(1.0, np.abs(ref).max())  # two results each within 5e-6 of float64


def test_xattn_refuses_bad_arguments(hip):
    from whisper_mojo_amd import _lib, whisper_tensor as wt
    q, W, bv, X = np.zeros((1, 576), np.float32), np.zeros((576, 576), np.float32), np.zeros(576, np.float32), np.zeros((1, 4, 576), np.float32)
    with pytest.raises(_lib.WhisperMiError):  # 9 heads
        wt.xattn(np.zeros_like(q), q, W, W, bv, X, 9, 1)
    q, W, bv, X = q[:, :64], W[:64, :64], bv[:64], X[:, :, :64]
    with pytest.raises(_lib.WhisperMiError):  # nsplit 65
        wt.xattn(np.zeros_like(q), q, W, W, bv, X, 1, 65)
