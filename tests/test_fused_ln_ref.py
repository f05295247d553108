"""Cases, float64 reference, bounds and float32 restatements for the LayerNorm that nine kernels carry inside them, and the
CPU proofs about them; tests/test_gpu_fused_ln_op.py asks the same of the kernels.

Every site computes one-pass statistics in fp32 — mean = Σx / K, var = Σx² / K − mean², rstd = 1 / sqrtf(max(var, 0) + 1e-5) — and
y = (x − mean)·rstd·γ + β.  On a row whose mean dwarfs its spread the subtraction cancels and var can come out below −eps; without the
clamp that is the square root of a negative number.

Rows: mean / σ in DC_RATIOS (σ per row), constant rows at ±c and ±(c one ulp up / down) for c in CONSTS, one row constant but for one
element.  γ / β away from 1 / 0 as _decoder_like draws them; one case with γ = 1, β = 0.

Reference: _ln64 (float64, one-pass, eps 1e-5).

Bound, per element: the terms of _ln_err (tests/test_gpu_decode_ops.py: Δmean, Δvar for statistics summed n deep) with the site's own
depth n (SITES, a comment beside each), but rstd taken through the exact interval instead of first order: with the clamp the kernel's
variance lies in [max(var − Δvar, 0), var + Δvar], so rstd lies in [1/sqrt(var + Δvar + eps), 1/sqrt(max(var − Δvar, 0) + eps)] —
finite only because of the clamp — and

    |Δy| <= |γ|·(|x − mean|·(Δrstd + 3u·rstd_hi) + Δmean·rstd_hi) + u·|y|,   Δrstd = max(rstd_hi − rstd, rstd − rstd_lo) + 2u·rstd_hi

(1 − t)^-1/2 − 1 >= t/2, so this is never below _ln_err and meets it as Δvar / (var + eps) -> 0; ln_bound returns the larger of the
two.  A 16-bit store is monotone: a value within e of a rounds into [round_T(a − e), round_T(a + e)] (ln_bound_t) — where e is far
below an ulp of T that is "the same 16-bit value, or one ulp at a rounding midpoint".

Restatements: one float32 function per summation order (order_*), each with the switches fma_sq (sq = fma(v, v, sq) or a rounded product
and an add), fma_var (var = fma(−mean, mean, sq / K) or a rounded square and a subtraction) and clamp — which of the first two the
compiler takes is its choice (-ffp-contract=on), and both must be safe."""
import numpy as np
import pytest

from test_gpu_decode_ops import DT_BF16, DT_F16, DT_F32, U, _ln64, _ln_err, _ln_stats, _round

F = np.float32
EPS = 1e-5
KS_ALL = (128, 384, 512, 768, 1024)
DC_RATIOS = (0, 4, 30, 100, 1000)
TEETH_MAX_DC = 30
# the issue's four constants, then those found by search_constants() so that every order at every K has three of them with
# var + eps < 0 under each contraction variant (test_every_order_reaches_a_negative_variance)
CONSTS = (1.7, 13.7, 100.7, 3.3, 52.83, 63.83, 272.83, 54.83)
EXACT_CONST = 2.0  # Σ and Σ of squares are exact in every order: x − mean == 0, the output is round_T(β) bit for bit


# ---- float32 arithmetic --------------------------------------------------------------------------------------------------------

def _fma(a, b, c):
    """round_f32(a·b + c) with one rounding.  a·b is exact in float64; the float64 sum s is rounded once more only when it lands
    exactly on a float32 rounding midpoint while the exact sum does not (TwoSum's error term says on which side)."""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # exact: s + err == p + c
    r = s.astype(F)
    d = r.astype(np.float64) - s
    with np.errstate(over="ignore"):
        other = np.nextafter(r, np.where(d > 0, F(-np.inf), F(np.inf)).astype(F))
    mid = (d != 0) & (np.abs(other.astype(np.float64) - s) == np.abs(d)) & (err != 0)
    toward = np.where(err > 0, np.maximum(r, other), np.minimum(r, other))
    return np.where(mid, toward, r).astype(F)


def _acc(sm, sq, v, fma_sq):
    return sm + v, (_fma(v, v, sq) if fma_sq else sq + v * v)


def _lane_sums(xl, fma_sq):
    """xl [..., n]: Σ and Σ of squares along the last axis, in order, from 0"""
    sm = np.zeros(xl.shape[:-1], F)
    sq = np.zeros(xl.shape[:-1], F)
    for j in range(xl.shape[-1]):
        sm, sq = _acc(sm, sq, xl[..., j], fma_sq)
    return sm, sq


def _butterfly(s, offsets, skip=None):
    """s [rows, lanes]: s += s[lane ^ o] for o in offsets (skip: a mutant without that level)"""
    lanes = np.arange(s.shape[1])
    for o in offsets:
        if o != skip:
            s = s + s[:, lanes ^ o]
    return s


# ---- the summation orders ------------------------------------------------------------------------------------------------------
# each: x [rows, K] float32 -> (Σx, Σx²) [rows] as the kernel's lane that normalises holds them.  drop: a mutant with one butterfly
# level (or one wave partial) missing.

def order_dec_linear(x, fma_sq, nw, kpw, drop=None):
    """dec_linear_kernel<…, LN = true>: wave w, lane group g holds x[(w + nw·i)·32 + 8 g + j], i < KPW, j < 8, added in that order;
    xor-16 and xor-32 join the four groups; the nw wave partials are added in wave order from 0."""
    R, K = x.shape
    assert K == nw * kpw * 32
    xl = x.reshape(R, kpw, nw, 4, 8).transpose(0, 2, 3, 1, 4).reshape(R, nw, 4, kpw * 8)
    sm, sq = _lane_sums(xl, fma_sq)
    out = []
    for s in (sm, sq):
        s = s.reshape(R * nw, 4)
        s = _butterfly(s, (1, 2), skip={"xor32": 2, "xor16": 1}.get(drop))[:, 0].reshape(R, nw)  # lane group g = lane >> 4: xor-16 is g ^ 1
        t = np.zeros(R, F)
        for k in range(nw - 1 if drop == "wave" else nw):
            t = t + s[:, k]
        out.append(t)
    return out


def order_rows8(x, fma_sq, drop=None):
    """dec_logits_kernel, dec_logits_split_kernel, dec_logits_split128_kernel (the same order by construction: two virtual threads per
    lane, the last butterfly level in registers) and score_ln_kernel: thread q of a row's 8 sums the float4 groups q + 8 i in order,
    then butterflies at offsets 1, 2, 4."""
    R, K = x.shape
    xl = x.reshape(R, K // 32, 8, 4).transpose(0, 2, 1, 3).reshape(R, 8, K // 8)
    sm, sq = _lane_sums(xl, fma_sq)
    skip = {"xor32": 4, "xor16": 2}.get(drop)  # this order's last two levels
    return [_butterfly(s, (1, 2, 4), skip)[:, 0] for s in (sm, sq)]


def order_wave64(x, fma_sq, drop=None):
    """no_speech_finish_kernel and lang_detect_kernel: lane l sums x[l + 64 i] in order, wave_sum (offsets 32 … 1)."""
    R, K = x.shape
    xl = x.reshape(R, K // 64, 64).transpose(0, 2, 1)
    sm, sq = _lane_sums(xl, fma_sq)
    skip = {"xor32": 32, "xor16": 16}.get(drop)
    return [_butterfly(s, (32, 16, 8, 4, 2, 1), skip)[:, 0] for s in (sm, sq)]


def order_rowpanel(x, fma_sq, drop=None):
    """gemm_nt_rowpanel_kernel<LNA>: lane group g holds x[32 k + 8 g + j], k < K / 32, j < 8, added in that order; xor-16, xor-32."""
    R, K = x.shape
    xl = x.reshape(R, K // 32, 4, 8).transpose(0, 2, 1, 3).reshape(R, 4, K // 4)
    sm, sq = _lane_sums(xl, fma_sq)
    skip = {"xor32": 2, "xor16": 1}.get(drop)
    return [_butterfly(s, (1, 2), skip)[:, 0] for s in (sm, sq)]


def _fullrow_cols():
    """[wave column wc][lane group g] -> the 24 columns of a 384-wide row in the order the epilogue adds them"""
    cols = np.zeros((4, 4, 24), np.int64)
    for wc in range(4):
        for g in range(4):
            cols[wc, g] = [((wc * 2 + j) * 16 if j < 2 else 128 + (wc * 4 + j - 2) * 16) + 4 * g + r for j in range(6) for r in range(4)]
    return cols


def order_fullrow(x, fma_sq, drop=None):
    """gemm_nt_fullrow_kernel<LNO>: a row's 384 columns sit in 4 waves x 4 lane groups, 6 column blocks x 4 values each, added in
    that order; xor-16, xor-32; the four wave partials meet as (w0 + w2) + (w1 + w3)."""
    R, K = x.shape
    assert K == 384
    xl = x[:, _fullrow_cols()]  # [R, wc, g, 24]
    sm, sq = _lane_sums(xl, fma_sq)
    out = []
    for s in (sm, sq):
        s = _butterfly(s.reshape(R * 4, 4), (1, 2), skip={"xor32": 2, "xor16": 1}.get(drop))[:, 0].reshape(R, 4)
        out.append((s[:, 0] + s[:, 2]) + (s[:, 1] + s[:, 3]))
    return out


def dec_linear_waves(K, elem_bytes):
    """(waves, k-steps per wave) as csrc/kernels_decoder.hip dec_linear_waves splits K: 16-bit operands take the fewest waves whose
    k-steps stay <= 3 (else <= 4), fp32 operands the most waves (<= 16) with <= 4 k-steps."""
    ks = K // 32
    if elem_bytes == 4:
        nw = next(c for c in range(16, 0, -1) if ks % c == 0 and ks // c <= 4)
    else:
        nw = next(c for lim in (3, 4) for c in range(1, 17) if ks % c == 0 and ks // c <= lim)
    return nw, ks // nw


# site -> (order, depth n of its statistics: sequential adds per lane + butterfly levels + cross-wave adds, K values it runs at)
def _dl(eb):
    return (lambda x, f, drop=None: order_dec_linear(x, f, *dec_linear_waves(x.shape[1], eb), drop=drop),
            lambda K: 8 * dec_linear_waves(K, eb)[1] + 2 + dec_linear_waves(K, eb)[0])  # 8·KPW in a lane + xor-16, xor-32 + nw partials


SITES = {
    "dec_linear16": _dl(2) + (KS_ALL,),                                   # 2x2, 4x3, 8x2, 8x3, 16x2: n = 20, 30, 26, 34, 34
    "dec_linear32": _dl(4) + (KS_ALL,),                                   # 4x1, 12x1, 16x1, 12x2, 16x2: n = 14, 22, 26, 30, 34
    "logits": (order_rows8, lambda K: K // 8 + 3, KS_ALL),                # K/8 in a lane + 3 butterfly levels (_ln_err's default)
    "score_ln": (order_rows8, lambda K: K // 8 + 3, KS_ALL),              # the same order
    "no_speech": (order_wave64, lambda K: K // 64 + 6, KS_ALL),           # K/64 in a lane + 6 butterfly levels
    "lang_detect": (order_wave64, lambda K: K // 64 + 6, KS_ALL),         # the same order
    "rowpanel": (order_rowpanel, lambda K: K // 4 + 2, (384,)),           # K/4 in a lane + xor-16, xor-32
    "fullrow": (order_fullrow, lambda K: 24 + 2 + 2, (384,)),             # 24 in a lane + xor-16, xor-32 + two levels over the waves
}
DISTINCT = ("dec_linear16", "dec_linear32", "logits", "no_speech", "rowpanel", "fullrow")  # one site per distinct order
VARIANTS = [(fs, fv) for fs in (False, True) for fv in (False, True)]


def restate(site, x, g, b, fma_sq=False, fma_var=False, clamp=True, fma_out=True, drop=None, mean_km1=False):
    """The site's LayerNorm in float32 -> (y [rows, K], var before the clamp [rows]).  fma_out: y = fma(t, γ, β), what -ffp-contract=on
    makes of the kernels' last line (either is inside the bound).  drop / mean_km1: the mutants of the teeth test."""
    x, g, b = (np.ascontiguousarray(a, F) for a in (x, g, b))
    K = x.shape[1]
    sm, sq = SITES[site][0](x, fma_sq, drop=drop)
    mean = sm / F(K - 1 if mean_km1 else K)
    q = sq / F(K)
    var = _fma(-mean, mean, q) if fma_var else q - mean * mean
    v = np.maximum(var, F(0)) if clamp else var
    with np.errstate(invalid="ignore", divide="ignore"):
        rstd = F(1) / np.sqrt(v + F(EPS))
    t = (x - mean[:, None]) * rstd[:, None]
    with np.errstate(invalid="ignore"):
        y = _fma(t, g, b) if fma_out else t * g + b
    return y.astype(F), var


# ---- cases ---------------------------------------------------------------------------------------------------------------------

def _ulps(c):
    c = F(c)
    return [c, np.nextafter(c, F(np.inf)), np.nextafter(c, F(-np.inf))]


def const_values():
    """every constant with both signs and its neighbours one ulp up and down, then the exact one"""
    vals = [s * v for c in CONSTS for v in _ulps(c) for s in (F(1), F(-1))]
    return np.array(vals + [F(EXACT_CONST), F(-EXACT_CONST)], F)


def ln_cases(K, seed=0):
    """name -> (x [rows, K], γ, β) float32.  dcR: 4 rows with mean / σ = R (float64), σ drawn per row from [0.5, 3), signs mixed;
    const: const_values(); near: 13.7 but for one element; unit: the dc rows again under γ = 1, β = 0."""
    r = np.random.default_rng(1000 * K + seed)
    g = (1 + 0.3 * r.standard_normal(K)).astype(F)
    b = (0.2 * r.standard_normal(K)).astype(F)
    cases = {}
    for R in DC_RATIOS:
        z = r.standard_normal((4, K))
        z = (z - z.mean(1, keepdims=True)) / z.std(1, keepdims=True)
        sig = r.uniform(0.5, 3.0, (4, 1))
        sign = np.array([[1.0], [-1.0], [1.0], [-1.0]])
        cases[f"dc{R}"] = (((z + sign * R * 1.001) * sig).astype(F), g, b)
    cases["const"] = (np.repeat(const_values()[:, None], K, 1), g, b)
    near = np.full((2, K), 13.7, F)
    near[0, (5 * K) // 7] = 14.7
    near[1, K - 1] = np.nextafter(F(13.7), F(np.inf))
    cases["near"] = (near, g, b)
    cases["unit"] = (np.concatenate([cases[f"dc{R}"][0][:2] for R in DC_RATIOS]), np.ones(K, F), np.zeros(K, F))
    return cases


def dc_ratio(name):
    return int(name[2:]) if name.startswith("dc") else None


def all_rows(K, seed=0):
    """the γ / β cases of ln_cases stacked -> (x [rows, K], γ, β, row names)"""
    cs = ln_cases(K, seed)
    names = [n for n in cs if n != "unit"]
    x = np.concatenate([cs[n][0] for n in names])
    tags = [f"{n}[{i}]" for n in names for i in range(len(cs[n][0]))]
    return x, cs[names[0]][1], cs[names[0]][2], tags


# ---- reference and bound -------------------------------------------------------------------------------------------------------

def ln_bound(x, g, b, n):
    """-> (float64 LayerNorm [rows, K], per-element bound on an fp32 evaluation with statistics summed n deep and the variance
    clamped at 0): the module docstring's interval form, never below _ln_err."""
    g64, b64 = g.astype(np.float64), b.astype(np.float64)
    x64, mu, var, d_mu, d_var = _ln_stats(x, n)
    var0 = np.maximum(var, 0.0)  # float64 roundoff only: a true variance is >= 0
    r = 1.0 / np.sqrt(var + EPS)
    r_lo = 1.0 / np.sqrt(var0 + d_var + EPS)
    r_hi = 1.0 / np.sqrt(np.maximum(var0 - d_var, 0.0) + EPS)
    d_r = np.maximum(r_hi - r, r - r_lo) + 2 * U * r_hi
    y = _ln64(x, g, b)
    exact = np.abs(g64) * (np.abs(x64 - mu) * (d_r + 3 * U * r_hi) + d_mu * r_hi) + U * np.abs(y)
    return y, np.maximum(exact, _ln_err(x, g, b, n))


def ln_bound_t(y, e, dt):
    """the store in dt of a value within e of y -> (y rounded to dt, bound): rounding is monotone, so the stored value lies between
    round(y − e) and round(y + e); bound 0 demands the same 16-bit value"""
    if dt == DT_F32:
        return y, e
    yt = _round(y, dt)
    return yt, np.maximum(_round(y + e, dt) - yt, yt - _round(y - e, dt))


def ratio(got, ref, bound):
    """largest error / bound; an element with bound 0 must be exact (ratio inf otherwise)"""
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(np.nan_to_num(q, nan=np.inf).max())


def search_constants(want=3, pool=None):
    """How CONSTS was extended: constants (two decimals) at which var + eps < 0 without the clamp, per (site, K, variant); returns the
    cells that have fewer than `want` hits in `pool` (default CONSTS)."""
    pool = CONSTS if pool is None else pool
    short = {}
    for site in DISTINCT:
        for K in SITES[site][2]:
            x = np.repeat(np.array(pool, F)[:, None], K, 1)
            one = np.ones(K, F)
            for fs, fv in VARIANTS:
                _, var = restate(site, x, one, one, fs, fv, clamp=False)
                hits = [c for c, v in zip(pool, var) if v + F(EPS) < 0]
                if len(hits) < want:
                    short[(site, K, fs, fv)] = hits
    return short


# ---- CPU tests -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("site", list(SITES))
def test_restatement_with_clamp_meets_every_bound(site):
    """(a) every contraction variant of every order, clamped, is finite and inside the bound on every case, in fp32 and through
    both 16-bit stores."""
    _, depth, Ks = SITES[site]
    worst = 0.0
    for K in Ks:
        for name, (x, g, b) in ln_cases(K).items():
            ref, e = ln_bound(x, g, b, depth(K))
            for fs, fv in VARIANTS:
                for fo in (False, True):
                    y, _ = restate(site, x, g, b, fs, fv, fma_out=fo)
                    assert np.isfinite(y).all(), (site, K, name, fs, fv)
                    w = ratio(y, ref, e)
                    for dt in (DT_BF16, DT_F16):
                        w = max(w, ratio(_round(y, dt), *ln_bound_t(ref, e, dt)))
                    assert w <= 1.0, (site, K, name, fs, fv, fo, w)
                    worst = max(worst, w)
    print(f"MEASURED restatement {site}: worst error / bound {worst:.3f}")


# cells in which no constant can go negative: every partial sum of a constant row is c·2^k or c²·2^k there (two adds per lane, then
# a balanced tree), so the sums are exact, mean == c and q == fl(c²) == fl(mean·mean) unless a contraction keeps the square unrounded
EXACT_CELLS = {("no_speech", 128, False, False), ("no_speech", 128, True, False)}


@pytest.mark.parametrize("site", DISTINCT)
def test_every_order_reaches_a_negative_variance(site):
    """(b) without the clamp every order has, at every K it runs at and under each contraction variant, at least three constants of
    the list with var + eps < 0 — the square root of a negative number — so the GPU test exercises the clamp at every site whatever
    the compiler contracted.  With the clamp the same rows are finite (a)."""
    short = {k: v for k, v in search_constants().items() if k[0] == site and k not in EXACT_CELLS}
    assert not short, short
    for K in SITES[site][2]:
        x = np.repeat(np.array(CONSTS, F)[:, None], K, 1)
        one = np.ones(K, F)
        for fs, fv in VARIANTS:
            y, var = restate(site, x, one, one, fs, fv, clamp=False)
            neg = var + F(EPS) < 0
            assert np.isnan(y[neg]).all() and np.isfinite(y[~neg]).all()
            print(f"{site} K {K} fma_sq {int(fs)} fma_var {int(fv)}: {int(neg.sum())} of {len(CONSTS)} constants negative, min var {var.min():.2e}")


@pytest.mark.parametrize("site", list(SITES))
def test_clamp_keeps_every_bit_where_the_variance_is_not_negative(site):
    _, _, Ks = SITES[site]
    for K in Ks:
        x, g, b, _ = all_rows(K)
        for fs, fv in VARIANTS:
            y1, var = restate(site, x, g, b, fs, fv, clamp=True)
            y0, _ = restate(site, x, g, b, fs, fv, clamp=False)
            keep = var >= 0
            assert np.array_equal(y0[keep].view(np.uint32), y1[keep].view(np.uint32))


@pytest.mark.parametrize("site", list(SITES))
def test_bound_has_teeth(site):
    """(c) a restatement without its xor-32 butterfly level (this order's last level but one where it has no xor-32), and one whose
    mean is divided by K − 1, leave the bound on every case with mean / σ <= 30, at every K (the K − 1 mutant from mean / σ = 4 on: on
    centred rows it changes nothing)."""
    _, depth, Ks = SITES[site]
    for K in Ks:
        for name, (x, g, b) in ln_cases(K).items():
            R = dc_ratio(name)
            if R is None or R > TEETH_MAX_DC:
                continue
            ref, e = ln_bound(x, g, b, depth(K))
            for kw in (dict(drop="xor32"), dict(mean_km1=True)):
                if R == 0 and "mean_km1" in kw:  # an equivalent mutant there: the rows are centred, 0 / (K − 1) == 0 / K
                    continue
                y, _ = restate(site, x, g, b, **kw)
                w = ratio(y, ref, e)
                assert w > 1.0, (site, K, name, kw, w)
                for dt in (DT_BF16, DT_F16):
                    assert ratio(_round(y, dt), *ln_bound_t(ref, e, dt)) > 1.0, (site, K, name, kw, dt)


def test_dec_linear_wave_partial_dropped_leaves_the_bound():
    for site in ("dec_linear16", "dec_linear32"):
        for K in KS_ALL:
            x, g, b = ln_cases(K)["dc4"]
            ref, e = ln_bound(x, g, b, SITES[site][1](K))
            assert ratio(restate(site, x, g, b, drop="wave")[0], ref, e) > 1.0


def test_cases_are_what_they_claim():
    for K in KS_ALL:
        cs = ln_cases(K)
        for R in DC_RATIOS:
            x = cs[f"dc{R}"][0].astype(np.float64)
            got = np.abs(x.mean(1)) / x.std(1)
            assert (np.abs(got - R * 1.001) <= 1e-3 * max(R, 1)).all(), (K, R, got)
        c = cs["const"][0]
        assert (c == c[:, :1]).all() and len(c) == 6 * len(CONSTS) + 2
        assert set(np.sign(c[:, 0])) == {-1.0, 1.0}
        assert (cs["unit"][1] == 1).all() and (cs["unit"][2] == 0).all()
        g, b = cs["dc0"][1], cs["dc0"][2]
        assert np.abs(g - 1).max() > 0.3 and np.abs(b).max() > 0.2
    assert [dec_linear_waves(K, 2) for K in KS_ALL] == [(2, 2), (4, 3), (8, 2), (8, 3), (16, 2)]
    assert [dec_linear_waves(K, 4) for K in KS_ALL] == [(4, 1), (12, 1), (16, 1), (12, 2), (16, 2)]
    assert sorted(_fullrow_cols().ravel().tolist()) == list(range(384))


def test_exact_constant_gives_beta_bit_for_bit():
    """±2: every partial sum is exact in every order, x − mean == 0, the output is β exactly — the one constant row with bound 0 in
    the sense of the GPU test (its 16-bit store must be round_T(β))."""
    for site in SITES:
        for K in SITES[site][2]:
            x = np.repeat(np.array([EXACT_CONST, -EXACT_CONST], F)[:, None], K, 1)
            _, g, b, _ = all_rows(K)
            for fs, fv in VARIANTS:
                y, var = restate(site, x, g, b, fs, fv)
                assert (var == 0).all() and np.array_equal(y, np.stack([b, b]))


def test_fma_helper_rounds_once():
    r = np.random.default_rng(5)
    a, b, c = (r.standard_normal(20000).astype(F) * F(10) ** r.integers(-3, 4, 20000).astype(F) for _ in range(3))
    from fractions import Fraction
    got = _fma(a, b, c)
    for i in range(0, 20000, 37):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = sorted((float(got[i]), float(np.nextafter(got[i], F(np.inf) if exact > Fraction(float(got[i])) else F(-np.inf)))))
        assert abs(exact - Fraction(float(got[i]))) <= (Fraction(hi) - Fraction(lo)) / 2
    assert _fma(F(1 + 2.0 ** -12), F(1 + 2.0 ** -12), F(-1)) == F(2.0 ** -11 + 2.0 ** -24)  # the product's low bits survive
