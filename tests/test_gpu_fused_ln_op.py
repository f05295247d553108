"""Op-level tests (-m gpu) of the LayerNorm inside nine kernels on rows whose mean dwarfs their spread — the input on
which a one-pass variance cancels, down to constant rows where fp32 gives var < −eps and only the clamp keeps 1 / sqrtf finite.
Cases, float64 reference, bounds and the float32 restatements are tests/test_fused_ln_ref.py's (proved there on the CPU).

The matrix product is made exact so that the LayerNorm is what is measured: the weight / embedding rows are rows of a signed
permutation matrix (entries ±1 and 0, exact in every dtype; N = K, or N > K with the further rows zero), no bias.  Output column j is
then ±LN(x)[π(j)] as the kernel formed it: for 16-bit operands the fp32 LayerNorm output rounded to T — it must lie between
round_T(a − e) and round_T(a + e) for the float64 a and the LayerNorm bound e (rounding is monotone; with e far below an ulp this is
"the same value, or one ulp at a midpoint") — and for fp32 operands within e plus the kernel's accumulation term.  One random-weight
case per hook goes through the existing bound builders, so the wiring is not only seen through permutations."""
import ctypes as C

import numpy as np
import pytest

import test_fused_ln_ref as gen
from test_gpu_decode_layer import ACC_EXTRA, ACC_STEP, SENT, _check as _lin_check, linear_ref
from test_gpu_decode_ops import DT_BF16, DT_F16, DT_F32, U, _logits_ref, _lowest_argmax, hip  # noqa: F401
from test_gpu_lang_detect_op import _check as _lang_check
from test_gpu_no_speech_op import _check as _ns_check
from test_gpu_score_op import _check as _score_check

pytestmark = pytest.mark.gpu

DTS = (DT_F32, DT_BF16, DT_F16)
NEG_CONST = 52.83  # var + eps < 0 in every order at every K under every contraction (test_every_order_reaches_a_negative_variance)


def _wt():
    from whisper_mojo_amd import whisper_tensor as wt
    return wt


def _perm(K, N, seed):
    """W [N, K]: row j < K is ±e_π(j), rows from K on are zero -> (W, π, signs)"""
    r = np.random.default_rng(seed)
    pi, sg = r.permutation(K), r.choice([-1.0, 1.0], K)
    W = np.zeros((N, K), np.float32)
    W[np.arange(K), pi] = sg
    return W, pi, sg


def _pool(K):
    x, g, b, tags = gen.all_rows(K)
    return x, g, b, tags


def _pick(K, B):
    """rows of the pool for a call of B rows: 1 -> the constant with a negative variance in every order; 17 -> one row of each DC
    ratio, the near-constant row, every constant, −c and c one ulp up of NEG_CONST, the exact constant; else the pool, repeated"""
    x, _, _, tags = _pool(K)
    at = lambda t: tags.index(t)
    c0 = at("const[0]")
    neg = c0 + 6 * gen.CONSTS.index(NEG_CONST)
    if B == 1:
        return np.array([neg])
    if B == 17:
        idx = [at(f"dc{R}[0]") for R in gen.DC_RATIOS] + [at("near[0]")] + [c0 + 6 * i for i in range(len(gen.CONSTS))]
        idx += [neg + 1, neg + 2, c0 + 6 * len(gen.CONSTS)]
        assert len(idx) == 17
        return np.array(idx)
    return np.arange(B) % len(x)


def _acc_term(kind, K, dt):
    """the kernel's existing fp32 accumulation term per unit |a| (16-bit operands: none — one exact product and zeros)"""
    if dt != DT_F32:
        return 0.0
    if kind == "linear":
        return (min(K, ACC_STEP) + ACC_EXTRA + 1) * U
    split = K in (128, 384)  # the logits kernels (_logits_ref): 3×bf16 split at K = 128 / 384, exact fp32 MFMA above
    return ((6 * K if split else K) * U + (2.0 ** -21 if split else 0.0)) * (1 + 3 * 2.0 ** -7)


def _expect(site, x, g, b, dt, pi, sg, N, kind):
    """-> (ref [B, N], bound [B, N]) of LN(x)·Wᵀ for the signed permutation (π, signs) padded with zero rows to N"""
    K = x.shape[1]
    y, e = gen.ln_bound(x, g, b, gen.SITES[site][1](K))
    yt, et = gen.ln_bound_t(y, e, dt)
    et = et + _acc_term(kind, K, dt) * np.abs(yt)
    ref, bound = np.zeros((len(x), N)), np.zeros((len(x), N))
    ref[:, :K], bound[:, :K] = yt[:, pi] * sg, et[:, pi]
    return ref, bound


def _check(tag, got, ref, bound):
    assert np.isfinite(got).all(), (tag, "not finite", np.argwhere(~np.isfinite(got))[:4].tolist())
    w = gen.ratio(got, ref, bound)
    print(f"MEASURED {tag}: worst error / bound {w:.3f}")
    err = np.abs(got - ref)
    assert w <= 1.0, (tag, w, np.argwhere(err > bound)[:4].tolist())
    return w


def _check_exact_const(tag, got, x, b, dt, pi, sg):
    """rows of ±EXACT_CONST: x − mean == 0 in every order, the kernel must return round_T(β) bit for bit"""
    rows = np.flatnonzero((np.abs(x) == gen.EXACT_CONST).all(1))
    want = gen._round(b, dt)[pi] * sg
    for r in rows:
        assert np.array_equal(got[r, :len(pi)], want), (tag, "constant row", r)
    return len(rows)


def _clamp_exercised(site, x):
    """some row of the call has var + eps < 0 in the site's order under each contraction variant (but the cells in which every sum of
    a constant row is exact: gen.EXACT_CELLS)"""
    K = x.shape[1]
    one = np.ones(K, np.float32)
    order = {"lang_detect": "no_speech", "score_ln": "logits"}.get(site, site)
    for fs, fv in gen.VARIANTS:
        if (order, K, fs, fv) in gen.EXACT_CELLS:
            continue
        _, var = gen.restate(site, x, one, one, fs, fv, clamp=False)
        assert (var + np.float32(gen.EPS) < 0).any(), (site, fs, fv)


# ---- dec_linear ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K", gen.KS_ALL)
def test_dec_linear_ln_prologue(hip, K, dt):
    """plain mode, N = K: B = 1 (the constant row that goes negative) and the whole pool in calls of B = 17"""
    site = "dec_linear32" if dt == DT_F32 else "dec_linear16"
    x, g, b, _ = _pool(K)
    W, pi, sg = _perm(K, K, K + dt)
    worst, exact = 0.0, 0
    calls = [_pick(K, 1), _pick(K, 17)] + [np.arange(i, i + 17) % len(x) for i in range(0, len(x), 17)]
    _clamp_exercised(site, x[calls[0]])
    _clamp_exercised(site, x[calls[1]])
    for idx in calls:
        xs = x[idx]
        out = _wt().dec_linear(xs, W, None, ln=(g, b), dtype=dt)
        ref, bound = _expect(site, xs, g, b, dt, pi, sg, K, "linear")
        worst = max(worst, _check(f"dec_linear dt {dt} K {K} B {len(idx)}", out, ref, bound))
        exact += _check_exact_const("dec_linear", out, xs, b, dt, pi, sg)
    assert exact >= 3
    print(f"MEASURED dec_linear plain dt {dt} K {K}: {worst:.3f}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K", gen.KS_ALL)
def test_dec_linear_ln_prologue_qkv(hip, K, dt):
    """QKV mode, N = 3 K, a permutation in each third: q from the output, k and v from the cache rows the launch appended (stored in
    the operand dtype: the values are already such values); every other cache row keeps its sentinel"""
    site = "dec_linear32" if dt == DT_F32 else "dec_linear16"
    x, g, b, _ = _pool(K)
    thirds = [_perm(K, K, 3 * K + dt + t) for t in range(3)]
    W = np.concatenate([t[0] for t in thirds])
    for B in (1, 17):
        xs = x[_pick(K, B)]
        _clamp_exercised(site, xs)
        kc0 = np.full((B, 4, K), SENT, np.float32)
        q, kc, vc = _wt().dec_linear(xs, W, None, ln=(g, b), dtype=dt, kv=(kc0, kc0), kv_dtype=dt, len=2)
        for name, got, (_, pi, sg) in (("q", q, thirds[0]), ("k", kc[:, 2], thirds[1]), ("v", vc[:, 2], thirds[2])):
            ref, bound = _expect(site, xs, g, b, dt, pi, sg, K, "linear")
            _check(f"dec_linear qkv {name} dt {dt} K {K} B {B}", got, ref, bound)
            _check_exact_const("qkv " + name, got, xs, b, dt, pi, sg)
        for cache in (kc, vc):
            assert (cache[:, [0, 1, 3]] == SENT).all()


@pytest.mark.parametrize("dt", DTS)
def test_dec_linear_random_weights(hip, dt):
    """wiring: random weights and a bias on the centred and the mean / σ = 4 rows, through linear_ref"""
    K, N = 384, 400
    cs = gen.ln_cases(K)
    x = np.concatenate([cs["dc0"][0], cs["dc4"][0]])
    g, b = cs["dc0"][1], cs["dc0"][2]
    r = np.random.default_rng(dt)
    W = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = (0.1 * r.standard_normal(N)).astype(np.float32)
    site = "dec_linear32" if dt == DT_F32 else "dec_linear16"
    out = _wt().dec_linear(x, W, bias, ln=(g, b), dtype=dt)
    _lin_check(f"dec_linear random dt {dt}", out, *linear_ref(x, W, bias, dt, ln=(g, b), depth=gen.SITES[site][1](K)))


# ---- logits / logits_lp --------------------------------------------------------------------------------------------------------

# (dtype, K, B): one row per kernel variant named in test_gpu_decode_ops.LOGITS_CASES — B = 1, 17, 65 select the 1-block, 4-block and
# (fp32 at K = 128 / 384) 128-row forms
LOGITS = [(DT_F32, K, B) for K in (128, 384, 512) for B in (1, 17, 65)] + \
         [(dt, K, B) for dt in (DT_BF16, DT_F16) for K in (128, 384, 512) for B in (1, 17)]


@pytest.mark.parametrize("lp", (False, True))
@pytest.mark.parametrize("dt,K,B", LOGITS)
def test_logits_ln(hip, dt, K, B, lp):
    x, g, b, _ = _pool(K)
    xs = x[_pick(K, B)]
    _clamp_exercised("logits", xs)
    N = K + 16 + 7  # further rows zero, a ragged last tile
    emb, pi, sg = _perm(K, N, 7 * K + dt)
    res = _wt().logits_argmax(xs, g, b, emb, dtype=dt, return_logprobs=lp)
    logits, ids = res[0], res[1]
    ref, bound = _expect("logits", xs, g, b, dt, pi, sg, N, "logits")
    _check(f"logits{'_lp' if lp else ''} dt {dt} K {K} B {B}", logits, ref, bound)
    _check_exact_const("logits", logits, xs, b, dt, pi, sg)
    np.testing.assert_array_equal(ids, _lowest_argmax(logits))
    if lp:
        assert np.isfinite(res[2]).all() and (res[2] <= 0).all()


@pytest.mark.parametrize("dt,K,B", [(DT_F32, 384, 17), (DT_BF16, 512, 17), (DT_F16, 128, 17)])
def test_logits_random_weights(hip, dt, K, B):
    cs = gen.ln_cases(K)
    x = np.concatenate([cs["dc0"][0], cs["dc4"][0]] * 3)[:B]
    g, b = cs["dc0"][1], cs["dc0"][2]
    emb = (np.random.default_rng(K).standard_normal((1000, K)) * 0.04).astype(np.float32)
    logits, ids = _wt().logits_argmax(x, g, b, emb, dtype=dt)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    assert (np.abs(logits - ref) <= bound).all()
    np.testing.assert_array_equal(ids, _lowest_argmax(logits))


# ---- no_speech, lang_detect, score_logits: the LayerNorm seen through a softmax -----------------------------------------------
# these hooks return probabilities, not logits: the per-logit reference and bound above go into each hook's own checker (2·e + r)

def _logit_bounds(sites, xs, g, b, dt, pi, sg, N):
    """per-logit (ref, bound) valid for every site named: the widest of their bounds (the references are one float64 LayerNorm)"""
    outs = [_expect(s, xs, g, b, dt, pi, sg, N, "logits") for s in sites]
    return outs[0][0], np.maximum.reduce([o[1] for o in outs])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K", gen.KS_ALL)
def test_no_speech_ln(hip, K, dt):
    """the sweep's LayerNorm (the logits kernels' order) and no_speech_finish_kernel's own (one wave, K / 64 per lane) on the same
    rows; the token's row is a permutation row"""
    x, g, b, _ = _pool(K)
    N = K + 23
    emb, pi, sg = _perm(K, N, 11 * K + dt)
    for B in (1, 5):
        xs = x[_pick(K, 17)[[6 + gen.CONSTS.index(NEG_CONST)] if B == 1 else [1, 2, 5, 6 + gen.CONSTS.index(NEG_CONST), 16]]]
        _clamp_exercised("no_speech", xs)
        _clamp_exercised("logits", xs)
        ref, bound = _logit_bounds(("logits", "no_speech"), xs, g, b, dt, pi, sg, N)
        for token in (0, K - 1):
            prob, lse = _wt().no_speech(xs, g, b, emb, token, dtype=dt)
            _ns_check(f"MEASURED no_speech dt {dt} K {K} B {B} token {token}", prob, lse, ref, bound, token, N)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K", gen.KS_ALL)
def test_lang_detect_ln(hip, K, dt):
    x, g, b, _ = _pool(K)
    N = K + 23
    emb, pi, sg = _perm(K, N, 13 * K + dt)
    r = np.random.default_rng(K)
    ids = np.concatenate([[N - 1], r.choice(np.arange(1, K), 126, replace=False), [0]]).astype(np.int32)  # 128 ids, one a zero row
    xs = x[_pick(K, 17)]
    _clamp_exercised("lang_detect", xs)
    ref, bound = _expect("lang_detect", xs, g, b, dt, pi, sg, N, "logits")
    got, probs = _wt().lang_detect(xs, g, b, emb, ids, dtype=dt)
    assert set(got.tolist()) <= set(ids.tolist())
    with np.errstate(divide="ignore"):  # the checker prints gap / 2e, and e is 0 on a row whose 16-bit values are all demanded exactly
        _lang_check(f"MEASURED lang_detect dt {dt} K {K}", got, probs, xs, g, b, emb, ids, dt, need_all=False, refs=(ref[:, ids], bound[:, ids]))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K", gen.KS_ALL)
def test_score_logits_ln(hip, K, dt):
    """M = 1 and 33 (the last 8-lane group of score_ln's second workgroup holds a clamped row index); a guard element after logprob
    and top_id comes back untouched"""
    from whisper_mojo_amd import _lib
    x, g, b, _ = _pool(K)
    N = K + 23
    emb, pi, sg = _perm(K, N, 17 * K + dt)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    for M in (1, 33):
        xs = np.ascontiguousarray(x[_pick(K, 1)] if M == 1 else x[np.concatenate([_pick(K, 17), _pick(K, 17)[:16]])])
        _clamp_exercised("score_ln", xs)
        ref, bound = _expect("score_ln", xs, g, b, dt, pi, sg, N, "logits")
        tg = (np.arange(M) % N).astype(np.int32)
        lp, top = np.full(M + 1, 7.5, np.float32), np.full(M + 1, -77, np.int32)
        _lib.check(_lib.lib().wm_op_score_logits(lp.ctypes.data_as(fp), top.ctypes.data_as(ip), xs.ctypes.data_as(fp), g.ctypes.data_as(fp),
                                                 b.ctypes.data_as(fp), emb.ctypes.data_as(fp), tg.ctypes.data_as(ip), M, N, K, dt))
        assert lp[M] == 7.5 and top[M] == -77
        _score_check(f"MEASURED score_logits dt {dt} K {K} M {M}", lp[:M], top[:M], ref, bound, tg, N, dt)


@pytest.mark.parametrize("hook", ("no_speech", "lang_detect", "score_logits"))
def test_softmax_hooks_random_weights(hip, hook):
    dt, K, N = DT_BF16, 384, 1000
    cs = gen.ln_cases(K)
    x = np.concatenate([cs["dc0"][0], cs["dc4"][0]])
    g, b = cs["dc0"][1], cs["dc0"][2]
    emb = (np.random.default_rng(3).standard_normal((N, K)) * 0.04).astype(np.float32)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    if hook == "no_speech":
        _ns_check(hook, *_wt().no_speech(x, g, b, emb, 939, dtype=dt), ref, bound, 939, N)
    elif hook == "lang_detect":
        ids = np.asarray([N - 1, 17, 500, 3, 0], np.int32)
        got, probs = _wt().lang_detect(x, g, b, emb, ids, dtype=dt)
        _lang_check(hook, got, probs, x, g, b, emb, ids, dt, need_all=False)
    else:
        tg = (np.arange(len(x)) * 97 % N).astype(np.int32)
        _score_check(hook, *_wt().score_logits(x, g, b, emb, tg, dtype=dt), ref, bound, tg, N, dt)


# ---- the encoder's two fused forms ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", (DT_BF16, DT_F16))
@pytest.mark.parametrize("M", (130, 300))  # the M of test_op_matmul_rowpanel_bf16 / test_ln_matmul_fused_and_refused_shapes
def test_ln_matmul_rowpanel_ln(hip, M, dt):
    K = 384
    x, g, b, _ = _pool(K)
    xs = x[_pick(K, M)]
    _clamp_exercised("rowpanel", xs)
    W, pi, sg = _perm(K, K, M + dt)
    out = np.full((M, K), 7.0, np.float32)
    _wt().ln_matmul(out, xs, g, b, W, None, dtype=dt, require_fused=True)
    ref, bound = _expect("rowpanel", xs, g, b, dt, pi, sg, K, "linear")
    _check(f"ln_matmul row-panel dt {dt} M {M}", out, ref, bound)
    assert _check_exact_const("ln_matmul", out, xs, b, dt, pi, sg) >= 2


@pytest.mark.parametrize("dt", (DT_BF16, DT_F16))
def test_ln_matmul_random_weights(hip, dt):
    K, M, N = 384, 130, 384
    cs = gen.ln_cases(K)
    x = np.concatenate([cs["dc0"][0], cs["dc4"][0]] * 17)[:M]
    g, b = cs["dc0"][1], cs["dc0"][2]
    r = np.random.default_rng(dt)
    W = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = (0.1 * r.standard_normal(N)).astype(np.float32)
    out = np.zeros((M, N), np.float32)
    _wt().ln_matmul(out, x, g, b, W, bias, dtype=dt, require_fused=True)
    # linear_ref's accumulation term has dec_linear's depth, min(K, 128) + 16; the row-panel kernel chains all 12 k-steps of a row in one
    # accumulator, depth K: the order-independent (K − 144)·u·Σ|terms| more, as _logits_ref takes it
    ref, bound = linear_ref(x, W, bias, dt, ln=(g, b), depth=gen.SITES["rowpanel"][1](K))
    at, wt_ = np.abs(gen._round(gen._ln64(x, g, b), dt)), np.abs(gen._round(W, dt))
    _lin_check(f"ln_matmul random dt {dt}", out, ref, bound + (K - ACC_STEP - ACC_EXTRA) * U * (at @ wt_.T))


@pytest.mark.parametrize("dt", (DT_BF16, DT_F16))
def test_mlp_block_next_ln(hip, dt):
    """d = 384 with the (M, ffn) of test_op_mlp_block_bf16; fc2_w = 0 and fc2_b = 0: the new residual stream is the input bit for bit
    (so the fc1 side — the row-panel LayerNorm on the same rows, GELU — put nothing but finite values into fc2), and xn_out is the
    full-row epilogue's LayerNorm of exactly the generated rows"""
    M, d, ffn = 300, 384, 1536
    x, g, b, _ = _pool(d)
    xs = np.ascontiguousarray(x[_pick(d, M)])
    _clamp_exercised("fullrow", xs)
    _clamp_exercised("rowpanel", xs)
    r = np.random.default_rng(dt)
    g1, b1 = (1 + 0.2 * r.standard_normal(d)).astype(np.float32), (0.1 * r.standard_normal(d)).astype(np.float32)
    w1, bb1 = (r.standard_normal((ffn, d)) / np.sqrt(d)).astype(np.float32), (0.1 * r.standard_normal(ffn)).astype(np.float32)
    got = xs.copy()
    xn = _wt().mlp_block(got, g1, b1, w1, bb1, np.zeros((d, ffn), np.float32), np.zeros(d, np.float32), next_ln=(g, b), dtype=dt)
    assert np.isfinite(got).all(), "the fc1 side put NaN into x"
    assert np.array_equal(got.view(np.uint32), xs.view(np.uint32))
    ident = np.arange(d)
    ref, bound = _expect("fullrow", xs, g, b, dt, ident, np.ones(d), d, "linear")
    _check(f"mlp_block next_ln dt {dt}", xn, ref, bound)
    assert _check_exact_const("mlp_block", xn, xs, b, dt, ident, np.ones(d)) >= 2
