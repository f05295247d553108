"""Op-level tests (-m gpu) of the kernels at Whisper-medium's shapes (d_model 1024 = 8 k-panels of 128, 16 heads, ffn 4096), against
float64 on the operands exactly as the kernels receive them.  References, hooks and bounds are those of
tests/test_gpu_decode_layer.py (linear_ref, ln_depth, the GELU model, the attention tolerance), tests/test_gpu_decode_ops.py
(_logits_ref, the tie construction), tests/test_gpu_logits_lp.py (the log-prob bound) and tests/test_gpu_score_op.py (the score
bound): imported, not restated, no new constant.

Accumulation depth at K = 4096.  linear_ref bounds the accumulation by h·u·Σ|terms| with h the most additions one term passes
through, and takes h = min(K, 128) + 16: 32 additions in a term's own k-step, 32 per later k-step of its wave's chain (<= 4), then
the <= 16 wave partials.  The K = 4096 form chains KG x KPW = 2 x 4 = 8 k-steps per wave (k-step w + 16·(4·kg + i)), so the same
reasoning gives h = 32·8 + 16 = 272 (acc_depth below, derived from the split as ln_depth is).  The bound used is the larger of the
two: the imported bound plus (272 - 144)·u·Σ|a_k ŵ_k|.

  * wm_op_dec_linear_long at K = 4096: N in {48, 1024, 1040}, B in {1, 17, 64, 128}, fp32 / bf16 / f16, residual in place and
    none, x_is_t; K = 3072 through it equals wm_op_dec_linear bit for bit; K = 2048, K = 4128 and a LayerNorm prologue refused;
  * one k-step carrying all the weight: k-steps 0, 15, 16, 63, 64, 127 and the (wave, group) corners 48, 79, 112 of the split;
  * the rest of a d = 1024 step through wm_op_dec_linear: fc1 (4096, 1024), qkv (3072, 1024) with the append and prefill rows,
    attn_out and cross-q (1024, 1024) with both capture forms (heads 15, 0, 9);
  * logits + fused argmax at K = 1024 (32 rows per workgroup): rows 1 .. 128 on the row-block boundaries, log-probs, ties, mask,
    timestamp rules, one k-panel carrying the operand;
  * the score sweep at K = 1024 (K in two halves); no_speech and lang_detect; attention_cached at 16 heads."""
import numpy as np
import pytest

from test_gpu_decode_layer import (ACC_EXTRA, ACC_STEP, SENT, _attn_check, _attn_inputs, _check, _run_case, _wt, linear_ref, ln_depth)
from test_gpu_decode_ops import (DT_BF16, DT_F16, DT_F32, U, _call_logits, _decoder_like, _ln64, _logits_ref, _lowest_argmax, _round,
                                 _tie_columns, hip)  # noqa: F401
from test_gpu_logits_lp import _check as _lp_check, _lp, _ranges, _tb
from test_gpu_parity import _attention_cached_ref
from test_gpu_score_op import _check as _score_check, _geometry, _score, _targets

pytestmark = pytest.mark.gpu

D, H, FFN = 1024, 16, 4096
DTS = (DT_F32, DT_BF16, DT_F16)
SPLIT = {dt: (16, 2) for dt in DTS}  # (waves, k-steps per wave) of K = 1024, as dec_linear_waves splits it for every operand type
LONG_SPLIT = (16, 2, 4)              # (waves, groups, k-steps per group) of K = 4096: k-step w + 16·(4·kg + i)


def acc_depth(split):
    """most additions a product passes through: 32 per k-step of its wave's chain, then the wave partials"""
    nw, kg, kpw = split
    return 32 * kg * kpw + nw


def long_ref(x, W, bias, dt, residual=None):
    """linear_ref with the accumulation depth of the K-long split where that is the larger (no LayerNorm, no GELU at this K)"""
    ref, bound = linear_ref(x, W, bias, dt, residual=residual)
    more = acc_depth(LONG_SPLIT) - (min(x.shape[1], ACC_STEP) + ACC_EXTRA)
    if more > 0:
        bound = bound + more * U * (np.abs(_round(x, dt)) @ np.abs(_round(W, dt)).T)
    return ref, bound


def _long(*a, **kw):
    return _wt().dec_linear_long(*a, **kw)


# ---- fc2 at K = 4096 ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N", [48, 1024, 1040])
def test_medium_k4096_vs_float64(hip, dt, N):
    """(N, K) = (N, 4096): N = 48 one column tile per workgroup, 1024 two, 1040 two with a last workgroup of one.  Per B: the
    decode step's form (operand-dtype rows, residual in place) and the plain one (fp32 rows, no residual), which must agree with
    x_is_t bit for bit for 16-bit operands."""
    K = FFN
    r = np.random.default_rng(7919 * N + dt)
    W = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = (0.1 * r.standard_normal(N)).astype(np.float32)
    for B in (1, 17, 64, 128):
        x = _round(r.standard_normal((B, K)) * 0.5, dt).astype(np.float32)
        res = (2 * r.standard_normal((B, N))).astype(np.float32)
        out = _long(x, W, bias, residual=res, in_place=True, dtype=dt, x_is_t=True)
        ref, bound = long_ref(x, W, bias, dt, residual=res)
        assert _check(f"K 4096 N {N} B {B} dt {dt} residual in place", out, ref, bound) <= 1.0
        if B in (17, 128):
            np.testing.assert_array_equal(out, _long(x, W, bias, residual=res, dtype=dt, x_is_t=True))  # residual in its own buffer
            plain = _long(x, W, bias, dtype=dt)
            ref, bound = long_ref(x, W, bias, dt)
            assert _check(f"K 4096 N {N} B {B} dt {dt} plain", plain, ref, bound) <= 1.0
            if dt != DT_F32:
                np.testing.assert_array_equal(plain, _long(x, W, bias, dtype=dt, x_is_t=True))


KSTEPS = (0, 15, 16, 63, 64, 127,  # first; last wave's first; second step of wave 0; last of group 0; first of group 1; last
          48, 79, 112)            # wave 0: last step of group 0; wave 15: first step of group 1; wave 0: last step of group 1


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N", [1024, 1040])
def test_medium_k4096_one_kstep_carries_the_weight(hip, dt, N):
    """K = 4096: x and W are nonzero in ONE 32-column k-step.  A dropped k-step gives bias + residual alone, a doubled one twice the
    product, one added into another group's registers after they were consumed nothing: each is O(1) against a bound of ~1e-5."""
    K, B = FFN, 5
    r = np.random.default_rng(N + dt)
    bias = (0.1 * r.standard_normal(N)).astype(np.float32)
    res = (2 * r.standard_normal((B, N))).astype(np.float32)
    assert all(0 <= ks < K // 32 for ks in KSTEPS)
    corners = {(ks % LONG_SPLIT[0], ks // (LONG_SPLIT[0] * LONG_SPLIT[2])) for ks in KSTEPS}
    assert {(0, 0), (15, 0), (0, 1), (15, 1)} <= corners
    for ks in KSTEPS:
        x = np.zeros((B, K), np.float32)
        x[:, 32 * ks:32 * ks + 32] = _round(r.standard_normal((B, 32)) * 0.5, dt)
        W = np.zeros((N, K), np.float32)
        W[:, 32 * ks:32 * ks + 32] = r.standard_normal((N, 32)) / np.sqrt(32)
        out = _long(x, W, bias, residual=res, in_place=True, dtype=dt, x_is_t=True)
        ref, bound = long_ref(x, W, bias, dt, residual=res)
        assert np.abs(ref - (bias + res.astype(np.float64))).mean() > 0.1  # the k-step's product is O(1)
        assert _check(f"K 4096 k-step {ks} dt {dt} N {N}", out, ref, bound) <= 1.0


@pytest.mark.parametrize("dt", DTS)
def test_medium_long_hook_k3072_equals_dec_linear(hip, dt):
    """K = 3072 runs the same kernel through either hook: equal bits, one and two column tiles."""
    wt = _wt()
    K = 3072
    r = np.random.default_rng(K + dt)
    for N, B in ((768, 17), (1040, 5)):
        x = _round(r.standard_normal((B, K)) * 0.5, dt).astype(np.float32)
        W = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
        bias = (0.1 * r.standard_normal(N)).astype(np.float32)
        res = (2 * r.standard_normal((B, N))).astype(np.float32)
        kw = dict(residual=res, in_place=True, dtype=dt, x_is_t=True)
        np.testing.assert_array_equal(_long(x, W, bias, **kw), wt.dec_linear(x, W, bias, **kw))


def test_medium_long_hook_refusals(hip):
    """wm_op_dec_linear_long takes K = 3072 and 4096 only and no LayerNorm prologue; wm_op_dec_linear goes on refusing K = 4096."""
    from whisper_mojo_amd import _lib
    wt = _wt()
    for K in (2048, 4128, 1024):
        with pytest.raises(_lib.WhisperMiError):
            _long(np.zeros((2, K), np.float32), np.zeros((16, K), np.float32))
    for K in (3072, 4096):
        ln = (np.ones(K, np.float32), np.zeros(K, np.float32))
        with pytest.raises(_lib.WhisperMiError):
            _long(np.zeros((2, K), np.float32), np.zeros((16, K), np.float32), ln=ln)
    with pytest.raises(_lib.WhisperMiError):
        wt.dec_linear(np.zeros((2, 4096), np.float32), np.zeros((16, 4096), np.float32))


# ---- the rest of a d = 1024 step ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind,Bs", [("fc1", (1, 64)), ("qkv", (5, 128)), ("attn_out", (5, 64)), ("crossq", (1, 128))])
def test_medium_dec_linear_vs_float64(hip, dt, kind, Bs):
    """The K = 1024 launches of a d_model 1024 decode step, as decode_core wires them (tests/test_gpu_decode_layer.py's _run_case):
    fc1 is (N, K) = (4096, 1024) with GELU, qkv (3072, 1024) with the cache append, attn_out and crossq (1024, 1024)."""
    extra = {"qkv": dt, "fc1": 0}.get(kind)
    for B in Bs:
        worst = _run_case(dt, kind, D, B, extra, SPLIT[dt], seed=7919 * D + 31 * B + 5 * dt + len(kind))
        assert worst <= 1.0


@pytest.mark.parametrize("dt", DTS)
def test_medium_qkv_prefill_rows(hip, dt):
    """Position-major prefill rows, P = 3 positions x 5 utterances from cache length 2: q against float64, K / V rows at (utterance,
    length + position), every other cache row untouched."""
    wt = _wt()
    P, n_utt, length, rows_cap = 3, 5, 2, 6
    B = P * n_utt
    r = np.random.default_rng(D + dt)
    x, g, b, W = _decoder_like(r, B, D, 3 * D, dt, scale=1.0 / np.sqrt(D))
    bias = (0.1 * r.standard_normal(3 * D)).astype(np.float32)
    k0 = np.full((n_utt, rows_cap, D), SENT, np.float32)
    q, kc, vc = wt.dec_linear(x, W, bias, ln=(g, b), dtype=dt, kv=(k0, k0), kv_dtype=DT_F32, kv_B=n_utt, len=length)
    ref, bound = linear_ref(x, W, bias, dt, ln=(g, b), depth=ln_depth(SPLIT[dt]))
    assert _check(f"prefill q dt {dt}", q, ref[:, :D], bound[:, :D]) <= 1.0
    touched = np.zeros((n_utt, rows_cap), bool)
    for row in range(B):
        u, cr = row % n_utt, length + row // n_utt
        touched[u, cr] = True
        assert _check(f"prefill k dt {dt}", kc[u, cr], ref[row, D:2 * D], bound[row, D:2 * D]) <= 1.0
        assert _check(f"prefill v dt {dt}", vc[u, cr], ref[row, 2 * D:], bound[row, 2 * D:]) <= 1.0
    assert (kc[~touched] == SENT).all() and (vc[~touched] == SENT).all()


@pytest.mark.parametrize("dt", DTS)
def test_medium_crossq_capture_both_forms(hip, dt):
    """Cross-q (1024, 1024) with the alignment-head capture, by step and by row map.  Heads 15 (the last of 16), 0 and 9 are
    selected; the output is unchanged and cap holds its sentinel wherever nothing was selected."""
    wt = _wt()
    B = 5
    r = np.random.default_rng(D + 3 * dt)
    x, g, b, W = _decoder_like(r, B, D, D, dt, scale=1.0 / np.sqrt(D))
    bias = (0.1 * r.standard_normal(D)).astype(np.float32)
    plain = wt.dec_linear(x, W, bias, ln=(g, b), dtype=dt)
    ref, bound = linear_ref(x, W, bias, dt, ln=(g, b), depth=ln_depth(SPLIT[dt]))
    assert _check(f"crossq dt {dt}", plain, ref, bound) <= 1.0
    sel = np.full(32, -1, np.int8)
    heads = [15, 0, 9]
    for k, h in enumerate(heads):
        sel[h] = k
    step0, steps = 4, 3
    for length in (3, 5, 7):
        cap0 = np.full((B, steps, len(heads) + 1, 64), SENT, np.float32)
        out, cap = wt.dec_linear(x, W, bias, ln=(g, b), dtype=dt, cap=cap0, cap_sel=sel, cap_step0=step0, len=length)
        np.testing.assert_array_equal(out, plain)
        want = cap0.copy()
        if 0 <= length - step0 < steps:
            for k, h in enumerate(heads):
                want[:, length - step0, k] = plain[:, 64 * h:64 * h + 64]
        np.testing.assert_array_equal(cap, want)
    import ctypes as C
    from whisper_mojo_amd import _lib
    fp = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))
    cap_dst = B + 2
    cmap = r.permutation(cap_dst)[:B].astype(np.int32)
    cmap[2] = -1
    cap = np.full((cap_dst, len(heads) + 1, 64), SENT, np.float32)
    out = np.zeros((B, D), np.float32)
    _lib.check(_lib.lib().wm_op_dec_linear_capmap(fp(out), fp(cap), fp(x), fp(W), fp(bias), fp(g), fp(b), B, D, D, dt,
                                                  sel.ctypes.data_as(C.POINTER(C.c_int8)), len(heads) + 1,
                                                  cmap.ctypes.data_as(C.POINTER(C.c_int32)), cap_dst))
    np.testing.assert_array_equal(out, plain)
    want = np.full_like(cap, SENT)
    for row in range(B):
        if cmap[row] >= 0:
            for k, h in enumerate(heads):
                want[cmap[row], k] = plain[row, 64 * h:64 * h + 64]
    np.testing.assert_array_equal(cap, want)


# ---- logits + fused argmax ------------------------------------------------------------------------------------------------------

# d_model 1024 runs 32 rows per workgroup for every operand type (dec_logits_kernel<TW,8,2>; <TW,8,1> up to 16 rows): 16 | 17 is the
# change of kernel, 32 | 33, 64 | 65 and 128 are row-block boundaries.  The full vocabulary for rows 1 and 65 only.
LOGITS_CASES = [(dt, B, 1000) for dt in DTS for B in (1, 16, 17, 32, 33, 64, 65, 128)] + [(dt, B, 51865) for dt in DTS for B in (1, 65)]


@pytest.mark.parametrize("dt,B,N", LOGITS_CASES)
def test_medium_logits_argmax_logprob_vs_float64(hip, dt, B, N):
    """Every logit within the arithmetic's bound of float64 (_logits_ref: exact-fp32 accumulation of K terms for fp32 weights), the
    fused argmax exact on the kernel's own logits; with log-probs: logits and ids bitwise those of the plain launch, the log-prob
    within the bound of tests/test_gpu_logits_lp.py, suppress mask on; and with the timestamp rules on (forced and mixed rows)."""
    r = np.random.default_rng(31 * D + 7 * B + N + dt)
    x, g, b, emb = _decoder_like(r, B, D, N, dt)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    logits, ids = _call_logits(x, g, b, emb, dt)
    ratio = np.abs(logits - ref) / bound
    print(f"logits dt {dt} B {B} N {N}: worst err/bound {ratio.max():.3g}, max |err| {np.abs(logits - ref).max():.3g}")
    assert np.isfinite(logits).all() and ratio.max() <= 1.0
    np.testing.assert_array_equal(ids, _lowest_argmax(logits))
    mask = np.zeros(N, np.float32)
    mask[[3, N // 2, N - 1]] = -np.inf
    tb = _tb(N)
    lg, li, lp = _lp(x, g, b, emb, dt, mask=mask)
    np.testing.assert_array_equal(lg, logits)
    np.testing.assert_array_equal(li, _lowest_argmax(logits + mask))
    _lp_check(f"dt {dt} B {B} N {N} rules off", lp, ref, bound, mask, None, li, tb, N)
    seen = set()
    for kinds in ([b_ % 2 == 0 for b_ in range(B)], [b_ % 2 == 1 for b_ in range(B)])[:2 if B == 1 else 1]:
        rg = _ranges(B, N, tb, kinds, ref, mask)
        lg, li, lp = _lp(x, g, b, emb, dt, mask=mask, ranges=rg, timestamp_begin=tb)
        pg, pi = _call_logits(x, g, b, emb, dt, mask=mask, ranges=rg, timestamp_begin=tb)
        np.testing.assert_array_equal(lg, logits)
        np.testing.assert_array_equal(pg, logits)
        np.testing.assert_array_equal(li, pi)
        _lp_check(f"dt {dt} B {B} N {N} rules on", lp, ref, bound, mask, rg, li, tb, N)
        seen |= {"forced" if i >= tb else "mixed" for i in li}
    assert seen == {"forced", "mixed"}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B", [5, 33])
def test_medium_logits_one_kpanel_carries_the_operand(hip, dt, B):
    """LayerNorm gamma and beta are zero outside ONE 128-column k-panel, so the normalised row the MFMAs receive is nonzero in that
    panel alone, for each of the 8 panels: a panel read at another's offset, dropped or doubled moves every logit by O(1)."""
    N = 1000
    r = np.random.default_rng(D + B + dt)
    x, g0, b0, emb = _decoder_like(r, B, D, N, dt)
    emb = (emb * np.float32(np.sqrt(8))).astype(np.float32)  # one panel carries what eight did
    for panel in range(D // 128):
        g, b = np.zeros_like(g0), np.zeros_like(b0)
        sl = slice(128 * panel, 128 * panel + 128)
        g[sl], b[sl] = g0[sl], b0[sl]
        ref, bound = _logits_ref(x, g, b, emb, dt)
        assert np.abs(ref).mean() > 0.1
        logits, ids = _call_logits(x, g, b, emb, dt)
        ratio = np.abs(logits - ref) / bound
        print(f"logits panel {panel} dt {dt} B {B}: worst err/bound {ratio.max():.3g}")
        assert np.isfinite(logits).all() and ratio.max() <= 1.0
        np.testing.assert_array_equal(ids, _lowest_argmax(logits))


@pytest.mark.parametrize("dt,B,N", [(DT_F32, 40, 51865), (DT_BF16, 16, 51865), (DT_F16, 65, 1000), (DT_F32, 128, 1000)])
def test_medium_argmax_ties(hip, dt, B, N):
    """Duplicate embedding rows tie at every reduction boundary of the fused argmax (tests/test_gpu_decode_ops.py's _tie_columns) and
    at the first (0, 1), a middle and the last (N - 2, N - 1) columns: the lowest id wins; -inf on it moves the pick to the higher."""
    r = np.random.default_rng(31 * D + N + dt)
    x, g, b, emb = _decoder_like(r, B, D, N, dt)
    a = _ln64(x, g, b)
    pairs = [(0, 1), (N // 2, N // 2 + 1), (N - 2, N - 1)] + _tie_columns(N)
    rows, used = {}, set()
    for lo, hi in pairs:
        row = len(rows)
        if row >= B or lo in used or hi in used:
            continue
        used |= {lo, hi}
        d = a[row] / np.linalg.norm(a[row])
        emb[lo] = emb[hi] = (d * 0.04 * np.sqrt(D) * 6).astype(np.float32)
        rows[row] = (lo, hi)
    assert {(0, 1), (N - 2, N - 1)} <= set(rows.values())
    logits, ids = _call_logits(x, g, b, emb, dt)
    np.testing.assert_array_equal(ids, _lowest_argmax(logits))
    for row, (lo, hi) in rows.items():
        assert logits[row, lo] == logits[row, hi] == logits[row].max() and ids[row] == lo, (row, lo, hi, ids[row])
    mask = np.zeros(N, np.float32)
    for lo, _ in rows.values():
        mask[lo] = -np.inf
    lm, im = _call_logits(x, g, b, emb, dt, mask=mask)
    np.testing.assert_array_equal(lm, logits)
    for row, (lo, hi) in rows.items():
        assert im[row] == hi, (row, lo, hi, im[row])


@pytest.mark.parametrize("dt", DTS)
def test_medium_logits_rows_independent_of_batch(hip, dt):
    """Bitwise: a row's logits, id and log-prob alone (one row block of 16), in a 32-row block, in 64 rows and in 128."""
    N = 1000
    r = np.random.default_rng(D + dt)
    x, g, b, emb = _decoder_like(r, 128, D, N, dt)
    big, ib, lb = _lp(x, g, b, emb, dt)
    for s, n in ((0, 1), (37, 1), (127, 1), (0, 32), (16, 17), (64, 64), (30, 3)):
        lg, li, lp = _lp(x[s:s + n], g, b, emb, dt)
        np.testing.assert_array_equal(lg, big[s:s + n])
        np.testing.assert_array_equal(li, ib[s:s + n])
        np.testing.assert_array_equal(lp, lb[s:s + n])


# ---- score sweep ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt,M,N", [(DT_F32, 1, 1000), (DT_F32, 15, 69), (DT_F32, 65, 1000), (DT_F32, 129, 51865), (DT_BF16, 17, 1000),
                                    (DT_BF16, 64, 1000), (DT_BF16, 129, 69), (DT_F16, 63, 1000), (DT_F16, 130, 69), (DT_F16, 127, 51865)])
def test_medium_score_vs_float64(hip, dt, M, N):
    """Log-sum-exp, target gather and arg-max of the score sweep at K = 1024, K walked in two halves (tests/test_gpu_score_op.py's
    bound and targets): ragged row counts around the 16-row wave tile, 64 and the 128-row block."""
    r = np.random.default_rng(17 * D + 5 * M + N + dt)
    x, g, b, emb = _decoder_like(r, M, D, N, dt)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    tg = _targets(r, ref, N)
    lp, top = _score(x, g, b, emb, tg, dt)
    _score_check(f"score dt {dt} K {D} M {M} N {N}", lp, top, ref, bound, tg, N, dt)


@pytest.mark.parametrize("dt,N", [(DT_F32, 1000), (DT_BF16, 51865), (DT_F16, 1000)])
def test_medium_score_targets_on_part_edges_and_ties(hip, dt, N):
    """Targets in the first and the last column tile of a vocabulary part (first and last column of each), for the first, a middle
    and the last part; and the arg-max with ties: duplicate embedding rows on both sides of a part boundary and inside one tile,
    aligned with the row so that they are its maximum — the lowest id wins."""
    parts, T = _geometry(N, dt)
    edges = []
    for part in sorted({0, parts // 2, parts - 1}):
        lo, hi = part * T * 16, min(N, (part + 1) * T * 16)
        edges += [lo, min(lo + 15, hi - 1), max(lo, (hi - 1) // 16 * 16), hi - 1]
    M = len(edges) + 3
    r = np.random.default_rng(N + dt)
    x, g, b, emb = _decoder_like(r, M, D, N, dt)
    a = _ln64(x, g, b)
    cut = (parts // 2) * T * 16 if parts > 1 else 16
    ties = [(cut - 1, cut), (5, 9), (N - 2, N - 1)]
    for i, (lo, hi) in enumerate(ties):
        row = len(edges) + i
        d = a[row] / np.linalg.norm(a[row])
        emb[lo] = emb[hi] = (d * 0.04 * np.sqrt(D) * 6).astype(np.float32)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    tg = np.array(edges + [hi for _, hi in ties], np.int32)
    lp, top = _score(x, g, b, emb, tg, dt)
    _score_check(f"score edges dt {dt} N {N}", lp, top, ref, bound, tg, N, dt)
    for i, (lo, hi) in enumerate(ties):
        row = len(edges) + i
        assert np.argmax(ref[row]) in (lo, hi) and top[row] == lo, (row, lo, hi, top[row])


@pytest.mark.parametrize("dt", DTS)
def test_medium_score_row_alone_equals_row_in_batch(hip, dt):
    """Bitwise: a row scored alone, inside one block of 128 rows and inside 200."""
    N = 1000
    r = np.random.default_rng(D + dt)
    x, g, b, emb = _decoder_like(r, 200, D, N, dt)
    tg = r.integers(0, N, 200).astype(np.int32)
    lp, top = _score(x, g, b, emb, tg, dt)
    l128, t128 = _score(x[:128], g, b, emb, tg[:128], dt)
    np.testing.assert_array_equal(l128, lp[:128])
    np.testing.assert_array_equal(t128, top[:128])
    for row in (0, 15, 16, 63, 64, 127, 128, 199):
        l1, t1 = _score(x[row:row + 1], g, b, emb, tg[row:row + 1], dt)
        assert l1[0] == lp[row] and t1[0] == top[row], (row, l1[0], lp[row])


# ---- no_speech, lang_detect, cached attention -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTS)
def test_medium_no_speech_and_lang_detect(hip, dt):
    """The no-speech probe and the language kernel at K = 1024 against float64 softmaxes of _logits_ref's logits (B = 5 takes the
    16-row logits kernel, B = 33 two 32-row blocks)."""
    wt = _wt()
    N = 1000
    for B in (5, 33):
        r = np.random.default_rng(2 * D + dt + B)
        x, g, b, emb = _decoder_like(r, B, D, N, dt)
        ref, bound = _logits_ref(x, g, b, emb, dt)
        token = 777
        prob, lse = wt.no_speech(x, g, b, emb, token, dtype=dt)
        m = ref.max(1)
        lse64 = m + np.log(np.exp(ref - m[:, None]).sum(1))
        tol = 2 * bound.max(1) + 1e-5
        assert (np.abs(lse - lse64) <= tol).all()
        assert (np.abs(np.log(prob) - (ref[:, token] - lse64)) <= tol).all()
        lang_ids = np.arange(900, 999, dtype=np.int32)
        ids, probs = wt.lang_detect(x, g, b, emb, lang_ids, dtype=dt)
        sub = ref[:, lang_ids]
        p64 = np.exp(sub - sub.max(1, keepdims=True))
        p64 /= p64.sum(1, keepdims=True)
        assert (np.abs(probs - p64) <= 2 * tol[:, None] + 1e-6).all()
        srt = np.sort(sub, 1)
        clear = srt[:, -1] - srt[:, -2] > 2 * bound.max(1)
        np.testing.assert_array_equal(ids[clear], lang_ids[np.argmax(sub, 1)][clear])


@pytest.mark.parametrize("kvdt", [DT_F32, DT_BF16])
def test_medium_attention_cached_16_heads(hip, kvdt):
    """wt.attention_cached at 16 heads — with fp32 K/V a cache row takes 256 lanes, the launcher's limit — at key counts 1, 5 and
    104, cache rows past the count holding NaN; the tolerance of tests/test_gpu_decode_layer.py."""
    wt = _wt()
    B = 3
    for i, t in enumerate((1, 5, 104)):
        r = np.random.default_rng(1000 * H + 10 * t + kvdt)
        kind = ("random", "dominant", "random")[i]
        odt = (DT_F32, kvdt, DT_F32)[i]
        q, k, v = _attn_inputs(r, B, t, H, kvdt, kind, j_dom=t - 1)
        pad = np.full((B, 3, 64 * H), np.nan, np.float32)
        out = np.zeros_like(q)
        wt.attention_cached(out, q, np.concatenate([k, pad], 1), np.concatenate([v, pad], 1), H, kv_dtype=kvdt, out_dtype=odt, len=t - 1)
        _attn_check(f"H {H} kv {kvdt} t {t} {kind} out {odt}", out, _attention_cached_ref(q, k, v, H), odt)
