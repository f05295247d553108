"""Op-level tests (-m gpu) of the kernels at Whisper-small's shapes (d_model 768 = 6 k-panels of 128, ffn 3072), against float64 on
the operands exactly as the kernels receive them.  References, hooks and bounds are those of tests/test_gpu_decode_layer.py
(linear_ref: accumulation depth, LayerNorm error, GELU model), tests/test_gpu_decode_ops.py (_logits_ref, the tie construction, the
timestamp decision), tests/test_gpu_logits_lp.py (the log-prob bound) and tests/test_gpu_score_op.py (the score bound): imported,
not restated, no new constant.  (linear_ref's accumulation depth min(K, 128) + 16 was reasoned for chains of <= 4 k-steps per
wave; the K = 3072 form chains 6, so the imported bound is the tighter of the two and is kept.  Measured on MI355X at K = 3072:
worst err / bound 0.0047 (fp32), 0.0031 (bf16), 0.0045 (f16) for fc2, 0.03 with one k-step carrying the weight, 0.12 through the GELU.)

  * dec_linear at (N, K) = (768, 3072) [two groups of three k-steps per wave, DESIGN §24], (3072, 768), (2304, 768) with the cache
    append, (768, 768) with both capture forms; B in {1, 5, 64, 128}; position-major prefill rows (P = 3); fp32 / bf16 / f16;
  * one k-step carrying all the weight: a dropped or doubled k-step moves the result by O(1);
  * logits + fused argmax at K = 768: N in {1000, 51865}, rows in {1, 64, 65, 128}, with and without log-probs, ties, suppress
    mask and timestamp rules;
  * the score sweep at K = 768: ragged row counts around the 64-row tile and the 128-row block;
  * refused shapes: K = 3104 and K = 2176."""
import numpy as np
import pytest

from test_gpu_decode_layer import SENT, _check, _run_case, _wt, linear_ref
from test_gpu_decode_ops import (DT_BF16, DT_F16, DT_F32, _call_logits, _ct, _decoder_like, _ln64, _logits_ref, _lowest_argmax, _round,
                                 _tie_columns, hip)  # noqa: F401
from test_gpu_logits_lp import _check as _lp_check, _lp, _ranges, _tb
from test_gpu_score_op import _check as _score_check, _score, _targets

pytestmark = pytest.mark.gpu

D = 768
DTS = (DT_F32, DT_BF16, DT_F16)
SPLIT = {DT_F32: (12, 2), DT_BF16: (8, 3), DT_F16: (8, 3)}  # (waves, k-steps per wave) of K = 768, as dec_linear_waves splits it


# ---- dec_linear -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind,Bs", [("fc2", (1, 5, 64, 128)), ("fc1", (1, 64)), ("qkv", (5, 128)), ("attn_out", (5, 64)),
                                     ("crossq", (1, 128))])
def test_small_dec_linear_vs_float64(hip, dt, kind, Bs):
    """The launches of a d_model 768 decode step, as decode_core wires them (tests/test_gpu_decode_layer.py's _run_case: LayerNorm
    prologue, bias / GELU / residual-in-place epilogues, 16-bit stores, the QKV cache append): fc2 is (N, K) = (768, 3072), fc1
    (3072, 768), qkv (2304, 768), attn_out and crossq (768, 768)."""
    extra = {"qkv": dt, "fc1": 0}.get(kind)
    for B in Bs:
        worst = _run_case(dt, kind, D, B, extra, SPLIT[dt], seed=7919 * D + 31 * B + 5 * dt + len(kind))
        assert worst <= 1.0


@pytest.mark.parametrize("dt", DTS)
def test_small_qkv_prefill_rows(hip, dt):
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
    ref, bound = linear_ref(x, W, bias, dt, ln=(g, b), depth=8 * SPLIT[dt][1] + 2 + SPLIT[dt][0])
    assert _check(f"prefill q dt {dt}", q, ref[:, :D], bound[:, :D]) <= 1.0
    touched = np.zeros((n_utt, rows_cap), bool)
    for row in range(B):
        u, cr = row % n_utt, length + row // n_utt
        touched[u, cr] = True
        assert _check(f"prefill k dt {dt}", kc[u, cr], ref[row, D:2 * D], bound[row, D:2 * D]) <= 1.0
        assert _check(f"prefill v dt {dt}", vc[u, cr], ref[row, 2 * D:], bound[row, 2 * D:]) <= 1.0
    assert (kc[~touched] == SENT).all() and (vc[~touched] == SENT).all()


@pytest.mark.parametrize("dt", DTS)
def test_small_crossq_capture_both_forms(hip, dt):
    """Cross-q (768, 768) with the alignment-head capture.  By step: cap holds the selected heads' 64 output columns at step
    len - cap_step0 and its sentinel elsewhere.  Heads 11 (the last of 12) and 0 and 7 are selected; the output is unchanged."""
    wt = _wt()
    B = 5
    r = np.random.default_rng(D + 3 * dt)
    x, g, b, W = _decoder_like(r, B, D, D, dt, scale=1.0 / np.sqrt(D))
    bias = (0.1 * r.standard_normal(D)).astype(np.float32)
    plain = wt.dec_linear(x, W, bias, ln=(g, b), dtype=dt)
    ref, bound = linear_ref(x, W, bias, dt, ln=(g, b), depth=8 * SPLIT[dt][1] + 2 + SPLIT[dt][0])
    assert _check(f"crossq dt {dt}", plain, ref, bound) <= 1.0
    sel = np.full(32, -1, np.int8)
    heads = [11, 0, 7]
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
    # by row map (wm_op_dec_linear_capmap): row r's selected heads go to cap row cmap[r]; -1 stores nothing; two rows nobody maps to
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


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N", [768, 1040])
def test_small_k3072_one_kstep_carries_the_weight(hip, dt, N):
    """K = 3072: all of W sits in ONE 32-column k-step — the last (95: wave 15, second group, third step), one in the middle of a
    wave's loop (52 = 4 + 16·3: wave 4, the second group's first step), the first of the second group's (48) and k-step 0.  A dropped
    k-step gives bias + residual alone, a doubled one twice the product: either is O(1) against a bound of ~1e-5.  N = 1040 takes the
    two-column-tile form."""
    wt = _wt()
    K, B = 3072, 5
    r = np.random.default_rng(N + dt)
    x = _round(r.standard_normal((B, K)) * 0.5, dt).astype(np.float32)
    bias = (0.1 * r.standard_normal(N)).astype(np.float32)
    res = (2 * r.standard_normal((B, N))).astype(np.float32)
    for ks in (95, 52, 48, 0):
        W = np.zeros((N, K), np.float32)
        W[:, 32 * ks:32 * ks + 32] = r.standard_normal((N, 32)) / np.sqrt(32)
        out = wt.dec_linear(x, W, bias, residual=res, in_place=True, dtype=dt, x_is_t=True)
        ref, bound = linear_ref(x, W, bias, dt, residual=res)
        assert np.abs(ref - (bias + res.astype(np.float64))).mean() > 0.1  # the k-step's product is O(1)
        assert _check(f"K 3072 k-step {ks} dt {dt} N {N}", out, ref, bound) <= 1.0


@pytest.mark.parametrize("dt", DTS)
def test_small_k3072_fp32_activations_and_wide(hip, dt):
    """K = 3072 with fp32 activation rows (the kernel rounds them itself) and N = 1040 (two column tiles per workgroup), GELU input
    form: act on the pre-activation, both modes; the same rows handed over in operand dtype give the same bits."""
    wt = _wt()
    K, N, B = 3072, 1040, 17
    r = np.random.default_rng(K + N + dt)
    x = _round(r.standard_normal((B, K)), dt).astype(np.float32)
    W = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = (0.1 * r.standard_normal(N)).astype(np.float32)
    for mode in (0, 1):
        out = wt.dec_linear(x, W, bias, dtype=dt, act=True, gelu_mode=mode)
        ref, bound = linear_ref(x, W, bias, dt, act=True, gelu_mode=mode)
        assert _check(f"K 3072 wide gelu {mode} dt {dt}", out, ref, bound) <= 1.0
        if dt != DT_F32:
            np.testing.assert_array_equal(out, wt.dec_linear(x, W, bias, dtype=dt, act=True, gelu_mode=mode, x_is_t=True))


def test_small_refused_k(hip):
    """K = 3104 (97 k-steps) and K = 2176 (68 = 17 x 4) are no shape of the skinny linear: WM_E_ARG, the output untouched."""
    from whisper_mojo_amd import _lib
    wt = _wt()
    for K in (3104, 2176):
        with pytest.raises(_lib.WhisperMiError):
            wt.dec_linear(np.zeros((2, K), np.float32), np.zeros((16, K), np.float32))
    ln = (np.ones(3072, np.float32), np.zeros(3072, np.float32))
    with pytest.raises(_lib.WhisperMiError):  # no LayerNorm prologue at K = 3072
        wt.dec_linear(np.zeros((2, 3072), np.float32), np.zeros((16, 3072), np.float32), ln=ln)


# ---- logits + fused argmax ------------------------------------------------------------------------------------------------------

# fp32 runs 32 rows per workgroup at d_model 768 (dec_logits_kernel<float,6,1|2>), 16-bit 64 (<TW,6,1|4>); 65 and 128 rows are more
# row blocks of the same kernels.  The full vocabulary for every row count in fp32 (the new tiling) and once per 16-bit type.
LOGITS_CASES = [(dt, B, 1000) for dt in DTS for B in (1, 64, 65, 128)] + \
    [(DT_F32, 1, 51865), (DT_F32, 64, 51865), (DT_F32, 65, 51865), (DT_F32, 128, 51865), (DT_BF16, 64, 51865), (DT_F16, 128, 51865),
     (DT_BF16, 1, 51865), (DT_F16, 65, 51865)]


@pytest.mark.parametrize("dt,B,N", LOGITS_CASES)
def test_small_logits_argmax_logprob_vs_float64(hip, dt, B, N):
    """Every logit within the arithmetic's bound of float64 (_logits_ref: exact-fp32 accumulation of K terms for fp32 weights, not the
    3 x bf16 split), the fused argmax exact on the kernel's own logits; with log-probs: logits and ids bitwise those of the plain
    launch, the log-prob within the bound of tests/test_gpu_logits_lp.py, suppress mask on; and with the timestamp rules on (forced
    and mixed rows)."""
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


@pytest.mark.parametrize("dt,B,N", [(DT_F32, 40, 51865), (DT_BF16, 16, 51865), (DT_F16, 65, 1000), (DT_F32, 128, 1000)])
def test_small_argmax_ties(hip, dt, B, N):
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
def test_small_logits_rows_independent_of_batch(hip, dt):
    """Bitwise: a row's logits, id and log-prob alone (one row block of 16), in 64 rows and in 128 (the coalesced state)."""
    N = 1000
    r = np.random.default_rng(D + dt)
    x, g, b, emb = _decoder_like(r, 128, D, N, dt)
    big, ib, lb = _lp(x, g, b, emb, dt)
    for s, n in ((0, 1), (37, 1), (127, 1), (0, 64), (64, 64), (30, 3)):
        lg, li, lp = _lp(x[s:s + n], g, b, emb, dt)
        np.testing.assert_array_equal(lg, big[s:s + n])
        np.testing.assert_array_equal(li, ib[s:s + n])
        np.testing.assert_array_equal(lp, lb[s:s + n])


# ---- score sweep ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt,M,N", [(DT_F32, 1, 1000), (DT_F32, 63, 69), (DT_F32, 65, 1000), (DT_F32, 129, 51865), (DT_BF16, 64, 1000),
                                    (DT_BF16, 129, 69), (DT_F16, 63, 1000), (DT_F16, 130, 69)])
def test_small_score_vs_float64(hip, dt, M, N):
    """Log-sum-exp, target gather and arg-max of the score sweep at K = 768 (tests/test_gpu_score_op.py's bound and targets)."""
    r = np.random.default_rng(17 * D + 5 * M + N + dt)
    x, g, b, emb = _decoder_like(r, M, D, N, dt)
    ref, bound = _logits_ref(x, g, b, emb, dt)
    tg = _targets(r, ref, N)
    lp, top = _score(x, g, b, emb, tg, dt)
    _score_check(f"score dt {dt} K {D} M {M} N {N}", lp, top, ref, bound, tg, N, dt)


@pytest.mark.parametrize("dt", DTS)
def test_small_score_row_alone_equals_row_in_batch(hip, dt):
    N = 1000
    r = np.random.default_rng(D + dt)
    x, g, b, emb = _decoder_like(r, 200, D, N, dt)
    tg = r.integers(0, N, 200).astype(np.int32)
    lp, top = _score(x, g, b, emb, tg, dt)
    for row in (0, 63, 64, 127, 128, 199):
        l1, t1 = _score(x[row:row + 1], g, b, emb, tg[row:row + 1], dt)
        assert l1[0] == lp[row] and t1[0] == top[row], (row, l1[0], lp[row])


@pytest.mark.parametrize("dt", DTS)
def test_small_no_speech_and_lang_detect(hip, dt):
    """The no-speech probe and the language kernel at K = 768 against float64 softmaxes of _logits_ref's logits."""
    wt = _wt()
    N, B = 1000, 5
    r = np.random.default_rng(2 * D + dt)
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
