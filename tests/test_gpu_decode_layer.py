"""Op-level tests (-m gpu) of the decode step's per-layer kernels, against float64 on the operands exactly as the kernels receive
them and through bitwise properties the code's comments claim:

  * dec_linear_kernel (wm_op_dec_linear: one launch_dec_linear wired as decode_core wires it): LayerNorm prologue, operand-dtype
    activations, bias / GELU / residual-in-place epilogues, the 16-bit store, the QKV cache append (step and prefill mapping) and
    the alignment-head capture, for every template instance the release dispatch reaches;
  * attn_decode_kernel / attn_combine_kernel (wm_op_attention_cached): 1..16 heads, key counts on the sweep's boundaries, the
    causal prefill form, the four-position cross-attention prefill, 16-bit outputs.

The float64 references and bounds live in this file; tests/test_decode_ops_ref.py pins them on the CPU (oracle compositions, the
prefill row mapping, a numpy emulation of the kernel's summation order inside the bound and perturbed emulations outside it)."""
import numpy as np
import pytest

from test_gpu_decode_ops import DT_BF16, DT_F16, DT_F32, U, _decoder_like, _ln64, _ln_err, _round, _ulp_tw
from test_gpu_parity import _attention_cached_ref

pytestmark = pytest.mark.gpu

SENT = -16384.0  # cache / capture sentinel: exact in fp32, bf16 and f16


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()  # raises if the HIP library is missing: no fallback
    import whisper_mojo_amd as pkg
    return pkg


# ---- dec_linear: reference and error bound ------------------------------------------------------------------------------------

# The kernel's LayerNorm statistics: a lane sums its 8·KPW values in sequence, two butterfly adds, then the nw wave partials in
# sequence: depth 8·KPW + 2 + nw, with (nw, KPW) as each case names them; the deepest split the kernel admits is the default.
LN_DEPTH = 8 * 4 + 2 + 16


def ln_depth(split):
    nw, kpw = split
    return 8 * kpw + 2 + nw


def ln_err_expected(x, g, b, depth=LN_DEPTH, draws=8, factor=4.0):
    """Per-element |fp32 LayerNorm - float64 LayerNorm| that a correct fp32 evaluation can be expected to stay within, capped by the
    worst-case bound _ln_err.  Reasoning: the fp32 result differs from float64 through two row-common quantities — the error of the
    mean and the relative error of rstd, both from the rounding of the two sums — and a few roundings per element (<= 4u·|y|:
    x - mean, ·rstd, ·gamma, + beta; sqrtf and the division are correctly rounded or within an ulp).  _ln_err bounds the sums'
    error by depth·u·Σ|x| (every rounding at its largest, all in one direction); with a DC offset and the one-pass variance that is
    ~100 times what roundings of random sign give, and it lets a twentieth of the 16-bit operands count as able to round the other
    way.  The realised size is measured here, independently of the kernel and of its dispatch: `draws` fp32 evaluations of the same
    formula in numpy, each with its own random summation order and fully sequential sums (depth K: deeper than any split of the
    kernel, so not smaller in distribution); the largest deviation from float64 over the draws, times `factor`, plus 4u·|y|.  With
    8 draws the largest is ~1.4 sigma of the row-common errors, so the allowance is ~5.7 sigma."""
    f = np.float32
    a = _ln64(x, g, b)
    K = x.shape[1]
    r = np.random.default_rng(K)
    xs = np.ascontiguousarray(x, f)
    dev = np.zeros_like(a)
    for _ in range(draws):
        xp = xs[:, r.permutation(K)]
        sm = np.cumsum(xp, axis=1, dtype=f)[:, -1:]
        sq = np.cumsum(xp * xp, axis=1, dtype=f)[:, -1:]
        mean = sm / f(K)
        var = sq / f(K) - mean * mean
        rstd = f(1) / np.sqrt(var + f(1e-5))
        y = ((xs - mean) * rstd) * g.astype(f) + b.astype(f)
        assert y.dtype == f
        dev = np.maximum(dev, np.abs(y.astype(np.float64) - a))
    return np.minimum(_ln_err(x, g, b, n=depth), factor * dev + 4 * U * np.abs(a))


# accumulation: products (exact in fp32 for 16-bit operands) summed in fp32.  The error of any fp32 summation is <= h·u·Σ|terms| with h
# the most additions one term passes through.  A term enters a 32-wide k-step (one 16x16x32 MFMA, or eight 16x16x4 ones) and passes
# at most 32 additions there in whatever order the hardware adds, then at most 32 per later k-step of its wave's chain (KPW <= 4),
# then the nw <= 16 wave partials: h = min(K, 128) + 16.  fp32 operands: each product may be rounded once more, or fused: h + 1.
ACC_STEP, ACC_EXTRA = 128, 16

C0 = float(np.float32(0.79788456))  # the kernel's constants, as fp32 holds them
C1 = float(np.float32(0.044715))
RS2 = float(np.float32(0.70710678118654752440))
# Accuracy of the device tanhf / erff, in ulps of their result.  No ulp table for the device math library ships with the toolkit, so
# measured once on MI355X through wm_op_gelu (another kernel, same gelu_f) with the error model of gelu64 on the grid
# linspace(-12, 12, 2^21 + 1): tanhf needs 0.500 ulp (worst at z = -5.157852), erff 0.744 ulp (at z = -1.372627).  The values used are
# twice the observed ones (the margin covers arguments between grid points); test_gelu_model_holds_on_a_dense_grid re-checks them.
GELU_T_OBSERVED = {0: 0.500, 1: 0.744}
GELU_T = {m: 2 * t for m, t in GELU_T_OBSERVED.items()}


def _erf64(a):
    import torch
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(a, np.float64))).numpy()


def _ulp32(v):
    """spacing of fp32 at |v| (normal range)"""
    _, e = np.frexp(np.abs(v))
    return np.ldexp(1.0, np.maximum(e, -125) - 24)


def gelu64(z, mode):
    """-> (g(z), g'(z), own error of the fp32 evaluation with a t-ulp tanhf / erff, per ulp t: (fixed part, part per ulp)).
    tanh form: u = C0·(z + C1·z³) — five roundings, relative 5u (the two terms have one sign) — T = tanhf(u), then 1 + T (one
    rounding, absolute u·|1 + T|: near T = -1 the sum cancels, so the error is kept absolute), 0.5·z·(1 + T) (0.5·z exact, one
    rounding).  erf form: a = z·RS2 (one rounding), E = erff(a), the rest alike."""
    z = np.asarray(z, np.float64)
    if mode == 0:
        u = C0 * (z + C1 * z ** 3)
        T = np.tanh(u)
        dT = 1 - T * T
        du = np.abs(u) * 5 * U
        gp = 0.5 * (1 + T) + 0.5 * z * dT * C0 * (1 + 3 * C1 * z * z)
    else:
        u = z * RS2
        T = _erf64(u)
        dT = 2 / np.sqrt(np.pi) * np.exp(-u * u)
        du = np.abs(u) * U
        gp = 0.5 * (1 + T) + 0.5 * z * dT * RS2
    g = 0.5 * z * (1 + T)
    fixed = 0.5 * np.abs(z) * (dT * du + U * np.abs(1 + T)) + U * np.abs(g)
    per_ulp = 0.5 * np.abs(z) * _ulp32(np.maximum(np.abs(T), 2.0 ** -100))
    return g, gp, fixed, per_ulp


def _near_midpoint(a, at, dt, e):
    """-> (a lies within e of the rounding midpoint on its side of at = round(a), the grid spacing at |at|).  The midpoint is half
    a spacing away from at; below a power of two the grid is twice as fine, so there it is a quarter of the upper spacing away.
    (_logits_ref takes the finer spacing on both sides of every value, which marks half of all operands.)"""
    ulp, ulp_below = _ulp_tw(at, dt)
    m, _ = np.frexp(np.abs(at))
    half = np.where((m == 0.5) & (np.abs(a) < np.abs(at)), 0.5 * ulp_below, 0.5 * ulp)
    return (half - np.abs(a - at)) <= e, ulp


def linear_ref(x, W, bias, dt, ln=None, act=False, gelu_mode=0, residual=None, depth=LN_DEPTH):
    """-> (ref [B, N] float64, bound [B, N]) of the kernel's fp32 result v = gelu?(a·ŵᵀ + bias) + residual, before any 16-bit store.
    ŵ = W rounded to dt.  a: the activations as the MFMA receives them — LN64(x) (rounded to dt for 16-bit operands, as the kernel
    rounds its own fp32 LayerNorm output) or x (rounded to dt: x_is_t rows already are such values, so both forms give one a).
      * accumulation: (min(K, 128) + 16 [+ 1 for fp32 operands])·u·Σ_k |a_k ŵ_k| (see ACC_STEP);
      * LayerNorm, with e = ln_err_expected (the realised fp32 error scale with a margin, never above the worst case _ln_err at the
        case's own summation depth): fp32 operands: Σ_k e_k·|ŵ_k|; 16-bit operands: one operand ulp·|ŵ_k| only where LN64(x)_k lies
        within e_k of a rounding midpoint (as _logits_ref does with the worst case);
      * bias, residual: one rounding each (u·|result|);
      * GELU: the pre-activation bound through sup |g'| over the bound's interval (|g'| + 1.2·bound: |g''| <= 1.13 for both forms),
        plus the activation's own error (gelu64) with GELU_T ulps for the device tanhf / erff."""
    K = x.shape[1]
    w = _round(W, dt)
    n = min(K, ACC_STEP) + ACC_EXTRA + (1 if dt == DT_F32 else 0)
    if ln is not None:
        a = _ln64(x, ln[0], ln[1])
        e = ln_err_expected(x, ln[0], ln[1], depth)
        if dt == DT_F32:
            v = n * U * np.abs(a) + e
        else:
            at = _round(a, dt)
            near, ulp = _near_midpoint(a, at, dt, e)
            v = n * U * np.abs(at) + near * ulp
            a = at
    else:
        a = _round(x, dt)
        v = n * U * np.abs(a)
    z = a @ w.T
    bound = v @ np.abs(w).T
    if bias is not None:
        z = z + bias.astype(np.float64)
        bound = bound + U * np.abs(z)
    if act:
        g, gp, fixed, per_ulp = gelu64(z, gelu_mode)
        bound = (np.abs(gp) + 1.2 * bound) * bound + fixed + GELU_T[gelu_mode] * per_ulp
        z = g
    if residual is not None:
        z = z + residual.astype(np.float64)
        bound = bound + U * np.abs(z)
    return z, bound


def store16(ref, bound, sdt):
    """The kernel's 16-bit store of an fp32 value within `bound` of ref -> (ref rounded to sdt, bound): zero (the same 16-bit value
    is demanded) except where a rounding midpoint lies within `bound` of ref: there the fp32 bound plus one ulp of sdt (half an
    ulp for each of the two roundings)."""
    if sdt == DT_F32:
        return ref, bound
    rt = _round(ref, sdt)
    near, ulp = _near_midpoint(ref, rt, sdt, bound)
    return rt, near * (bound + ulp)


def qkv_scatter(rows, n_utt, kv_B, length):
    """row r of a QKV launch -> (utterance, cache row): the step form (kv_B == 0) and the position-major prefill form."""
    return [(r % kv_B, length + r // kv_B) if kv_B > 0 else (r, length) for r in range(rows)]


def _wt():
    from whisper_mojo_amd import whisper_tensor as wt
    return wt


def _check(tag, got, ref, bound):
    """every element within its bound; prints worst err / bound over the elements with a non-zero bound"""
    err = np.abs(got - ref)
    assert np.isfinite(got).all()
    pos = bound > 0
    ratio = (err[pos] / bound[pos]).max() if pos.any() else 0.0
    print(f"{tag}: worst err/bound {ratio:.3g} ({int(pos.sum())}/{err.size} elements with a bound), max |err| {err.max():.3g}")
    bad = err > bound
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:4].tolist(), err[bad][:4], bound[bad][:4])
    return ratio


def _inputs(r, kind, dt, d, B):
    """Operands of one launch as decode_core makes it.  kind -> (K, N, LN?)."""
    K, N = {"qkv": (d, 3 * d), "attn_out": (d, d), "crossq": (d, d), "fc1": (d, 4 * d), "fc2": (4 * d, d)}[kind]
    bias = (0.1 * r.standard_normal(N)).astype(np.float32)
    if kind in ("qkv", "crossq", "fc1"):
        x, g, b, W = _decoder_like(r, B, K, N, dt, scale=1.0 / np.sqrt(K))
        return dict(x=x, W=W, bias=bias, ln=(g, b))
    x = _round(r.standard_normal((B, K)) * (1.0 if kind == "attn_out" else 0.5), dt).astype(np.float32)  # already operand-dtype values
    W = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    res = (2 * r.standard_normal((B, N))).astype(np.float32)
    return dict(x=x, W=W, bias=bias, residual=res)


# (dtype, launch, d_model, (B <= 16, B > 16), extra, (nw, KPW)): the kernel instance dec_linear_kernel<TW, KPW, LN, NT, XT> each launch reaches
# in a release build, (nw, KPW) as dec_linear_waves splits K (it sets the LayerNorm statistics' depth); every instance runs with both B.  extra: kv_dtype for "qkv", gelu_mode for "fc1".
# B = 256 is 4 prefill positions x 64 utterances.  fp32 operands never take XT (launch_dec_linear_t asks sizeof(TW) == 2).
LINEAR_CASES = [
    (DT_BF16, "qkv", 128, (1, 17), DT_F32, (2, 2)),        # <bf16,2,true,1>        2x2, N = 384
    (DT_BF16, "qkv", 384, (16, 256), DT_BF16, (4, 3)),     # <bf16,3,true,2>        4x3, N = 1152
    (DT_BF16, "qkv", 512, (15, 64), DT_BF16, (8, 2)),      # <bf16,2,true,2>        8x2, N = 1536
    (DT_BF16, "attn_out", 128, (16, 150), None, (2, 2)),   # <bf16,2,false,1,true>  2x2
    (DT_BF16, "attn_out", 384, (1, 64), None, (4, 3)),     # <bf16,3,false,1,true>  4x3
    (DT_BF16, "attn_out", 512, (15, 17), None, (8, 2)),    # <bf16,2,false,1,true>  8x2
    (DT_BF16, "crossq", 128, (15, 64), None, (2, 2)),      # <bf16,2,true,1>
    (DT_BF16, "crossq", 384, (16, 17), None, (4, 3)),      # <bf16,3,true,1>
    (DT_BF16, "crossq", 512, (1, 150), None, (8, 2)),      # <bf16,2,true,1>        8x2
    (DT_BF16, "fc1", 128, (16, 64), 0, (2, 2)),            # <bf16,2,true,1>        N = 512
    (DT_BF16, "fc1", 384, (15, 150), 1, (4, 3)),           # <bf16,3,true,2>        N = 1536
    (DT_BF16, "fc1", 512, (1, 17), 0, (8, 2)),             # <bf16,2,true,2>        N = 2048
    (DT_BF16, "fc2", 128, (1, 256), None, (8, 2)),         # <bf16,2,false,1,true>  8x2, K = 512
    (DT_BF16, "fc2", 384, (16, 17), None, (16, 3)),         # <bf16,3,false,1,true>  16x3, K = 1536
    (DT_BF16, "fc2", 512, (15, 64), None, (16, 4)),         # <bf16,4,false,1,true>  16x4, K = 2048
    (DT_F16, "qkv", 128, (16, 64), DT_F16, (2, 2)),        # <f16,2,true,1>
    (DT_F16, "qkv", 384, (1, 17), DT_F32, (4, 3)),         # <f16,3,true,2>
    (DT_F16, "qkv", 512, (15, 150), DT_F16, (8, 2)),       # <f16,2,true,2>
    (DT_F16, "attn_out", 128, (1, 17), None, (2, 2)),      # <f16,2,false,1,true>
    (DT_F16, "attn_out", 384, (15, 256), None, (4, 3)),    # <f16,3,false,1,true>
    (DT_F16, "attn_out", 512, (16, 64), None, (8, 2)),     # <f16,2,false,1,true>   8x2
    (DT_F16, "crossq", 128, (16, 150), None, (2, 2)),      # <f16,2,true,1>
    (DT_F16, "crossq", 384, (1, 64), None, (4, 3)),        # <f16,3,true,1>
    (DT_F16, "crossq", 512, (15, 17), None, (8, 2)),       # <f16,2,true,1>         8x2
    (DT_F16, "fc1", 128, (15, 17), 1, (2, 2)),             # <f16,2,true,1>
    (DT_F16, "fc1", 384, (1, 64), 0, (4, 3)),              # <f16,3,true,2>
    (DT_F16, "fc1", 512, (16, 150), 1, (8, 2)),            # <f16,2,true,2>
    (DT_F16, "fc2", 128, (15, 64), None, (8, 2)),          # <f16,2,false,1,true>   8x2
    (DT_F16, "fc2", 384, (1, 150), None, (16, 3)),          # <f16,3,false,1,true>   16x3
    (DT_F16, "fc2", 512, (16, 17), None, (16, 4)),          # <f16,4,false,1,true>   16x4
    (DT_F32, "qkv", 128, (15, 17), DT_F32, (4, 1)),        # <float,1,true,1>       4x1
    (DT_F32, "qkv", 384, (16, 64), DT_F32, (12, 1)),        # <float,1,true,2>       12x1
    (DT_F32, "qkv", 512, (1, 256), DT_F32, (16, 1)),        # <float,1,true,2>       16x1
    (DT_F32, "attn_out", 128, (1, 64), None, (4, 1)),      # <float,1,false,1>      4x1 (x_is_t set as proj_residual sets it: ignored)
    (DT_F32, "attn_out", 384, (15, 17), None, (12, 1)),     # <float,1,false,1>      12x1
    (DT_F32, "attn_out", 512, (16, 150), None, (16, 1)),    # <float,1,false,1>      16x1
    (DT_F32, "crossq", 128, (16, 17), None, (4, 1)),       # <float,1,true,1>
    (DT_F32, "crossq", 384, (1, 150), None, (12, 1)),       # <float,1,true,1>
    (DT_F32, "crossq", 512, (15, 64), None, (16, 1)),       # <float,1,true,1>
    (DT_F32, "fc1", 128, (1, 150), 0, (4, 1)),             # <float,1,true,1>       N = 512
    (DT_F32, "fc1", 384, (16, 17), 1, (12, 1)),             # <float,1,true,2>
    (DT_F32, "fc1", 512, (15, 64), 0, (16, 1)),             # <float,1,true,2>
    (DT_F32, "fc2", 128, (16, 17), None, (16, 1)),          # <float,1,false,1>      16x1, K = 512
    (DT_F32, "fc2", 384, (15, 64), None, (16, 3)),          # <float,3,false,1>      16x3, K = 1536
    (DT_F32, "fc2", 512, (1, 256), None, (16, 4)),          # <float,4,false,1>      16x4, K = 2048
]


def _run_case(dt, kind, d, B, extra, split, seed):
    """one launch as decode_core makes it, checked against float64 -> worst ratio"""
    wt = _wt()
    r = np.random.default_rng(seed)
    a = _inputs(r, kind, dt, d, B)
    tag = f"dt {dt} {kind} d {d} B {B}"
    depth = ln_depth(split)
    if kind == "qkv":
        kvdt = extra
        P = 4 if B == 256 else 1
        n_utt, length, rows_cap = B // P, 3, 9
        kc0 = np.full((n_utt, rows_cap, d), SENT, np.float32)
        q, kc, vc = wt.dec_linear(a["x"], a["W"], a["bias"], ln=a["ln"], dtype=dt, kv=(kc0, kc0), kv_dtype=kvdt,
                                  kv_B=n_utt if P > 1 else 0, len=length)
        ref, bound = linear_ref(a["x"], a["W"], a["bias"], dt, ln=a["ln"], depth=depth)
        worst = _check(tag + " q", q, ref[:, :d], bound[:, :d])
        where = qkv_scatter(B, n_utt, n_utt if P > 1 else 0, length)
        for name, cache, c0 in (("k", kc, d), ("v", vc, 2 * d)):
            rt, bt = store16(ref[:, c0:c0 + d], bound[:, c0:c0 + d], kvdt)
            got = np.stack([cache[u, row] for u, row in where])
            worst = max(worst, _check(f"{tag} {name} (kv dtype {kvdt})", got, rt, bt))
            untouched = np.ones(cache.shape[:2], bool)
            for u, row in where:
                untouched[u, row] = False
            assert (cache[untouched] == SENT).all()
        return worst
    if kind in ("attn_out", "fc2"):
        out = wt.dec_linear(a["x"], a["W"], a["bias"], residual=a["residual"], in_place=True, dtype=dt, x_is_t=True)
        ref, bound = linear_ref(a["x"], a["W"], a["bias"], dt, residual=a["residual"])
        return _check(tag, out, ref, bound)
    if kind == "crossq":
        out = wt.dec_linear(a["x"], a["W"], a["bias"], ln=a["ln"], dtype=dt)
        ref, bound = linear_ref(a["x"], a["W"], a["bias"], dt, ln=a["ln"], depth=depth)
        return _check(tag, out, ref, bound)
    mode = extra  # fc1: GELU, stored in operand dtype
    out = wt.dec_linear(a["x"], a["W"], a["bias"], ln=a["ln"], dtype=dt, act=True, gelu_mode=mode, out_is_t=True)
    assert np.array_equal(_round(out, dt), out)  # representable in the store dtype
    ref, bound = linear_ref(a["x"], a["W"], a["bias"], dt, ln=a["ln"], act=True, gelu_mode=mode, depth=depth)
    f32 = wt.dec_linear(a["x"], a["W"], a["bias"], ln=a["ln"], dtype=dt, act=True, gelu_mode=mode)
    worst = _check(f"{tag} gelu {mode} fp32 store", f32, ref, bound)
    np.testing.assert_array_equal(out, _round(f32, dt))  # the 16-bit store rounds the same fp32 value
    # the act = 0 output of the same launch is the pre-activation the GELU case is checked against
    pre = wt.dec_linear(a["x"], a["W"], a["bias"], ln=a["ln"], dtype=dt)
    pref, pbound = linear_ref(a["x"], a["W"], a["bias"], dt, ln=a["ln"], depth=depth)
    worst = max(worst, _check(f"{tag} pre-activation", pre, pref, pbound))
    rt, bt = store16(ref, bound, dt)
    return max(worst, _check(f"{tag} gelu {mode} store dtype {dt}", out, rt, bt))


@pytest.mark.parametrize("dt,kind,d,Bs,extra,split", LINEAR_CASES)
def test_dec_linear_vs_float64(hip, dt, kind, d, Bs, extra, split):
    """Every element of every launch a decode step makes within the arithmetic's bound of float64 (linear_ref), for both a
    one-row-block and a several-row-block batch.
    Worst err / bound measured on MI355X (fp32-level checks; min..max over the two B and the q / pre-activation / GELU sub-checks):
      qkv      d 128: bf16 0.003..0.012   f16 0.067..0.53    fp32 0.013..0.019
      qkv      d 384: bf16 0.0044..0.91   f16 0.0027..0.28   fp32 0.009..0.015
      qkv      d 512: bf16 0.0031..0.71   f16 0.29..0.36     fp32 0.0039..0.012
      attn_out d 128: bf16 0.007..0.0077  f16 0.0049..0.0088 fp32 0.0053..0.011
      attn_out d 384: bf16 0.0042..0.0051 f16 0.0045..0.0066 fp32 0.0059..0.0064
      attn_out d 512: bf16 0.0046..0.0051 f16 0.0043..0.0067 fp32 0.0054..0.0069
      crossq   d 128: bf16 0.0072..0.0081 f16 0.0075..0.38   fp32 0.013..0.015
      crossq   d 384: bf16 0.0048..0.75   f16 0.0033..0.43   fp32 0.0052..0.019
      crossq   d 512: bf16 0.003..0.75    f16 0.12..0.33     fp32 0.01..0.011
      fc1      d 128: bf16 0.0072..0.27   f16 0.0086..0.58   fp32 0.0086..0.36
      fc1      d 384: bf16 0.011..0.93    f16 0.21..0.51     fp32 0.012..0.24
      fc1      d 512: bf16 0.0047..0.69   f16 0.073..0.71    fp32 0.0081..0.32
      fc2      d 128: bf16 0.0043..0.0062 f16 0.0049..0.0056 fp32 0.0052..0.0054
      fc2      d 384: bf16 0.0036..0.0041 f16 0.0025..0.0047 fp32 0.005..0.0052
      fc2      d 512: bf16 0.0029..0.0041 f16 0.0031..0.0035 fp32 0.0031..0.0052
    Smallest of all 175 printed checks 0.0019.  The values above ~0.3 are rows in which a LayerNorm output marked as within the fp32
    error of a 16-bit midpoint did round the other way (error = that operand's ulp·|w|, most of the row's bound) or, fc1 in fp32, where
    the GELU's own error dominates near its zero crossing; the 16-bit stores (cache, out_is_t) reach 0.99: one store ulp against
    bound + one ulp.  A case is only worth running while its worst ratio stays above ~1e-3."""
    for B in Bs:
        worst = _run_case(dt, kind, d, B, extra, split, seed=7919 * d + 31 * B + 5 * dt + len(kind))
        assert worst <= 1.0


# op-only shapes the model never uses but the kernel accepts: other K splits, ragged N (the "second column tile does not exist"
# guard with LN and with GELU), XT with two column tiles.
@pytest.mark.parametrize("dt,K,N,B,flags,split", [
    (DT_BF16, 64, 37, 17, "ln", (1, 2)),  # <bf16,2,true,1>        1x2
    (DT_F32, 64, 37, 5, "ln,gelu", (2, 1)),  # <float,1,true,1>       2x1
    (DT_F16, 256, 1037, 17, "ln,gelu", (4, 2)),  # <f16,2,true,2>         4x2, the last workgroup has one column tile
    (DT_BF16, 768, 1037, 16, "ln", (8, 3)),  # <bf16,3,true,2>        8x3
    (DT_F32, 768, 37, 33, "plain", (12, 2)),  # <float,2,false,1>      12x2
    (DT_F32, 256, 1037, 3, "ln,gelu", (8, 1)),  # <float,1,true,2>       8x1
    (DT_BF16, 1024, 1037, 20, "xt,res", (16, 2)),  # <bf16,2,false,2,true>  16x2
    (DT_F16, 1024, 37, 150, "plain", (16, 2)),  # <f16,2,false,1>        16x2 (fp32 x rounded by the kernel)
    (DT_F16, 2048, 1040, 4, "xt", (16, 4)),  # <f16,4,false,2,true>   16x4
    (DT_BF16, 1536, 1037, 18, "plain,res", (16, 3)),  # <bf16,3,false,2>    16x3
])
def test_dec_linear_op_only_shapes(hip, dt, K, N, B, flags, split):
    wt = _wt()
    r = np.random.default_rng(K * 13 + N + B + dt)
    fl = set(flags.split(","))
    bias = (0.1 * r.standard_normal(N)).astype(np.float32)
    res = (2 * r.standard_normal((B, N))).astype(np.float32) if "res" in fl else None
    if "ln" in fl:
        x, g, b, W = _decoder_like(r, B, K, N, dt, scale=1.0 / np.sqrt(K))
        ln = (g, b)
    else:
        x = r.standard_normal((B, K)).astype(np.float32)
        if "xt" in fl:
            x = _round(x, dt).astype(np.float32)
        W, ln = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32), None
    for mode in ((0, 1) if "gelu" in fl else (0,)):
        out = wt.dec_linear(x, W, bias, ln=ln, residual=res, dtype=dt, x_is_t="xt" in fl, act="gelu" in fl, gelu_mode=mode)
        ref, bound = linear_ref(x, W, bias, dt, ln=ln, act="gelu" in fl, gelu_mode=mode, residual=res, depth=ln_depth(split))
        assert _check(f"dt {dt} K {K} N {N} B {B} {flags} mode {mode}", out, ref, bound) <= 1.0


def test_dec_linear_refuses_bad_arguments(hip):
    from whisper_mojo_amd import _lib
    wt = _wt()
    x, W = np.zeros((2, 128), np.float32), np.zeros((384, 128), np.float32)
    ln = (np.ones(128, np.float32), np.zeros(128, np.float32))
    cache = np.zeros((2, 4, 128), np.float32)
    E = _lib.WhisperMiError
    with pytest.raises(E):  # K = 4096 does not split over 16 waves x 4 steps
        wt.dec_linear(np.zeros((2, 4096), np.float32), np.zeros((16, 4096), np.float32))
    with pytest.raises(E):  # K not a multiple of 32
        wt.dec_linear(np.zeros((2, 48), np.float32), np.zeros((16, 48), np.float32))
    with pytest.raises(E):  # LayerNorm reads fp32 rows
        wt.dec_linear(x, W, ln=ln, dtype=DT_BF16, x_is_t=True)
    with pytest.raises(E):  # out_is_t with a residual
        wt.dec_linear(x, W, residual=np.zeros((2, 384), np.float32), dtype=DT_BF16, out_is_t=True)
    with pytest.raises(E):  # out_is_t with a cache
        wt.dec_linear(x, W, dtype=DT_BF16, out_is_t=True, kv=(cache, cache))
    with pytest.raises(E):  # the cache row len = 4 does not exist
        wt.dec_linear(x, W, kv=(cache, cache), len=4)
    with pytest.raises(E):  # prefill: 2 positions from len = 3 need 5 rows
        wt.dec_linear(x, W, kv=(cache[:1], cache[:1]), kv_B=1, len=3)
    with pytest.raises(E):  # more rows than utterances
        wt.dec_linear(np.zeros((3, 128), np.float32), W, kv=(cache, cache), len=0)
    sel = np.full(32, -1, np.int8)
    sel[1] = 2
    with pytest.raises(E):  # slot 2 of a 2-slot capture
        wt.dec_linear(x, W[:128], cap=np.zeros((2, 3, 2, 64), np.float32), cap_sel=sel)
    sel[1], sel[5] = 0, 1
    with pytest.raises(E):  # head 5 of a 2-head projection
        wt.dec_linear(x, W[:128], cap=np.zeros((2, 3, 2, 64), np.float32), cap_sel=sel)


def test_gelu_model_holds_on_a_dense_grid(hip):
    """The error model of gelu64 with GELU_T ulps for the device tanhf / erff holds for gelu_f as wm_op_gelu runs it, on
    linspace(-12, 12, 2^21 + 1); prints the ulps the observed errors need (GELU_T_OBSERVED was read off this line)."""
    wt = _wt()
    z = np.linspace(-12, 12, 2 ** 21 + 1).astype(np.float32)
    z = np.concatenate([z, np.zeros((-z.size) % 8, np.float32)])  # wm_op_gelu leaves a tail of size % 8 untouched
    for mode in (0, 1):
        got = z.copy().reshape(1, -1)
        wt.gelu(got, mode)
        g, _, fixed, per_ulp = gelu64(z.astype(np.float64), mode)
        err = np.abs(got[0] - g)
        need = np.where(err > fixed, (err - fixed) / np.maximum(per_ulp, 1e-300), 0.0)
        i = int(np.argmax(need))
        print(f"gelu mode {mode}: device {'tanhf' if mode == 0 else 'erff'} needs {need.max():.3f} ulp (at z = {z[i]:.6f}); "
              f"worst err / (fixed + GELU_T ulps) {(err / (fixed + GELU_T[mode] * per_ulp + 1e-300)).max():.3f}")
        assert (err <= fixed + GELU_T[mode] * per_ulp).all()


# ---- dec_linear: bitwise properties -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt,kind,d", [(DT_BF16, "fc1", 384), (DT_F32, "qkv", 128), (DT_F16, "fc2", 128), (DT_F32, "crossq", 512)])
def test_linear_rows_are_independent(hip, dt, kind, d):
    """A row's output is the same bits for any B and any position in the batch, and the same call twice gives the same bits."""
    wt = _wt()
    r = np.random.default_rng(d + dt)
    a = _inputs(r, kind, dt, d, 150)
    kw = dict(dtype=dt, ln=a.get("ln"), x_is_t="ln" not in a, act=kind == "fc1")

    def call(rows):
        res = a["residual"][rows] if "residual" in a else None
        return wt.dec_linear(a["x"][rows], a["W"], a["bias"], residual=res, in_place=res is not None, **kw)
    full = call(np.arange(150))
    np.testing.assert_array_equal(call(np.arange(150)), full)
    perm = r.permutation(150)
    np.testing.assert_array_equal(call(perm), full[perm])
    np.testing.assert_array_equal(call(np.arange(149, 150)), full[149:])
    np.testing.assert_array_equal(call(np.arange(20, 37)), full[20:37])


@pytest.mark.parametrize("dt,K,ln", [(DT_BF16, 384, True), (DT_F32, 512, True), (DT_F16, 128, False), (DT_F32, 128, False)])
def test_linear_two_column_tiles_equal_one(hip, dt, K, ln):
    """Columns of an N >= 1024 call (two column tiles per workgroup) equal the same columns computed from a < 1024-row slice of W
    and bias (one tile per workgroup, same k order), bit for bit."""
    wt = _wt()
    r = np.random.default_rng(K + dt)
    N, B = 1037, 19
    x, g, b, W = _decoder_like(r, B, K, N, dt, scale=1.0 / np.sqrt(K))
    bias = (0.1 * r.standard_normal(N)).astype(np.float32)
    kw = dict(dtype=dt, ln=(g, b) if ln else None, act=True)
    wide = wt.dec_linear(x, W, bias, **kw)
    for c0, c1 in ((0, 512), (496, 1008), (1008, 1037), (16, 37)):
        np.testing.assert_array_equal(wt.dec_linear(x, W[c0:c1], bias[c0:c1], **kw), wide[:, c0:c1])


@pytest.mark.parametrize("dt,K,N", [(DT_BF16, 384, 384), (DT_F16, 2048, 512), (DT_BF16, 1024, 1040)])
def test_linear_x_is_t_equals_fp32_activations(hip, dt, K, N):
    """16-bit values handed over in operand dtype give the bits the same values give as fp32 rows ("results are unchanged"); the
    residual in place equals the residual out of place."""
    wt = _wt()
    r = np.random.default_rng(K + N + dt)
    x = _round(r.standard_normal((40, K)), dt).astype(np.float32)
    W = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = r.standard_normal(N).astype(np.float32)
    res = r.standard_normal((40, N)).astype(np.float32)
    a = wt.dec_linear(x, W, bias, residual=res, in_place=True, dtype=dt, x_is_t=True)
    np.testing.assert_array_equal(a, wt.dec_linear(x, W, bias, residual=res, in_place=True, dtype=dt, x_is_t=False))
    np.testing.assert_array_equal(a, wt.dec_linear(x, W, bias, residual=res, in_place=False, dtype=dt, x_is_t=True))


@pytest.mark.parametrize("dt,kvdt,d,n_utt", [(DT_F32, DT_F32, 128, 1), (DT_BF16, DT_BF16, 384, 17), (DT_F16, DT_F32, 128, 64),
                                             (DT_F16, DT_F16, 512, 17), (DT_BF16, DT_F32, 128, 17)])
def test_qkv_append_equals_plain_linear(hip, dt, kvdt, d, n_utt):
    """q / k / v written by the cache mode equal, bit for bit, the three column blocks of the same projection run as a plain linear
    (rounded to kv_dtype for 16-bit caches); every other cache element keeps its sentinel; the prefill call writes the cache bits
    and returns the q bits of P single-position calls."""
    wt = _wt()
    r = np.random.default_rng(d + n_utt + dt + 3 * kvdt)
    rows_cap = 8
    for P in (1, 2, 4, 5):
        B = P * n_utt
        x, g, b, W = _decoder_like(r, B, d, 3 * d, dt, scale=1.0 / np.sqrt(d))
        bias = (0.1 * r.standard_normal(3 * d)).astype(np.float32)
        plain = wt.dec_linear(x, W, bias, ln=(g, b), dtype=dt)
        for length in (0, 1, rows_cap - P):
            k0 = np.full((n_utt, rows_cap, d), SENT, np.float32)
            q, kc, vc = wt.dec_linear(x, W, bias, ln=(g, b), dtype=dt, kv=(k0, k0), kv_dtype=kvdt, kv_B=n_utt if P > 1 else 0, len=length)
            np.testing.assert_array_equal(q, plain[:, :d])
            ek, ev = k0.copy(), k0.copy()
            for row, (u, cr) in enumerate(qkv_scatter(B, n_utt, n_utt if P > 1 else 0, length)):
                ek[u, cr] = _round(plain[row, d:2 * d], kvdt)
                ev[u, cr] = _round(plain[row, 2 * d:], kvdt)
            np.testing.assert_array_equal(kc, ek)
            np.testing.assert_array_equal(vc, ev)
            if P > 1 and length == 1:  # prefill equals stepwise: P single-position calls, each appending to the last one's cache
                ks, vs = k0.copy(), k0.copy()
                for p in range(P):
                    qs, ks, vs = wt.dec_linear(x[p * n_utt:(p + 1) * n_utt], W, bias, ln=(g, b), dtype=dt, kv=(ks, vs), kv_dtype=kvdt,
                                               len=length + p)
                    np.testing.assert_array_equal(qs, q[p * n_utt:(p + 1) * n_utt])
                np.testing.assert_array_equal(ks, kc)
                np.testing.assert_array_equal(vs, vc)


@pytest.mark.parametrize("dt,d,B", [(DT_F32, 128, 3), (DT_BF16, 384, 17), (DT_F16, 512, 20)])
def test_capture_window_and_heads(hip, dt, d, B):
    """cap holds exactly the output columns of the selected heads at step = len - cap_step0; one step below and one past the window,
    and for unselected heads, cap keeps its sentinel; the output itself is unchanged by the capture."""
    wt = _wt()
    r = np.random.default_rng(d + B)
    H = d // 64
    x, g, b, W = _decoder_like(r, B, d, d, dt, scale=1.0 / np.sqrt(d))
    bias = (0.1 * r.standard_normal(d)).astype(np.float32)
    plain = wt.dec_linear(x, W, bias, ln=(g, b), dtype=dt)
    sel = np.full(32, -1, np.int8)
    heads = [H - 1, 0] if H > 1 else [0]  # slot 0 = the last head, slot 1 = head 0
    n_sel = len(heads) + 1                # one slot no head writes
    for k, h in enumerate(heads):
        sel[h] = k
    step0, steps = 4, 3
    for length in (3, 4, 5, 6, 7):
        cap0 = np.full((B, steps, n_sel, 64), SENT, np.float32)
        out, cap = wt.dec_linear(x, W, bias, ln=(g, b), dtype=dt, cap=cap0, cap_sel=sel, cap_step0=step0, len=length)
        np.testing.assert_array_equal(out, plain)
        want = cap0.copy()
        if 0 <= length - step0 < steps:
            for k, h in enumerate(heads):
                want[:, length - step0, k] = plain[:, 64 * h:64 * h + 64]
        np.testing.assert_array_equal(cap, want)


# ---- attn_decode / attn_combine ------------------------------------------------------------------------------------------------

def prefill_counts(P, q_B, length):
    """key count of row p·q_B + b of a causal prefill from cache length `length`"""
    return [length + 1 + r // q_B for r in range(P * q_B)]


def _attn_inputs(r, B, t, H, kvdt, kind, j_dom=None, chunk=None):
    """q [B, d], k / v [B, t, d] (already kv-dtype values).  random; dominant: key j_dom ~12 above the rest in every head; spread: the
    keys outside chunk `chunk` (a slice) ~80 below (their chunks' partial sums underflow: attn_combine's l > 0 guard); equal: q = 0."""
    d = 64 * H
    q = (r.standard_normal((B, d)) * 1.5).astype(np.float32)
    k = r.standard_normal((B, t, d)).astype(np.float32)
    v = r.standard_normal((B, t, d)).astype(np.float32)
    if kind == "equal":
        q[:] = 0
    for h in range(H):
        sl = slice(64 * h, 64 * h + 64)
        shift = q[:, sl] / (0.125 * (q[:, sl] ** 2).sum(1, keepdims=True) + 1e-30)  # moves the score by 1
        if kind == "dominant":
            k[:, j_dom, sl] += 12 * shift
        if kind == "spread":
            out = np.ones(t, bool)
            out[chunk] = False
            k[:, out, sl] -= 80 * shift[:, None, :]
    return q, _round(k, kvdt).astype(np.float32), _round(v, kvdt).astype(np.float32)


def _attn_check(tag, got, ref, odt):
    """fp32 output: the project's 2e-5·max(1, |ref|) (test_op_attention_cached).  16-bit output: values representable in the dtype and
    equal to the rounded reference, except where that fp32 tolerance reaches a rounding midpoint of the reference (store16)."""
    tol = 2e-5 * np.maximum(1.0, np.abs(ref))
    if odt != DT_F32:
        assert np.array_equal(_round(got, odt), got)
        ref, tol = store16(ref, tol, odt)
    err = np.abs(got - ref)
    pos = tol > 0
    print(f"{tag}: max err {err.max():.3g}, worst err/tol {(err[pos] / tol[pos]).max() if pos.any() else 0.0:.3g} "
          f"({int(pos.sum())}/{err.size} elements with a tolerance)")
    assert np.isfinite(got).all() and (err <= tol).all(), (tag, np.argwhere(err > tol)[:4].tolist(), err.max())


KINDS = ("random", "dominant", "equal", "random")
ODTS = (DT_F32, DT_BF16, DT_F16)


# attn_decode_kernel<TKV, LPH, FAST, NT = false, U = 4> (the single-workgroup form): <float,16,false,false,4>, <bf16,8,true,false,4>,
# <f16,8,true,false,4>; H sets LPR = H·LPH, rps and the block size.  H = 16 with fp32 K/V is LPR = 256, the launcher's limit.
@pytest.mark.parametrize("kvdt", [DT_F32, DT_BF16, DT_F16])
@pytest.mark.parametrize("H", [1, 2, 6, 8, 16])
def test_attention_single_workgroup_boundaries(hip, H, kvdt):
    """Key counts on the sweep's own boundaries (rps rows per step, rps·U per iteration, as launch_attn_decode computes them), score
    shapes and output dtypes rotating over them; the cache rows past the key count hold NaN and must not reach the output."""
    wt = _wt()
    rps = (512 if kvdt == DT_F32 else 256) // (H * (16 if kvdt == DT_F32 else 8))
    step = rps * 4
    B = 3
    for i, t in enumerate(sorted({1, rps, rps + 1, step - 1, step, step + 1, 2 * step, 2 * step + 1, 448})):
        r = np.random.default_rng(1000 * H + 10 * t + kvdt)
        kind, odt = KINDS[i % 4] if t > 1 else "random", ODTS[(i + H) % 3]
        q, k, v = _attn_inputs(r, B, t, H, kvdt, kind, j_dom=t - 1)  # dominant: the last row slot of the last iteration
        pad = np.full((B, 3, 64 * H), np.nan, np.float32)
        out = np.zeros_like(q)
        wt.attention_cached(out, q, np.concatenate([k, pad], 1), np.concatenate([v, pad], 1), H, kv_dtype=kvdt, out_dtype=odt, len=t - 1)
        _attn_check(f"H {H} kv {kvdt} t {t} (rps {rps}) {kind} out {odt}", out, _attention_cached_ref(q, k, v, H), odt)


# attn_decode_kernel<TKV, LPH, FAST, NT = true, U = 4> + attn_combine_kernel: <float,16,false,true,4>, <bf16,8,true,true,4>,
# <f16,8,true,true,4>
@pytest.mark.parametrize("kvdt", [DT_F32, DT_BF16, DT_F16])
@pytest.mark.parametrize("H", [2, 6, 8])
def test_attention_chunked_vs_float64(hip, H, kvdt):
    wt = _wt()
    B = 2
    for i, (t, nc) in enumerate(((1500, 3), (1500, 16), (1500, 47), (300, 10))):
        chunk = -(-t // nc)
        mid = slice((nc // 2) * chunk, min(t, (nc // 2 + 1) * chunk))
        for kind in (("random", "spread") if i % 2 == 0 else ("dominant", "equal", "spread")):
            r = np.random.default_rng(100 * H + t + nc + kvdt)
            odt = ODTS[(i + H + len(kind)) % 3]
            q, k, v = _attn_inputs(r, B, t, H, kvdt, kind, j_dom=mid.start + chunk // 2, chunk=mid)
            out = np.zeros_like(q)
            wt.attention_cached(out, q, k, v, H, kv_dtype=kvdt, n_chunks=nc, out_dtype=odt)
            _attn_check(f"H {H} kv {kvdt} t {t} chunks {nc} {kind} out {odt}", out, _attention_cached_ref(q, k, v, H), odt)


def test_attention_refuses_bad_arguments(hip):
    from whisper_mojo_amd import _lib
    wt = _wt()
    E = _lib.WhisperMiError
    q, k = np.zeros((4, 17 * 64), np.float32), np.zeros((4, 8, 17 * 64), np.float32)
    with pytest.raises(E):  # 17 heads
        wt.attention_cached(np.zeros_like(q), q, k, k, 17)
    q, k = np.zeros((4, 128), np.float32), np.zeros((2, 8, 128), np.float32)
    with pytest.raises(E):  # causal prefill of 2 positions from len = 7 needs 9 rows
        wt.attention_cached(np.zeros_like(q), q, k, k, 2, q_B=2, len=7)
    with pytest.raises(E):  # nq = 4 belongs to the chunked form
        wt.attention_cached(np.zeros_like(q), q, k[:1], k[:1], 2, q_B=1, len=0, nq=4)
    with pytest.raises(E):  # prefill without a length
        wt.attention_cached(np.zeros_like(q), q, k, k, 2, q_B=2)


@pytest.mark.parametrize("kvdt,H,q_B", [(DT_F32, 2, 1), (DT_BF16, 6, 3), (DT_F16, 8, 17), (DT_F32, 16, 3), (DT_BF16, 1, 17)])
def test_causal_prefill_equals_single_queries(hip, kvdt, H, q_B):
    """Row p·q_B + b of a q_B > 0 call equals, bit for bit, the single-query call of utterance b with len + 1 + p keys, whose cache
    holds NaN past that count (the causal bound itself: a row that swept one key more would differ); and equals float64."""
    wt = _wt()
    length, cap_rows, d = 5, 16, 64 * H
    for P in (2, 4, 5):
        r = np.random.default_rng(H + q_B + P + kvdt)
        q, k, v = _attn_inputs(r, P * q_B, cap_rows, H, kvdt, "random")
        k, v = k[:q_B].copy(), v[:q_B].copy()
        k[:, length + P:] = np.nan
        v[:, length + P:] = np.nan
        odt = ODTS[(P + H) % 3]
        pre = np.zeros_like(q)
        wt.attention_cached(pre, q, k, v, H, kv_dtype=kvdt, out_dtype=odt, q_B=q_B, len=length)
        counts = prefill_counts(P, q_B, length)
        _attn_check(f"prefill H {H} kv {kvdt} q_B {q_B} P {P} out {odt}", pre, _attention_cached_ref(q, k, v, H, counts=counts, q_B=q_B), odt)
        for row in range(P * q_B):
            b, n = row % q_B, counts[row]
            kk, vv = k[b:b + 1].copy(), v[b:b + 1].copy()
            kk[:, n:] = np.nan
            vv[:, n:] = np.nan
            one = np.zeros((1, d), np.float32)
            wt.attention_cached(one, q[row:row + 1], kk, vv, H, kv_dtype=kvdt, out_dtype=odt, len=n - 1)
            np.testing.assert_array_equal(one[0], pre[row])


@pytest.mark.parametrize("kvdt,H,q_B", [(DT_F32, 2, 1), (DT_F32, 6, 5), (DT_BF16, 2, 5), (DT_BF16, 6, 1)])
def test_four_position_prefill_equals_single_queries(hip, kvdt, H, q_B):
    """nq = 4 (attn_decode_kernel<.., NT = true, U = 4, NQ = 4>): the four rows of utterance b equal four single-query chunked calls
    ("same arithmetic per query"), bit for bit, and float64; so does the q_B > 0 chunked call without nq."""
    wt = _wt()
    t, nc = 300, 10
    r = np.random.default_rng(H + q_B + kvdt)
    q, k, v = _attn_inputs(r, 4 * q_B, t, H, kvdt, "random")
    k, v = k[:q_B], v[:q_B]
    for odt in (DT_F32, DT_BF16):
        four = np.zeros_like(q)
        wt.attention_cached(four, q, k, v, H, kv_dtype=kvdt, n_chunks=nc, out_dtype=odt, q_B=q_B, nq=4)
        _attn_check(f"nq 4 H {H} kv {kvdt} q_B {q_B} out {odt}", four, _attention_cached_ref(q, k, v, H, q_B=q_B), odt)
        rows = np.zeros_like(q)
        wt.attention_cached(rows, q, k, v, H, kv_dtype=kvdt, n_chunks=nc, out_dtype=odt, q_B=q_B)
        np.testing.assert_array_equal(rows, four)
        for row in range(4 * q_B):
            b = row % q_B
            one = np.zeros((1, 64 * H), np.float32)
            wt.attention_cached(one, q[row:row + 1], k[b:b + 1], v[b:b + 1], H, kv_dtype=kvdt, n_chunks=nc, out_dtype=odt)
            np.testing.assert_array_equal(one[0], four[row])


@pytest.mark.parametrize("kvdt,H,t,nc", [(DT_F32, 6, 200, 1), (DT_BF16, 8, 1500, 16), (DT_F16, 2, 97, 3)])
def test_attention_rows_are_independent(hip, kvdt, H, t, nc):
    wt = _wt()
    r = np.random.default_rng(H + t)
    q, k, v = _attn_inputs(r, 7, t, H, kvdt, "random")

    def call(rows):
        out = np.zeros((len(rows), 64 * H), np.float32)
        wt.attention_cached(out, q[rows], k[rows], v[rows], H, kv_dtype=kvdt, n_chunks=nc)
        return out
    full = call(np.arange(7))
    np.testing.assert_array_equal(call(np.arange(7)), full)
    perm = r.permutation(7)
    np.testing.assert_array_equal(call(perm), full[perm])
    np.testing.assert_array_equal(call(np.array([5])), full[5:6])
