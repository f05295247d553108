"""CPU side of the op tests of the encoder's two ring GEMM kernels, gemm_nt_rowpanel_kernel ("rowpanel") and gemm_nt_fullrow_kernel
("fullrow") (the GPU side is tests/test_gpu_enc_ring_gemm_op.py, the hook wm_op_gemm_nt_ring).

Builds on tests/test_enc_gemm_ref.py (case constructors, layouts, operands, float64 reference, the bound bar = 2·Δout with the lds
kernel's ε_g: both ring kernels call gelu_fast4) and on tests/test_fused_ln_ref.py (order_fullrow, ln_bound, ln_bound_t).  The cases
are registered in test_enc_gemm_ref.EXTRA, so its operands() / reference() serve them; its own CASES stay what they were.

What is restated here, in float32 numpy:
    rowpanel: acc = bias (the accumulator starts from the LDS copy of the bias); acc += one MFMA per k-step of 32, in order;
              v = gelu_fast4(acc) if act; round to TO.  No addends (the launcher gives such shapes to another kernel).
    fullrow:  acc = 0; acc += one MFMA per k-step of 32, in order (the X and Y half-stages of a k64 feed different columns, so every
              element still sees its k-steps in order); v = acc + bias; v = gelu_fast4(v) if act; v += (residual (+ pos)) or pos; fp32.
              LNO: one-pass statistics of v in order_fullrow's order, y = (v − mean)·rstd·γ + β rounded to T.

LNO rows are checked against the float64 LayerNorm of a KNOWN fp32 C (the exact expectation, or the C the launch returned) under
test_fused_ln_ref's full-row bound through the 16-bit store (ln_bound_t).  That bound is informative when it is below two ulps of T
of the value; it cannot be where y = t·γ + β cancels: the fp32 error is about 2^-21·(|t·γ| + |β|) (statistics 28 deep), two ulps of
T are at least 2^-9·|y| (f16) or 2^-6·|y| (bf16), so only elements with |y| < 2^-12·(|t·γ| + |β|) (f16) are uninformative — a share
of about 2^-12 times the density of y near 0, which is below 1 for these γ, β.  SHARE_CAP = 0.5 % leaves a factor of ten over that.
"""
import os
import re

import numpy as np
import pytest

import test_enc_gemm_ref as E
import test_fused_ln_ref as T

SENTINEL = E.SENTINEL
PAIRS16 = E.PAIRS[:4]
RP_MS = (1, 31, 33, 65, 97, 127, 128, 129, 257)
FR_MS = (1, 63, 64, 65, 127, 128, 129, 257)
FR_KS = (128, 256, 384, 1152, 1536)
BIG_M, BIG_N = 8193, 3072
SHARE_CAP = 0.005
LN_DEPTH = T.SITES["fullrow"][1](384)


def R(dt, out, M, N, epi, group_n=0, ldc_pad=0):
    return dict(E.E(dt, out, M, N, 384, epi, "rowpanel", group_n=group_n), ldc_pad=ldc_pad)


def Fr(dt, M, K, epi, batch=1, lno=False):
    return dict(E.E(dt, "f32", M, 384, K, epi, "fullrow", batch=batch), lno=lno)


def Fc(dt, C, stride, L, epi, batch, lno=False):
    return dict(E.conv_case(dt, "f32", C, stride, L, 384, epi, "fullrow", batch), lno=lno)


BIG_CASES = [R("bf16", "f32", BIG_M, BIG_N, "bias"), R("f16", "f16", BIG_M, BIG_N, "bias")]

EXACT_ROWPANEL = [
    R("bf16", "bf16", 1, 128, "none"),
    R("bf16", "f32", 31, 384, "bias", group_n=128),               # N = 384 with fp32 output is the row-panel kernel's only as a scatter
    R("f16", "f16", 33, 1152, "bias", group_n=384),
    R("f16", "f32", 65, 1536, "none", group_n=768),               # cross-K/V of the tiny model: two groups
    R("bf16", "bf16", 97, 3072, "bias", group_n=768),
    R("bf16", "f32", 127, 1152, "bias", ldc_pad=8),               # QKV's N
    R("f16", "f16", 128, 384, "none", ldc_pad=16),
    R("f16", "f32", 129, 128, "bias"),
    R("bf16", "bf16", 257, 1536, "bias", group_n=128, ldc_pad=8),  # twelve groups, padded rows
    R("f16", "f32", 257, 3072, "none", ldc_pad=8),
    R("bf16", "f32", 65, 384, "bias", group_n=384),
    R("f16", "f16", 129, 1536, "bias"),                           # fc1's N
] + BIG_CASES

EXACT_FULLROW = [
    Fr("bf16", 1, 128, "none"),
    Fr("f16", 63, 256, "bias"),
    Fr("bf16", 64, 384, "bias_res"),
    Fr("f16", 65, 1152, "bias_res_inplace"),
    Fr("bf16", 127, 1536, "bias_pos"),
    Fr("f16", 128, 128, "bias_pos_res"),
    Fr("bf16", 129, 256, "bias_pos_res"),
    Fr("f16", 257, 1536, "bias_res"),
    Fr("bf16", 257, 128, "bias_pos"),
    Fr("f16", 129, 384, "none"),
    Fr("bf16", 65, 256, "bias_res_inplace", batch=2),
    Fr("f16", 1, 1536, "bias_res_inplace", batch=3),
    Fc("bf16", 128, 1, 130, "bias_pos", 2),
    Fc("f16", 128, 2, 129, "bias_res", 3),
    Fc("bf16", 384, 2, 257, "bias_pos", 2),                       # conv2: stride 2, positional addend, several clips
    Fc("f16", 384, 1, 65, "bias_pos_res", 1),
    Fc("bf16", 384, 1, 63, "bias_res_inplace", 3),
]

EXACT_LNO = [
    Fr("bf16", 1, 128, "bias", lno=True),
    Fr("f16", 65, 1536, "bias_res", lno=True),
    Fr("bf16", 129, 384, "bias_res_inplace", batch=2, lno=True),
    Fc("f16", 384, 2, 257, "bias_pos", 2, lno=True),
    Fr("bf16", 257, 256, "bias_pos_res", lno=True),
    Fr("f16", 128, 1152, "none", lno=True),
]

EXACT_CASES = EXACT_ROWPANEL + EXACT_FULLROW + EXACT_LNO


def _float_rp(dt, out, act, pat):
    return dict(E.F(dt, out, 384, act, pat, "rowpanel", M=129, N=256), epi="bias")


FLOAT_CASES = ([_float_rp(dt, out, act, pat) for pat in ("normal", "outlier") for dt, out in PAIRS16 for act in (None, 0, 1)] +
               [E.F(dt, "f32", K, act, pat, "fullrow", M=129, N=384)
                for pat in ("normal", "outlier") for K in (128, 1536) for dt in ("bf16", "f16") for act in (None, 0, 1)])


def _act_lno(c, act):
    return dict(c, act=act, pat="normal", lno=True)


# ACT with LNO: conv2's configuration (GELU, positional addend, next LayerNorm, several clips), and the erf form at the shallow K
FLOAT_LNO = [_act_lno(Fc("bf16", 384, 2, 257, "bias_pos", 2), 0), _act_lno(Fc("f16", 128, 2, 129, "bias_pos", 2), 0),
             _act_lno(Fr("f16", 129, 128, "bias"), 1), _act_lno(Fr("bf16", 65, 1536, "bias_res"), 1)]

SWEEP_CASES = ([dict(E.G(dt, out, 384, mode, "rowpanel")) for dt, out in PAIRS16 for mode in (0, 1)] +
               [dict(E.G(dt, "f32", 128, mode, "fullrow"), N=384) for dt in ("bf16", "f16") for mode in (0, 1)])

# LNA on the row-panel kernel, what tests/test_gpu_fused_ln_op.py lacks: (dt, out, M, N, group_n, act); selection weights, no bias
LNA_CASES = [("bf16", "bf16", 130, 384, 0, None), ("f16", "f16", 65, 768, 384, None), ("bf16", "f32", 130, 768, 128, None),
             ("f16", "f32", 130, 384, 128, 0), ("bf16", "bf16", 97, 512, 0, 1), ("bf16", "f32", BIG_M, BIG_N, 0, None)]

ALL = EXACT_CASES + FLOAT_CASES + FLOAT_LNO + SWEEP_CASES
case_id = E.case_id
CASES = {case_id(c): c for c in ALL}
E.EXTRA.update(CASES)
RESTATED = {}


# ---------------------------------------------------------------------------------------------------------------------------------
# the launch geometry restated

def wave_rows(M):
    """rows present in every (panel, wave) of the row-panel kernel: wave w of panel pn owns rows pn·128 + 32 w .. + 31"""
    return [min(max(M - (pn * 128 + w * 32), 0), 32) for pn in range((M + 127) // 128) for w in range(4)]


def unit_ranges(M, N, grid_cap=512):
    """launch_rowpanel_t: units = (panel, column tile), column tile fastest; workgroup b walks [b·n/grid, (b + 1)·n/grid)"""
    nct = N // 128
    n = ((M + 127) // 128) * nct
    grid = min(n, grid_cap)
    return nct, [(b * n // grid, (b + 1) * n // grid) for b in range(grid)]


# ---------------------------------------------------------------------------------------------------------------------------------
# LNO: parameters, reference and bound

def lno_params(c):
    r = E._rng("lno" + case_id(c))
    return (1 + 0.3 * r.standard_normal(384)).astype(np.float32), (0.2 * r.standard_normal(384)).astype(np.float32)


def ulp_t(v, dt):
    """the spacing of T at |v| (f16: never below its subnormal spacing)"""
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(v)))
    e = np.where(np.isfinite(e), e, -140.0)
    return 2.0 ** (np.maximum(e, -14.0) - 10) if dt == "f16" else 2.0 ** (e - 7)


def lno_reference(c, c_flat):
    """c_flat: a flat fp32 C of the case -> (flat float64 lno_out expected: the float64 LayerNorm of those very rows rounded to T,
    sentinel where nothing is written; the bound per cell)"""
    lay = E.layout(c)
    g, b = lno_params(c)
    want = np.full(lay["c_len"], float(SENTINEL))
    bound = np.zeros(lay["c_len"])
    for bz in range(c["batch"]):
        idx = E.cells(lay, bz * lay["strideC"], c["M"])
        rows = np.ascontiguousarray(c_flat[idx], np.float32).reshape(c["M"], 384)
        y, e = T.ln_bound(rows, g, b, LN_DEPTH)
        yt, et = T.ln_bound_t(y, e, E.DTYPE[c["dt"]])
        E.put(want, lay, bz * lay["strideC"], c["M"], yt)
        E.put(bound, lay, bz * lay["strideC"], c["M"], et)
    return want, bound


def lno_check(c, got, c_flat):
    """-> (largest error / bound on the written rows, share of elements whose bound is two ulps of T or more) after asserting that
    everything else holds the sentinel"""
    want, bound = lno_reference(c, c_flat)
    m = E.written_mask(c)
    assert (got[~m] == SENTINEL).all(), "lno_out: a guard row was written"
    assert np.isfinite(got[m]).all()
    loose = bound[m] >= 2 * ulp_t(want[m], c["dt"])
    return T.ratio(got[m], want[m], bound[m]), float(loose.mean())


def lno_restate(c, c_flat, fma_sq=False, fma_var=False, fma_out=True):
    lay = E.layout(c)
    g, b = lno_params(c)
    out = np.full(lay["c_len"], SENTINEL, np.float32)
    for bz in range(c["batch"]):
        rows = np.ascontiguousarray(c_flat[E.cells(lay, bz * lay["strideC"], c["M"])], np.float32).reshape(c["M"], 384)
        y, _ = T.restate("fullrow", rows, g, b, fma_sq, fma_var, fma_out=fma_out)
        E.put(out, lay, bz * lay["strideC"], c["M"], T._round(y, E.DTYPE[c["dt"]]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic restated

def restate(c, reverse=False):
    """the flat C of the module docstring's two restatements (reverse: the k-steps in the opposite order, for the exactness proof)"""
    lay = E.layout(c)
    A, W, bias, pos, res = E.operands(c)
    M, N, K, gn = c["M"], c["N"], c["K"], c["group_n"]
    got = E.c_init(c)
    W64 = W.astype(np.float64)
    steps = list(range(0, K, 32))[::-1 if reverse else 1]
    for b in range(c["batch"]):
        Ab = E.a_rows(c, b).astype(np.float64)
        acc = np.zeros((M, N), np.float32)
        if c["kern"] == "rowpanel" and bias is not None:
            acc = acc + bias[None, :]
        for k0 in steps:
            acc = (acc + (Ab[:, k0:k0 + 32] @ W64[:, k0:k0 + 32].T).astype(np.float32)).astype(np.float32)
        v = acc
        if c["kern"] == "fullrow" and bias is not None:
            v = (acc + bias[None, :]).astype(np.float32)
        if c["act"] is not None:
            v = E.gelu_fast_f32(v, c["act"])
        if res is not None or pos is not None:
            assert c["kern"] == "fullrow"
            ex = np.zeros((M, N), np.float32) if res is None else np.array(res[b], np.float32)
            if pos is not None:
                ex = (ex + pos).astype(np.float32)
            v = (v + ex).astype(np.float32)
        v = E.rnd(v, c["out"])
        for g in range(lay["n_grp"]):
            cols = slice(g * gn, (g + 1) * gn) if gn else slice(0, N)
            E.put(got, lay, b * lay["strideC"] + g * lay["group_stride"], M, v[:, cols])
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU tests

def test_case_ids_are_unique_and_apart_from_the_tiled_lists():
    assert len(CASES) == len(ALL) and not set(CASES) & set(E.CASES)


def test_every_case_names_the_ring_kernel_the_dispatch_picks():
    for c in ALL:
        addends = any(x in c["epi"] for x in ("res", "pos"))
        assert E.kernel_for(c["dt"], c["out"], c["N"], c["K"], addends, c["batch"], c["group_n"]) == c["kern"] in E.RING, case_id(c)
        if c.get("lno"):
            assert c["kern"] == "fullrow"
        lay = E.layout(c)
        assert lay["lda"] % 8 == 0 and lay["strideA"] % 8 == 0 and lay["ldr"] % 4 == 0 and lay["strideR"] % 4 == 0
        wide = c["out"] != "f32" or c.get("lno")
        assert lay["ldc"] % (8 if wide else 4) == 0 and lay["strideC"] % (8 if wide else 4) == 0 and lay["group_stride"] % (8 if wide else 4) == 0
    for dt, out, M, N, gn, act in LNA_CASES:
        assert E.kernel_for(dt, out, N, 384, False, 1, gn) == "rowpanel" or (N == 384 and out == "f32" and gn == 0)
        assert not (N == 384 and out == "f32" and gn == 0)  # that shape would go to the full-row kernel, which refuses ln_g


@pytest.mark.parametrize("c", [c for c in EXACT_CASES if c["M"] != BIG_M], ids=case_id)
def test_exact_cases_are_exact_in_fp32_ref(c):
    """test_enc_gemm_ref's argument: integers in [-8, 8], addends multiples of 1/4 up to 64, Σ|a||w| + addends below 2^20 — every partial
    sum in any order is a multiple of 1/4 below 2^20.  Both restatement orders reproduce the float64 reference bit for bit."""
    A, W, bias, pos, res = E.operands(c)
    for a in (A, W):
        assert (a == np.round(a)).all() and np.abs(a).max() <= 8
    for a in (bias, pos) + tuple(res[:c["batch"]] if res else ()):
        if a is not None:
            assert (a * 4 == np.round(a * 4)).all() and np.abs(a).max() <= 64
    n_add = sum(x in c["epi"] for x in ("bias", "pos", "res"))
    assert 64 * c["K"] + 64 * n_add < 2 ** 20 and c["K"] <= 1536  # Σ|a||w| <= 8·8·K: no draw can leave the range
    bits = E.expected_bits(c)
    assert np.array_equal(restate(c).view(np.uint32), bits)
    assert np.array_equal(restate(c, reverse=True).view(np.uint32), bits)
    m = E.written_mask(c)
    lay = E.layout(c)
    assert (E.reference(c)[0][~m] == SENTINEL).all() and (~m).sum() >= c["batch"] * lay["n_grp"] * lay["ldc"] + c.get("ldc_pad", 0) * c["M"]


def test_exactness_holds_at_the_deepest_k_and_for_the_large_launch():
    """K = 1536 is in the lists, and the range argument covers the 8193-row pair without evaluating it here: 8·8·384 + 64 < 2^20"""
    assert any(c["K"] == 1536 for c in EXACT_FULLROW) and any(c["K"] == 1536 for c in EXACT_LNO)
    for c in BIG_CASES:
        assert c["K"] == 384 and c["epi"] == "bias" and 64 * c["K"] + 64 < 2 ** 20


@pytest.mark.parametrize("c", FLOAT_CASES + FLOAT_LNO + SWEEP_CASES, ids=case_id)
def test_restatement_inside_the_bound_ref(c):
    got = restate(c)
    r = E.ratio(got, c)
    key = (c["kern"], c["dt"], c["out"], c["act"])
    RESTATED[key] = max(RESTATED.get(key, 0.0), r)
    print(f"RESTATED {case_id(c)}: error / bar = {r:.3f}")
    assert r <= 1.0, r
    if c.get("lno"):
        for fs, fv in T.VARIANTS:
            w, share = lno_check(c, lno_restate(c, got, fs, fv), got)
            print(f"RESTATED lno {case_id(c)} fma_sq {int(fs)} fma_var {int(fv)}: error / bound = {w:.3f}, uninformative share {share:.5f}")
            assert w <= 1.0 and share <= SHARE_CAP, (w, share)


@pytest.mark.parametrize("c", EXACT_LNO, ids=case_id)
def test_lno_restatement_inside_an_informative_bound_ref(c):
    """On the exact C the restated LayerNorm (every contraction variant) is inside the bound everywhere, and the bound is below two
    ulps of T on all but SHARE_CAP of the elements."""
    c32 = E.expected_bits(c).view(np.float32)
    worst = 0.0
    for fs, fv in T.VARIANTS:
        for fo in (False, True):
            w, share = lno_check(c, lno_restate(c, c32, fs, fv, fo), c32)
            worst = max(worst, w)
            assert w <= 1.0 and share <= SHARE_CAP, (fs, fv, fo, w, share)
    print(f"RESTATED lno {case_id(c)}: worst error / bound {worst:.3f}, uninformative share {share:.5f} (cap {SHARE_CAP})")
    # the bound has teeth: without the xor-32 butterfly level the restatement leaves it
    g, b = lno_params(c)
    lay = E.layout(c)
    rows = c32[E.cells(lay, 0, c["M"])].reshape(c["M"], 384)
    y, e = T.ln_bound(rows, g, b, LN_DEPTH)
    bad, _ = T.restate("fullrow", rows, g, b, drop="xor32")
    assert T.ratio(T._round(bad, E.DTYPE[c["dt"]]), *T.ln_bound_t(y, e, E.DTYPE[c["dt"]])) > 1.0


def test_lists_cover_what_they_claim():
    rp, fr = EXACT_ROWPANEL, EXACT_FULLROW
    # row-panel: shapes, types, epilogues, scatter, padded rows
    assert {c["N"] for c in rp} == {128, 384, 1152, 1536, 3072} and {c["K"] for c in rp} == {384}
    assert {(c["dt"], c["out"]) for c in rp} == set(PAIRS16) and {c["epi"] for c in rp} == {"none", "bias"}
    assert {c["group_n"] for c in rp} == {0, 128, 384, 768}
    for c in rp:
        lay = E.layout(c)
        if c["group_n"]:
            assert lay["group_stride"] > c["M"] * lay["ldc"]  # a gap after every group
    assert any(c["ldc_pad"] and c["out"] == "f32" for c in rp) and any(c["ldc_pad"] and c["out"] != "f32" for c in rp)
    assert any(c["ldc_pad"] and c["group_n"] for c in rp)
    # the wave-ragged classes that decide st_pend, from the panel arithmetic
    small = sorted({c["M"] for c in rp if c["M"] != BIG_M})
    assert small == sorted(RP_MS)
    classes = {M: set("full" if n == 32 else "absent" if n == 0 else "partial" for n in wave_rows(M)) for M in small}
    assert classes[1] == {"partial", "absent"} and classes[128] == {"full"} and classes[31] == {"partial", "absent"}
    assert classes[33] == {"full", "partial", "absent"} and classes[129] == {"full", "partial", "absent"}
    for want in ("full", "partial", "absent"):
        assert any(want in v for v in classes.values())
    # every count of present rows 1 .. 31 is not needed; the boundaries are: one row, 31 rows, and a full wave followed by a ragged one
    assert {n for M in small for n in wave_rows(M)} >= {0, 1, 31, 32}
    # a wave that stores (st_pend true) followed in the same workgroup's stream by a panel whose wave does not: M = 129, 257 with N > 128
    assert any(c["M"] in (129, 257) and c["N"] > 128 for c in rp)
    for out in ("f32", "bf16", "f16"):  # each store path sees a ragged wave and a full one
        ms = {c["M"] for c in rp if c["out"] == out}
        assert any("partial" in set("full" if n == 32 else "absent" if n == 0 else "partial" for n in wave_rows(M)) for M in ms)
    # the large launch: three or more units per workgroup, a start inside a panel, a panel switch inside a range, a ragged last panel
    assert {(c["dt"], c["out"]) for c in BIG_CASES} == {("bf16", "f32"), ("f16", "f16")} and len([c for c in ALL if c["M"] > 1000]) == 2
    nct, rng = unit_ranges(BIG_M, BIG_N)
    assert len(rng) == 512 and min(u1 - u0 for u0, u1 in rng) >= 3
    assert any(u0 % nct for u0, _ in rng) and any(u0 // nct != (u1 - 1) // nct for u0, u1 in rng)
    assert BIG_M % 128 == 1 and rng[-1][1] == 65 * nct
    nct64, rng64 = unit_ranges(8192, BIG_N)  # exactly 64 panels would not do: every range sits inside one panel
    assert all(u0 // nct64 == (u1 - 1) // nct64 for u0, u1 in rng64)
    for c in rp:  # every other case: one unit per workgroup
        if c["M"] != BIG_M:
            assert all(u1 - u0 == 1 for u0, u1 in unit_ranges(c["M"], c["N"])[1])
    # full-row
    assert {c["K"] for c in fr} == set(FR_KS) and {c["M"] for c in fr} >= set(FR_MS) and {c["dt"] for c in fr} == {"bf16", "f16"}
    assert {c["epi"] for c in fr} == set(E.EPIS)
    assert {(c["dt"], c["epi"]) for c in fr} >= {(d, "bias_pos_res") for d in ("bf16", "f16")}
    conv = [c for c in fr if c["conv"]]
    assert {(c["conv"][0], c["conv"][1]) for c in conv} == {(128, 1), (128, 2), (384, 1), (384, 2)} and {c["batch"] for c in conv} == {1, 2, 3}
    for c in conv:
        lay = E.layout(c)
        assert c["K"] == 3 * c["conv"][0] and lay["lda"] < c["K"] and lay["strideC"] == (c["M"] + 1) * 384
        assert (c["M"] - 1) * lay["lda"] + c["K"] <= lay["strideA"]
    assert any(c["epi"] == "bias_res" and E.layout(c)["ldr"] > 384 for c in fr)
    assert any(c["epi"] == "bias_res_inplace" and c["batch"] > 1 for c in fr)
    assert {c["K"] // 32 for c in fr} >= {4, 8}  # fewer half-stage groups than the steady-state loop needs: only the last group runs
    # LNO
    assert {1, 65, 129} <= {c["M"] for c in EXACT_LNO} and any(c["batch"] == 2 for c in EXACT_LNO) and any(c["K"] == 1536 for c in EXACT_LNO)
    assert {c["dt"] for c in EXACT_LNO} == {"bf16", "f16"} and all(c["act"] is None for c in EXACT_LNO)
    assert any(c["act"] == 0 and c["conv"] and c["conv"][1] == 2 and "pos" in c["epi"] and c["batch"] > 1 for c in FLOAT_LNO)
    # float and sweep
    assert {(c["dt"], c["out"], c["act"], c["pat"]) for c in FLOAT_CASES if c["kern"] == "rowpanel"} == \
        {(d, o, a, p) for d, o in PAIRS16 for a in (None, 0, 1) for p in ("normal", "outlier")}
    assert all(c["M"] == 129 and c["K"] == 384 for c in FLOAT_CASES if c["kern"] == "rowpanel")
    assert {(c["dt"], c["K"], c["act"], c["pat"]) for c in FLOAT_CASES if c["kern"] == "fullrow"} == \
        {(d, K, a, p) for d in ("bf16", "f16") for K in (128, 1536) for a in (None, 0, 1) for p in ("normal", "outlier")}
    assert any(c["pat"] == "outlier" and np.abs(E.operands(c)[0]).max() == 4096.0 for c in FLOAT_CASES)
    assert {(c["kern"], c["act"], c["out"] == "f32") for c in SWEEP_CASES} == \
        {("rowpanel", m, f) for m in (0, 1) for f in (True, False)} | {("fullrow", m, True) for m in (0, 1)}
    # LNA: 16-bit output, a scatter, an activation, the multi-unit launch
    assert any(o != "f32" for _, o, *_ in LNA_CASES) and any(g for *_, g, _ in LNA_CASES) and {a for *_, a in LNA_CASES} >= {0, 1}
    assert any(M == BIG_M and N == BIG_N for _, _, M, N, _, _ in LNA_CASES)


def test_both_ring_kernels_call_the_fast_gelu_in_every_instance():
    """bar uses the lds kernel's ε_g: every GELU of the two kernels' bodies (both output types of the row-panel kernel, ACT of the
    full-row kernel) must be gelu_fast4, none gelu_f."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "whisper.mojo_amd", "csrc", "kernels_encoder.hip")).read()
    rp = src[src.index("void gemm_nt_rowpanel_kernel("):src.index("static int launch_rowpanel_t(")]
    fr = src[src.index("void gemm_nt_fullrow_kernel("):src.index("static bool fullrow_ok(")]
    assert len(re.findall(r"\bgelu_fast4\(", rp)) == 2 and len(re.findall(r"\bgelu_fast4\(", fr)) == 1
    assert not re.search(r"\bgelu_f\(", rp + fr)
