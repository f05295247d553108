"""GPU op tests of the encoder's two ring GEMM kernels (gemm_nt_rowpanel_kernel, gemm_nt_fullrow_kernel) through wm_op_gemm_nt_ring:
bit equality on exact integer cases, float64 with the per-element bound of DESIGN §32 on float cases and a GELU sweep, the full-row
kernel's fused next-LayerNorm rows against the float64 LayerNorm of the fp32 rows beside them, the row-panel kernel's fused LayerNorm
through selection weights.  Cases, references, bounds and the CPU proofs about them: tests/test_enc_ring_gemm_ref.py."""
import ctypes as C

import numpy as np
import pytest

import test_enc_gemm_ref as E
import test_enc_ring_gemm_ref as gen

pytestmark = pytest.mark.gpu

WM_E_ARG = -1
SENTINEL = gen.SENTINEL


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    return _lib.lib()


def _launch(c, batch=None, first=0):
    """the hook on case c -> (flat C as it came back, flat lno_out or None, the kernel that ran); batch / first: a launch on `batch`
    batches from `first` on"""
    from whisper_mojo_amd import whisper_tensor as wt
    lay = E.layout(c)
    A, W, bias, pos, res = E.operands(c)
    B = c["batch"] if batch is None else batch
    a_len = (B - 1) * lay["strideA"] + (c["M"] - 1) * lay["lda"] + c["K"]
    A = A[first * lay["strideA"]:][:a_len]
    C0 = E.c_init(c)[first * lay["strideC"]:][:B * lay["strideC"]].copy()
    inplace = c["epi"].endswith("inplace")
    r = None
    if res is not None and not inplace:
        r = res[-1][first * lay["strideR"]:][:B * lay["strideR"]]
    L0 = np.full(C0.size, SENTINEL, np.float32) if c.get("lno") else None
    ran = wt.gemm_nt_ring(C0, A, W, c["M"], lda=lay["lda"], batch=B, strideA=lay["strideA"], ldc=lay["ldc"], strideC=lay["strideC"], bias=bias,
                          pos=pos, residual=r, ldr=lay["ldr"], strideR=lay["strideR"], residual_in_place=inplace, act=c["act"] is not None,
                          gelu_mode=c["act"] or 0, group_n=c["group_n"], group_stride=lay["group_stride"], dtype=E.DTYPE[c["dt"]],
                          out_dtype=E.DTYPE[c["out"]], lno=gen.lno_params(c) if c.get("lno") else None, lno_out=L0)
    return C0, L0, ran


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("c", gen.EXACT_CASES, ids=gen.case_id)
def test_exact_cases_bit_equal(hip, c):
    """Integer operands and quarter-integer addends: C equals the float64 reference bit for bit (16-bit output: rounded to TO); guard
    rows, gaps between column groups, padded columns and everything past M keep the sentinel; the kernel that ran is the one the case
    names; a second launch gives the same bits; batch b of a batched launch equals the single launch on its slice.  With lno_*: C is
    still that, and the 16-bit rows are the float64 LayerNorm of it under the full-row bound, sentinel elsewhere."""
    got, lno, ran = _launch(c)
    assert ran == c["kern"]
    want = E.expected_bits(c)
    bad = np.flatnonzero(got.view(np.uint32) != want)
    assert bad.size == 0, (len(bad), bad[:4].tolist(), got[bad[:4]].tolist(), want.view(np.float32)[bad[:4]].tolist())
    again, lno2, _ = _launch(c)
    assert _same(again, got)
    if lno is not None:
        w, share = gen.lno_check(c, lno, got)
        print(f"MEASURED lno {gen.case_id(c)}: error / bound = {w:.3f}, uninformative share {share:.5f}")
        assert w <= 1.0, w
        assert _same(lno2, lno)
    if c["batch"] > 1:
        sc = E.layout(c)["strideC"]
        for b in range(c["batch"]):
            one, lno1, ran1 = _launch(c, batch=1, first=b)
            assert ran1 == c["kern"] and _same(one, got[b * sc:(b + 1) * sc]), b
            assert lno is None or _same(lno1, lno[b * sc:(b + 1) * sc]), b


def _float_check(c):
    got, lno, ran = _launch(c)
    assert ran == c["kern"]
    want, bar = E.reference(c)
    m = E.written_mask(c)
    assert (got[~m] == SENTINEL).all(), "a guard row was written"
    assert np.isfinite(got[m]).all()
    err = np.abs(got.astype(np.float64) - want)
    q = np.where(m & (err > 0), err / np.maximum(bar, 1e-300), 0.0)
    i = int(np.argmax(q))
    print(f"MEASURED ring gemm {gen.case_id(c)}: error / bar = {q[i]:.3f} at flat {i} (row {i % E.layout(c)['strideC'] // E.layout(c)['ldc']}): "
          f"got {got[i]!r} want {want[i]!r} bar {bar[i]:.3e}")
    assert q[i] <= 1.0, (q[i], i, float(got[i]), float(want[i]), float(bar[i]))
    again, lno2, _ = _launch(c)
    assert _same(again, got)
    if lno is not None:  # ACT with LNO: the 16-bit rows against the float64 LayerNorm of the C that came back
        w, share = gen.lno_check(c, lno, got)
        print(f"MEASURED lno {gen.case_id(c)}: error / bound = {w:.3f}, uninformative share {share:.5f}")
        assert w <= 1.0, w
        assert _same(lno2, lno)


@pytest.mark.parametrize("c", gen.FLOAT_CASES + gen.FLOAT_LNO, ids=gen.case_id)
def test_float_cases_vs_float64(hip, c):
    """Random and outlier operands pre-rounded to T against float64: every element inside bar = 2·Δout of DESIGN §32 (ε_g of the fast
    GELU), guard rows untouched, a second launch the same bits."""
    _float_check(c)


@pytest.mark.parametrize("c", gen.SWEEP_CASES, ids=gen.case_id)
def test_gelu_sweep_vs_float64(hip, c):
    """z[m, n] = W[n, m] is one exact product: the epilogue's GELU on test_enc_gemm_ref's sweep, with Δz = 0."""
    _float_check(c)


@pytest.mark.parametrize("dt,out,M,N,gn,act", gen.LNA_CASES, ids=lambda v: str(v))
def test_rowpanel_fused_layernorm(hip, dt, out, M, N, gn, act):
    """LayerNorm applied while the row-panel kernel loads its fp32 A rows, seen through selection weights (rows of a signed permutation,
    then zero rows: the product is exact) with tests/test_gpu_fused_ln_op.py's rows and bound — at 16-bit output, through a column
    scatter, under both GELU forms and in the launch that gives every workgroup three units."""
    from test_gpu_fused_ln_op import _expect, _perm, _pick, _pool
    from whisper_mojo_amd import whisper_tensor as wt
    K, dti = 384, E.DTYPE[dt]
    x, g, b, _ = _pool(K)
    xs = np.ascontiguousarray(x[_pick(K, M)])
    W, pi, sg = _perm(K, N, M + N + dti)
    ref, bound = _expect("rowpanel", xs, g, b, dti, pi, sg, N, "linear")
    if act is not None:  # a value within `bound` of ref goes through the fast GELU and the store: DESIGN §32's Δy and Δout with Δz = bound
        y = E.gelu64(ref, act)
        d = E.L_G * bound + 2 * (E.eps_gelu(ref, y, act, "rowpanel") + 2.0 ** -23 * np.abs(y) + E.U[out] * np.abs(y) + E.FLOOR +
                                 (np.where(np.abs(y) < 2.0 ** -14, 2.0 ** -25, 0.0) if out == "f16" else 0.0))
        ref, bound = y, d
    c = gen.R(dt, out, M, N, "none", group_n=gn)
    lay = E.layout(c)
    got = np.full(lay["c_len"], SENTINEL, np.float32)
    ran = wt.gemm_nt_ring(got, xs, W, M, ldc=lay["ldc"], group_n=gn, group_stride=lay["group_stride"], act=act is not None, gelu_mode=act or 0,
                          dtype=dti, out_dtype=E.DTYPE[out], ln=(g, b))
    assert ran == "rowpanel"
    assert (got[~E.written_mask(c)] == SENTINEL).all(), "a guard row was written"
    mat = np.empty((M, N), np.float32)
    for grp in range(lay["n_grp"]):
        cols = slice(grp * gn, (grp + 1) * gn) if gn else slice(0, N)
        mat[:, cols] = got[E.cells(lay, grp * lay["group_stride"], M)].reshape(M, -1)
    assert np.isfinite(mat).all()
    err = np.abs(mat - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.nan_to_num(np.where(err == 0, 0.0, err / bound), nan=np.inf)
    i = np.unravel_index(int(np.argmax(q)), q.shape)
    print(f"MEASURED rowpanel LNA {dt}->{out} M {M} N {N} g {gn} act {act}: error / bound {q[i]:.3f} at {i}: got {mat[i]!r} want {ref[i]!r}")
    assert q[i] <= 1.0, (q[i], i, float(mat[i]), float(ref[i]), float(bound[i]))


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def test_hook_refuses_bad_arguments(hip):
    """WM_E_ARG, nothing launched, C and lno_out as they went in."""
    M = 8
    ran = C.c_int32(7)
    one = lambda *s: np.ones(s, np.float32)
    sent = lambda n: np.full(n, SENTINEL, np.float32)
    # a row-panel call (N = 256, K = 384) and a full-row call (N = 384, K = 128), both valid
    rp = dict(C=sent((M + 1) * 256), A=one(M * 384), W=one(256, 384), N=256, K=384, lda=384, ldc=256, dtype=1, out_dtype=1)
    fr = dict(C=sent((M + 1) * 384), A=one(M * 128), W=one(384, 128), N=384, K=128, lda=128, ldc=384, dtype=2, out_dtype=0)
    base = dict(bias=None, pos=None, residual=None, r_len=0, M=M, batch=1, strideA=0, strideC=0, ldr=0, strideR=0, inplace=0, act=0, gelu_mode=0,
                group_n=0, group_stride=0, ln_g=None, ln_b=None, lno_g=None, lno_b=None, lno_out=None, lno_len=0)
    lno_out = sent((M + 1) * 384)
    res = one(M * 384)

    def call(ok, **kw):
        a = dict(base, **ok)
        a.update(c_len=a["C"].size, a_len=a["A"].size)
        a.update(kw)
        return hip.wm_op_gemm_nt_ring(_fp(a["C"]), a["c_len"], _fp(a["A"]), a["a_len"], _fp(a["W"]), _fp(a["bias"]), _fp(a["pos"]),
                                      _fp(a["residual"]), a["r_len"], a["M"], a["N"], a["K"], a["batch"], a["lda"], a["strideA"], a["ldc"],
                                      a["strideC"], a["ldr"], a["strideR"], a["inplace"], a["act"], a["gelu_mode"], a["group_n"],
                                      a["group_stride"], a["dtype"], a["out_dtype"], _fp(a["ln_g"]), _fp(a["ln_b"]), _fp(a["lno_g"]),
                                      _fp(a["lno_b"]), _fp(a["lno_out"]), a["lno_len"], C.byref(ran) if a.get("ran", True) else None)
    ln384, ln128 = dict(ln_g=one(384), ln_b=one(384)), dict(ln_g=one(128), ln_b=one(128))
    lno = dict(lno_g=one(384), lno_b=one(384), lno_out=lno_out, lno_len=lno_out.size)
    bad = [(fr, ln128),                                                   # ln_g on a full-row shape
           (rp, dict(lno_g=one(256), lno_b=one(256), lno_out=lno_out, lno_len=lno_out.size)),  # lno_out on a row-panel shape
           (rp, dict(ln384, pos=one(M * 256))),                           # an addend with ln_g
           (rp, dict(ln384, residual=one(M * 256), r_len=M * 256, ldr=256)),
           (rp, dict(ln_g=one(384))), (fr, dict(lno, lno_b=None)), (fr, dict(lno, lno_out=None)), (fr, dict(lno, lno_len=M * 384 - 1)),
           (fr, dict(lno, ldc=388, c_len=(M + 1) * 388)),                 # 16-bit rows need ldc % 8
           (rp, dict(ldc=260)), (rp, dict(group_n=128, group_stride=(M + 1) * 128 + 4, ldc=128)),
           (rp, dict(C=None)), (rp, dict(A=None)), (rp, dict(W=None)), (rp, dict(ran=False)), (rp, dict(M=0)), (rp, dict(batch=0)),
           (rp, dict(lda=0)), (rp, dict(lda=380)), (rp, dict(ldc=0)), (rp, dict(ldc=128)), (rp, dict(dtype=3)), (rp, dict(out_dtype=2)),
           (rp, dict(a_len=M * 384 - 1)), (rp, dict(c_len=M * 256 - 1)), (rp, dict(M=M + 2)), (rp, dict(act=2)), (rp, dict(gelu_mode=2)),
           (rp, dict(group_n=32, group_stride=(M + 1) * 32)), (rp, dict(inplace=1)),
           (fr, dict(residual=res, r_len=M * 384 - 1, ldr=384)), (fr, dict(residual=res, r_len=M * 384, ldr=380)),
           (fr, dict(batch=2, strideA=M * 128, strideC=(M + 1) * 384)), (fr, dict(inplace=1, residual=res, r_len=res.size, ldr=384)),
           # shapes of the tiled kernels are wm_op_gemm_nt_epi's: fp32 operands, K = 64
           (rp, dict(dtype=0, out_dtype=0)), (rp, dict(K=64, lda=64, W=one(256, 64)))]
    for ok, kw in bad:
        assert call(ok, **kw) == WM_E_ARG, kw
        assert (rp["C"] == SENTINEL).all() and (fr["C"] == SENTINEL).all() and (lno_out == SENTINEL).all(), kw
    assert call(rp) == 0 and ran.value == 2 and (rp["C"][:M * 256] == 384).all() and (rp["C"][M * 256:] == SENTINEL).all()
    assert call(fr, **lno) == 0 and ran.value == 3 and (fr["C"][:M * 384] == 128).all() and (fr["C"][M * 384:] == SENTINEL).all()
    assert (lno_out[:M * 384] == 1).all() and (lno_out[M * 384:] == SENTINEL).all()  # a constant row: x − mean == 0, the row is β
