"""GPU op tests of the encoder's two tiled GEMM kernels (gemm_nt_kernel, gemm_nt_lds_kernel) and their shared epilogue through
wm_op_gemm_nt_epi: bit equality on exact integer cases, float64 with the per-element bound of DESIGN §32 on float cases and on a GELU
sweep.  Cases, references, bounds and the proof that the kernels' arithmetic restated on the CPU stays inside them:
tests/test_enc_gemm_ref.py."""
import ctypes as C

import numpy as np
import pytest

import test_enc_gemm_ref as gen

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
    """the hook on case c -> (flat C as it came back, the kernel that ran); batch / first: a launch on `batch` batches from `first` on"""
    from whisper_mojo_amd import whisper_tensor as wt
    lay = gen.layout(c)
    A, W, bias, pos, res = gen.operands(c)
    B = c["batch"] if batch is None else batch
    a_len = (B - 1) * lay["strideA"] + (c["M"] - 1) * lay["lda"] + c["K"]
    A = A[first * lay["strideA"]:][:a_len]
    C0 = gen.c_init(c)[first * lay["strideC"]:][:B * lay["strideC"]].copy()
    inplace = c["epi"].endswith("inplace")
    r = None
    if res is not None and not inplace:
        r = res[-1][first * lay["strideR"]:][:B * lay["strideR"]]
    ran = wt.gemm_nt_epi(C0, A, W, c["M"], lda=lay["lda"], batch=B, strideA=lay["strideA"], ldc=lay["ldc"], strideC=lay["strideC"], bias=bias,
                         pos=pos, residual=r, ldr=lay["ldr"], strideR=lay["strideR"], residual_in_place=inplace, act=c["act"] is not None,
                         gelu_mode=c["act"] or 0, group_n=c["group_n"], group_stride=lay["group_stride"], dtype=gen.DTYPE[c["dt"]],
                         out_dtype=gen.DTYPE[c["out"]])
    return C0, ran


@pytest.mark.parametrize("c", gen.EXACT_CASES, ids=gen.case_id)
def test_exact_cases_bit_equal(hip, c):
    """Integer operands and quarter-integer addends: the output equals the float64 reference bit for bit (16-bit output: rounded to
    TO), guard rows and gaps keep the sentinel, the kernel that ran is the one the case names, a second launch gives the same bits,
    and batch b of a batched launch equals the single launch on batch b's slice."""
    got, ran = _launch(c)
    assert ran == c["kern"]
    want = gen.expected_bits(c)
    bad = np.argwhere(got.view(np.uint32) != want)
    assert bad.size == 0, (len(bad), bad[:4].ravel().tolist(), got[bad[:4].ravel()].tolist(), want.view(np.float32)[bad[:4].ravel()].tolist())
    again, _ = _launch(c)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))
    if c["batch"] > 1:
        sc = gen.layout(c)["strideC"]
        for b in range(c["batch"]):
            one, ran1 = _launch(c, batch=1, first=b)
            assert ran1 == c["kern"] and np.array_equal(one.view(np.uint32), got[b * sc:(b + 1) * sc].view(np.uint32)), b


@pytest.mark.parametrize("c", gen.FLOAT_CASES, ids=gen.case_id)
def test_float_cases_vs_float64(hip, c):
    """Random and outlier operands pre-rounded to T against float64: every element inside bar = 2·Δout of DESIGN §32."""
    got, ran = _launch(c)
    assert ran == c["kern"]
    ratio = gen.ratio(got, c)
    print(f"MEASURED gemm {gen.case_id(c)}: error / bar = {ratio:.3f}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("c", gen.SWEEP_CASES, ids=gen.case_id)
def test_gelu_sweep_vs_float64(hip, c):
    """z[m, n] = W[n, m] is one exact product: the epilogue's GELU on a dense sweep of [-12, 12], ±0, the fast form's exp2 overflow
    near -10.05 and |z| down to 2^-40 — finite and inside the bound with Δz = 0."""
    got, ran = _launch(c)
    assert ran == c["kern"]
    ratio = gen.ratio(got, c)
    print(f"MEASURED gelu sweep {gen.case_id(c)}: error / bar = {ratio:.3f}")
    assert ratio <= 1.0, ratio


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def test_hook_refuses_bad_arguments(hip):
    """WM_E_ARG, nothing launched, the output sentinel intact."""
    M, N, K = 8, 128, 64
    A, W = np.ones(M * K, np.float32), np.ones((N, K), np.float32)
    out = np.full((M + 1) * N, SENTINEL, np.float32)
    res = np.ones(M * N, np.float32)
    ran = C.c_int32(7)
    ok = dict(C=out, c_len=out.size, A=A, a_len=A.size, W=W, bias=None, pos=None, residual=None, r_len=0, M=M, N=N, K=K, batch=1, lda=K,
              strideA=0, ldc=N, strideC=0, ldr=0, strideR=0, inplace=0, act=0, gelu_mode=0, group_n=0, group_stride=0, dtype=1, out_dtype=1)

    def call(**kw):
        a = dict(ok, **kw)
        return hip.wm_op_gemm_nt_epi(_fp(a["C"]), a["c_len"], _fp(a["A"]), a["a_len"], _fp(a["W"]), _fp(a["bias"]), _fp(a["pos"]),
                                     _fp(a["residual"]), a["r_len"], a["M"], a["N"], a["K"], a["batch"], a["lda"], a["strideA"], a["ldc"],
                                     a["strideC"], a["ldr"], a["strideR"], a["inplace"], a["act"], a["gelu_mode"], a["group_n"],
                                     a["group_stride"], a["dtype"], a["out_dtype"], C.byref(ran) if a.get("ran", True) else None)
    bad = [dict(C=None), dict(A=None), dict(W=None), dict(ran=False), dict(M=0), dict(M=-1), dict(N=0), dict(K=0), dict(batch=0), dict(lda=0),
           dict(ldc=0), dict(dtype=3), dict(dtype=-1), dict(out_dtype=2), dict(out_dtype=3), dict(dtype=0, out_dtype=1),
           dict(N=192), dict(N=64), dict(K=48), dict(K=16), dict(group_n=32, group_stride=(M + 1) * 32), dict(group_n=96, group_stride=(M + 1) * 96),
           dict(inplace=1, out_dtype=1), dict(inplace=1, dtype=2, out_dtype=2),
           dict(a_len=M * K - 1), dict(c_len=M * N - 1), dict(residual=res, r_len=M * N - 1, ldr=N), dict(M=M + 2), dict(batch=2, strideA=M * K, strideC=(M + 1) * N),
           dict(lda=K + 8), dict(ldc=N + 128), dict(lda=K + 1), dict(ldc=N + 2), dict(gelu_mode=2), dict(act=2)]
    for kw in bad:
        assert call(**kw) == WM_E_ARG, kw
        assert (out == SENTINEL).all(), kw
    # the ring kernels are not this hook's: K = 384 without addends (row-panel), N = 384 with fp32 output (full-row)
    W3, A3 = np.ones((N, 384), np.float32), np.ones(M * 384, np.float32)
    assert call(W=W3, A=A3, a_len=A3.size, K=384, lda=384) == WM_E_ARG and ran.value == 2
    W4, o4 = np.ones((384, 128), np.float32), np.full((M + 1) * 384, SENTINEL, np.float32)
    A4 = np.ones(M * 128, np.float32)
    assert call(C=o4, c_len=o4.size, W=W4, A=A4, a_len=A4.size, N=384, K=128, lda=128, ldc=384, out_dtype=0) == WM_E_ARG and ran.value == 3
    assert (out == SENTINEL).all() and (o4 == SENTINEL).all()
    assert call() == 0 and ran.value == 1 and (out[:M * N] == K).all() and (out[M * N:] == SENTINEL).all()
