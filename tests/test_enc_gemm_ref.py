"""CPU side of the op tests of the encoder's two tiled GEMM kernels, gemm_nt_kernel ("direct") and gemm_nt_lds_kernel ("lds"), and of
the gemm_epilogue they share (the GPU side is tests/test_gpu_enc_gemm_op.py, the hook wm_op_gemm_nt_epi).

Holds the case lists, the float64 references, the per-element bound and float32 numpy restatements of the kernels' arithmetic.  The
tests here prove without a GPU that the exact cases are exact in fp32 in any summation order, that the XCD tile remap is a bijection
on every grid the cases launch, that the restatement alone stays inside every bound, and that the lists cover what they claim.

(a) Exact cases.  A, W integers in [-8, 8]; bias, pos, residual multiples of 1/4 with |.| <= 64; no activation.  Every partial sum is
a multiple of 1/4 below 2^20, so fp32 holds it exactly whatever the order and whether the MFMA rounds or truncates: the output must
equal the float64 reference bit for bit (16-bit output: the reference rounded to TO).

(b) Float cases, per output element, with S = Σ|a_k||w_k| and z = Σ a_k w_k + bias in float64 on operands pre-rounded to T:
    Δz   <= (K + 1)·2^-23·(S + |bias|)                     any order, round or truncate per add       (sweep: z is exact, Δz = 0)
    Δy   <= L_g·Δz + ε_g(z)     act on, L_g = sup|gelu'| < 1.13;      Δy = Δz     act off
    Δout <= Δy + 2^-24·(|y| + |pos| + |res| + |out|) + u_TO·|out| + 2^-120   (+ 2^-25 for f16 output below 2^-14)
    bar   = 2·Δout                                          u_TO = 2^-9 bf16, 2^-12 f16, 0 fp32
2^-120 stands for fp32 subnormal results (flushed or not) of values up to 12·2^-126.

ε_g of the direct kernel (gelu_f: y = 0.5·x·(1 + T(u)) in fp32, T = tanhf / erff), with c_lib the library's ulp bound (OpenCL's
table, which the device library meets: tanh 5, erf 16) and ulp(T) <= 2^-23·|T|:
    mode 0: u = S·(x + C·x³): five roundings, all terms of one sign           Δu <= 5·2^-24·|u|           T' = 1 - T²
    mode 1: u = x·fl(1/√2): one rounding and the constant's own error δc      Δu <= (2^-24 + δc)·|u|      T' = 2/√π·exp(-u²)
    ΔT <= c_lib·2^-23·|T| + T'·Δu;      ε_g = 0.5·|x|·(ΔT + 2^-24·|1 + T|) + 2^-24·|y|
    (1 + T cancels for x < 0: the error is absolute, of order |x|·2^-23, not relative to the small result.)
ε_g of the lds kernel (gelu_fast4).  Mode 1 is the same erff form: the bound above.  Mode 0 is y = x·rcp(1 + exp2(e)),
e = x·fma(x², K2, K1), which is the tanh form rewritten: 0.5·x·(1 + tanh(u)) = x / (1 + 2^e*) with e* = x·(K1* + K2*·x²),
K1* = -2·S·log2(e), K2* = K1*·C.  K1, K2 are fp32 products of fp32 constants, off by δK = max|K/K* - 1| (computed below); x² and the
fma round once each and both terms of the polynomial have one sign, the product rounds once:
    Δe <= |e|·(3·2^-24 + δK)
    t = exp2(e) (1 ulp): relative (ln 2·Δe + 2^-23); it enters y through 1/(1 + t), weight σ = t/(1 + t)
    1 + t: 2^-24;  rcp: 1 ulp = 2^-23;  x·r: 2^-24
    ε_g = |y|·(σ·(ln 2·|e|·(3·2^-24 + δK) + 2^-23) + 2^-22)
σ -> 0 for x > 0 (e << 0), so the relative error there is 2^-22; for x < 0 it grows with |e|·ln 2, which is 87 at x = -10 where
e = 126: 2e-5 relative, of a result below 1e-36.  The header's "relative error ~1e-6" holds for |x| < 4.  Past e = 128 (x < -10.05)
exp2 is inf and the result -0 against a true value below 2^-124: inside the 2^-120 floor.
"""
import functools
import math

import numpy as np
import pytest

from test_enc_ops_ref import DTYPE, SENTINEL, U, _rng, rnd

KERN = ("direct", "lds")
RING = ("rowpanel", "fullrow")  # the ring kernels (tests/test_enc_ring_gemm_ref.py): gelu_fast4 like the lds kernel
EXTRA = {}  # case id -> case of a module that builds on this one; CASES below stays this module's own lists
PAIRS = (("bf16", "bf16"), ("bf16", "f32"), ("f16", "f16"), ("f16", "f32"), ("f32", "f32"))
EPIS = ("none", "bias", "bias_res", "bias_res_inplace", "bias_pos", "bias_pos_res")
L_G = 1.13
FLOOR = 2.0 ** -120
S_PI = np.float32(0.79788456)
COEFF = np.float32(0.044715)
LOG2E32 = np.float32(1.4426950408889634)
K1F = np.float32(np.float32(np.float32(-2.0) * S_PI) * LOG2E32)   # wm_device.h gelu_fast4: constexpr float arithmetic
K2F = np.float32(K1F * COEFF)
K1X = -2.0 * float(S_PI) * 1.4426950408889634
K2X = K1X * float(COEFF)
DELTA_K = max(abs(float(K1F) / K1X - 1.0), abs(float(K2F) / K2X - 1.0))
RSQRT2_32 = np.float32(0.70710678118654752440)
DELTA_C = abs(float(RSQRT2_32) * math.sqrt(2.0) - 1.0)
C_LIB = {0: 5.0, 1: 16.0}


def kernel_for(dt, out, N, K, addends, batch=1, group_n=0):
    """the launcher's dispatch (kernels_encoder.hip gemm_nt_kernel_for) restated: what every case must name"""
    if dt != "f32":
        if out == "f32" and N == 384 and K % 128 == 0 and group_n == 0:
            return "fullrow"
        if batch == 1 and not addends and K == 384 and N <= 3072 and group_n % 128 == 0:
            return "rowpanel"
        if K % 64 == 0:
            return "lds"
    return "direct"


# ---------------------------------------------------------------------------------------------------------------------------------
# cases.  conv = (C_in, stride, L): A is the padded token-major input [batch][L + 2][C_in], lda = stride·C_in, K = 3·C_in,
# M = (L - 1) / stride + 1, strideA = (L + 2)·C_in.

def E(dt, out, M, N, K, epi, kern, batch=1, conv=None, group_n=0):
    return dict(dt=dt, out=out, M=M, N=N, K=K, epi=epi, kern=kern, batch=batch, conv=conv, group_n=group_n, act=None, pat="exact")


def conv_case(dt, out, C, stride, L, N, epi, kern, batch):
    return E(dt, out, (L - 1) // stride + 1, N, 3 * C, epi, kern, batch=batch, conv=(C, stride, L))


def case_id(c):
    s = f"{c['pat']}-{c['kern']}-{c['dt']}-{c['out']}-{c['M']}x{c['N']}x{c['K']}-{c['epi']}"
    if c["batch"] > 1 or c["conv"]:
        s += f"-b{c['batch']}"
    if c["conv"]:
        s += f"-conv{c['conv'][0]}s{c['conv'][1]}"
    if c["group_n"]:
        s += f"-g{c['group_n']}"
    if c["act"] is not None:
        s += f"-gelu{c['act']}"
    if c.get("ldc_pad"):
        s += f"-ldc+{c['ldc_pad']}"
    if c.get("lno"):
        s += "-lno"
    return s


EXACT_CASES = [
    # lds kernel: every M of the ragged list, every N, every K depth, the four 16-bit type pairs, every epilogue form
    E("bf16", "bf16", 1, 128, 64, "none", "lds"),                 # G = 1, nt = 1
    E("bf16", "f32", 63, 256, 128, "bias", "lds"),                # G = 2, one prefetch
    E("f16", "f16", 64, 768, 768, "bias", "lds"),                 # G = 6
    E("f16", "f32", 65, 1024, 1024, "bias_res", "lds"),           # G = 8
    E("bf16", "f32", 127, 768, 2304, "bias_res_inplace", "lds"),  # G = 6, conv2 of small's K
    E("bf16", "bf16", 128, 1024, 3072, "bias_pos", "lds"),        # G = 8
    E("f16", "f32", 129, 768, 4096, "bias_pos_res", "lds"),       # G = 12
    E("f16", "f16", 200, 256, 64, "bias", "lds"),                 # G = 4
    E("bf16", "f32", 257, 768, 128, "bias_res_inplace", "lds"),   # G = 18
    E("bf16", "bf16", 257, 1024, 768, "none", "lds"),             # G = 24
    E("f16", "f32", 257, 128, 1024, "bias_pos", "lds"),           # G = 3
    E("bf16", "f32", 769, 128, 64, "bias_res", "lds"),            # G = 7: seven row panels
    E("f16", "f16", 129, 128, 4096, "none", "lds"),               # G = 2
    E("bf16", "f32", 65, 256, 384, "bias_res", "lds"),            # K = 384 with an addend: not the row-panel kernel
    # direct kernel: fp32 at K = 32, 96, 768; 16-bit at K = 96 and 288 (conv1's K)
    E("f32", "f32", 65, 128, 32, "none", "direct"),
    E("f32", "f32", 129, 256, 96, "bias_res_inplace", "direct"),
    E("f32", "f32", 257, 768, 768, "bias_pos_res", "direct"),
    E("f32", "f32", 1, 1024, 96, "bias", "direct"),
    E("f32", "f32", 63, 128, 768, "bias_pos", "direct"),
    E("f32", "f32", 128, 256, 32, "bias_res", "direct"),
    E("bf16", "bf16", 127, 128, 96, "bias", "direct"),
    E("f16", "f32", 200, 256, 288, "bias_res", "direct"),
    E("bf16", "f32", 64, 768, 288, "bias_pos", "direct"),
    E("f16", "f16", 129, 1024, 96, "none", "direct"),
    # conv form, batch 1, 2, 3: lda = C and 2C, K = 3C
    conv_case("bf16", "bf16", 96, 1, 130, 128, "bias", "direct", 2),
    conv_case("f32", "f32", 96, 2, 129, 256, "bias_res", "direct", 3),
    conv_case("f16", "f32", 256, 2, 513, 128, "bias_pos", "lds", 3),       # G = 9
    conv_case("bf16", "f32", 768, 1, 65, 256, "bias_res", "lds", 2),       # G = 4
    conv_case("f16", "f32", 256, 1, 129, 256, "bias_pos_res", "lds", 2),   # G = 8
    conv_case("bf16", "bf16", 768, 2, 63, 128, "bias", "lds", 1),          # G = 1
    # cross-K/V scatter
    E("f16", "f32", 129, 1536, 768, "bias", "lds", group_n=768),           # G = 24
    E("bf16", "bf16", 65, 3072, 128, "none", "lds", group_n=768),          # G = 24
    E("bf16", "f32", 63, 2048, 1024, "bias", "lds", group_n=1024),         # G = 16
    E("f16", "f16", 200, 4096, 64, "bias", "lds", group_n=1024),           # G = 64
    E("f32", "f32", 65, 1536, 32, "bias", "direct", group_n=768),
]


def F(dt, out, K, act, pat, kern, M=129, N=256):
    epi = {None: "bias_res", 0: "bias_pos", 1: "bias"}[act]
    return dict(dt=dt, out=out, M=M, N=N, K=K, epi=epi, kern=kern, batch=1, conv=None, group_n=0, act=act, pat=pat)


FLOAT_CASES = ([F(dt, out, K, act, "normal", "direct" if dt == "f32" else "lds")
                for K in (64, 768, 4096) for dt, out in PAIRS for act in (None, 0, 1)] +
               [F(dt, out, K, act, "outlier", "direct" if dt == "f32" else "lds")
                for K in (768, 4096) for dt, out in PAIRS for act in (None, 0)] +
               [F(dt, out, 288, act, "normal", "direct") for dt, out in PAIRS if dt != "f32" for act in (None, 0, 1)])


def G(dt, out, K, mode, kern):
    return dict(dt=dt, out=out, M=K, N=256, K=K, epi="none", kern=kern, batch=1, conv=None, group_n=0, act=mode, pat="sweep")


SWEEP_CASES = ([G(dt, out, 64, mode, "direct" if dt == "f32" else "lds") for dt, out in PAIRS for mode in (0, 1)] +
               [G(dt, out, 96, mode, "direct") for dt, out in PAIRS if dt != "f32" for mode in (0, 1)])


def grid_of(c):
    return (c["N"] // 128, (c["M"] + 127) // 128, c["batch"])


# ---------------------------------------------------------------------------------------------------------------------------------
# layouts and operands

def layout(c):
    """element counts and strides of the hook call: one guard row after the last row of every batch and of every column group"""
    M, N, K, B = c["M"], c["N"], c["K"], c["batch"]
    gn = c["group_n"]
    row_w = gn if gn else N
    ldc = row_w + c.get("ldc_pad", 0)  # ldc_pad: columns between the rows of C that the kernel must leave alone
    n_grp = N // gn if gn else 1
    group_stride = (M + 1) * ldc
    strideC = n_grp * group_stride
    if c["conv"]:
        Cin, stride, L = c["conv"]
        lda, strideA = stride * Cin, (L + 2) * Cin
    else:
        lda, strideA = K, M * K
    a_len = (B - 1) * strideA + (M - 1) * lda + K
    ldr, strideR = N + 8, M * (N + 8) + 16  # ldr > N, strideR != strideC
    return dict(ldc=ldc, row_w=row_w, n_grp=n_grp, group_stride=group_stride, strideC=strideC, c_len=B * strideC, lda=lda, strideA=strideA, a_len=a_len,
                ldr=ldr, strideR=strideR, r_len=B * strideR)


def cells(lay, base, M):
    """the M rows of row_w columns at base, ldc apart, as an index into the flat C: a slice where the rows touch (val then ravelled)"""
    if lay["ldc"] == lay["row_w"]:
        return slice(base, base + M * lay["ldc"])
    return base + np.arange(M)[:, None] * lay["ldc"] + np.arange(lay["row_w"])[None, :]


def put(flat, lay, base, M, val):
    flat[cells(lay, base, M)] = val if lay["ldc"] != lay["row_w"] or np.ndim(val) == 0 else np.asarray(val).reshape(-1)


def _rows(flat, base, M, ld, width):
    return np.lib.stride_tricks.as_strided(flat[base:], (M, width), (ld * flat.itemsize, flat.itemsize), writeable=False)


def _case(cid):
    return CASES[cid] if cid in CASES else EXTRA[cid]


def sweep_values(dt):
    """256·K z values are available; the sweep uses the first 16384: dense over [-12, 12], the exp2 overflow of the fast form near
    -10.05, ±0, |x| < 2^-10 down to 2^-40, ±12 — rounded to T"""
    k = np.arange(10, 41, dtype=np.float64)
    small = np.concatenate([2.0 ** -k, -(2.0 ** -k), 1.5 * 2.0 ** -k])
    v = np.concatenate([[0.0, -0.0, 12.0, -12.0], small, np.linspace(-10.2, -9.9, 3000), np.linspace(-12.0, 12.0, 16384 - 4 - small.size - 3000)])
    assert v.size == 16384
    return rnd(v.astype(np.float32), dt)


@functools.lru_cache(maxsize=None)
def _operands(cid):
    c = _case(cid)
    lay = layout(c)
    r = _rng(cid)
    M, N, K, B = c["M"], c["N"], c["K"], c["batch"]
    dt = c["dt"]
    if c["pat"] == "exact":
        A = r.integers(-8, 9, lay["a_len"]).astype(np.float32)
        W = r.integers(-8, 9, (N, K)).astype(np.float32)
        q = lambda n: (r.integers(-256, 257, n) / 4.0).astype(np.float32)
    elif c["pat"] == "sweep":
        z = sweep_values(dt)
        W = np.zeros((N, K), np.float32)
        W[:256, :64] = z.reshape(256, 64)  # z[m, n] = W[n, m] for m < 64, n < 256; rows 64.. of a deeper K read zero columns
        A = np.eye(M, K, dtype=np.float32).ravel()
        q = None
    else:
        s = K ** -0.25  # both operands scaled: the product carries 1/sqrt(K) and z ~ N(0, 1)
        A = (r.standard_normal(lay["a_len"]) * s).astype(np.float32)
        W = (r.standard_normal((N, K)) * s).astype(np.float32)
        if c["pat"] == "outlier":  # 2^12 in one k-panel of every seventh row
            A2 = A.reshape(M, K)
            A2[3::7, K // 2 + 5] = 4096.0
        A, W = rnd(A, dt), rnd(W, dt)
        q = lambda n: r.standard_normal(n).astype(np.float32)
    epi = c["epi"]
    bias = q(N) if "bias" in epi else None
    pos = q(M * N).reshape(M, N) if "pos" in epi else None
    res = None
    if "res" in epi:
        if epi.endswith("inplace"):
            res = [q(M * N).reshape(M, N) for _ in range(B)]
        else:
            flat = q(lay["r_len"])
            res = [_rows(flat, b * lay["strideR"], M, lay["ldr"], N) for b in range(B)]
            res.append(flat)
    for a in (A, W, bias, pos):
        if a is not None:
            a.setflags(write=False)
    return A, W, bias, pos, res


def operands(c):
    return _operands(case_id(c))


def c_init(c):
    """the caller's C: sentinel everywhere, the residual rows where the launch runs in place"""
    lay = layout(c)
    C0 = np.full(lay["c_len"], SENTINEL, np.float32)
    if c["epi"].endswith("inplace"):
        res = operands(c)[4]
        for b in range(c["batch"]):
            put(C0, lay, b * lay["strideC"], c["M"], res[b])
    return C0


def a_rows(c, b):
    lay = layout(c)
    return _rows(operands(c)[0], b * lay["strideA"], c["M"], lay["lda"], c["K"])


def gelu64(z, mode):
    """the two forms without the cancellation of 1 + tanh / 1 + erf at negative z (float64's own 1 + tanh(u) is 0 below u = -19):
    0.5·z·(1 + tanh(u)) = z / (1 + exp(-2u)) and 0.5·z·(1 + erf(v)) = 0.5·z·erfc(-v), the same real functions"""
    z = np.asarray(z, np.float64)
    if mode == 0:
        with np.errstate(over="ignore"):
            return z / (1.0 + np.exp(-2.0 * float(S_PI) * (z + float(COEFF) * z ** 3)))
    erfc = np.frompyfunc(math.erfc, 1, 1)
    return 0.5 * z * erfc(-z / math.sqrt(2.0)).astype(np.float64)


def eps_gelu(z, y, mode, kern):
    """the module docstring's eps_g at z (float64), y = gelu64(z, mode)"""
    x, ay = np.asarray(z, np.float64), np.abs(y)
    if kern != "direct" and mode == 0:
        e = x * (K1X + K2X * x * x)
        with np.errstate(divide="ignore", invalid="ignore"):
            sigma = np.clip(np.where(x != 0, 1.0 - y / x, 0.5), 0.0, 1.0)  # t / (1 + t) = 1 - y / x
        return ay * (sigma * (math.log(2.0) * np.abs(e) * (3 * 2.0 ** -24 + DELTA_K) + 2.0 ** -23) + 2.0 ** -22)
    if mode == 0:
        u = float(S_PI) * (x + float(COEFF) * x ** 3)
        T = np.tanh(u)
        dT, du = 1.0 - T * T, 5 * 2.0 ** -24 * np.abs(u)
    else:
        u = x / math.sqrt(2.0)
        T = np.frompyfunc(math.erf, 1, 1)(u).astype(np.float64)
        dT, du = 2.0 / math.sqrt(math.pi) * np.exp(-u * u), (2.0 ** -24 + DELTA_C) * np.abs(u)
    return 0.5 * np.abs(x) * (C_LIB[mode] * 2.0 ** -23 * np.abs(T) + dT * du + 2.0 ** -24 * np.abs(1.0 + T)) + 2.0 ** -24 * ay


@functools.lru_cache(maxsize=None)
def _reference(cid):
    """-> (expected flat C in float64 with the untouched cells at the sentinel, bar per cell or None for an exact case)"""
    c = _case(cid)
    lay = layout(c)
    A, W, bias, pos, res = operands(c)
    M, N, gn = c["M"], c["N"], c["group_n"]
    want = c_init(c).astype(np.float64)
    bar = None if c["pat"] == "exact" else np.zeros(lay["c_len"])
    W64, aW = W.astype(np.float64), np.abs(W.astype(np.float64))
    for b in range(c["batch"]):
        Ab = a_rows(c, b).astype(np.float64)
        z = Ab @ W64.T
        bb = 0.0 if bias is None else bias.astype(np.float64)[None, :]
        z = z + bb
        y = z if c["act"] is None else gelu64(z, c["act"])
        p = 0.0 if pos is None else pos.astype(np.float64)
        rr = 0.0 if res is None else res[b].astype(np.float64)
        out = y + p + rr
        if bar is not None:
            dz = 0.0 if c["pat"] == "sweep" else (c["K"] + 1) * 2.0 ** -23 * (np.abs(Ab) @ aW.T + np.abs(bb))
            dy = dz if c["act"] is None else L_G * dz + eps_gelu(z, y, c["act"], c["kern"])
            d = dy + 2.0 ** -24 * (np.abs(y) + np.abs(p) + np.abs(rr) + np.abs(out)) + U[c["out"]] * np.abs(out) + FLOOR
            if c["out"] == "f16":
                d = d + np.where(np.abs(out) < 2.0 ** -14, 2.0 ** -25, 0.0)
            d = 2.0 * d
        for g in range(lay["n_grp"]):
            base = b * lay["strideC"] + g * lay["group_stride"]
            cols = slice(g * gn, (g + 1) * gn) if gn else slice(0, N)
            put(want, lay, base, M, out[:, cols])
            if bar is not None:
                put(bar, lay, base, M, d[:, cols])
    want.setflags(write=False)
    return want, bar


def reference(c):
    return _reference(case_id(c))


def written_mask(c):
    lay = layout(c)
    m = np.zeros(lay["c_len"], bool)
    for b in range(c["batch"]):
        for g in range(lay["n_grp"]):
            base = b * lay["strideC"] + g * lay["group_stride"]
            put(m, lay, base, c["M"], True)
    return m


def expected_bits(c):
    """an exact case's output as the hook returns it: the float64 reference rounded to TO (exact for fp32), sentinel elsewhere"""
    want, _ = reference(c)
    w32 = want.astype(np.float32)
    assert (w32.astype(np.float64) == want).all()
    return rnd(w32, c["out"]).view(np.uint32)


def ratio(got, c):
    """largest |got - ref| / bar over the written cells (0 / 0 = 0), after checking that nothing else was written"""
    want, bar = reference(c)
    m = written_mask(c)
    assert (got[~m] == SENTINEL).all(), "a guard row was written"
    err = np.abs(got[m].astype(np.float64) - want[m])
    assert np.isfinite(got[m]).all()
    return float(np.max(np.where(err > 0, err / np.maximum(bar[m], 1e-300), 0.0)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic restated in float32 numpy

def remap(lin, gx, gy, gz):
    """gemm_nt_lds_kernel's XCD-aware tile order: linear workgroup id -> (bx, by, bz)"""
    G = gx * gy * gz
    x, q, per, rem = lin & 7, lin >> 3, G >> 3, G & 7
    t = x * per + min(x, rem) + q
    return t % gx, (t // gx) % gy, t // gx // gy


def gelu_fast_f32(x, mode):
    x = np.asarray(x, np.float32)
    if mode == 1:
        return gelu_f_f32(x, 1)
    with np.errstate(over="ignore", under="ignore"):
        x2 = (x * x).astype(np.float32)
        poly = (x2.astype(np.float64) * float(K2F) + float(K1F)).astype(np.float32)  # one rounding: the fma
        e = (x * poly).astype(np.float32)
        d = (np.exp2(e).astype(np.float32) + np.float32(1.0)).astype(np.float32)
        return (x * (np.float32(1.0) / d).astype(np.float32)).astype(np.float32)


def gelu_f_f32(x, mode):
    x = np.asarray(x, np.float32)
    if mode == 0:
        x3 = ((x * x).astype(np.float32) * x).astype(np.float32)
        inner = (S_PI * (x + (COEFF * x3).astype(np.float32)).astype(np.float32)).astype(np.float32)
        t = np.tanh(inner).astype(np.float32)
    else:
        u = (x * RSQRT2_32).astype(np.float32)
        t = np.frompyfunc(math.erf, 1, 1)(u.astype(np.float64)).astype(np.float64).astype(np.float32)
    return ((np.float32(0.5) * x).astype(np.float32) * (np.float32(1.0) + t).astype(np.float32)).astype(np.float32)


def restate(c):
    """the flat C the kernels' arithmetic gives in float32: one fp32 accumulator per element, advanced one MFMA at a time (k-steps of
    32 for 16-bit operands, of 4 for fp32; inside a step the sum is taken in float64 and rounded once), then gemm_epilogue's order:
    v = acc + bias; v = gelu(v); v += (res + pos); round to TO"""
    lay = layout(c)
    A, W, bias, pos, res = operands(c)
    M, N, K, gn = c["M"], c["N"], c["K"], c["group_n"]
    step = 4 if c["dt"] == "f32" else 32
    got = c_init(c)
    W64 = W.astype(np.float64)
    for b in range(c["batch"]):
        Ab = a_rows(c, b).astype(np.float64)
        acc = np.zeros((M, N), np.float32)
        for k0 in range(0, K, step):
            acc = (acc + (Ab[:, k0:k0 + step] @ W64[:, k0:k0 + step].T).astype(np.float32)).astype(np.float32)
        v = acc if bias is None else (acc + bias[None, :]).astype(np.float32)
        if c["act"] is not None:
            v = gelu_fast_f32(v, c["act"]) if c["kern"] == "lds" else gelu_f_f32(v, c["act"])
        ex = np.zeros((M, N), np.float32)
        if res is not None:
            ex = np.array(res[b], np.float32)
        if pos is not None:
            ex = (ex + pos).astype(np.float32)
        v = rnd((v + ex).astype(np.float32), c["out"])
        for g in range(lay["n_grp"]):
            base = b * lay["strideC"] + g * lay["group_stride"]
            cols = slice(g * gn, (g + 1) * gn) if gn else slice(0, N)
            put(got, lay, base, M, v[:, cols])
    return got


CASES = {case_id(c): c for c in EXACT_CASES + FLOAT_CASES + SWEEP_CASES}
RESTATED = {}  # (kern, dt, out, act) -> the restatement's largest error / bar (DESIGN §32's second column)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU tests

def test_case_ids_are_unique():
    assert len(CASES) == len(EXACT_CASES) + len(FLOAT_CASES) + len(SWEEP_CASES)


@pytest.mark.parametrize("c", EXACT_CASES, ids=case_id)
def test_exact_cases_are_exact_in_fp32_ref(c):
    """Operands are integers in [-8, 8] (exact in bf16 and f16), addends multiples of 1/4 up to 64, and Σ|a||w| + the addends stays
    below 2^20: every partial sum in any order is a multiple of 1/4 below 2^20, which fp32 holds exactly.  The restatement (one summation
    order) and a reversed order both reproduce the float64 reference bit for bit."""
    A, W, bias, pos, res = operands(c)
    for a in (A, W):
        assert (a == np.round(a)).all() and np.abs(a).max() <= 8
        assert (rnd(a, "bf16") == a).all() and (rnd(a, "f16") == a).all()
    add = np.zeros((c["M"], c["N"]))
    for a in (bias, pos) + tuple(res[:c["batch"]] if res else ()):
        if a is not None:
            assert (a * 4 == np.round(a * 4)).all() and np.abs(a).max() <= 64
    n_add = sum(x in c["epi"] for x in ("bias", "pos", "res"))
    worst = 0.0
    for b in range(c["batch"]):
        worst = max(worst, float((np.abs(a_rows(c, b).astype(np.float64)) @ np.abs(W.astype(np.float64)).T).max()))
    assert worst + 64 * n_add < 2 ** 20 and c["K"] <= 4096
    assert c["act"] is None
    bits = expected_bits(c)
    assert np.array_equal(restate(c).view(np.uint32), bits)
    m = written_mask(c)
    assert (reference(c)[0][~m] == SENTINEL).all() and (~m).sum() >= c["batch"] * layout(c)["n_grp"] * layout(c)["ldc"]


def test_remap_is_a_bijection_ref():
    """On every grid an lds case launches (and every G up to 64 besides) the remap maps [0, G) one-to-one onto the tiles."""
    grids = {grid_of(c) for c in CASES.values() if c["kern"] == "lds"} | {(g, 1, 1) for g in range(1, 65)} | {(2, 3, 3), (6, 3, 1)}
    for gx, gy, gz in grids:
        G = gx * gy * gz
        tiles = {remap(lin, gx, gy, gz) for lin in range(G)}
        assert len(tiles) == G and all(0 <= x < gx and 0 <= y < gy and 0 <= z < gz for x, y, z in tiles), (gx, gy, gz)


@pytest.mark.parametrize("c", FLOAT_CASES + SWEEP_CASES, ids=case_id)
def test_restatement_inside_the_bound_ref(c):
    r = ratio(restate(c), c)
    key = (c["kern"], c["dt"], c["out"], c["act"])
    RESTATED[key] = max(RESTATED.get(key, 0.0), r)
    print(f"RESTATED {case_id(c)}: error / bar = {r:.3f}")
    assert r <= 1.0, r


def test_cases_cover_what_they_are_there_for():
    ex = EXACT_CASES
    for c in CASES.values():  # every case names the kernel the dispatch picks, and none reaches the ring kernels
        addends = any(x in c["epi"] for x in ("res", "pos"))
        assert kernel_for(c["dt"], c["out"], c["N"], c["K"], addends, c["batch"], c["group_n"]) == c["kern"] in KERN, case_id(c)
        assert not (c["N"] == 384 and c["out"] == "f32") and not (c["K"] == 384 and not addends)
        assert c["N"] % 128 == 0 and c["K"] % 32 == 0 and (c["group_n"] == 0 or c["N"] % c["group_n"] == 0)
    lds = [c for c in ex if c["kern"] == "lds"]
    direct = [c for c in ex if c["kern"] == "direct"]
    assert {1, 63, 64, 65, 127, 128, 129, 200, 257} <= {c["M"] for c in lds} and {1, 63, 64, 65, 127, 128, 129, 200, 257} <= {c["M"] for c in ex}
    assert {128, 256, 768, 1024} <= {c["N"] for c in lds} and {128, 256, 768, 1024} <= {c["N"] for c in direct}
    assert {64, 128, 768, 1024, 2304, 3072, 4096} <= {c["K"] for c in lds}
    assert {32, 96, 768} <= {c["K"] for c in direct if c["dt"] == "f32"}
    assert {96, 288} <= {c["K"] for c in direct if c["dt"] != "f32"}
    assert {(c["dt"], c["out"]) for c in lds} == set(PAIRS[:4]) and {(c["dt"], c["out"]) for c in direct} == set(PAIRS)
    assert {c["epi"] for c in lds} == set(EPIS) and {c["epi"] for c in direct} == set(EPIS)
    conv = [c for c in ex if c["conv"]]
    assert {c["batch"] for c in conv} == {1, 2, 3}
    assert {(c["conv"][0], c["conv"][1], c["kern"]) for c in conv} >= {(96, 1, "direct"), (96, 2, "direct"), (256, 1, "lds"), (256, 2, "lds"),
                                                                        (768, 1, "lds"), (768, 2, "lds")}
    for c in conv:
        lay = layout(c)
        assert c["K"] == 3 * c["conv"][0] and lay["lda"] < c["K"] and lay["strideA"] == (c["conv"][2] + 2) * c["conv"][0]
        assert lay["strideC"] == (c["M"] + 1) * lay["ldc"] and lay["strideR"] != lay["strideC"] and lay["ldr"] > c["N"]
        # the last window of a batch ends inside that batch's padded input
        assert (c["M"] - 1) * lay["lda"] + c["K"] <= lay["strideA"]
    sc = [c for c in ex if c["group_n"]]
    assert {(c["group_n"], c["N"] // c["group_n"]) for c in sc} >= {(768, 2), (768, 4), (1024, 2), (1024, 4)}
    assert {c["out"] for c in sc} >= {"f32", "bf16", "f16"} and all(layout(c)["group_stride"] == (c["M"] + 1) * layout(c)["ldc"] for c in sc)
    Gs = {math.prod(grid_of(c)) for c in lds}
    assert {1, 3, 7, 8, 9, 12, 18, 24} <= Gs
    # float cases: K = 64, 768, 4096 at 129 x 256 for the five pairs, each with no activation and both GELU modes; the outlier; the sweep
    for K in (64, 768, 4096):
        assert {(c["dt"], c["out"], c["act"]) for c in FLOAT_CASES if c["K"] == K and c["pat"] == "normal" and (c["M"], c["N"]) == (129, 256)} == \
            {(d, o, a) for d, o in PAIRS for a in (None, 0, 1)}
    assert any(c["pat"] == "outlier" and np.abs(operands(c)[0]).max() == 4096.0 for c in FLOAT_CASES)
    assert {(c["kern"], c["act"], c["out"] == "f32") for c in SWEEP_CASES} == {(k, m, f) for k in KERN for m in (0, 1) for f in (True, False)}
    for dt in ("bf16", "f16", "f32"):
        z = sweep_values(dt)
        assert z.min() == -12.0 and z.max() == 12.0 and (z == 0).sum() >= 2 and np.signbit(z[z == 0]).any()
        assert ((z > -10.1) & (z < -10.0)).any() and ((np.abs(z) < 2.0 ** -10) & (z != 0)).sum() >= 40  # f16 flushes what lies below 2^-24
        assert (np.diff(np.sort(np.unique(z))) <= (0.13 if dt == "bf16" else 0.01)).all()
    # the fast form's exponent crosses exp2's overflow inside the sweep
    assert -float(np.float32(-10.2)) * (K1X + K2X * 10.2 ** 2) < -128 or float(np.float32(-10.2)) * (K1X + K2X * 10.2 ** 2) > 128
    assert DELTA_K < 2.0 ** -22 and DELTA_C < 2.0 ** -24
