"""GPU: the kernels of the log-mel front end one at a time (wm_op_fe_*, wm_op_window_gather, and the DFT through wm_op_matmul_nt;
DESIGN §37) against the stage references of tests/test_frontend_ref.py.

A stage that rounds once per element (frames, the clamp / rescale, the gather) is held to numpy's fp32 bit for bit.  A stage that
accumulates is held to float64 under a bound derived from its code, not measured:
  DFT GEMM   |err| <= 417 u sum_n |a_n| per row (u = 2^-24): at most 416 accumulation roundings and one rounding of the basis entry,
             whose magnitude is <= 1.
  mel_log    |err| <= (L + 2) u / ln 10 + 2 ulp32(|ref|), L the filter's band length: the fp32 sum of L non-negative terms, the
             rounding of the coefficient and one rounding of the power (the inputs are chosen so that re^2 and im^2 are exact), carried
             through d log10(s) = ds / (s ln 10); and log10f's documented 2 ulp.
Each such case prints its worst err / bound; the bar is 1."""
import ctypes as C

import numpy as np
import pytest

from test_frontend_ref import (CLAMP, fb64, frames, long_partials, mel_sum, norm, norm_long, rfft_spec, ulp32, window_gather,
                               zero_tails)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FILL = -7.0


@pytest.fixture(scope="module")
def wt():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib, whisper_tensor
    _lib.lib()
    return whisper_tensor


@pytest.fixture(scope="module")
def tables(wt):
    return {n: wt.fe_tables(n) for n in (16, 80)}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- frames -----------------------------------------------------------------------------------------------------------------
# N = 201: the shortest row the long path takes; 360: two frames, the left reflection in both; 330: the left and the right
# reflection in frame 1; 160 000: a chunk at the start, one that ends at the last frame (which reflects on the right), one in the middle
@pytest.mark.parametrize("N,t0,n", [(201, 0, 1), (360, 0, 2), (330, 0, 2), (160000, 0, 3), (160000, 992, 8), (160000, 480, 480)])
def test_frames_bitwise(wt, tables, N, t0, n):
    window = tables[16][0]
    pcm = np.random.default_rng(N + t0).uniform(-1, 1, (3, N)).astype(np.float32)
    lens = [N, 1, 0]  # the samples past a length stay in the buffer: zero_tails_kernel has to clear them before a reflection reads them
    got, guard = wt.fe_frames(pcm, n, t0, n_samples=lens, fill=FILL)
    want = frames(zero_tails(pcm, lens), window, t0, n)
    assert want.dtype == np.float32 and got.shape == want.shape == (3, n, 416)
    assert np.array_equal(bits(got), bits(want))
    assert (bits(got[:, :, 400:]) == 0).all()
    assert (guard == FILL).all(), "a store behind the last frame"
    if t0 == 0:
        assert (got[2] == 0).all() and np.count_nonzero(got[1]) <= 2  # silence, and one sample that two frames at the most see
    raw, guard = wt.fe_frames(pcm, n, t0, fill=FILL)  # no lengths: the rows as they are
    assert np.array_equal(bits(raw), bits(frames(pcm, window, t0, n))) and (guard == FILL).all()


# ---- the DFT as a GEMM: wm_op_matmul_nt(M, 512, 416, fp32) is launch_gemm_nt<float, float> on gemm_nt_kernel, as the runtime's ----
def dft(wt, a, basis):
    out = np.full((a.shape[0], 512), FILL, np.float32)
    wt.matmul(out, a, basis)
    return out


def test_dft_one_hot_rows_return_the_basis(wt, tables):
    basis = tables[16][1]
    a = np.zeros((400, 416), np.float32)
    a[np.arange(400), np.arange(400)] = 1.0
    got = dft(wt, a, basis)
    # row n = column n of the basis; the accumulator starts at +0, so a -0 entry (-sin 0) comes back as +0
    assert np.array_equal(bits(got), bits(basis[:, :400].T + np.float32(0.0)))
    assert (bits(got[:, 201:256]) == 0).all() and (bits(got[:, 457:]) == 0).all()


@pytest.mark.parametrize("M", [1, 129, 777])
def test_dft_against_float64_rfft(wt, tables, M):
    basis = tables[16][1]
    a = np.zeros((M, 416), np.float32)
    a[:, :400] = np.random.default_rng(M).uniform(-1, 1, (M, 400))
    got = dft(wt, a, basis)
    ref = rfft_spec(a)
    bound = 417 * U * np.abs(a.astype(np.float64)).sum(axis=1, keepdims=True)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / bound).max())
    print(f"dft M={M}: worst err / bound = {worst:.4f}")
    assert (err <= bound).all(), (M, worst)
    assert (bits(got[:, 201:256]) == 0).all() and (bits(got[:, 457:]) == 0).all()


# ---- mel_log ----------------------------------------------------------------------------------------------------------------
def mel_log_check(got, spec, n_mels, band, label, cols=None):
    """got [B, n_mels, n] against float64 on the float64 filter bank -> worst err / bound"""
    s = np.asarray(spec, np.float64)
    power = s[..., :201] ** 2 + s[..., 256:457] ** 2
    msum = mel_sum(power, fb64(n_mels))
    assert ((msum == 0) | (msum > 10 * CLAMP)).all(), "a mel sum next to the clamp"
    ref = np.log10(np.maximum(msum, CLAMP))
    L = (band[:, 1] - band[:, 0]).astype(np.float64)
    bound = (L[None, :, None] + 2) * U / np.log(10.0) + 2 * ulp32(ref)
    g = got if cols is None else got[:, :, cols]
    assert g.shape == ref.shape and np.isfinite(g).all()
    err = np.abs(g.astype(np.float64) - ref)
    worst = float((err / bound).max())
    print(f"mel_log {label}: worst err / bound = {worst:.4f}")
    assert (err <= bound).all(), (label, worst, np.argwhere(err > bound)[:4].tolist())
    return worst


def exact_squares(x):
    """x rounded to 11 significant bits: x * x is then exact in fp32"""
    m, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(np.round(m * 2048.0) / 2048.0, e).astype(np.float32)


def random_spec(rng, B, n):
    """re, im with exact squares and re^2 + im^2 in [1e-6, 1] in every bin"""
    amp = np.sqrt(10.0 ** rng.uniform(np.log10(4e-6), np.log10(0.9), (B, n, 201)))
    th = rng.uniform(0, 2 * np.pi, (B, n, 201))
    spec = np.zeros((B, n, 512), np.float32)
    spec[..., :201] = exact_squares(amp * np.cos(th))
    spec[..., 256:457] = exact_squares(amp * np.sin(th))
    p = spec[..., :201].astype(np.float64) ** 2 + spec[..., 256:457].astype(np.float64) ** 2
    assert p.min() >= 1e-6 and p.max() <= 1.0
    spec[..., 201:256] = rng.uniform(-1, 1, (B, n, 55))  # what no filter may read
    spec[..., 457:] = rng.uniform(-1, 1, (B, n, 55))
    return spec


@pytest.mark.parametrize("n_mels", [16, 80])
def test_mel_log_probe_reads_every_coefficient(wt, tables, n_mels):
    """frame f holds one unit bin, f: the output [m][f] is the coefficient fb[f][m] itself, or the clamp outside the band"""
    band = tables[n_mels][3]
    spec = np.zeros((2, 201, 512), np.float32)
    spec[0, np.arange(201), np.arange(201)] = 1.0  # re
    spec[1, np.arange(201), 256 + np.arange(201)] = -1.0  # im; the sign is deliberate: only im^2 enters, so it cannot matter
    got = wt.fe_mel_log(spec, n_mels, logmel=np.full((2, n_mels, 201), FILL, np.float32))
    mel_log_check(got, spec, n_mels, band, f"probe n_mels={n_mels}")
    assert np.array_equal(bits(got[0]), bits(got[1]))
    assert np.unique(bits(got[0][fb64(n_mels).T == 0])).size == 1  # one clamp value wherever the filter is zero


@pytest.mark.parametrize("n_mels", [16, 80])
@pytest.mark.parametrize("n", [1, 31, 33, 64])
def test_mel_log_random_power(wt, tables, n_mels, n):
    spec = random_spec(np.random.default_rng(n_mels * 100 + n), 2, n)
    got = wt.fe_mel_log(spec, n_mels, logmel=np.full((2, n_mels, n), FILL, np.float32))
    mel_log_check(got, spec, n_mels, tables[n_mels][3], f"random n_mels={n_mels} n={n}")


@pytest.mark.parametrize("n_mels", [16, 80])
def test_mel_log_writes_its_chunk_of_a_longer_row_only(wt, tables, n_mels):
    out_frames, t_out, n = 100, 37, 33
    spec = random_spec(np.random.default_rng(n_mels), 2, n)
    got = wt.fe_mel_log(spec, n_mels, out_frames=out_frames, t_out=t_out, logmel=np.full((2, n_mels, out_frames), FILL, np.float32))
    keep = np.r_[0:t_out, t_out + n:out_frames]
    assert (bits(got[:, :, keep]) == bits(np.float32(FILL))).all(), "a store outside the chunk's columns"
    mel_log_check(got, spec, n_mels, tables[n_mels][3], f"chunk n_mels={n_mels}", cols=np.arange(t_out, t_out + n))


# ---- the clamp / rescale ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 1023, 1025, 3200])
def test_mel_norm_bitwise(wt, n):
    rng = np.random.default_rng(n)
    for at in ("ends", 1023):
        if at == 1023 and n <= 1023:
            continue
        x = rng.uniform(-10, 1, (3, n)).astype(np.float32)  # the clamp bites: values down to 11.5 below the maximum
        if at == "ends":
            x[0, 0], x[1, n - 1] = 2.5, 2.25
        else:
            x[0, 1023] = 2.5  # the last element of the first sweep of 1024 threads
        x[2] = -10.0  # silence
        got = wt.fe_mel_norm(x)
        want = norm(x)
        assert want.dtype == np.float32 and np.array_equal(bits(got), bits(want)), (n, at)
        assert (got[2] == -1.5).all()
        if n > 1:
            assert got[0].min() == np.float32((2.5 - 8 + 4) / 4)


@pytest.mark.parametrize("n", [1, 4095, 4097, 256 * 4096 + 5, 2048 * 1024 + 3])
def test_mel_norm_long_bitwise(wt, n):
    """P = min(256, ceil(n / 4096)) partial blocks and G = min(2048, ceil(n / 1024)) blocks in the wide pass: one block, two, and both caps"""
    rng = np.random.default_rng(n)
    x = np.empty((2, n), np.float32)
    x[0] = rng.uniform(-10, 0, n)
    x[1] = rng.uniform(-20, -10, n)
    P, blk = long_partials(n)
    i0 = n - 1
    i1 = int(np.argmax(blk != blk[i0])) if P > 1 else n // 2  # the two maxima in different partial blocks wherever there are two
    x[0, i0] = 3.0  # floors: -5 and -15 -- a row that reduces the other's partials clamps at the wrong value
    if n > 1:
        x[1, i1] = -7.0
    got = wt.fe_mel_norm(x, long_mode=True)
    want = norm(x)
    assert np.array_equal(bits(want), bits(norm_long(x)))
    assert np.array_equal(bits(got), bits(want)), n
    if n > 1:
        assert got[0].min() == np.float32(-0.25) and got[1].min() == np.float32(-2.75) and got[1].max() == np.float32(-0.75)


# ---- the encoder windows of sequential long-form ---------------------------------------------------------------------------
@pytest.mark.parametrize("W", [200, 3000])
def test_window_gather_exact(wt, W):
    F, n_mels = W + 437, 16
    mel = np.random.default_rng(W).uniform(-1, 1, (2, n_mels, F)).astype(np.float32)
    half = W // 2
    items = [(1, 0, W), (0, 37, W - 63), (1, 100, 0), (0, F - half, half), (1, F - W, W), (0, 5, 1)]  # the recordings out of order
    got = wt.window_gather(mel, items, W, fill=FILL)
    assert np.array_equal(bits(got), bits(window_gather(mel, items, W)))
    assert (got[2] == 0).all() and (got[1][:, W - 63:] == 0).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_every_hook_refuses_a_bad_argument(wt):
    from whisper_mojo_amd import _lib
    E_ARG = "error -1"
    pcm = np.zeros((2, 1600), np.float32)
    for bad in (lambda: wt.fe_frames(np.zeros((1, 200), np.float32), 1),  # N <= 200
                lambda: wt.fe_frames(pcm, 0),
                lambda: wt.fe_frames(pcm, 4, 7),  # frames [7, 11) of 10
                lambda: wt.fe_frames(pcm, 1, -1),
                lambda: wt.fe_frames(pcm, 1, 0, n_samples=[1600, 1601]),
                lambda: wt.fe_frames(pcm, 1, 0, n_samples=[-1, 0]),
                lambda: wt.fe_mel_log(np.zeros((1, 4, 512), np.float32), 0),
                lambda: wt.fe_mel_log(np.zeros((1, 4, 512), np.float32), 129),
                lambda: wt.fe_mel_log(np.zeros((1, 4, 512), np.float32), 16, out_frames=8, t_out=5),
                lambda: wt.fe_mel_log(np.zeros((1, 4, 512), np.float32), 16, out_frames=8, t_out=-1),
                lambda: wt.fe_mel_norm(np.zeros((1, 0), np.float32)),
                lambda: wt.window_gather(np.zeros((2, 16, 50), np.float32), [(2, 0, 10)], 20),  # no such recording
                lambda: wt.window_gather(np.zeros((2, 16, 50), np.float32), [(0, 41, 10)], 20),  # seek + len > F
                lambda: wt.window_gather(np.zeros((2, 16, 50), np.float32), [(0, 0, 21)], 20),  # len > W
                lambda: wt.window_gather(np.zeros((2, 16, 50), np.float32), [(0, -1, 5)], 20),
                lambda: wt.window_gather(np.zeros((2, 16, 50), np.float32), [(0, 0, 5)], 0)):
        with pytest.raises(_lib.WhisperMiError, match=E_ARG):
            bad()
    x, y = np.zeros((1, 8), np.float32), np.zeros((1, 8), np.float32)
    fp = C.POINTER(C.c_float)
    L = _lib.lib()
    assert L.wm_op_fe_mel_norm(y.ctypes.data_as(fp), x.ctypes.data_as(fp), 1, 8, 2) == -1  # long_mode is 0 or 1
    assert L.wm_op_fe_mel_norm(None, x.ctypes.data_as(fp), 1, 8, 0) == -1
    assert L.wm_op_fe_mel_norm(y.ctypes.data_as(fp), x.ctypes.data_as(fp), 0, 8, 0) == -1
    assert L.wm_op_fe_frames(None, x.ctypes.data_as(fp), None, 1, 1600, 1, 0) == -1
    assert L.wm_op_fe_mel_log(None, x.ctypes.data_as(fp), 1, 1, 16, 1, 0) == -1
    assert L.wm_op_window_gather(y.ctypes.data_as(fp), x.ctypes.data_as(fp), None, 1, 1, 1, 8, 8) == -1
