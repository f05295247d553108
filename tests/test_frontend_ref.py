"""CPU only: the numpy restatement of the log-mel front end one stage at a time, and the host tables of the library
(wm_op_fe_tables) against float64.

The stage references are what tests/test_gpu_frontend_op.py holds the kernels of kernels_frontend.hip to: `frames`, `rfft_power`,
`mel_log`, `norm` and `norm_long` compute in the dtype they are given, so the same functions serve as the bitwise fp32 reference of a
one-rounding stage and as the float64 reference of a stage that accumulates.  Chained in float64 they are the oracle's log_mel."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import golden

N_FFT, HOP, N_FREQ, COLS = 400, 160, 201, 416
CLAMP = 1e-10


# ---- tables in float64 ------------------------------------------------------------------------------------------------------
def window64():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)  # periodic Hann


def basis64():
    """[512, 416]: row k = cos(2 pi k n / 400), row 256 + k = -sin(...), k < 201, n < 400; the angle reduced in integers first."""
    r = (np.arange(N_FREQ)[:, None] * np.arange(N_FFT)[None, :]) % N_FFT
    ang = 2.0 * np.pi * r.astype(np.float64) / N_FFT
    b = np.zeros((512, COLS), np.float64)
    b[:N_FREQ, :N_FFT] = np.cos(ang)
    b[256:256 + N_FREQ, :N_FFT] = -np.sin(ang)
    return b


def fb64(n_mels):
    from oracle import logmel_oracle as lo
    return lo.mel_filter_bank(n_mels=n_mels)  # [201, n_mels]


def ulp32(x):
    """the spacing of float32 at |x| (x float64 or float32), as float64"""
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


# ---- stage references -------------------------------------------------------------------------------------------------------
def zero_tails(pcm, lens):
    x = np.array(pcm, copy=True)
    for b, n in enumerate(lens):
        x[b, int(n):] = 0
    return x


def frames(pcm, window, t0, n):
    """pcm [B, N] -> [B, n, 416]: frame t holds pcm[reflect(160 (t0 + t) + j - 200)] * window[j] for j < 400 (numpy 'reflect': the
    edge sample is not repeated), zeros in columns 400..415.  One multiply per element in the dtype of pcm and window."""
    B, N = pcm.shape
    i = HOP * (t0 + np.arange(n))[:, None] + np.arange(N_FFT)[None, :] - N_FFT // 2
    i = np.where(i < 0, -i, i)
    i = np.where(i >= N, 2 * (N - 1) - i, i)
    assert i.min() >= 0 and i.max() < N
    out = np.zeros((B, n, COLS), np.result_type(pcm, window))
    out[:, :, :N_FFT] = pcm[:, i] * window[None, None, :]
    return out


def rfft_spec(fr):
    """frames [..., 416] -> float64 [..., 512] as the DFT GEMM lays it out: re at k, im at 256 + k, zeros elsewhere"""
    X = np.fft.rfft(np.asarray(fr, np.float64)[..., :N_FFT], axis=-1)
    out = np.zeros(fr.shape[:-1] + (512,), np.float64)
    out[..., :N_FREQ] = X.real
    out[..., 256:256 + N_FREQ] = X.imag
    return out


def rfft_power(fr):
    s = rfft_spec(fr)
    return s[..., :N_FREQ] ** 2 + s[..., 256:256 + N_FREQ] ** 2


def mel_sum(power, fb):
    """power [B, n, 201], fb [201, n_mels] -> float64 [B, n_mels, n]"""
    return np.einsum("bnk,km->bmn", np.asarray(power, np.float64), np.asarray(fb, np.float64))


def mel_log(power, fb):
    return np.log10(np.maximum(mel_sum(power, fb), CLAMP))


def norm(x):
    """rows [B, n] -> (max(x, rowmax - 8) + 4) / 4 in the dtype of x, one operation at a time"""
    t = x.dtype.type
    floor = x.max(axis=1, keepdims=True) - t(8)
    return (np.maximum(x, floor) + t(4)) / t(4)


def long_partials(n):
    """P of launch_mel_norm_long and, per element, the partial block that reduces it: element i belongs to block (i // 256) % P"""
    P = min(256, (n + 4095) // 4096)
    return P, (np.arange(n) // 256) % P


def norm_long(x):
    """norm as the long path computes it: per row P partial maxima, their maximum, then the same clamp and rescale"""
    t = x.dtype.type
    P, blk = long_partials(x.shape[1])
    part = np.full((x.shape[0], P), -np.inf, x.dtype)
    for b in range(x.shape[0]):
        np.maximum.at(part[b], blk, x[b])
    floor = part.max(axis=1, keepdims=True) - t(8)
    return (np.maximum(x, floor) + t(4)) / t(4)


def window_gather(mel, items, W):
    out = np.zeros((len(items), mel.shape[1], W), mel.dtype)
    for r, (b, seek, ln) in enumerate(items):
        out[r, :, :ln] = mel[b, :, seek:seek + ln]
    return out


def long_chunk_frames(F, B, long_fe_rows=16 * 3000):
    """nt of frontend_long_run: frames per chunk and utterance"""
    return max(32, min((F + 31) // 32 * 32, long_fe_rows // B // 32 * 32))


def log_mel_chain(audio, n_frames, n_mels):
    """the five stages chained in float64 on one clip padded / trimmed to the window"""
    N = HOP * n_frames
    x = np.zeros((1, N), np.float64)
    a = np.asarray(audio, np.float64)[:N]
    x[0, :len(a)] = a
    lg = mel_log(rfft_power(frames(x, window64(), 0, n_frames)), fb64(n_mels))  # [1, n_mels, n_frames]
    return lg.reshape(1, -1), n_mels, n_frames


# ---- the references against the oracle --------------------------------------------------------------------------------------
def test_chained_stages_reproduce_the_oracle():
    from oracle import logmel_oracle as lo
    g = golden("logmel")
    for i in range(4):
        audio = lo.synth_audio(int(g[f"seed{i}"]), int(g[f"n{i}"]))
        lg, n_mels, n_frames = log_mel_chain(audio, 3000, 80)
        want = lo.log_mel(audio).astype(np.float64)
        for fn in (norm, norm_long):
            got = fn(lg).reshape(n_mels, n_frames)
            err = np.abs(got - want).max()
            print(f"logmel case {i} {fn.__name__}: max |chain - oracle| = {err:.3e}")
            assert err <= 1e-6, (i, fn.__name__, err)
        # and with it the HF fixture, within the bounds tests/test_logmel.py holds the oracle to
        got32 = norm(lg).reshape(n_mels, n_frames).astype(np.float32)
        assert np.abs(got32[:, g["cols"]] - g[f"mel{i}_cols"]).max() < 5e-5
        assert np.abs(got32.astype(np.float64).sum(1) - g[f"mel{i}_rowsum"]).max() < 5e-2
        assert np.abs(got32.astype(np.float64).sum(0) - g[f"mel{i}_colsum"]).max() < 2e-3


def test_frames_reference_is_numpy_reflect_padding():
    rng = np.random.default_rng(0)
    w = window64()
    for N, F in ((201, 1), (360, 2), (1600, 10)):
        x = rng.uniform(-1, 1, (2, N))
        xp = np.pad(x, ((0, 0), (200, 200)), mode="reflect")
        idx = np.arange(N_FFT)[None, :] + HOP * np.arange(F)[:, None]
        want = xp[:, idx] * w
        got = frames(x, w, 0, F)
        assert np.array_equal(got[:, :, :N_FFT], want) and (got[:, :, N_FFT:] == 0).all()
        for t0 in range(F):  # a chunk that starts at t0 is a slice of the whole
            assert np.array_equal(frames(x, w, t0, F - t0), got[:, t0:])


def test_norm_long_equals_norm_bit_for_bit():
    rng = np.random.default_rng(1)
    for n in (1, 255, 4095, 4097, 256 * 4096 + 5):
        x = rng.uniform(-10, 2, (2, n)).astype(np.float32)
        x[1] -= 9
        assert np.array_equal(norm(x).view(np.uint32), norm_long(x).view(np.uint32)), n
    assert norm(np.full((1, 7), -10, np.float32)).tolist() == [[-1.5] * 7]  # silence


def test_basis_and_window_against_independent_forms():
    """the float64 tables the library is held to, against numpy's own: rfft of the identity and np.hanning"""
    X = np.fft.rfft(np.eye(N_FFT), axis=1).T  # [201, 400]: X[k, n] = exp(-2 pi i k n / 400)
    b = basis64()
    assert np.abs(b[:N_FREQ, :N_FFT] - X.real).max() < 1e-14 and np.abs(b[256:256 + N_FREQ, :N_FFT] - X.imag).max() < 1e-14
    assert np.abs(window64() - np.hanning(N_FFT + 1)[:-1]).max() < 1e-15


# ---- the library's tables ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wt():
    """Host-only calls into the library.  torch comes first where it is installed: a process that loads libwhispermi.so before it
    imports torch gets `no ROCm-capable device is detected` from the library's first HIP call once torch has initialised HIP, so
    this file run in front of a GPU test file (pytest tests/test_frontend_ref.py tests/test_gpu_frontend_op.py) would fail that
    file.  The whole suite imports torch while it collects."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    from whisper_mojo_amd import _lib, whisper_tensor
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return whisper_tensor


def within_one_ulp(got32, ref64):
    """|got - fl32(ref)| <= ulp32(ref), elementwise"""
    r32 = np.asarray(ref64, np.float64).astype(np.float32)
    return np.abs(got32.astype(np.float64) - r32.astype(np.float64)) <= ulp32(r32)


@pytest.mark.parametrize("n_mels", [16, 80])
def test_library_tables_against_float64(wt, n_mels):
    window, dft, fb, band = wt.fe_tables(n_mels)
    assert window.shape == (400,) and dft.shape == (512, 416) and fb.shape == (201, n_mels) and band.shape == (n_mels, 2)
    assert within_one_ulp(window, window64()).all()
    b64 = basis64()
    ok = within_one_ulp(dft, b64)
    assert ok.all(), np.argwhere(~ok)[:5]
    pad = np.zeros(dft.shape, bool)  # rows 201..255 and 457..511, columns 400..415: the GEMM reads them, they must add nothing
    pad[201:256], pad[457:], pad[:, 400:] = True, True, True
    assert (dft[pad].view(np.uint32) == 0).all()
    f64 = fb64(n_mels)
    ok = within_one_ulp(fb, f64)
    assert ok.all(), [(int(k), int(m), float(fb[k, m]), float(f64[k, m])) for k, m in np.argwhere(~ok)[:5]]
    peak = f64.max(axis=0)
    k = np.arange(N_FREQ)[:, None]
    inside = (band[None, :, 0] <= k) & (k < band[None, :, 1])
    assert (band[:, 0] >= 0).all() and (band[:, 1] <= N_FREQ).all()
    assert (band[:, 1] > band[:, 0]).all(), "an empty band"
    assert inside[f64 > 1e-12 * peak[None, :]].all(), "a bin that carries weight lies outside its band"
    assert (fb[~inside] == 0).all(), "a coefficient outside its band, which mel_log_kernel never reads"
    # nothing in the table sits where the float64 and the fp32 value could fall on different sides of the clamp of the probe test
    pos = f64[f64 > 0]
    assert not ((pos > CLAMP / 10) & (pos < CLAMP * 10)).any()
    print(f"n_mels {n_mels}: band lengths {int((band[:, 1] - band[:, 0]).min())}..{int((band[:, 1] - band[:, 0]).max())}, "
          f"smallest positive coefficient {pos.min():.3e}")


def test_tables_hook_refuses_bad_arguments(wt):
    from whisper_mojo_amd import _lib
    for n_mels in (0, -1, 129):
        with pytest.raises(_lib.WhisperMiError, match="error -1"):
            wt.fe_tables(n_mels)
    w, d = np.zeros(400, np.float32), np.zeros((512, 416), np.float32)
    f, b = np.zeros((201, 16), np.float32), np.zeros((16, 2), np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    args = [w.ctypes.data_as(fp), d.ctypes.data_as(fp), f.ctypes.data_as(fp), b.ctypes.data_as(ip)]
    for hole in range(4):
        a = list(args)
        a[hole] = None
        assert _lib.lib().wm_op_fe_tables(16, *a) == -1
