"""GPU: resample_kernel alone (wm_op_resample) against the float64 restatement of tests/test_resample_ref.py run on the
same float32 taps.

The bar of every value is the dot-product bound, derived and not measured: |y - y64| <= gamma_n * sum_k |h_k x_k| with gamma_n =
n u / (1 - n u), u = 2^-24 and n = (non-zero taps of the output's phase) + 1.  The kernel's fmaf chain rounds once per tap, which the
bound covers.  Each case prints its worst err / bound; the bar is 1.  The output starts as a sentinel, so a store at or beyond a row's
n_out shows, and rows are compared bit for bit where the contract says a value depends on its own row alone."""
import numpy as np
import pytest

from test_resample_ref import out_len, ratio, resample64, taps32

pytestmark = pytest.mark.gpu

RATES = [8000, 11025, 22050, 44100, 48000]
FILL = -7.0
U = 2.0 ** -24


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_mojo_amd import _lib
    _lib.lib()
    return _lib


def lengths(sr_in):
    orig, _, width = ratio(sr_in)
    return [1, width, orig, orig + 1, 3 * orig + 5, 4001]


def check_rows(hip, rows, sr_in, label, js=None):
    """every row through one launch; -> worst err / bound.  js: per row the outputs to compare (None: all)"""
    out, n_out = hip.op_resample(rows, sr_in, fill=FILL)
    h = taps32(sr_in)
    worst = 0.0
    for b, x in enumerate(rows):
        x32 = np.asarray(x, np.float32) / (32768.0 if np.asarray(x).dtype == np.int16 else 1.0)
        assert n_out[b] == out_len(len(x), sr_in), (label, b)
        assert (out[b, n_out[b]:] == FILL).all(), (label, b, "a store at or beyond n_out")
        sel = None if js is None else js[b]
        y, mag, cnt = resample64(x32, sr_in, h, sel)
        n = cnt + 1
        bound = n * U / (1 - n * U) * mag
        err = np.abs(out[b, :n_out[b]].astype(np.float64) - y)
        if sel is not None:
            err, bound = err[sel], bound[sel]
        assert np.isfinite(out[b, :n_out[b]]).all()
        bad = err > bound
        assert not bad.any(), (label, b, int(np.argmax(bad)), float(err[bad].max()))
        live = bound > 0
        if live.any():
            worst = max(worst, float((err[live] / bound[live]).max()))
    print(f"resample {label}: {len(rows)} rows, worst err / bound = {worst:.3f}")
    return worst


@pytest.mark.parametrize("sr_in", RATES)
def test_uniform_rows_of_every_length(hip, sr_in):
    rng = np.random.default_rng(sr_in)
    rows = [rng.uniform(-1, 1, n).astype(np.float32) for n in lengths(sr_in)]
    assert check_rows(hip, rows, sr_in, f"{sr_in} uniform") <= 1.0


@pytest.mark.parametrize("sr_in", RATES)
def test_impulses_at_both_edges(hip, sr_in):
    rows = []
    for n in lengths(sr_in):
        first, last = np.zeros(n, np.float32), np.zeros(n, np.float32)
        first[0], last[n - 1] = 1.0, 1.0
        rows += [first, last]
    assert check_rows(hip, rows, sr_in, f"{sr_in} impulses") <= 1.0
    # the impulse response is the table itself: output j of an impulse at sample 0 is h[j % new][width - (j // new) * orig]
    orig, new, width = ratio(sr_in)
    out, n_out = hip.op_resample([rows[-2]], sr_in, fill=FILL)
    h = taps32(sr_in)
    for j in range(min(int(n_out[0]), 4 * new)):
        k = width - (j // new) * orig
        assert out[0, j] == (h[j % new, k] if k >= 0 else 0.0), j


@pytest.mark.parametrize("sr_in", RATES)
def test_constant_row_gives_the_dc_gain(hip, sr_in):
    orig, new, width = ratio(sr_in)
    n = 4001
    rows = [np.ones(n, np.float32)]
    assert check_rows(hip, rows, sr_in, f"{sr_in} constant") <= 1.0
    out, n_out = hip.op_resample(rows, sr_in, fill=FILL)
    h = taps32(sr_in).astype(np.float64)
    dc, nz = h.sum(1), (h != 0).sum(1) + 1
    j = np.arange(int(n_out[0]))
    inner = ((j // new) * orig - width >= 0) & ((j // new) * orig + width + orig <= n)  # every tap of the output reads a real sample
    assert inner.sum() > new
    p = j[inner] % new
    bound = nz[p] * U / (1 - nz[p] * U) * np.abs(h).sum(1)[p]
    assert (np.abs(out[0, j[inner]] - dc[p]) <= bound).all()
    print(f"resample {sr_in} constant: DC gain of the phases in [{dc.min():.6f}, {dc.max():.6f}]")
    assert np.abs(dc - 1.0).max() < 0.05  # about 1: a property of the table, which test_resample_ref.py pins bit for bit


def test_ragged_batch_equals_every_row_alone(hip):
    rng = np.random.default_rng(7)
    rows = [rng.uniform(-1, 1, n).astype(np.float32) for n in (4001, 1, 1777)]
    out, n_out = hip.op_resample(rows, 44100, fill=FILL)
    assert n_out.tolist() == [out_len(len(r), 44100) for r in rows]
    for b, r in enumerate(rows):
        alone, n1 = hip.op_resample([r], 44100, fill=FILL)
        assert n1[0] == n_out[b]
        assert np.array_equal(out[b, :n_out[b]].view(np.uint32), alone[0, :n1[0]].view(np.uint32)), b
        assert (out[b, n_out[b]:] == FILL).all() and out[b, n_out[b]:].size >= 8, b
        swapped, _ = hip.op_resample([rows[(b + 1) % 3], r], 44100, fill=FILL)  # another position, another neighbour
        assert np.array_equal(swapped[1, :n1[0]].view(np.uint32), alone[0, :n1[0]].view(np.uint32)), b


@pytest.mark.parametrize("sr_in", [44100, 48000, 8000])
def test_int16_equals_float_on_the_scaled_samples(hip, sr_in):
    rng = np.random.default_rng(sr_in + 1)
    rows = []
    for n in (1777, 5, 4001):
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        x[:3] = (-32768, 32767, 0)
        x[-1] = -32768
        rows.append(x)
    a, na = hip.op_resample(rows, sr_in, fill=FILL)
    assert a.dtype == np.float32 and hip.pack_pcm(rows)[2] == hip.WM_I16
    b, nb = hip.op_resample([r.astype(np.float32) / np.float32(32768.0) for r in rows], sr_in, fill=FILL)
    assert na.tolist() == nb.tolist()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_identity_rate_copies_and_converts(hip):
    x = np.random.default_rng(3).uniform(-1, 1, 1500).astype(np.float32)
    out, n = hip.op_resample([x], 16000, fill=FILL)
    assert n[0] == 1500 and np.array_equal(out[0, :1500], x) and (out[0, 1500:] == FILL).all()
    i = np.asarray([-32768, 32767, 0, 1, -1], np.int16)
    out, n = hip.op_resample([i], 16000, fill=FILL)
    assert out[0, :5].tolist() == [-1.0, 32767 / 32768, 0.0, 1 / 32768, -1 / 32768]


def test_indices_beyond_32_bits(hip):
    """13.5 M int16 samples at 44 100 Hz: new * n = 2.16e9 leaves 32 bits, as does the byte offset of the row's end.  The head, the
    2^31 crossing of j * orig and the tail are compared; every length and the sentinel behind the row as always."""
    sr_in, n = 44100, 13_500_000
    orig, new, _ = ratio(sr_in)
    assert new * n > 2 ** 31
    x = np.random.default_rng(11).integers(-20000, 20000, n).astype(np.int16)
    n_out = out_len(n, sr_in)
    cross = 2 ** 31 // orig
    js = [np.r_[0:40, cross - 20:cross + 20, n_out - 40:n_out]]
    assert check_rows(hip, [x], sr_in, "44100 long row", js) <= 1.0
