"""GPU op tests of the encoder's attention kernels (flash_attn_enc_v2_kernel for bf16 / f16, flash_attn_enc_kernel for fp32) and of
layernorm_rows_kernel with both of its stores, against float64 with the per-element bounds of DESIGN §25.  Cases, references, bounds and
the proof that the kernels' arithmetic restated on the CPU stays inside them: tests/test_enc_ops_ref.py."""
import ctypes as C

import numpy as np
import pytest

import test_enc_ops_ref as gen

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


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _attention_batch(q, k, v, H, dt):
    from whisper_mojo_amd import whisper_tensor as wt
    out = np.full(q.shape, SENTINEL, np.float32)
    wt.attention_batch(out, q, k, v, H, dtype=gen.DTYPE[dt])
    return out


@pytest.mark.parametrize("dt", gen.DTYPES)
@pytest.mark.parametrize("c", gen.ATTN_CASES, ids=gen.case_id)
def test_attention_vs_float64(hip, c, dt):
    """One launch over B utterances against float64 on the rounded operands, every output element inside
    2·(u_T·(A + |ref|) + n_ctx·2^-24·A) (f16: + the subnormal-p term).  A wrong contribution of one key, a key mask off by one, a row
    maximum refreshed wrongly or a wrong utterance / head offset leaves that bar by orders of magnitude (the mutation list in §25)."""
    q, k, v = gen.attn_case(c)
    got = _attention_batch(q, k, v, c["H"], dt)
    assert np.isfinite(got).all()
    ratio = gen.attn_ratio(got, c, dt)
    print(f"MEASURED attention {gen.case_id(c)} {dt}: error / bar = {ratio:.3f}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("c", gen.SELECT_CASES, ids=lambda c: f"{c['n']}-{c['H']}-{c['B']}")
def test_attention_selects_one_key_exactly(hip, c):
    """Row i of (b, h) puts all its mass on key perm(i): out[b, i, h] == V[b, perm(i), h] bit for bit in all three types — the key order
    of v2's transposing LDS read, v1's pos map and the (b, h) indexing with no tolerance at all."""
    q, k, v, want, _ = gen.select_case(c)
    for dt in gen.DTYPES:
        got = _attention_batch(q, k, v, c["H"], dt)
        bad = np.argwhere(_bits(got) != _bits(want))
        assert bad.size == 0, (dt, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("dt", gen.DTYPES)
@pytest.mark.parametrize("c", [c for c in gen.ATTN_CASES if gen.case_id(c) in (
    "random-129-6-4", "random-64-6-3", "random-191-8-2", "random-17-12-2", "stair_up-257-12-2-step10", "spike_last-65-8-2-lev0")], ids=gen.case_id)
def test_attention_batch_equals_singles(hip, c, dt):
    """Row b of the batched launch is bit-equal to wm_op_attention on utterance b alone — with the XCD remap on in the batch (B·H % 8 == 0)
    and off, and whatever it is in the single launch; a repeated launch gives equal bits."""
    from whisper_mojo_amd import whisper_tensor as wt
    q, k, v = gen.attn_case(c)
    got = _attention_batch(q, k, v, c["H"], dt)
    for b in range(c["B"]):
        one = np.full(q.shape[1:], SENTINEL, np.float32)
        wt.attention(one, q[b], k[b], v[b], c["H"], dtype=gen.DTYPE[dt])
        assert np.array_equal(_bits(one), _bits(got[b])), b
    assert np.array_equal(_bits(_attention_batch(q, k, v, c["H"], dt)), _bits(got))


def _layer_norm_t(x, g, b, dt, want_t=True, want_f=True):
    """the launch with rows + 1 rows of sentinel-filled device output: the guard row must come back untouched (rows = 1 or odd: the second
    half-wave of the last wave re-reads row rows - 1 and must store nothing)"""
    from whisper_mojo_amd import whisper_tensor as wt
    rows, cols = x.shape
    out_t = np.full((rows + 1, cols), SENTINEL, np.float32) if want_t else None
    out_f = np.full((rows + 1, cols), SENTINEL, np.float32) if want_f else None
    wt.layer_norm_t(x, g, b, gen.EPS, gen.DTYPE[dt], out_t=out_t, out_f=out_f)
    for o in (out_t, out_f):
        if o is not None:
            assert (o[rows] == SENTINEL).all()
    return (None if out_t is None else out_t[:rows]), (None if out_f is None else out_f[:rows])


@pytest.mark.parametrize("cols", gen.LN_COLS)
@pytest.mark.parametrize("kind", gen.LN_KINDS)
def test_layer_norm_both_stores(hip, kind, cols):
    """layernorm_rows_kernel<T, cols/128> at every row count of the half-wave-per-row layout's tail: out_f inside the bound of float64,
    out_t bit-equal to out_f rounded to T (one y feeds both stores), out_f bit-equal with and without out_t, the same bits from
    wm_op_layer_norm, and nothing written past the last row."""
    from whisper_mojo_amd import whisper_tensor as wt
    worst = 0.0
    for rows in gen.LN_ROWS:
        x, g, b = gen.ln_case(kind, rows, cols)
        outs = {}
        for dt in gen.DTYPES:
            out_t, out_f = _layer_norm_t(x, g, b, dt)
            assert np.isfinite(out_f).all()
            worst = max(worst, gen.ln_ratio(out_f, x, g, b))
            assert np.array_equal(_bits(out_t), _bits(gen.rnd(out_f, dt))), (rows, dt)
            _, only_f = _layer_norm_t(x, g, b, dt, want_t=False)
            only_t, _ = _layer_norm_t(x, g, b, dt, want_f=False)
            assert np.array_equal(_bits(only_f), _bits(out_f)) and np.array_equal(_bits(only_t), _bits(out_t)), (rows, dt)
            outs[dt] = out_f
        assert np.array_equal(_bits(outs["bf16"]), _bits(outs["f32"])) and np.array_equal(_bits(outs["f16"]), _bits(outs["f32"]))
        plain = wt.Tensor(rows, cols)
        wt.layer_norm(plain, x, g, b, gen.EPS)
        assert np.array_equal(_bits(plain), _bits(outs["f32"]))
    print(f"MEASURED layer_norm {kind} cols {cols}: error / bound = {worst:.3f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("cols", gen.LN_COLS)
def test_layer_norm_constant_rows(hip, cols):
    """Rows whose float64 variance is 0 (means 1, 13, 100 and 1.7, 13.7, 100.7) or one ulp from it: the one-pass variance comes out at
    or below 0 in float32.  The output is finite and inside the bound (the kernel clamps the variance at 0 before it adds eps)."""
    x, g, b = gen.ln_const_case(cols)
    for dt in gen.DTYPES:
        out_t, out_f = _layer_norm_t(x, g, b, dt)
        assert np.isfinite(out_f).all() and np.isfinite(out_t).all(), (dt, np.argwhere(~np.isfinite(out_f))[:4].tolist())
        ratio = gen.ln_ratio(out_f, x, g, b)
        print(f"MEASURED layer_norm constant rows cols {cols} {dt}: error / bound = {ratio:.3f}")
        assert ratio <= 1.0, ratio
        assert np.array_equal(_bits(out_t), _bits(gen.rnd(out_f, dt)))


def test_hooks_refuse_bad_arguments(hip):
    """WM_E_ARG, nothing launched, the output sentinel intact."""
    q = np.ones((2, 16, 128), np.float32)
    out = np.full(q.shape, SENTINEL, np.float32)
    for B, n, H, dt in ((0, 16, 2, 1), (-1, 16, 2, 1), (2, 0, 2, 1), (2, 16, 0, 1), (2, 16, 65, 1), (2, 16, 2, 3), (2, 16, 2, -1)):
        assert hip.wm_op_attention_batch(_fp(out), _fp(q), _fp(q), _fp(q), B, n, H, dt) == WM_E_ARG
    assert hip.wm_op_attention_batch(_fp(out), None, _fp(q), _fp(q), 2, 16, 2, 1) == WM_E_ARG
    assert (out == SENTINEL).all()
    x, g = np.ones((4, 256), np.float32), np.ones(256, np.float32)
    ot, of = np.full(x.shape, SENTINEL, np.float32), np.full(x.shape, SENTINEL, np.float32)
    assert hip.wm_op_layer_norm_t(None, None, _fp(x), _fp(g), _fp(g), 4, 256, 1e-5, 1) == WM_E_ARG
    for rows, cols, dt in ((0, 256, 1), (4, 0, 1), (4, 200, 1), (4, 1152, 1), (4, 256, 3), (4, 256, -1)):
        assert hip.wm_op_layer_norm_t(_fp(ot), _fp(of), _fp(x), _fp(g), _fp(g), rows, cols, 1e-5, dt) == WM_E_ARG
    assert hip.wm_op_layer_norm_t(_fp(ot), _fp(of), None, _fp(g), _fp(g), 4, 256, 1e-5, 1) == WM_E_ARG
    assert (ot == SENTINEL).all() and (of == SENTINEL).all()
