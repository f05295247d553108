"""Op-level tests (-m gpu) of the pass-control and data-movement kernels: init_tokens / init_tokens_rows, set_rows_step,
set_step, pack_tokens, dec_embed, the two row copies (no_speech_capture, score_collect) and mel_transpose_pad with B > 1 — each hook
makes exactly the runtime's launch on the caller's sentinel-filled buffers, which come back whole.  The expectations are the few lines of
numpy in tests/test_ts_states_ref.py; everything is integers or exact bits."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_decode_ops import DT_BF16, DT_F16, DT_F32, _round, hip  # noqa: F401
from test_ts_states_ref import init_tokens_expect, mel_image_expect, pack_tokens_expect, ragged_prompts, rows_copy_expect

pytestmark = pytest.mark.gpu

S = -77  # sentinel (exact in bf16 / f16 too)
WM_E_ARG = -1
TS = (12, 8, 5, 1)


def _bufs(B, B_held, out_stride, rows_held, tok_rows, ts, lp, key_lo):
    i = lambda *s: np.full(s, S, np.int32)
    return dict(out_tokens=i(B_held, out_stride), n_tokens=i(B_held), finished=i(B_held), ctl=i(4),
                tok_rows=i(rows_held, B) if tok_rows else None, pos_rows=i(rows_held, B) if tok_rows else None,
                ts_state=i(B_held, 8) if ts else None, logprobs=np.full((B_held, out_stride), S, np.float32) if lp else None,
                lp_sum=np.full(B_held, S, np.float32) if lp else None, key_lo=i(B_held) if key_lo else None)


def _same(got, want):
    for k, w in want.items():
        if w is None:
            assert got.get(k) is None
        else:
            np.testing.assert_array_equal(got[k], w, err_msg=k)


@pytest.mark.parametrize("opt", [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)])
@pytest.mark.parametrize("n_prompt", [1, 4, 16])
@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_init_tokens_shared_prompt(hip, B, n_prompt, opt):
    """init_tokens_kernel: B across the 256-thread block, each optional pointer present and absent; rows past B, ids past the prompt,
    position rows past n_prompt and ctl's pad words keep the sentinel."""
    from whisper_mojo_amd import whisper_tensor as wt
    tok_rows, ts, lp = opt
    prompt = [(7 * i + 3) % 50 for i in range(n_prompt)]
    bufs = _bufs(B, B + 3, 21, n_prompt + 2, tok_rows, ts, lp, False)
    want = init_tokens_expect(bufs, B, 21, prompt=prompt, ts=TS)
    got = wt.init_tokens(bufs, B, prompt=prompt, ts=TS if ts else None)
    _same(got, want)
    assert (got["out_tokens"][B:] == S).all() and (got["out_tokens"][:B, n_prompt:] == S).all() and got["ctl"].tolist() == [0, 0, S, S]


@pytest.mark.parametrize("opt", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("Lmax", [1, 5, 16])
@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_init_tokens_row_prompts(hip, B, Lmax, opt):
    """init_tokens_rows_kernel: len[b] from 1 to Lmax; the dead slots in front of a shorter prompt hold (row[0], position 0), key_lo =
    Lmax - len, and nothing is written outside [Lmax][B]."""
    from whisper_mojo_amd import whisper_tensor as wt
    ts, lp = opt
    lens = np.array([1 + (b * 7) % Lmax for b in range(B)], np.int32)
    lens[0], lens[-1] = Lmax, (1 if B > 1 else Lmax)
    table = np.full((B, Lmax + 2), 99, np.int32)
    for b in range(B):
        table[b, :lens[b]] = [(b + 5 * i) % 97 for i in range(lens[b])]
    bufs = _bufs(B, B + 3, 19, Lmax + 2, True, ts, lp, True)
    want = init_tokens_expect(bufs, B, 19, table=table, lens=lens, Lmax=Lmax, ts=TS)
    got = wt.init_tokens(bufs, B, table=table, lens=lens, Lmax=Lmax, ts=TS if ts else None)
    _same(got, want)
    assert (got["tok_rows"][Lmax:] == S).all() and (got["pos_rows"][Lmax:] == S).all() and (got["key_lo"][B:] == S).all()
    assert (got["tok_rows"][:Lmax] != 99).all() and (got["key_lo"][:B] == Lmax - lens).all()


@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_set_rows_step_and_set_step(hip, B):
    from whisper_mojo_amd import whisper_tensor as wt
    lens = np.array([1 + (b * 5) % 11 for b in range(B)], np.int32)
    for delta in (-1, 0):
        ctl, pos = np.full(4, S, np.int32), np.full(B + 2, S, np.int32)
        wt.set_rows_step(ctl, pos, lens, 11, delta, B)
        assert ctl.tolist() == [11, S, S, S] and (pos[:B] == lens + delta).all() and (pos[B:] == S).all()
    for with_pos, with_tok, set_len in ((1, 1, 1), (1, 0, 0), (0, 1, 1), (0, 0, 0), (0, 0, 1)):
        ctl = np.full(4, S, np.int32)
        pos = np.full(B + 2, S, np.int32) if with_pos else None
        tok = np.full(B + 2, S, np.int32) if with_tok else None
        wt.set_step(ctl, pos, tok, 9, set_len, 4, 50258, B, B + 2)
        assert ctl.tolist() == [9 if set_len else S, S, S, S]
        if with_pos:
            assert (pos[:B] == 4).all() and (pos[B:] == S).all()
        if with_tok:
            assert (tok[:B] == 50258).all() and (tok[B:] == S).all()


@pytest.mark.parametrize("rows,rows_cap", [(1, 1), (5, 8), (0, 3), (257, 260)])
@pytest.mark.parametrize("stride,out_stride", [(7, 12), (12, 12), (300, 448)])
def test_pack_tokens(hip, rows, rows_cap, stride, out_stride):
    """rows < rows_cap (the rows between are zeroed), n_tokens below, at and above stride (truncated), stride past one 256-thread sweep."""
    from whisper_mojo_amd import whisper_tensor as wt
    r = np.random.default_rng(rows + stride)
    out = r.integers(1, 51865, (max(rows, 1), out_stride)).astype(np.int32)
    n = np.array([(0, stride - 1, stride, min(stride + 1, out_stride), out_stride, 1)[k % 6] for k in range(max(rows, 1))], np.int32)
    dst = np.full((rows_cap + 2, 1 + stride), S, np.int32)
    want = pack_tokens_expect(dst, out, n, rows, rows_cap, stride)
    wt.pack_tokens(dst, out, n, rows, rows_cap, stride)
    np.testing.assert_array_equal(dst, want)
    assert (dst[rows_cap:] == S).all() and (dst[rows:rows_cap] == 0).all()


@pytest.mark.parametrize("d", [128, 384, 768, 1024])
def test_dec_embed(hip, d):
    """x[b] = tok_emb[tok[b]] + pos_emb[pos[b]], one fp32 add: bitwise; ids 0 and vocab - 1, positions 0 and n_pos - 1; then the
    position-major rows an init launch returned, fed as the prefill feeds them."""
    from whisper_mojo_amd import whisper_tensor as wt
    r = np.random.default_rng(d)
    vocab, n_pos = 300, 64
    te, pe = r.standard_normal((vocab, d)).astype(np.float32), r.standard_normal((n_pos, d)).astype(np.float32)
    tok = np.array([0, vocab - 1, 5, 0, vocab - 1] + r.integers(0, vocab, 28).tolist(), np.int32)
    pos = np.array([0, n_pos - 1, n_pos - 1, 7, 0] + r.integers(0, n_pos, 28).tolist(), np.int32)
    x = np.full((tok.size + 1, d), S, np.float32)
    wt.dec_embed(x, te, pe, tok, pos)
    np.testing.assert_array_equal(x[:-1], np.float32(te[tok]) + np.float32(pe[pos]))
    assert (x[-1] == S).all()
    B, Lmax = 6, 5
    lens = np.array([5, 1, 3, 2, 4, 1], np.int32)
    table = np.array(ragged_prompts(B, vocab, 5, 5), np.int32) + 200
    bufs = wt.init_tokens(_bufs(B, B, 8, Lmax, True, False, False, True), B, table=table, lens=lens, Lmax=Lmax)
    t, p = bufs["tok_rows"].ravel(), bufs["pos_rows"].ravel()
    x = np.full((Lmax * B + 1, d), S, np.float32)
    wt.dec_embed(x, te, pe, t, p)
    for row in range(Lmax * B):
        i, b = divmod(row, B)
        pad = Lmax - lens[b]
        tid, ps = (table[b, 0], 0) if i < pad else (table[b, i - pad], i - pad)
        np.testing.assert_array_equal(x[row], te[tid] + pe[ps])
    assert (x[-1] == S).all()


@pytest.mark.parametrize("n_rows", [1, 17, 200])
@pytest.mark.parametrize("d", [128, 384])
def test_row_copies(hip, n_rows, d):
    """no_speech_capture (the plain copy) and score_collect (by destination map: -1 entries skipped, permutations): rows that were not
    addressed keep the sentinel, bit for bit."""
    from whisper_mojo_amd import whisper_tensor as wt
    r = np.random.default_rng(n_rows + d)
    rows = r.standard_normal((n_rows, d)).astype(np.float32)
    out = np.full((n_rows + 2, d), S, np.float32)
    want = rows_copy_expect(out, rows, None)
    wt.rows_copy(out, rows)
    np.testing.assert_array_equal(out, want)
    assert (out[n_rows:] == S).all()
    perm = r.permutation(n_rows + 5).astype(np.int32)[:n_rows]  # into a larger buffer: five rows stay unaddressed
    holes = perm.copy()
    holes[::3] = -1
    for dst in (perm, holes, np.full(n_rows, -1, np.int32), np.arange(n_rows, dtype=np.int32)[::-1].copy()):
        out = np.full((n_rows + 5, d), S, np.float32)
        want = rows_copy_expect(out, rows, dst)
        wt.rows_copy(out, rows, dst)
        np.testing.assert_array_equal(out, want)
        untouched = np.setdiff1d(np.arange(n_rows + 5), dst[dst >= 0])
        assert (out[untouched] == S).all() and len(untouched) >= 5


@pytest.mark.parametrize("dt", [DT_F32, DT_BF16, DT_F16])
@pytest.mark.parametrize("Cc,L,B", [(80, 130, 3), (128, 64, 2), (80, 1, 1), (16, 65, 2)])
def test_mel_transpose_pad(hip, Cc, L, B, dt):
    """The padded token-major image of B clips: bitwise the rounded transpose, rows 0 and L + 1 and channels >= C zero, the guard clip
    behind the last one untouched."""
    from whisper_mojo_amd import whisper_tensor as wt
    r = np.random.default_rng(Cc + L + B + dt)
    mel = (r.standard_normal((B, Cc, L)) * 1.5).astype(np.float32)
    Cp = (Cc + 31) // 32 * 32
    img = np.full((B + 1, L + 2, Cp), S, np.float32)
    wt.mel_transpose_pad(img, mel, dt)
    want = mel_image_expect(mel, Cp, _round(mel, dt).astype(np.float32))
    np.testing.assert_array_equal(img[:B], want)
    assert (img[:B, 0] == 0).all() and (img[:B, L + 1] == 0).all() and (img[:B, :, Cc:] == 0).all() and (img[B] == S).all()


def test_refusals_launch_nothing(hip):
    """Every refusal of every new hook: WM_E_ARG, the outputs untouched."""
    from whisper_mojo_amd import _lib
    L = _lib.lib()
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    i = lambda *s: np.full(s, S, np.int32)
    f = lambda *s: np.full(s, S, np.float32)
    clean = lambda *a: all((x == S).all() for x in a if x is not None)

    def init(B=2, B_held=2, stride=6, n_prompt=3, lens=None, row_stride=0, Lmax=0, rows_held=4, tok_rows=True, key_lo=False, ts=False, lp=1, tb=8,
             eos=5, vocab=12, pos_rows=True):
        b = _bufs(B, max(B_held, 1), stride, rows_held, tok_rows, ts, lp > 0, key_lo)
        if not pos_rows:
            b["pos_rows"] = None
        if lp == 2:
            b["lp_sum"] = None
        prompt = np.arange(1, 17, dtype=np.int32) if lens is None else np.tile(np.arange(1, row_stride + 1, dtype=np.int32), (B, 1))
        ln = None if lens is None else np.asarray(lens, np.int32)
        rc = L.wm_op_init_tokens(ip(b["out_tokens"]), ip(b["n_tokens"]), ip(b["finished"]), ip(b["ctl"]), ip(b["tok_rows"]), ip(b["pos_rows"]),
                                 ip(b["ts_state"]), fp(b["logprobs"]), fp(b["lp_sum"]), ip(b["key_lo"]), ip(prompt), n_prompt, ip(ln), row_stride, Lmax,
                                 rows_held, B, B_held, stride, vocab, tb, eos, -1)
        return rc, clean(*b.values())

    assert init()[0] == 0 and init(lens=[2, 4], row_stride=5, Lmax=4, key_lo=True, ts=True)[0] == 0
    for kw in (dict(B=0), dict(B_held=1), dict(n_prompt=0), dict(n_prompt=17, stride=32, rows_held=20), dict(n_prompt=7), dict(rows_held=2),
               dict(pos_rows=False), dict(lp=2), dict(key_lo=True), dict(ts=True, tb=0), dict(ts=True, tb=12), dict(ts=True, eos=9),
               dict(lens=[2, 4], row_stride=5, Lmax=4), dict(lens=[2, 4], row_stride=5, Lmax=4, key_lo=True, tok_rows=False),
               dict(lens=[2, 5], row_stride=5, Lmax=4, key_lo=True), dict(lens=[0, 4], row_stride=5, Lmax=4, key_lo=True),
               dict(lens=[2, 4], row_stride=3, Lmax=4, key_lo=True), dict(lens=[2, 4], row_stride=5, Lmax=4, key_lo=True, rows_held=3),
               dict(lens=[2, 4], row_stride=8, Lmax=7, key_lo=True, stride=3, rows_held=7)):
        assert init(**kw) == (WM_E_ARG, True), kw

    ctl, pos, tok = i(4), i(4), i(4)
    ln = np.array([1, 2, 3], np.int32)
    for a in ((None, ip(pos), ip(ln), 3, 0, 3, 4), (ip(ctl), None, ip(ln), 3, 0, 3, 4), (ip(ctl), ip(pos), None, 3, 0, 3, 4),
              (ip(ctl), ip(pos), ip(ln), 3, 0, 0, 4), (ip(ctl), ip(pos), ip(ln), 3, 0, 3, 2)):
        assert L.wm_op_set_rows_step(*a) == WM_E_ARG and clean(ctl, pos)
    for a in ((None, ip(pos), ip(tok), 1, 1, 1, 1, 3, 4), (ip(ctl), ip(pos), ip(tok), 1, 1, 1, 1, 0, 4), (ip(ctl), ip(pos), ip(tok), 1, 1, 1, 1, 5, 4)):
        assert L.wm_op_set_step(*a) == WM_E_ARG and clean(ctl, pos, tok)

    dst, out, n = i(3, 5), np.ones((2, 6), np.int32), np.array([2, 6], np.int32)
    bad_n, neg_n = np.array([2, 7], np.int32), np.array([-1, 2], np.int32)
    for a in ((None, ip(out), ip(n), 6, 2, 3, 3, 4), (ip(dst), None, ip(n), 6, 2, 3, 3, 4), (ip(dst), ip(out), None, 6, 2, 3, 3, 4),
              (ip(dst), ip(out), ip(n), 6, 2, 1, 3, 4), (ip(dst), ip(out), ip(n), 6, 2, 3, 2, 4), (ip(dst), ip(out), ip(n), 6, 2, 3, 3, 0),
              (ip(dst), ip(out), ip(n), 0, 2, 3, 3, 4), (ip(dst), ip(out), ip(n), 6, -1, 3, 3, 4), (ip(dst), ip(out), ip(neg_n), 6, 2, 3, 3, 4),
              (ip(dst), ip(out), ip(bad_n), 3, 2, 3, 3, 4)):  # min(7, 4) ids of a row that holds 3
        assert L.wm_op_pack_tokens(*a) == WM_E_ARG and clean(dst)

    x, te, pe = f(3, 8), np.zeros((5, 8), np.float32), np.zeros((4, 8), np.float32)
    ok_t, ok_p = np.array([0, 4], np.int32), np.array([3, 0], np.int32)
    for t_, p_, B_, Bh in ((np.array([0, 5], np.int32), ok_p, 2, 3), (np.array([-1, 4], np.int32), ok_p, 2, 3), (ok_t, np.array([4, 0], np.int32), 2, 3),
                           (ok_t, np.array([0, -1], np.int32), 2, 3), (ok_t, ok_p, 0, 3), (ok_t, ok_p, 2, 1)):
        assert L.wm_op_dec_embed(fp(x), fp(te), fp(pe), ip(t_), ip(p_), B_, Bh, 8, 5, 4) == WM_E_ARG and clean(x)
    assert L.wm_op_dec_embed(fp(x), None, fp(pe), ip(ok_t), ip(ok_p), 2, 3, 8, 5, 4) == WM_E_ARG and clean(x)
    assert L.wm_op_dec_embed(fp(x), fp(te), fp(pe), ip(ok_t), ip(ok_p), 2, 3, 0, 5, 4) == WM_E_ARG and clean(x)

    o, rows = f(3, 8), np.zeros((2, 8), np.float32)
    for a in ((None, fp(rows), None, 2, 3, 8), (fp(o), None, None, 2, 3, 8), (fp(o), fp(rows), None, 0, 3, 8), (fp(o), fp(rows), None, 2, 1, 8),
              (fp(o), fp(rows), None, 2, 3, 6), (fp(o), fp(rows), ip(np.array([0, 3], np.int32)), 2, 3, 8),
              (fp(o), fp(rows), ip(np.array([-2, 1], np.int32)), 2, 3, 8)):
        assert L.wm_op_rows_copy(*a) == WM_E_ARG and clean(o)

    img, mel = f(2, 6, 32), np.zeros((1, 16, 4), np.float32)
    for a in ((None, fp(mel), 1, 2, 16, 4, 0), (fp(img), None, 1, 2, 16, 4, 0), (fp(img), fp(mel), 0, 2, 16, 4, 0), (fp(img), fp(mel), 3, 2, 16, 4, 0),
              (fp(img), fp(mel), 1, 2, 0, 4, 0), (fp(img), fp(mel), 1, 2, 16, 0, 0), (fp(img), fp(mel), 1, 2, 16, 4, 3), (fp(img), fp(mel), 1, 2, 16, 4, -1)):
        assert L.wm_op_mel_transpose_pad(*a) == WM_E_ARG and clean(img)
